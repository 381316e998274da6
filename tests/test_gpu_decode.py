"""Archive blocks decoded on the device: k_dec_init, k_dec_qual, k_dec_place and
k_dec_seq through sa_decode_blocks, fq.Decoder and seqarc_amd -d --gpu-decode.
Inputs are test_decode_emu's corpus; a decoded block must equal the block that was
encoded and what sa_decode_block gives, a corrupt block must get the status the
driver's CPU emulation (tests/cpu_emu/decoder_emu.cpp) gives it, the number of
launches must be the one computed from the symbol counts, and the command line
must write the files of -d without the switch."""
import os
import subprocess

import numpy as np
import pytest

import oracle_py
import synth
from conftest import ROOT, TEST1, TEST2
from test_decode_emu import OK, UNSUPPORTED, VALID, case, corrupt_cases, equal_to_input
from test_decoder_host import run_drv

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "fastqueeze_amd", "bin", "seqarc_amd")


@pytest.fixture
def knobs(monkeypatch):
    """SA_DEC_SLICE / SA_DEC_INFLIGHT for the Decoders made in the test (read at sa_decoder_create)."""
    def set_(slice_=None, inflight=None):
        for name, v in (("SA_DEC_SLICE", slice_), ("SA_DEC_INFLIGHT", inflight)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    set_()
    return set_


def _decode(c, dec=None):
    d = dec or fq.Decoder(0)
    try:
        return d.decode(c.enc, c.caps, c.cfg, c.tmpl, c.long), d.info()
    finally:
        if dec is None:
            d.close()


def _check(c, res):
    assert len(res) == len(c.blocks)
    for i, (blk, (got, ok, st), (hblk, hok)) in enumerate(zip(c.blocks, res, c.host)):   # input order
        assert st == OK and got is not None, (c.name, i, st)
        assert equal_to_input(blk, got), (c.name, i)
        assert got.seq.tobytes() == hblk.seq.tobytes() and got.qual.tobytes() == hblk.qual.tobytes(), (c.name, i)
        assert got.names.tobytes() == hblk.names.tobytes() and ok == hok, (c.name, i)


@pytest.mark.parametrize("name", VALID)
def test_valid_blocks_equal_the_input(knobs, name):
    c = case(name)
    res, info = _decode(c)
    _check(c, res)
    assert info["unsupported"] == 0 and info["groups"] >= 1 and info["slice"] == 1 << 18, info


@pytest.mark.parametrize("name,slice_", [("poly_a", 1), ("shapes", 61)])
def test_slices(knobs, name, slice_):
    """Chains stopped and resumed through the stored state after every `slice` symbols, in
    exactly ceil(total / slice) launches a chain."""
    knobs(slice_=slice_)
    c = case(name)
    res, info = _decode(c)
    _check(c, res)
    total = int(c.blocks[0].seq_lens.sum())
    assert len(c.blocks) == 1 and info["slice"] == slice_, info
    assert info["qual_launches"] == info["seq_launches"] == -(-total // slice_), (info, total)


def test_groups_and_a_second_call(knobs):
    knobs(inflight=2)
    c = case("groups")
    dec = fq.Decoder(0)
    try:
        res, info = _decode(c, dec)
        _check(c, res)
        assert info["groups"] == 3 and info["inflight"] == 2, info
        res, info2 = _decode(c, dec)   # the same buffers and tables: re-initialised
        _check(c, res)
        assert {k: info2[k] for k in ("groups", "inflight", "qual_launches", "seq_launches")} == \
               {k: info[k] for k in ("groups", "inflight", "qual_launches", "seq_launches")}
    finally:
        dec.close()


def test_corrupt_blocks_beside_a_good_one(knobs, tmp_path):
    exe = tmp_path / "decoder_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", str(exe), os.path.join(ROOT, "tests", "cpu_emu", "decoder_emu.cpp")],
                   check=True)
    c = case("shapes")
    bad = corrupt_cases()
    blocks = [(blk, False, cap) for _, blk, cap, _ in bad[:2]] + [(c.enc[0], False, c.caps[0])] + \
             [(blk, False, cap) for _, blk, cap, _ in bad[2:]]
    _, want, _ = run_drv(exe, tmp_path, "ref", c.cfg, c.tmpl, 1 << 18, blocks)
    dec = fq.Decoder(0)
    try:
        res = dec.decode([b for b, _, _ in blocks], [cap for _, _, cap in blocks], c.cfg, c.tmpl)
        info = dec.info()
    finally:
        dec.close()
    assert info["groups"] == 1, info
    for i, ((got, ok, st), w) in enumerate(zip(res, want)):
        assert st == w[0], (i, st, w)
        if st == OK:
            assert int(ok) == w[1], (i, ok, w)
    got, ok, st = res[2]
    assert st == OK and ok == c.host[0][1] and equal_to_input(c.blocks[0], got)
    assert sum(1 for _, _, st in res if st != OK) >= 3


def test_lossy_config_is_unsupported(knobs):
    c = case("shapes")
    dec = fq.Decoder(0)
    try:
        res = dec.decode(c.enc, c.caps, fq.Config(lossy=1.0), c.tmpl)
        assert [(b, st) for b, _, st in res] == [(None, UNSUPPORTED)] and dec.info()["unsupported"] == 1
    finally:
        dec.close()


# ---- the command line ------------------------------------------------------------
def _both(tmp_path, arc, tag, env=None):
    """-d and -d --gpu-decode over one archive: (host process, device process), files compared."""
    ap = tmp_path / f"{tag}.arc"
    ap.write_bytes(arc)
    e = dict(os.environ, **(env or {}))
    for k in ("SA_DEC_SLICE", "SA_DEC_INFLIGHT"):
        if not env or k not in env:
            e.pop(k, None)
    rh = subprocess.run([CLI, "-d", "-t", "2", str(ap), str(tmp_path / f"{tag}_h")], capture_output=True, text=True, timeout=120)
    rg = subprocess.run([CLI, "-d", "-t", "2", "-v", "--gpu-decode", str(ap), str(tmp_path / f"{tag}_g")], capture_output=True,
                        text=True, timeout=120, env=e)
    assert rg.returncode == rh.returncode, (rh.stderr, rg.stderr)
    outs = sorted(p.name[len(tag) + 2:] for p in tmp_path.glob(f"{tag}_h*"))
    assert outs and outs == sorted(p.name[len(tag) + 2:] for p in tmp_path.glob(f"{tag}_g*")), outs
    for o in outs:
        assert (tmp_path / f"{tag}_h{o}").read_bytes() == (tmp_path / f"{tag}_g{o}").read_bytes(), o
    return rh, rg


@pytest.mark.parametrize("name", ["pair_bin", "pair_tok"])
def test_cli_reference_pair(tmp_path, name):
    c = case(name)
    tmpl = c.tmpl.copy()
    tmpl[0] = c.cfg.bin_mode   # (the archive's name mode is its template's first byte)
    arc = fq.arc_archive(c.enc, c.blocks, "ERR2755197_test_1.fq", "ERR2755197_test_2.fq", tmpl, c.cfg,
                         plus_bare=fq.bare_plus(open(TEST2, "rb").read()))
    rh, rg = _both(tmp_path, arc, name)
    assert rh.returncode == 0, rh.stderr
    assert (tmp_path / f"{name}_g_1.fastq").read_bytes() == open(TEST1, "rb").read()
    assert (tmp_path / f"{name}_g_2.fastq").read_bytes() == open(TEST2, "rb").read()
    assert "sa_decode_blocks: groups 1," in rg.stderr and "the host decodes it" not in rg.stderr, rg.stderr


def test_cli_groups(tmp_path):
    c = case("groups")
    arc = fq.arc_archive(c.enc, c.blocks, "g_1.fq", "g_2.fq", c.tmpl, c.cfg)
    rh, rg = _both(tmp_path, arc, "groups", {"SA_DEC_INFLIGHT": "2"})
    assert rh.returncode == 0, rh.stderr
    assert "inflight 2," in rg.stderr and "groups 3," in rg.stderr, rg.stderr   # (windows of -t 2 blocks: 2 + 2 + 1)


def test_cli_corrupt_block_exits_as_the_host_path(tmp_path):
    c = case("shapes")
    flip = [blk for name, blk, _, _ in corrupt_cases() if name == "qual_flip"][0]
    arc = fq.arc_archive([c.enc[0], flip], [c.blocks[0], c.blocks[0]], "s.fq", None, c.tmpl, c.cfg)
    rh, rg = _both(tmp_path, arc, "flip")
    assert rh.returncode != 0, rh.stderr
    last = lambda r: [ln for ln in r.stderr.splitlines() if "block 1" in ln and "--gpu-decode" not in ln]
    assert last(rh) == last(rg) and last(rh), (rh.stderr, rg.stderr)


def test_cli_lossy_archive_runs_without_the_switch(tmp_path):
    t, _ = synth.generate(300, seed=21)
    blocks = fq.blocks_from_fastq(t)
    cfg = fq.Config(lossy=0.5)
    enc = [oracle_py.encode_block(b, cfg.slevel, cfg.qlevel, cfg.md5, cfg.bin_mode, cfg.lossy) for b in blocks]
    arc = fq.arc_archive(enc, blocks, "l.fq", None, np.zeros(512, np.uint8), cfg, plus_bare=fq.bare_plus(t))
    rh, rg = _both(tmp_path, arc, "lossy")
    assert "--gpu-decode does not apply (the archive was made with -l): running without it" in rg.stderr, rg.stderr
    assert "sa_decode_blocks:" not in rg.stderr
