"""The driver of sa_decode_blocks (fastqueeze_amd/csrc/sa_decoder.h: dec_run) on
the host, by tests/cpu_emu/decoder_emu.cpp: the pre-pass, the plan, the groups,
a number of slice launches fixed before the first one, the status of every
block and the MD5 check, over a backend that runs the chains as decode_emu does.
The point of the driver is that it cannot wait without end: a backend that
makes no progress must come back after exactly the computed launches with
SA_DEC_STUCK, under a wall-clock limit.  Built plainly and with
-fsanitize=address,undefined; inputs are test_decode_emu's corpus.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_decode_emu import (LAYOUT, OK, UNSUPPORTED, case, corrupt_cases, emu, equal_to_input, run_emu,  # noqa: F401
                             _emu_block)

import fastqueeze_amd as fq

STUCK = 7
LIMIT_S = 120   # a run that does not return within it has failed (the runs take a second or two)


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    d = tmp_path_factory.mktemp("decoder_emu")
    src = os.path.join(ROOT, "tests", "cpu_emu", "decoder_emu.cpp")
    exe, san = d / "decoder_emu", d / "decoder_emu_san"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-o", str(exe), src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(san), src], check=True)
    return exe, san


def run_drv(exe, tmp_path, tag, cfg, tmpl, slice_, blocks, cap=0, mode="run", lossy=False):
    """blocks: [(bytes, long_reads, cap)] -> (head dict, [(status, md5_ok, nreads)], outdir)."""
    f = tmp_path / f"{tag}.bin"
    f.write_bytes(struct.pack("<iiiiII", -1 if lossy else cfg.slevel, cfg.qlevel, 1 if cfg.md5 else 0, 1 if cfg.bin_mode else 0,
                              slice_, len(blocks)) + np.ascontiguousarray(tmpl, np.uint8).tobytes() +
                  b"".join(struct.pack("<III", len(e), 1 if lg else 0, c) + e for e, lg, c in blocks))
    outdir = tmp_path / f"{tag}_out"
    outdir.mkdir()
    try:
        r = subprocess.run([str(exe), mode, str(f), str(cap), str(outdir)], capture_output=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        pytest.fail(f"decoder_emu {mode} did not return within {LIMIT_S} s")
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    rows = [[int(x) for x in ln.split()] for ln in r.stdout.decode().split("\n")[:-1]]
    head = dict(zip(("rc", "groups", "inflight", "slice", "qual_launches", "seq_launches", "unsupported", "calls"), rows[0]))
    assert len(rows) == 1 + len(blocks)
    return head, [tuple(r) for r in rows[1:]], outdir


def _check_case(exe, tmp_path, name, cap, slice_=1 << 18, tag=None):
    c = case(name)
    head, rows, outdir = run_drv(exe, tmp_path, tag or f"{name}_{cap}", c.cfg, c.tmpl, slice_, list(zip(c.enc, c.long, c.caps)), cap)
    assert head["rc"] == 0 and head["unsupported"] == 0, head
    for i, (blk, row, (hblk, hok)) in enumerate(zip(c.blocks, rows, c.host)):   # input order
        assert row[0] == OK and row[2] == blk.nreads and bool(row[1]) == hok, (name, i, row)
        got = _emu_block(outdir, i, c.caps[i])
        assert equal_to_input(blk, got), (name, i)
        assert got.seq.tobytes() == hblk.seq.tobytes() and got.qual.tobytes() == hblk.qual.tobytes(), (name, i)
    return head


@pytest.mark.parametrize("cap", [1, 2, 0])
@pytest.mark.parametrize("name", ["groups", "shapes", "pair_bin"])
def test_corpus_through_the_driver(drv, tmp_path, name, cap):
    head = _check_case(drv[0], tmp_path, name, cap)
    nb = len(case(name).blocks)
    want = nb if cap == 0 else min(cap, nb)
    assert head["inflight"] == want and head["groups"] == -(-nb // want), head
    if name == "groups" and cap == 2:
        assert head["groups"] == 3, head


@pytest.mark.parametrize("slice_", [61, 4096])
def test_launch_counts_are_computed_from_the_symbol_counts(drv, tmp_path, slice_):
    head = _check_case(drv[0], tmp_path, "shapes", 0, slice_, f"sl{slice_}")
    total = int(case("shapes").blocks[0].seq_lens.sum())
    assert head["slice"] == slice_ and head["qual_launches"] == head["seq_launches"] == -(-total // slice_), head


def test_launch_count_of_a_group_is_its_largest_block(drv, tmp_path):
    c = case("groups")
    head = _check_case(drv[0], tmp_path, "groups", 2, 4096, "g_sl")
    tot = [int(b.seq_lens.sum()) for b in c.blocks]
    want = sum(-(-max(tot[k:k + 2]) // 4096) for k in range(0, 5, 2))
    assert head["qual_launches"] == head["seq_launches"] == want, (head, tot)


def test_stuck_backend_returns_after_the_computed_launches(drv, tmp_path):
    """A device that makes no progress: exactly the computed launches, then SA_DEC_STUCK on
    every block, and the call returns (the subprocess has a wall-clock limit)."""
    c = case("groups")
    blocks = list(zip(c.enc, c.long, c.caps))
    tot = [int(b.seq_lens.sum()) for b in c.blocks]
    for exe, tag in ((drv[0], "stuck"), (drv[1], "stuck_san")):
        head, rows, _ = run_drv(exe, tmp_path, tag, c.cfg, c.tmpl, 4096, blocks, 2, mode="stuck")
        want = sum(-(-max(tot[k:k + 2]) // 4096) for k in range(0, 5, 2))
        assert head["rc"] == 5 and head["groups"] == 3, head
        assert head["qual_launches"] == head["seq_launches"] == want, head
        # per group: alloc, upload, init, chains x 2, place, download, finish, and the launches; free_bytes once
        assert head["calls"] == 1 + 8 * 3 + 2 * want, head
        assert [r[0] for r in rows] == [STUCK] * 5, rows


def test_backend_that_advances_one_block(drv, tmp_path):
    c = case("groups")
    blocks = list(zip(c.enc, c.long, c.caps))
    head, rows, outdir = run_drv(drv[0], tmp_path, "but0", c.cfg, c.tmpl, 4096, blocks, 0, mode="stuck_but0")
    assert head["rc"] == 4 and head["groups"] == 1, head
    assert [r[0] for r in rows] == [OK] + [STUCK] * 4, rows
    assert bool(rows[0][1]) == c.host[0][1] and equal_to_input(c.blocks[0], _emu_block(outdir, 0, c.caps[0]))


def test_corrupt_blocks_beside_a_good_one(drv, emu, tmp_path):
    """Each damaged block gets the status decode_emu gives it, in one group with the good block."""
    c = case("shapes")
    bad = corrupt_cases()
    blocks = [(blk, False, cap) for _, blk, cap, _ in bad[:2]] + [(c.enc[0], False, c.caps[0])] + \
             [(blk, False, cap) for _, blk, cap, _ in bad[2:]]
    r, ref, _ = run_emu(emu[0], tmp_path, "ref", c.cfg, c.tmpl, 4096, blocks)
    assert r.returncode == 0 and len(ref) == len(blocks)
    for exe, tag in ((drv[0], "bad"), (drv[1], "bad_san")):
        head, rows, outdir = run_drv(exe, tmp_path, tag, c.cfg, c.tmpl, 4096, blocks)
        assert head["groups"] == 1 and head["rc"] == sum(1 for row in ref if row[1] != OK), head
        for i, (row, want) in enumerate(zip(rows, ref)):
            assert row[0] == want[1], (i, row, want)
            if want[1] == OK:
                assert row[1] == want[2], (i, row, want)   # (a flipped byte can decode to the end: md5_ok says so)
        assert rows[2][:2] == (OK, int(c.host[0][1])) and equal_to_input(c.blocks[0], _emu_block(outdir, 2, c.caps[0]))
        assert any(row[0] == LAYOUT for row in rows)   # (side_count fails in the pre-pass and never reaches a group)


def test_lossy_config_is_unsupported_without_a_backend_call(drv, tmp_path):
    c = case("shapes")
    head, rows, _ = run_drv(drv[0], tmp_path, "lossy", c.cfg, c.tmpl, 4096, list(zip(c.enc, c.long, c.caps)), lossy=True)
    assert head["rc"] == 1 and head["unsupported"] == 1 and head["calls"] == 0 and head["groups"] == 0, head
    assert rows[0][0] == UNSUPPORTED


def test_under_sanitizers(drv, tmp_path):
    for name, cap, slice_ in (("groups", 2, 1 << 18), ("shapes", 0, 61), ("pair_bin", 0, 1 << 18), ("level_q3", 0, 1 << 18),
                              ("long", 0, 1 << 18)):
        _check_case(drv[1], tmp_path, name, cap, slice_, f"san_{name}")
