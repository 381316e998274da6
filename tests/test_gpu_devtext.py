"""Text resident on the device (sa_devtext.hip): fq.DevText / fq.DevBlock,
Inflater.inflate_to and Encoder.stage_devblocks against the host cut
(sa_cut_next_se / sa_cut_next_pe), the texts themselves and Encoder.stage_text,
and seqarc_amd -c --gpu-text against the same command without the switch.
The cut's logic runs on the CPU first, under sanitizers (tests/test_devcut.py:
the same sa_devcut.h functions, the same inputs from tests/devcut_cases.py)."""
import gzip
import subprocess

import pytest

import devcut_cases as dc
import oracle_py
import synth
import test_inflate as ti
from test_cli import EXE

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def synth_dev():
    """The synthetic pair appended whole, once: cuts do not consume."""
    a, b = dc.synth_pair()
    d1, d2 = fq.DevText(len(a)), fq.DevText(len(b))
    d1.append(a)
    d2.append(b)
    assert d1.avail == len(a) and d1.room == 0
    yield d1, d2
    d1.close()
    d2.close()


@pytest.fixture(scope="module")
def synth_ref():
    """fq.cut_pe / fq.cut_se of the synthetic pair per block size: block lengths."""
    a, b = dc.synth_pair()
    out = {}
    for bs in dc.BLOCK_SIZES[:4]:
        out[(bs, True)] = [(e1 - s1, e2 - s2) for (s1, e1), (s2, e2) in fq.cut_pe(a, b, bs)]
        out[(bs, False)] = [(e - s, 0) for s, e in fq.cut_se(a, bs)]
    return out


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("bi", range(4))
def test_whole_input(synth_dev, synth_ref, bi, pe):
    """1. The synthetic pair in one devtext per mate, one cut call: every length
    is fq.cut_pe's / fq.cut_se's."""
    bs = dc.BLOCK_SIZES[bi]
    d1, d2 = synth_dev
    first = dc.first_line(dc.synth_pair()[0])
    assert d1.peek(0, len(first)) == first
    blocks, end = d1.cut(bs, first, mate=d2 if pe else None)
    want = synth_ref[(bs, pe)]
    assert len(want) == (dc.SYNTH_PE if pe else dc.SYNTH_SE)[bi]
    assert end == fq.CUT_DONE and blocks == want
    count_ms, cut_ms = d1.kernel_ms
    assert count_ms > 0 and cut_ms > 0


@pytest.mark.parametrize("pe", [True, False])
@pytest.mark.parametrize("bs", [8192, 65537, 1048576])
def test_pieces(synth_ref, bs, pe):
    """2. 300,001-byte pieces through a 3 MiB devtext, cut and take after each
    piece ('more', the move to the front, read positions off the tile grid): the
    blocks are the whole input's, and the last block's text is the input's end."""
    a, b = dc.synth_pair()
    first = dc.first_line(a)
    d1, d2 = fq.DevText(dc.PIECE_CAP), fq.DevText(dc.PIECE_CAP)
    fed = [0, 0]
    got, ends, blk = [], set(), None
    try:
        while True:
            progress = 0
            for i, (d, t) in enumerate(((d1, a), (d2, b))[: 2 if pe else 1]):
                n = min(dc.PIECE, len(t) - fed[i], d.room)
                d.append(t[fed[i]:fed[i] + n])
                fed[i] += n
                progress += n
            e1, e2 = fed[0] == len(a), fed[1] == len(b)
            while True:
                blocks, end = d1.cut(bs, first, eof=e1, mate=d2 if pe else None, mate_eof=e2, max_blocks=7)
                ends.add(end)
                for l1, l2 in blocks:
                    if blk is not None:
                        blk.close()
                    blk = d1.take(l1, d2 if pe else None, l2)
                got += blocks
                progress += len(blocks)
                if end != fq.CUT_FULL:
                    break
            if end in (fq.CUT_DONE, fq.CUT_NONE) or not progress:
                break
        assert end == fq.CUT_DONE and got == synth_ref[(bs, pe)]
        # (a 300,001-byte piece holds more than seven 8 KiB blocks, so those calls stop at max_blocks)
        assert fq.CUT_MORE in ends and (bs != 8192 or fq.CUT_FULL in ends)
        t1, t2 = blk.fetch()
        assert t1 == a[len(a) - got[-1][0]:] and (not pe or t2 == b[len(b) - got[-1][1]:])
        assert d1.avail == 0 and d1.room == dc.PIECE_CAP
    finally:
        if blk is not None:
            blk.close()
        d1.close()
        d2.close()


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c["name"])
def test_hand_built(case):
    """3. The hand-built cases of the CPU test: one cut call, the host cut's answer."""
    t1, t2 = case["t1"], case["t2"]
    want, wend = dc.host_cut(fq, t1, t2, case["bs"], case["eof"], case["max_blocks"])
    if case["end"] is not None:
        assert wend == case["end"]
    if case["blocks"] is not None:
        assert len(want) == case["blocks"]
    d1 = fq.DevText(max(len(t1), 16))
    d2 = fq.DevText(max(len(t2), 16)) if t2 is not None else None
    try:
        d1.append(t1)
        if t2:
            d2.append(t2)
        got, end = d1.cut(case["bs"], dc.first_line(t1), eof=case["eof"], mate=d2, max_blocks=case["max_blocks"])
        assert (got, end) == (want, wend)
    finally:
        d1.close()
        if d2 is not None:
            d2.close()


@pytest.mark.parametrize("level", [6, 1])
def test_inflate_into_devtext(level):
    """4. BGZF members inflated straight into a devtext whose write position is
    off the 16-byte grid: take + fetch give the text; a member with a flipped
    byte gives a status and leaves avail alone; too many members give -3."""
    text = dc.synth_pair()[0][:3_000_000]
    z = ti.bgzf(text, level)
    ms, consumed, total = fq.bgzf_scan(z)
    assert consumed == len(z) and total == len(text)
    inf = fq.Inflater(0)
    dt = fq.DevText(len(text) + 600_000)
    try:
        lead = b"@lead\nAC\n+\nII\n"[:13]
        dt.append(lead)
        half = len(ms) // 2   # two calls: the second starts where the first ended
        rc, status = inf.inflate_to(dt, z, ms[:half])
        assert rc == 0 and not status.any() and inf.last_kernel_ms > 0
        rc, status = inf.inflate_to(dt, z, ms[half:])
        assert rc == 0 and not status.any()
        assert dt.avail == len(lead) + len(text)
        blk = dt.take(dt.avail)
        assert blk.fetch() == (lead + text, None)
        blk.close()
        # the newline counts of inflated text: the cut agrees with the host's
        rc, _ = inf.inflate_to(dt, z, ms)
        assert rc == 0
        first = dc.first_line(text)
        got, end = dt.cut(65537, first, eof=True)
        assert (got, end) == dc.host_cut(fq, text, None, 65537, True, 4096)
        # a flipped byte inside member 3's deflate stream
        bad = bytearray(z)
        bad[int(ms[3]["in_off"]) + 100] ^= 0x40
        before = dt.avail
        rc, status = inf.inflate_to(dt, bytes(bad), ms[:8])
        assert rc >= 1 and status[3] != 0 and dt.avail == before
        # more text than the room
        assert dt.room < total
        rc, _ = inf.inflate_to(dt, z, ms)
        assert rc == -3 and dt.avail == before
        assert dt.peek(0, len(first)) == first
    finally:
        dt.close()
        inf.close()


def _blocks_both_ways(enc, cfg, a, b, bs, batch):
    """The pair cut on the device and taken as devblocks, staged in batches by
    stage_devblocks, and the same texts from the host by stage_text."""
    first = dc.first_line(a)
    d1, d2 = fq.DevText(len(a)), fq.DevText(len(b))
    out_dev, out_host = [], []
    try:
        d1.append(a)
        d2.append(b)
        lens, end = d1.cut(bs, first, mate=d2)
        assert end == fq.CUT_DONE
        p1 = p2 = 0
        for i in range(0, len(lens), batch):
            blks, texts = [], []
            for l1, l2 in lens[i:i + batch]:
                blks.append(d1.take(l1, d2, l2))
                texts.append((a[p1:p1 + l1], b[p2:p2 + l2]))
                p1 += l1
                p2 += l2
            i_dev = enc.stage_devblocks(blks, slot=(i // batch) & 1)
            for x in blks:
                x.close()
            enc.run(cfg)
            out_dev += enc.fetch()
            i_host = enc.stage_text(texts)
            enc.run(cfg)
            out_host += enc.fetch()
            assert i_dev == i_host
        return out_dev, out_host, (a[:lens[0][0]], b[:lens[0][1]])
    finally:
        d1.close()
        d2.close()


def test_stage_and_encode():
    """5. stage_devblocks + run + fetch give the bytes stage_text gives for the
    same texts: the golden pair in one block, the synthetic pair at 1 MiB in
    batches of 4; block 0 also equals the oracle."""
    enc = fq.Encoder(0)
    try:
        for (a, b), bs, batch, nblocks in ((dc.golden_pair(), fq.BLOCK_SIZE, 1, 1), (dc.synth_pair(), 1 << 20, 4, 28)):
            blk0 = fq.parse_pe(*[t[:n] for t, n in zip((a, b), [e - s for s, e in fq.cut_pe(a, b, bs)[0]])])
            cfg = fq.Config(bin_mode=int(fq.analyze_ids(blk0, False)[0]))
            dev, host, _ = _blocks_both_ways(enc, cfg, a, b, bs, batch)
            assert len(dev) == nblocks and dev == host
            assert dev[0] == oracle_py.encode_block(blk0, cfg.slevel, cfg.qlevel, cfg.md5, cfg.bin_mode)
    finally:
        enc.close()


# ---- the command line: seqarc_amd -c --gpu-text ------------------------------

@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_text")
    a, b = dc.synth_pair()
    z1, z2 = ti.bgzf(a), ti.bgzf(b)
    for name, data in (("bgzf_1.fq.gz", z1), ("bgzf_2.fq.gz", z2), ("plain_1.fq", a), ("plain_2.fq", b),
                       ("one_1.fq.gz", gzip.compress(synth.generate(6000, paired=False, seed=66)[0], 1))):
        (d / name).write_bytes(data)
    return d, z1


def _archive(d, tag, f1, f2, extra):
    args = ["-c", "-f", "--block-size", "1", "--batch", "4"] + extra + ["-1", str(d / f1)]
    r = subprocess.run([EXE] + args + (["-2", str(d / f2)] if f2 else []) + ["-o", str(d / tag)], capture_output=True,
                       cwd=d, timeout=120)
    assert r.returncode == 0, (tag, r.stderr[-2000:])
    return (d / f"{tag}.arc").read_bytes(), r.stderr.decode()


def test_cli_archive(cli_files):
    """6. --gpu-text on the BGZF of the synthetic pair writes the archive the same
    command writes without the switch, PE and SE; -v names the path for every input."""
    d, _ = cli_files
    for f2 in ("bgzf_2.fq.gz", None):
        host, _ = _archive(d, "host", "bgzf_1.fq.gz", f2, [])
        dev, log = _archive(d, "dev", "bgzf_1.fq.gz", f2, ["--gpu-text", "-v"])
        assert dev == host, f2
        lines = [ln for ln in log.splitlines() if "--gpu-text: " in ln and "member(s)" in ln]
        assert len(lines) == (2 if f2 else 1) and "bgzf_1.fq.gz" in lines[0], log
        assert "does not apply" not in log


def test_cli_inputs_the_switch_cannot_take(cli_files):
    """7. A plain pair and a one-member gzip file: the archives of a run without
    the switch, and -v says that it does not apply; with --ingest-only a usage error."""
    d, _ = cli_files
    for f1, f2 in (("plain_1.fq", "plain_2.fq"), ("one_1.fq.gz", None)):
        host, _ = _archive(d, "host", f1, f2, [])
        dev, log = _archive(d, "dev", f1, f2, ["--gpu-text", "-v"])
        assert dev == host and "--gpu-text does not apply" in log, f1
    r = subprocess.run([EXE, "-c", "-f", "--ingest-only", "--gpu-text", "-1", str(d / "bgzf_1.fq.gz"), "-o", str(d / "u")],
                       capture_output=True, cwd=d, timeout=60)
    assert r.returncode != 0 and b"usage:" in r.stderr and b"--gpu-text" in r.stderr


def test_cli_broken_input(cli_files):
    """8. A BGZF file cut inside a member, junk after the last member, a wrong
    CRC and a zeroed trailer: a non-zero exit each, as on the host path, and no hang."""
    d, z = cli_files
    ms, _, _ = fq.bgzf_scan(z)
    crc = bytearray(z)
    crc[int(ms[3]["in_off"]) + int(ms[3]["in_len"])] ^= 1
    # member 3's trailer zeroed (a hole in the file): ISIZE 0 and CRC 0 in front of data is no empty member
    end3 = int(ms[3]["in_off"]) + int(ms[3]["in_len"])
    hole = z[:end3] + bytes(8) + z[end3 + 8:]
    for name, data in (("cut", z[: len(z) * 2 // 3]), ("tail", z + b"\x1f\x8bjunk"), ("crc", bytes(crc)), ("hole", hole)):
        (d / f"{name}_1.fq.gz").write_bytes(data)
        for extra in ([], ["--gpu-text"]):
            r = subprocess.run([EXE, "-c", "-f", "--block-size", "1", "--batch", "4"] + extra +
                               ["-1", str(d / f"{name}_1.fq.gz"), "-o", str(d / name)], capture_output=True, cwd=d, timeout=60)
            assert r.returncode != 0, (name, extra, r.stderr[-500:])
