"""Ordinary gzip inflated into text that stays on the device: sa_gunzip_run_dev
through fq.Gunzipper.run_to / gunzip_to into a fq.DevText, against Python's zlib,
Gunzipper.gunzip and the host cut, and seqarc_amd -c --gpu-text --gpu-gunzip
against the same command without switches.  The fixtures are those of
tests/test_gunzip.py, in chunks of 32 KiB; most tests put the devtext's write
position off the 16-byte grid first (k_gz_crc's vector loads assume the text
pointer they get is aligned, so the library must hand the kernels the devtext's
base and add the write position to the offsets).  The input side of the command
line runs on the CPU first, under sanitizers (tests/test_devinput.py)."""
import gzip
import subprocess

import numpy as np
import pytest

import devcut_cases as dc
import synth
import test_gunzip as tg
import test_inflate as ti
from test_cli import EXE

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu

LEAD = b"@lead\nA"   # 7 bytes: the write position leaves the 16-byte grid
INFO_KEYS = ("chunks", "candidates", "waves_confirmed", "false_skipped", "members_ended")


@pytest.fixture
def gz(monkeypatch):
    monkeypatch.setenv("SA_GUNZIP_CHUNK", "32768")
    monkeypatch.delenv("SA_GUNZIP_GRID", raising=False)
    monkeypatch.delenv("SA_GUNZIP_RATIO", raising=False)
    g = fq.Gunzipper(0)
    assert g.chunk == 32768
    yield g
    g.close()


def _fetch_all(dt):
    """Everything the devtext holds, taken out."""
    blk = dt.take(dt.avail)
    try:
        return blk.fetch()[0]
    finally:
        blk.close()


def _total(calls, key):
    return sum(c[key] for c in calls)


@pytest.mark.parametrize("lead", [b"", LEAD], ids=["wr0", "wr7"])
@pytest.mark.parametrize("name", ["fq_l1", "fq_l6"])
def test_off_grid_write_position(gz, name, lead):
    """1. The 2 MB fixtures into a devtext whose write position is 0 / 7: the text
    is zlib's behind the lead, the device cut at 8192 and 65537 gives fq.cut_se's
    lengths (the newline tiles of the appended text are right), and every call
    did what Gunzipper.gunzip's did on the same input."""
    z, t = tg.fixtures()[name]
    assert gz.gunzip(z) == t
    want_calls = [{k: c[k] for k in INFO_KEYS} for c in gz.calls]
    dt = fq.DevText(4 << 20)
    try:
        if lead:
            dt.append(lead)
        assert gz.gunzip_to(dt, z) == len(t) and gz.last_kernel_ms > 0
        assert [{k: c[k] for k in INFO_KEYS} for c in gz.calls] == want_calls
        assert dt.avail == len(lead) + len(t)
        got_lead = b""
        if lead:   # the lead leaves: the read position is off the tile grid, the text is the fixture's
            blk = dt.take(len(lead))
            got_lead = blk.fetch()[0]
            blk.close()
        for bs in (8192, 65537):
            blocks, end = dt.cut(bs, dc.first_line(t), eof=True)
            assert end == fq.CUT_DONE and blocks == [(e - s, 0) for s, e in fq.cut_se(t, bs)], bs
        assert got_lead + _fetch_all(dt) == lead + t
    finally:
        dt.close()


def test_slabs_out_cap_and_compaction(gz):
    """2. The level-6 fixture in slabs of 100,000 compressed bytes, 600,000 text
    bytes a call at most, through a devtext of 1 MiB that is emptied in pieces of
    300,001 bytes between the calls: the unread text moves to the front several
    times, with the read position off the tile grid; the pieces are the text."""
    z, t = tg.fixtures()["fq_l6"]
    a = np.frombuffer(z, np.uint8)
    dt = fq.DevText(1 << 20)
    state = fq.GunzipState()
    pieces, at, carry, appended, ncalls = [], 0, np.zeros(0, np.uint8), 0, 0
    try:
        for _ in range(200):
            while dt.avail >= 300_001:
                blk = dt.take(300_001)
                pieces.append(blk.fetch()[0])
                blk.close()
            take = min(100_000, a.size - at)
            buf = np.concatenate([carry, a[at:at + take]])
            at += take
            assert dt.room >= 600_000
            rc, tb, used = gz.run_to(dt, buf, state, at == a.size, out_cap=600_000)
            assert rc == 0 and tb <= 600_000, gz.last_info
            ncalls += 1
            appended += tb
            carry = buf[used:]
            if state.ended or (at == a.size and not carry.size):
                break
            assert tb or used or take, "no progress"
        else:
            raise AssertionError("too many calls")
        assert appended == len(t) and ncalls >= len(z) // 100_000
        pieces.append(_fetch_all(dt))
        assert len(pieces) >= 6 and b"".join(pieces) == t
    finally:
        dt.close()


SHAPES = ["three_members", "sync_flush_100k", "period_32500", "period_32768", "period_40000", "dist_32768_marker",
          "marker_chain", "planted_false", "fixed", "level0", "members_30x2k", "empty_member", "empty_between",
          "trailing_bytes"]


def test_shapes(gz):
    """3. test_gpu_gunzip.py's shapes one after the other into one devtext through
    one gunzipper, a few bytes of each left unread for the next: each text lands
    behind the last one's, with that test's member counts."""
    dt = fq.DevText(4 << 20)
    try:
        dt.append(LEAD)
        tail = LEAD
        for name in SHAPES:
            z, t = tg.fixtures()[name]
            assert gz.gunzip_to(dt, z) == len(t), (name, gz.calls)
            want_members = {"three_members": 3, "members_30x2k": 30, "empty_between": 3}.get(name, 1)
            assert _total(gz.calls, "members_ended") == want_members, name
            if name == "planted_false":
                assert _total(gz.calls, "false_skipped") >= 1
            have = tail + t
            assert dt.avail == len(have), name
            keep = min(11, len(have))
            blk = dt.take(len(have) - keep)
            got = blk.fetch()[0]
            blk.close()
            assert got == have[:len(have) - keep], name
            tail = have[len(have) - keep:]
        assert _fetch_all(dt) == tail
    finally:
        dt.close()


def test_corrupt_streams(gz):
    """4. The corrupt set: a positive return value (the emulation's where it names
    one), the write position where it was and the text in front of it untouched; a
    valid file through the same gunzipper and devtext afterwards gives its text.
    out_cap above the room is -3, out_cap too small for the first wave an error."""
    fx = tg.fixtures()
    dt = fq.DevText(6 << 20)
    try:
        for i, (name, data, want) in enumerate(tg.corrupt()):
            dt.append(LEAD)
            a = np.frombuffer(data, np.uint8)
            state = fq.GunzipState()
            buf, good = a, 0
            for _ in range(64):
                before = dt.avail
                rc, tb, used = gz.run_to(dt, buf, state, True)
                if rc:
                    break
                good += tb
                buf = buf[used:]
                assert (tb or used) and not state.ended and buf.size, (name, "the stream ended without an error")
            assert rc > 0 and (want is None or rc == want), (name, rc, gz.last_info)
            assert tb == 0 and dt.avail == before == len(LEAD) + good, name
            z, t = fx[("fq_l1", "three_members", "planted_false")[i % 3]]
            assert gz.gunzip_to(dt, z) == len(t), name
            got = _fetch_all(dt)
            assert got[:len(LEAD)] == LEAD and got[len(LEAD) + good:] == t, name
            if name != "flipped_byte":   # (a flipped byte can decode, to other text, until the CRC tells)
                assert got[len(LEAD):len(LEAD) + good] == tg.fq_text()[:good], name
        dt.append(LEAD)
        z, t = fx["fq_l6"]
        assert gz.run_to(dt, z, fq.GunzipState(), out_cap=dt.room + 1)[0] == -3 and dt.avail == len(LEAD)
        with pytest.raises(fq.SeqArcError, match="out_cap is too small"):
            gz.run_to(dt, z, fq.GunzipState(), out_cap=1000)
        assert dt.avail == len(LEAD)
        assert gz.gunzip_to(dt, z) == len(t) and _fetch_all(dt) == LEAD + t
    finally:
        dt.close()


def test_default_chunk_small_grid(monkeypatch, test_pair):
    """5. The default chunk size on three workgroups (SA_GUNZIP_GRID=3) on the golden
    pair tripled and gzipped: every wave of k_gz_crc takes many tasks in turn from
    the devtext."""
    monkeypatch.delenv("SA_GUNZIP_CHUNK", raising=False)
    monkeypatch.setenv("SA_GUNZIP_GRID", "3")
    g = fq.Gunzipper(0)
    text = (test_pair[0] + test_pair[1]) * 3
    dt = fq.DevText(len(text) + 4096)
    try:
        assert g.grid == 3 and g.chunk == 64 << 10
        z = gzip.compress(text, 6, mtime=0)
        dt.append(LEAD)
        assert g.gunzip_to(dt, z) == len(text)
        assert g.last_info["chunks"] >= 10 and g.last_info["waves_confirmed"] >= 3 * g.last_info["chunks"] / 4, g.last_info
        assert _fetch_all(dt) == LEAD + text
    finally:
        dt.close()
        g.close()


def test_stage_and_encode(gz):
    """6. gzip of the golden pair -> gunzip_to per mate -> cut -> take ->
    stage_devblocks -> run -> fetch: the bytes stage_text gives for the same texts."""
    a, b = dc.golden_pair()
    enc = fq.Encoder(0)
    d1, d2 = fq.DevText(len(a) + 4096), fq.DevText(len(b) + 4096)
    try:
        assert gz.gunzip_to(d1, gzip.compress(a, 6, mtime=0)) == len(a)
        assert gz.gunzip_to(d2, gzip.compress(b, 1, mtime=0)) == len(b)
        lens, end = d1.cut(fq.BLOCK_SIZE, dc.first_line(a), mate=d2)
        assert end == fq.CUT_DONE and lens == [(e1 - s1, e2 - s2) for (s1, e1), (s2, e2) in fq.cut_pe(a, b, fq.BLOCK_SIZE)]
        blk0 = fq.parse_pe(a[:lens[0][0]], b[:lens[0][1]])
        cfg = fq.Config(bin_mode=int(fq.analyze_ids(blk0, False)[0]))
        blks, texts, p1, p2 = [], [], 0, 0
        for l1, l2 in lens:
            blks.append(d1.take(l1, d2, l2))
            texts.append((a[p1:p1 + l1], b[p2:p2 + l2]))
            p1 += l1
            p2 += l2
        i_dev = enc.stage_devblocks(blks)
        for x in blks:
            x.close()
        enc.run(cfg)
        dev = enc.fetch()
        i_host = enc.stage_text(texts)
        enc.run(cfg)
        assert i_dev == i_host and dev == enc.fetch() and len(dev) == len(lens) >= 1
    finally:
        d1.close()
        d2.close()
        enc.close()


# ---- 7. the command line: seqarc_amd -c --gpu-text --gpu-gunzip ----------------

BOTH = ["--gpu-text", "--gpu-gunzip", "-v"]


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gunzip_text")
    a, b = dc.synth_pair()   # synth.generate(40_000, paired=True, seed=65)
    for lvl in (1, 6):
        (d / f"l{lvl}_1.fq.gz").write_bytes(gzip.compress(a, lvl, mtime=0))
        (d / f"l{lvl}_2.fq.gz").write_bytes(gzip.compress(b, lvl, mtime=0))
    (d / "bgzf_1.fq.gz").write_bytes(ti.bgzf(a))
    return d, a


def _archive(d, tag, f1, f2, extra, ok=True):
    args = ["-c", "-f", "--block-size", "1", "--batch", "4"] + extra + ["-1", str(d / f1)]
    r = subprocess.run([EXE] + args + (["-2", str(d / f2)] if f2 else []) + ["-o", str(d / tag)], capture_output=True,
                       cwd=d, timeout=120)
    if not ok:
        return r.returncode, r.stderr.decode()
    assert r.returncode == 0, (tag, r.stderr[-2000:])
    return (d / f"{tag}.arc").read_bytes(), r.stderr.decode()


def _lines(log, call):
    return [ln for ln in log.splitlines() if "--gpu-text: " in ln and call in ln]


@pytest.mark.parametrize("lvl", [1, 6])
def test_cli_archive(cli_files, lvl):
    """Both switches on a gzip pair and on its first mate alone: the archive of the
    run without switches; -v names the gunzip path once per input, the switch
    applies and the host never takes over."""
    d, _ = cli_files
    for f2 in (f"l{lvl}_2.fq.gz", None):
        host, _ = _archive(d, f"host{lvl}", f"l{lvl}_1.fq.gz", f2, [])
        dev, log = _archive(d, f"dev{lvl}", f"l{lvl}_1.fq.gz", f2, BOTH)
        assert dev == host, f2
        lines = _lines(log, "sa_gunzip_run_dev")
        assert len(lines) == (2 if f2 else 1) and f"l{lvl}_1.fq.gz" in lines[0] and "gunzip kernels" in lines[0], log
        assert "does not apply" not in log and "the host takes over" not in log, log


def test_cli_mixed_inputs(cli_files):
    """Mate 1 BGZF, mate 2 gzip: the same archive, one -v line of each kind."""
    d, _ = cli_files
    host, _ = _archive(d, "mixhost", "bgzf_1.fq.gz", "l6_2.fq.gz", [])
    dev, log = _archive(d, "mixdev", "bgzf_1.fq.gz", "l6_2.fq.gz", BOTH)
    assert dev == host and "does not apply" not in log, log
    assert len(_lines(log, "sa_inflate_members_dev")) == 1 and len(_lines(log, "sa_gunzip_run_dev")) == 1, log


@pytest.mark.parametrize("kind", ["runs", "stored"])
def test_cli_takeover(cli_files, kind):
    """test_gpu_gunzip.py's file of enormous ratio and its stored-only file: the host
    takes over from the state, says so under -v, and its text reaches the same
    devtext -- the archive is the host path's."""
    d, a = cli_files
    z = (gzip.compress(synth.generate(60, paired=False, seed=67)[0] * 500, 6, mtime=0) if kind == "runs"
         else gzip.compress(a, 0, mtime=0))
    (d / f"{kind}_1.fq.gz").write_bytes(z)
    host, _ = _archive(d, f"{kind}host", f"{kind}_1.fq.gz", None, [])
    dev, log = _archive(d, f"{kind}dev", f"{kind}_1.fq.gz", None, BOTH)
    assert dev == host, log
    assert "the host takes over" in log and len(_lines(log, "sa_gunzip_run_dev")) == 1 and "does not apply" not in log, log


def test_cli_broken_input(cli_files):
    """A file cut at two thirds and a file with a wrong CRC: a non-zero exit with
    both switches, as without them, and no hang."""
    d, a = cli_files
    z = (d / "l6_1.fq.gz").read_bytes()
    crc = bytearray(z)
    crc[-8] ^= 1
    for name, data in (("cut", z[:len(z) * 2 // 3]), ("crc", bytes(crc))):
        (d / f"{name}_1.fq.gz").write_bytes(data)
        for extra in ([], BOTH):
            rc, log = _archive(d, name, f"{name}_1.fq.gz", None, extra, ok=False)
            assert rc != 0, (name, extra, log[-500:])
