"""Ordinary gzip inflated on the device (k_gz_find, k_gz_spec, k_gz_chain,
k_gz_resolve and k_gz_crc through sa_gunzip_run, fq.Gunzipper and seqarc_amd
--gpu-gunzip) against Python's zlib, on the fixtures of tests/test_gunzip.py --
which runs the same code on the host, under sanitizers too, before any of it
runs here.  Chunks of 32 KiB (SA_GUNZIP_CHUNK) make the small fixtures many
waves; every test creates its own gunzipper."""
import gzip
import zlib

import numpy as np
import pytest

import synth
import test_gunzip as tg
from test_cli import _run
from test_inflate import bgzf

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu

CANARY = 0x5c


@pytest.fixture
def gz(monkeypatch):
    monkeypatch.setenv("SA_GUNZIP_CHUNK", "32768")
    monkeypatch.delenv("SA_GUNZIP_GRID", raising=False)
    monkeypatch.delenv("SA_GUNZIP_RATIO", raising=False)
    g = fq.Gunzipper(0)
    assert g.chunk == 32768
    yield g
    g.close()


def _total(calls, key):
    return sum(c[key] for c in calls)


@pytest.mark.parametrize("name", ["fq_l1", "fq_l6"])
def test_fastq_matches_zlib(gz, name):
    """(a) the 2 MB fixtures: zlib's bytes, the member's CRC-32 and ISIZE checked; at
    level 6 at least 3/4 of the chunks' waves are confirmed (zlib closes a block
    every 16 Ki symbols at the latest, so every 32 KiB chunk holds a block start:
    13 of 14 in the emulation) -- the text does not come from one wave."""
    z, t = tg.fixtures()[name]
    assert gz.gunzip(z) == t
    assert len(gz.calls) == 1 and gz.last_info["status"] == 0 and gz.last_info["members_ended"] == 1
    assert gz.last_info["chunks"] == -(-len(z) // 32768) and gz.last_kernel_ms > 0
    print(name, gz.last_info)
    if name == "fq_l6":
        assert gz.last_info["waves_confirmed"] >= 3 * gz.last_info["chunks"] / 4, gz.last_info


@pytest.mark.parametrize("name", ["three_members", "sync_flush_100k", "period_32500", "period_32768", "period_40000",
                                  "dist_32768_marker", "marker_chain", "planted_false", "fixed", "level0", "members_30x2k",
                                  "empty_member", "empty_between", "trailing_bytes"])
def test_shapes(gz, name):
    """(b) members with FEXTRA / FNAME headers, pigz's empty stored blocks, matches at
    the largest distances across the chunks, markers copied from markers, a planted
    false candidate; stored-only and fixed-only streams, many small members, an
    empty member, bytes after the last member."""
    z, t = tg.fixtures()[name]
    assert gz.gunzip(z) == t, gz.calls
    want_members = {"three_members": 3, "members_30x2k": 30, "empty_between": 3}.get(name, 1)
    assert _total(gz.calls, "members_ended") == want_members
    if name == "planted_false":
        assert _total(gz.calls, "false_skipped") >= 1
    if name == "members_30x2k":
        assert len(gz.calls) >= 4   # a wave ends eight members at the most


def test_default_chunk_small_grid(monkeypatch, test_pair):
    """(c) the default chunk size on the golden pair (three times over) gzipped, on three workgroups
    (SA_GUNZIP_GRID=3, read at sa_gunzipper_create): every wave takes several
    chunks in turn, reusing its ring and tables."""
    monkeypatch.delenv("SA_GUNZIP_CHUNK", raising=False)
    monkeypatch.setenv("SA_GUNZIP_GRID", "3")
    g = fq.Gunzipper(0)
    try:
        assert g.grid == 3 and g.chunk == 64 << 10
        text = (test_pair[0] + test_pair[1]) * 3   # (the repeats lie further back than the window)
        z = gzip.compress(text, 6, mtime=0)
        assert g.gunzip(z) == text
        assert g.last_info["chunks"] == -(-len(z) // g.chunk) and g.last_info["chunks"] >= 10
        assert g.last_info["waves_confirmed"] >= 3 * g.last_info["chunks"] / 4, g.last_info
    finally:
        g.close()


def _run_all(g, data, cap, slab=None):
    """sa_gunzip_run over the data until the stream ends or fails, every call's
    text behind the last one's in one canary-filled array: (rc, array, text bytes)."""
    out = np.full(cap, CANARY, np.uint8)
    a = np.frombuffer(data, np.uint8)
    slab = slab or a.size
    state = fq.GunzipState()
    at = pos = 0
    carry = np.zeros(0, np.uint8)
    for _ in range(64 + a.size // slab):
        take = min(slab, a.size - at)
        buf = np.concatenate([carry, a[at:at + take]])
        at += take
        rc, ob, used = g.run(buf, state, out[pos:], at == a.size)
        pos += ob
        carry = buf[used:]
        if rc or state.ended or (at == a.size and not carry.size):
            return rc, out, pos
        assert ob or used or take, "no progress"
    raise AssertionError("too many calls")


def test_corrupt_streams(gz):
    """(d) the corrupt set, and valid files between them through the same
    gunzipper: the statuses of the emulation, and no byte of the output array
    past the text a call reports is touched."""
    fx = tg.fixtures()
    for i, (name, data, want) in enumerate(tg.corrupt()):
        rc, out, n = _run_all(gz, data, len(tg.fq_text()) + 4096)
        assert rc > 0 and (want is None or rc == want), (name, rc, gz.last_info)
        assert (out[n:] == CANARY).all(), name
        if name != "flipped_byte":
            assert out[:n].tobytes() == tg.fq_text()[:n], name
        z, t = fx[("fq_l1", "three_members", "planted_false")[i % 3]]
        rc, out, n = _run_all(gz, z, len(t) + 4096)
        assert rc == 0 and out[:n].tobytes() == t and (out[n:] == CANARY).all()
    # out_cap too small for the first wave's text: a call error, nothing written
    out = np.full(1000, CANARY, np.uint8)
    with pytest.raises(fq.SeqArcError, match="out_cap is too small"):
        gz.run(fx["fq_l6"][0], fq.GunzipState(), out)
    assert (out == CANARY).all()


def test_resumption_in_slabs(gz):
    """(e) the level-6 fixture in slabs of 100,000 compressed bytes through the
    state: the whole-buffer run's text; and with an out_cap that cuts the text at
    wave boundaries."""
    z, t = tg.fixtures()["fq_l6"]
    assert gz.gunzip(z, slab=100_000) == t
    assert len(gz.calls) >= len(z) // 100_000
    rc, out, n = _run_all(gz, z, len(t), slab=100_000)
    assert rc == 0 and n == len(t) and out.tobytes() == t
    assert gz.gunzip(z, out_cap=600_000) == t and len(gz.calls) >= 4


# ---- (f) seqarc_amd --gpu-gunzip ----------------------------------------------
def _cli(tmp_path, tag, f1, f2, extra, ingest):
    mode = ["--ingest-only", "--ingest-crc", "-t", "8"] if ingest else ["--batch", "4"]
    r = _run(["-c", "-f", "--block-size", "1"] + mode + extra + ["-1", str(f1)] + (["-2", str(f2)] if f2 else []) +
             ["-o", str(tmp_path / tag)], tmp_path)
    err = r.stderr.decode()
    if r.returncode != 0 or not ingest:
        return r.returncode, err, (tmp_path / f"{tag}.arc").read_bytes() if r.returncode == 0 else None
    crc = [ln for ln in err.splitlines() if "crc32" in ln][0].split()[-1]
    line = [ln for ln in err.splitlines() if "block(s)" in ln][0]
    return 0, err, (crc, line.split()[1], line.split(" -> ")[0].split()[-1])


@pytest.fixture(scope="module")
def pair():
    return synth.generate(40_000, paired=True, seed=65)


def test_cli_ingest(tmp_path, pair):
    """The ingest of a gzip pair with --gpu-gunzip delivers the plain pair's text
    (CRC and block count), at levels 1 and 6; the device path did the work."""
    a, b = pair
    (tmp_path / "p_1.fq").write_bytes(a)
    (tmp_path / "p_2.fq").write_bytes(b)
    rc, _, plain = _cli(tmp_path, "plain", tmp_path / "p_1.fq", tmp_path / "p_2.fq", [], True)
    assert rc == 0
    for lvl in (1, 6):
        (tmp_path / f"l{lvl}_1.fq.gz").write_bytes(gzip.compress(a, lvl, mtime=0))
        (tmp_path / f"l{lvl}_2.fq.gz").write_bytes(gzip.compress(b, lvl, mtime=0))
        rc, log, got = _cli(tmp_path, f"l{lvl}", tmp_path / f"l{lvl}_1.fq.gz", tmp_path / f"l{lvl}_2.fq.gz",
                            ["--gpu-gunzip", "-v"], True)
        assert rc == 0 and got == plain, log
        assert log.count("--gpu-gunzip: ") == 2 and "gunzip kernels" in log and "the host takes over" not in log, log


@pytest.mark.parametrize("kind", ["one", "three", "runs", "stored"])
def test_cli_archives(tmp_path, pair, kind):
    """The archive with the switch is the archive without it: one-member and
    three-member files; a file of enormous ratio and a stored-only file, where the
    host takes over from the state and says so under -v."""
    a, _ = pair
    if kind == "one":
        z = gzip.compress(a, 6, mtime=0)
    elif kind == "three":
        cut = a.index(b"\n@", len(a) // 3) + 1   # (any cut: the members are one stream of text)
        z = gzip.compress(a[:cut], 6, mtime=0) + gzip.compress(a[cut:2 * cut], 1, mtime=0) + gzip.compress(a[2 * cut:], 9, mtime=0)
    elif kind == "runs":
        z = gzip.compress(synth.generate(60, paired=False, seed=67)[0] * 500, 6, mtime=0)
    else:
        z = gzip.compress(a, 0, mtime=0)
    f = tmp_path / f"{kind}_1.fq.gz"
    f.write_bytes(z)
    rc0, _, host = _cli(tmp_path, "host", f, None, [], False)
    rc1, log, dev = _cli(tmp_path, "dev", f, None, ["--gpu-gunzip", "-v"], False)
    assert rc0 == 0 and rc1 == 0 and dev == host, log
    assert "gunzip kernels" in log
    assert ("the host takes over" in log) == (kind in ("runs", "stored")), log


def test_cli_errors_and_routing(tmp_path, pair):
    """A truncated file and a file with a wrong CRC exit non-zero with and without
    the switch; with both switches BGZF still goes through k_inflate_bgzf and a
    one-member gzip through the new path; --gpu-inflate alone keeps its message."""
    a, b = pair
    z = gzip.compress(a, 6, mtime=0)
    bad_crc = bytearray(z)
    bad_crc[-8] ^= 1
    for k, data in (("cut", z[:len(z) * 2 // 3]), ("crc", bytes(bad_crc))):
        f = tmp_path / f"{k}_1.fq.gz"
        f.write_bytes(data)
        for extra in ([], ["--gpu-gunzip"]):
            rc, log, _ = _cli(tmp_path, k, f, None, extra, True)
            assert rc != 0, (k, extra, log)
    (tmp_path / "b_1.fq.gz").write_bytes(bgzf(a))
    (tmp_path / "b_2.fq.gz").write_bytes(bgzf(b))
    both = ["--gpu-inflate", "--gpu-gunzip", "-v"]
    rc, log, got = _cli(tmp_path, "bgzf", tmp_path / "b_1.fq.gz", tmp_path / "b_2.fq.gz", both, True)
    assert rc == 0 and "inflate kernel" in log and "--gpu-gunzip: " not in log, log
    (tmp_path / "one_1.fq.gz").write_bytes(z)
    rc, log, got1 = _cli(tmp_path, "one", tmp_path / "one_1.fq.gz", None, both, True)
    assert rc == 0 and "gunzip kernels" in log and "not BGZF" not in log, log
    rc, log, got0 = _cli(tmp_path, "one_inf", tmp_path / "one_1.fq.gz", None, ["--gpu-inflate", "-v"], True)
    assert rc == 0 and got0 == got1 and "not BGZF, inflating it on the host" in log and "--gpu-gunzip" not in log
