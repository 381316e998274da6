"""BGZF members inflated on the device (k_inflate_bgzf through
sa_inflate_members, fq.Inflater and seqarc_amd --gpu-inflate) against Python's
zlib, on the fixtures of tests/test_inflate.py -- which runs the same per-member
code on the host, the malformed set under sanitizers, before any of it runs
here.  The corrupt-input cases test status reporting."""
import gzip
import zlib

import numpy as np
import pytest

import synth
import test_inflate as ti
from test_cli import _run

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu

CANARY = 0x5c


@pytest.fixture(scope="module")
def inflater():
    f = fq.Inflater(0)
    yield f
    f.close()


def _valid_members():
    return [(cd, len(d), zlib.crc32(d)) for _, cd, d in ti.fixtures()]


def test_valid_fixtures_one_call(inflater):
    """(a) every valid fixture in one call: zlib's bytes, every status 0."""
    fx = ti.fixtures()
    buf, ms, total = ti.pack_members(_valid_members())
    out = np.full(total, CANARY, np.uint8)
    rc, status = inflater.inflate_into(buf, ms, out)
    assert rc == 0 and not status.any(), status
    for (name, _, d), m in zip(fx, ms):
        assert out[int(m["out_off"]):int(m["out_off"]) + len(d)].tobytes() == d, name
    assert inflater.last_kernel_ms > 0


def test_malformed_among_valid(inflater):
    """(b) the malformed set mixed among valid members: the return value counts
    the bad ones, the hand-built ones report their codes, every valid member is
    right and no byte outside the bad members' own output ranges is touched."""
    fx, bad = ti.fixtures(), ti.malformed()
    members, want = [], []   # want: the expected bytes, or (expected status or None)
    for i, (name, cd, isize, crc, st) in enumerate(bad):
        z = ti.zlib_verdict(cd, isize, crc)
        members.append((cd, isize, crc))
        want.append((name, z if z is not None else st, z is None))
        if i % 3 == 0 or i < 8:
            vn, vcd, vd = fx[(i // 3) % len(fx)]
            members.append((vcd, len(vd), zlib.crc32(vd)))
            want.append((vn, vd, False))
    buf, ms, total = ti.pack_members(members)
    out = np.full(total, CANARY, np.uint8)
    expect = np.full(total, CANARY, np.uint8)
    rc, status = inflater.inflate_into(buf, ms, out)
    assert rc == sum(1 for w in want if w[2]) == int(np.count_nonzero(status))
    for (name, w, is_bad), m, st in zip(want, ms, status):
        a, b = int(m["out_off"]), int(m["out_off"]) + int(m["isize"])
        if is_bad:
            assert st != 0 and (w is None or st == w), (name, int(st), w)
            expect[a:b] = out[a:b]   # (a failed member's own range is undefined)
        else:
            assert st == 0, (name, int(st))
            expect[a:b] = np.frombuffer(w, np.uint8)
    assert np.array_equal(out, expect)


@pytest.mark.parametrize("grid", [3, None])
def test_waves_loop_over_members(monkeypatch, grid):
    """(c) 40 members on three waves (SA_INFL_GRID=3, read at sa_inflater_create:
    every wave takes 13 or 14 members in turn, reusing its window and tables) and
    on the default grid."""
    if grid is None:
        monkeypatch.delenv("SA_INFL_GRID", raising=False)
    else:
        monkeypatch.setenv("SA_INFL_GRID", str(grid))
    fx = ti.fixtures()
    members = [(cd, len(d), zlib.crc32(d)) for k in range(40) for _, cd, d in [fx[(k * 3 + k // 11) % len(fx)]]]
    buf, ms, total = ti.pack_members(members)
    f = fq.Inflater(0)
    try:
        assert f.grid == grid if grid else f.grid >= 40
        out, status = f.inflate_members(buf, ms)
    finally:
        f.close()
    assert not status.any(), status
    want = b"".join(zlib.decompressobj(-15).decompress(cd) for cd, _, _ in members)
    assert len(out) == total and out == want


def test_bad_descriptor_is_a_call_error(inflater):
    """(d) a member that points past in_bytes or out_bytes, or is larger than
    64 KiB: a negative return before anything is copied or launched."""
    buf, ms, total = ti.pack_members(_valid_members())
    for field, delta in (("in_off", len(buf)), ("in_len", len(buf)), ("out_off", total), ("isize", 70000)):
        bad = ms.copy()
        bad[field][4] += delta
        out = np.full(total, CANARY, np.uint8)
        with pytest.raises(fq.SeqArcError, match="member 4"):
            inflater.inflate_into(buf, bad, out)
        assert (out == CANARY).all() and inflater.last_kernel_ms == 0, field
    # the last member one byte past the output
    out = np.full(total - 1, CANARY, np.uint8)
    with pytest.raises(fq.SeqArcError, match=f"member {len(ms) - 1}"):
        inflater.inflate_into(buf, ms, out)
    assert (out == CANARY).all()


def test_inflate_bgzf_golden_pair(inflater, test_pair):
    """(e) Inflater.inflate_bgzf on the BGZF of the golden pair; a failed member is named."""
    for text in test_pair:
        assert inflater.inflate_bgzf(ti.bgzf(text, 6)) == text
    z = bytearray(ti.bgzf(test_pair[0][:200000], 1))
    ms, _, _ = fq.bgzf_scan(bytes(z))
    z[int(ms[2]["in_off"]) + 100] ^= 0x40
    with pytest.raises(fq.SeqArcError, match="member 2 failed to inflate: status [1-6]"):
        inflater.inflate_bgzf(bytes(z))
    with pytest.raises(fq.SeqArcError, match="ends inside a member"):
        inflater.inflate_bgzf(ti.bgzf(test_pair[0][:200000])[:-40])


def _ingest(tmp_path, tag, f1, f2, extra):
    r = _run(["-c", "-f", "--ingest-only", "--ingest-crc", "--block-size", "1", "-t", "8"] + extra +
             ["-1", str(f1), "-2", str(f2), "-o", str(tmp_path / tag)], tmp_path)
    assert r.returncode == 0, (tag, r.stderr)
    err = r.stderr.decode()
    crc = [ln for ln in err.splitlines() if "crc32" in ln][0].split()[-1]
    line = [ln for ln in err.splitlines() if "block(s)" in ln][0]
    return crc, line.split()[1], line.split(" -> ")[0].split()[-1]


def test_cli_gpu_inflate(tmp_path):
    """(f) seqarc_amd --gpu-inflate: the ingest of a BGZF pair delivers the plain
    pair's text; the archive is the one the host inflate gives; broken BGZF is
    the same error; a plain gzip file takes the host path."""
    a, b = synth.generate(40_000, paired=True, seed=65)
    files = {"plain": (a, b), "bgzf": (ti.bgzf(a), ti.bgzf(b))}
    for k, (x, y) in files.items():
        (tmp_path / f"{k}_1.fq").write_bytes(x)
        (tmp_path / f"{k}_2.fq").write_bytes(y)
    plain = _ingest(tmp_path, "plain", tmp_path / "plain_1.fq", tmp_path / "plain_2.fq", [])
    gpu = _ingest(tmp_path, "bgzf_gpu", tmp_path / "bgzf_1.fq", tmp_path / "bgzf_2.fq", ["--gpu-inflate", "-v"])
    assert gpu == plain

    def archive(tag, f1, f2, extra):
        args = ["-c", "-f", "--block-size", "1", "--batch", "4"] + extra + ["-1", str(f1)]
        r = _run(args + (["-2", str(f2)] if f2 else []) + ["-o", str(tmp_path / tag)], tmp_path)
        assert r.returncode == 0, (tag, r.stderr)
        return (tmp_path / f"{tag}.arc").read_bytes(), r.stderr.decode()

    host, _ = archive("host", tmp_path / "bgzf_1.fq", tmp_path / "bgzf_2.fq", [])
    dev, log = archive("dev", tmp_path / "bgzf_1.fq", tmp_path / "bgzf_2.fq", ["--gpu-inflate", "-v"])
    assert dev == host
    assert log.count("--gpu-inflate: ") == 2 and "inflate kernel" in log, log
    # BGZF cut inside a member, and with bytes that are no member after the last
    for k, data in (("bgzf_cut", files["bgzf"][0][: len(files["bgzf"][0]) * 2 // 3]),
                    ("bgzf_tail", files["bgzf"][0] + b"\x1f\x8bjunk")):
        bad = tmp_path / f"{k}_1.fq"
        bad.write_bytes(data)
        r = _run(["-c", "-f", "--ingest-only", "--gpu-inflate", "-t", "4", "-1", str(bad), "-o", str(tmp_path / k)],
                 tmp_path)
        assert r.returncode != 0, k
    # a member whose CRC is wrong: the host path's error exit
    ms, _, _ = fq.bgzf_scan(files["bgzf"][0])
    z = bytearray(files["bgzf"][0])
    z[int(ms[3]["in_off"]) + int(ms[3]["in_len"])] ^= 1
    (tmp_path / "crc_1.fq").write_bytes(bytes(z))
    # member 3's trailer zeroed (a hole in the file): ISIZE 0 and CRC 0 in front of data is no empty member
    z = bytearray(files["bgzf"][0])
    end3 = int(ms[3]["in_off"]) + int(ms[3]["in_len"])
    z[end3:end3 + 8] = bytes(8)
    (tmp_path / "hole_1.fq").write_bytes(bytes(z))
    for k in ("crc", "hole"):
        for extra in ([], ["--gpu-inflate"]):
            r = _run(["-c", "-f", "--ingest-only", "-t", "4"] + extra + ["-1", str(tmp_path / f"{k}_1.fq"), "-o",
                                                                          str(tmp_path / k)], tmp_path)
            assert r.returncode != 0, (k, extra)
    # one-member plain gzip: the host path, said under -v, the same archive
    (tmp_path / "one_1.fq.gz").write_bytes(gzip.compress(synth.generate(6000, paired=False, seed=66)[0], 1))
    g0, _ = archive("one", tmp_path / "one_1.fq.gz", None, [])
    g1, log = archive("one_dev", tmp_path / "one_1.fq.gz", None, ["--gpu-inflate", "-v"])
    assert g1 == g0 and "not BGZF, inflating it on the host" in log
