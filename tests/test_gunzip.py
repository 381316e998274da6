"""The speculative gzip inflate of fastqueeze_amd/csrc/sa_gunzip.h, run on the
host by tests/cpu_emu/gunzip_emu.cpp (finder, waves, chain, resolve and CRC one
after the other, through the gz_run that sa_gunzip_run is), against Python's
zlib, at chunk sizes of 4, 16 and 64 KiB.  The same program built with address +
undefined-behaviour sanitizers runs every fixture directly: a call's input, its
output and every wave's symbol range are heap blocks of exactly their sizes.
No GPU.

The fixtures (also used by tests/test_gpu_gunzip.py) are the smallest shapes
where the scheme goes wrong; see fixtures() and corrupt()."""
import functools
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import synth
from conftest import ROOT
from test_inflate import BitWriter, _texts, deflate

CHUNKS = (4096, 16384, 65536)
OK, E_INPUT, E_BLOCK, E_CODES, E_DIST, E_SIZE, E_CRC, E_HEADER = range(8)
GZ_FULL, GZ_END, GZ_BREAKS = 17, 18, 19
HDR = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"


def member(raw: bytes, data: bytes, header: bytes = HDR) -> bytes:
    """A gzip member around the raw-deflate bytes of `data`."""
    return header + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def stored(payload: bytes, final: bool = False) -> bytes:
    """One byte-aligned stored block."""
    assert len(payload) <= 0xffff
    return bytes([1 if final else 0]) + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload


@functools.lru_cache(maxsize=None)
def fq_text():
    a, _ = synth.generate(5600, paired=True, seed=78)
    assert 1_900_000 < len(a) < 2_200_000
    return a


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]


def _periodic(period, total, seed):
    """A text of that period, each repeat with ~1 % of its bytes changed, so that
    the matches are short and the blocks many."""
    rng = np.random.default_rng(seed)
    base = _acgt(rng, period)
    parts = []
    for _ in range(total // period + 1):
        base = base.copy()
        at = rng.integers(0, period, period // 100)
        base[at] = _acgt(rng, at.size)
        parts.append(base)
    return np.concatenate(parts)[:total].tobytes()


def _flushed(data, step, mode, level=6):
    """raw deflate of data with a flush of that mode every `step` bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return b"".join(c.compress(data[i:i + step]) + c.flush(mode) for i in range(0, len(data), step)) + c.flush()


@functools.lru_cache(maxsize=None)
def fixtures():
    """{name: (gzip bytes, text)}: the valid files."""
    fq = fq_text()
    small = _texts()[0]
    fx = {}
    for lvl in (1, 6, 9):
        fx[f"fq_l{lvl}"] = (gzip.compress(fq, lvl, mtime=0), fq)
    # three members, one with FEXTRA and FNAME (and FCOMMENT and FHCRC: gz_header_len skips all four)
    third = len(fq) // 3
    parts = [fq[:third], fq[third:2 * third], fq[2 * third:]]
    fancy = (b"\x1f\x8b\x08\x1e\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 6) + b"XY\x02\x00ab" + b"reads_1.fq\0" +
             b"a comment\0" + b"\x12\x34")
    fx["three_members"] = (gzip.compress(parts[0], 6, mtime=0) + member(deflate(parts[1], 6), parts[1], fancy) +
                           gzip.compress(parts[2], 1, mtime=0), fq)
    fx["fixed"] = (member(deflate(small[:300000], 6, zlib.Z_FIXED), small[:300000]), small[:300000])
    fx["level0"] = (member(deflate(small[:300000], 0), small[:300000]), small[:300000])
    fx["sync_flush_100k"] = (member(_flushed(fq, 100_000, zlib.Z_SYNC_FLUSH), fq), fq)   # pigz's shape: empty stored blocks
    # matches at the largest distances zlib emits (32768 - 262), period 32768 and period 40000,
    # in small blocks (a partial flush every 20,000 bytes): every chunk boundary is crossed by far matches
    for period in (32500, 32768, 40000):
        t = _periodic(period, 700_000, period)
        fx[f"period_{period}"] = (member(_flushed(t, 20_000, zlib.Z_PARTIAL_FLUSH, 9), t), t)
    # chunk n copies from chunk n - 1, which copied from n - 2: markers are copied from markers, far
    # past the first 32 Ki symbols of a wave
    t = _periodic(20_000, 1_600_000, 5)
    fx["marker_chain"] = (member(_flushed(t, 120_000, zlib.Z_PARTIAL_FLUSH, 6), t), t)
    # a match at distance exactly 32768 right after a wave's start: a stored block of 32768 bytes,
    # a dynamic block (a candidate) of 20,000 bytes, then a fixed block whose one match of length
    # 258 reaches back 32768: markers 20000 .. 20257, read from the ring slots they are written to
    head, mid = small[:32768], small[40000:60000]
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    w.fixed_litlen(285)
    w.code(29, 5)
    w.bits(32768 - 24577, 13)
    w.fixed_litlen(256)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    t = head + mid + head[20000:20258]
    fx["dist_32768_marker"] = (member(stored(head) + c.compress(mid) + c.flush(zlib.Z_SYNC_FLUSH) + w.done(), t), t)
    # a planted false candidate: a stored block whose payload is a valid non-final dynamic block,
    # starting at byte 65536 of the file -- the first bit of a chunk at every chunk size here
    ta, tc = small[:100_000], small[100_000:400_000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    part_a = c.compress(ta) + c.flush(zlib.Z_FULL_FLUSH)
    part_c = c.compress(tc) + c.flush()
    cp = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = cp.compress(small[400_000:430_000]) + cp.flush(zlib.Z_SYNC_FLUSH)
    assert payload[0] & 7 == 4 and len(payload) < 0xffff
    pad = bytes(65536 - 10 - len(part_a) - 5 - 5)
    raw = part_a + stored(pad) + stored(payload) + part_c
    assert (HDR + raw).index(payload) == 65536
    t = ta + pad + payload + tc
    fx["planted_false"] = (member(raw, t), t)
    # FASTQ, then 8 MB of zeros in the same member: blocks of 4 MB of text that no symbol range
    # holds -- the path leaves in the middle of a stream
    t = small[:300_000] + bytes(8 << 20)
    fx["fq_then_zeros"] = (gzip.compress(t, 6, mtime=0), t)
    fx["zeros_8m"] = (gzip.compress(bytes(8 << 20), 6, mtime=0), bytes(8 << 20))
    t = b"".join(small[i * 2000:(i + 1) * 2000] for i in range(30))
    fx["members_30x2k"] = (b"".join(gzip.compress(small[i * 2000:(i + 1) * 2000], 6, mtime=0) for i in range(30)), t)
    fx["empty_member"] = (gzip.compress(b"", 6, mtime=0), b"")
    fx["empty_between"] = (gzip.compress(small[:50_000], 6, mtime=0) + gzip.compress(b"", 6, mtime=0) +
                           gzip.compress(small[50_000:90_000], 6, mtime=0), small[:90_000])
    fx["trailing_bytes"] = (gzip.compress(small[:50_000], 6, mtime=0) + b"not a member", small[:50_000])
    for name, (z, t) in fx.items():
        if name != "trailing_bytes":
            assert gzip.decompress(z) == t, name
    return fx


@functools.lru_cache(maxsize=None)
def corrupt():
    """[(name, gzip bytes, expected status or None = any non-zero)]; zlib fails on every one."""
    z, t = fixtures()["fq_l6"]
    three = fixtures()["three_members"][0]
    out = []
    b = bytearray(z)
    b[len(z) // 2] ^= 0x5a
    out.append(("flipped_byte", bytes(b), None))
    b = bytearray(z)
    b[-8] ^= 1
    out.append(("crc_wrong", bytes(b), E_CRC))
    b = bytearray(z)
    b[-4] ^= 1
    out.append(("isize_wrong", bytes(b), E_SIZE))
    end0 = len(gzip.compress(fq_text()[:len(fq_text()) // 3], 6, mtime=0))
    b = bytearray(three)
    b[end0 - 7] ^= 0x80   # the first member's CRC, two members before the end
    out.append(("crc_wrong_first_member", bytes(b), E_CRC))
    out.append(("truncated", z[:len(z) * 2 // 3], E_INPUT))
    out.append(("truncated_in_trailer", z[:-3], E_INPUT))
    out.append(("not_gzip", b"@read1\nACGT\n+\nIIII\n" * 100, E_HEADER))
    for name, data, _ in out:
        with pytest.raises((zlib.error, EOFError, gzip.BadGzipFile)):
            gzip.decompress(data)
    return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("gunzip_emu")
    src = os.path.join(ROOT, "tests", "cpu_emu", "gunzip_emu.cpp")
    exe, san = d / "gunzip_emu", d / "gunzip_emu_san"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(san), src], check=True)
    return exe, san


CALL_FIELDS = ("rc", "in_bytes", "in_used", "out_bytes", "chunks", "candidates", "confirmed", "false_skipped", "members",
               "end_wave", "end_why", "late_markers")


def run_emu(exe, tmp_path, data, chunk, ratio=8, slab=0, out_cap=64 << 20, tag="x"):
    """One gunzip_emu run: (calls, (rc, text bytes, file bytes consumed, how), text, state)."""
    f, o, s = tmp_path / f"{tag}.gz", tmp_path / f"{tag}.out", tmp_path / f"{tag}.state"
    f.write_bytes(data)
    r = subprocess.run([str(exe), "run", str(f), str(chunk), str(ratio), str(slab), str(out_cap), str(o), str(s)],
                       capture_output=True)
    assert r.returncode == 0 and (r.stderr == b"" or b"gunzip_emu: sa_gunzip_run" in r.stderr), r.stderr.decode()[-2000:]
    lines = [ln.split() for ln in r.stdout.decode().splitlines()]
    calls = [dict(zip(CALL_FIELDS, map(int, ln[1:]))) for ln in lines if ln[0] == "call"]
    fin = [ln for ln in lines if ln[0] == "final"][0]
    sb = s.read_bytes()
    in_stream, bit, win_len, crc = struct.unpack_from("<IIII", sb, 0)
    state = dict(in_stream=in_stream, bit=bit, win_len=win_len, crc=crc, len=struct.unpack_from("<Q", sb, 16)[0],
                 window=sb[24:24 + 32768])
    return calls, (int(fin[1]), int(fin[2]), int(fin[3]), fin[4]), o.read_bytes(), state


def zlib_resume(rest: bytes, state) -> bytes:
    """What the host does when the device path leaves: the text of the rest of the
    file from a state.  Inside a stream: a raw inflate primed with the bits left
    of the current byte (here: the whole rest shifted down by them) and the
    state's window as its dictionary; the running CRC and length go on and are
    compared with the trailer; the members after it are ordinary gzip."""
    out = b""
    if state["in_stream"]:
        n = int.from_bytes(rest, "little") >> state["bit"]
        shifted = n.to_bytes(len(rest), "little")
        wl = state["win_len"]
        d = zlib.decompressobj(-15, zdict=state["window"][32768 - wl:]) if wl else zlib.decompressobj(-15)
        out = d.decompress(shifted)
        assert d.eof
        used = len(shifted) - len(d.unused_data)   # shifted bytes; the stream ended inside the last of them
        want = struct.pack("<II", zlib.crc32(out, state["crc"]), (state["len"] + len(out)) & 0xffffffff)
        ends = [e for e in (used, used + 1) if rest[e:e + 8] == want]
        assert ends, "the running CRC and length do not continue to the member's trailer"
        rest = rest[ends[0] + 8:]
    else:
        assert state["crc"] == 0 and state["len"] == 0
    while rest[:2] == b"\x1f\x8b":
        d = zlib.decompressobj(31)
        out += d.decompress(rest)
        assert d.eof
        rest = d.unused_data
    return out


def gunzip_all(exe, tmp_path, data, chunk, **kw):
    """The file's text by the emulation, finished by zlib where the path leaves."""
    calls, fin, text, state = run_emu(exe, tmp_path, data, chunk, **kw)
    assert fin[0] == 0 and fin[3] in ("end", "handover"), (fin, calls[-1])
    assert all(c["in_used"] <= c["in_bytes"] for c in calls)
    if fin[3] == "handover":
        text += zlib_resume(data[fin[2]:], state)
    return text, calls, fin


@pytest.mark.parametrize("chunk", CHUNKS)
def test_fixtures_match_zlib(emu, tmp_path, chunk):
    for name, (z, t) in fixtures().items():
        text, calls, fin = gunzip_all(emu[0], tmp_path, z, chunk, tag=name)
        assert text == t, (name, fin, calls[-1])
        members = sum(c["members"] for c in calls)
        if name.startswith("fq_l"):
            # every chunk but a few holds a block start, and the waves meet: the work is spread
            assert fin[3] == "end" and members == 1 and len(calls) == 1
            # (zlib closes a block every 16 Ki symbols at the latest: under 64 KiB of compressed bytes)
            assert calls[0]["confirmed"] >= 3 * min(calls[0]["chunks"], len(z) // 65536) // 4, (name, calls[0])
        if name == "three_members":
            assert fin[3] == "end" and members == 3
        if name == "members_30x2k" and chunk != 16384:
            # the nine-break rule: no call ends more than eight members per confirmed wave
            # (at 16 KiB the file is two chunks and a wave's eight members are less than one:
            # the low-progress rule hands the file to the host)
            assert fin[3] == "end" and members == 30 and len(calls) >= 2
            assert all(c["members"] <= 8 * c["confirmed"] for c in calls)
            assert any(c["end_why"] == GZ_BREAKS for c in calls)
        if name == "marker_chain" and chunk < 65536:
            assert sum(c["late_markers"] for c in calls) > 0, "no marker past a wave's first 32 Ki symbols"
        if name == "planted_false":
            assert sum(c["false_skipped"] for c in calls) >= 1
        if name in ("zeros_8m", "fq_then_zeros") and chunk == 4096:
            assert fin[3] == "handover" and calls[-1]["end_why"] == GZ_FULL, (name, fin, calls[-1])
        if name == "trailing_bytes":
            assert fin[2] == len(z) - len(b"not a member")


def test_handover_state_is_inside_a_stream(emu, tmp_path):
    """FASTQ, then zeros: the device path confirms the FASTQ's blocks, then leaves
    at a block start that is not on a byte boundary, with a window."""
    z, t = fixtures()["fq_then_zeros"]
    calls, fin, text, state = run_emu(emu[0], tmp_path, z, 4096, tag="hz")
    assert fin[3] == "handover" and state["in_stream"] == 1 and state["win_len"] == 32768 and 0 < len(text) < len(t)
    assert state["len"] == len(text) and state["crc"] == zlib.crc32(text)
    assert text + zlib_resume(z[fin[2]:], state) == t


@pytest.mark.parametrize("chunk", CHUNKS)
def test_resumption_in_slabs(emu, tmp_path, chunk):
    """The level-6 fixture in slabs of 100,000 compressed bytes through the state:
    every slab is cut inside a block, the confirmed prefix ends before the cut and
    the rest is carried; the text equals the whole-buffer run's."""
    z, t = fixtures()["fq_l6"]
    calls, fin, text, _ = run_emu(emu[0], tmp_path, z, chunk, slab=100_000, tag="slabs")
    assert fin == (0, len(t), len(z), "end") and text == t
    assert len(calls) >= len(z) // 100_000 and all(c["in_used"] < c["in_bytes"] for c in calls[:-1])
    whole = run_emu(emu[0], tmp_path, z, chunk, tag="whole")[2]
    assert text == whole
    # a small out_cap cuts the text at wave boundaries instead
    calls, fin, text, _ = run_emu(emu[0], tmp_path, z, chunk, out_cap=600_000, tag="cap")
    assert fin == (0, len(t), len(z), "end") and text == t and all(c["out_bytes"] <= 600_000 for c in calls)
    # out_cap too small for the first wave: a call error
    calls, fin, text, _ = run_emu(emu[0], tmp_path, z, chunk, out_cap=1000, tag="tiny")
    assert fin[0] == -2 and fin[3] == "error" and text == b""


def _check_corrupt(exe, tmp_path, chunk):
    for name, data, want in corrupt():
        calls, fin, text, _ = run_emu(exe, tmp_path, data, chunk, tag=name)
        assert fin[3] == "error" and fin[0] > 0 and (want is None or fin[0] == want), (name, chunk, fin, calls[-1])
        if name != "flipped_byte":   # (a flipped byte can decode, to other text, until the CRC tells)
            assert text == fq_text()[:len(text)], name   # what was delivered before the error is the stream's text


@pytest.mark.parametrize("chunk", CHUNKS)
def test_corrupt_input(emu, tmp_path, chunk):
    _check_corrupt(emu[0], tmp_path, chunk)


def test_under_sanitizers(emu, tmp_path):
    """The stand-alone program built with -fsanitize=address,undefined, run
    directly: every fixture and the corrupt set, in slabs too; it must report
    nothing (run_emu asserts an empty stderr) and give the same text."""
    for name, (z, t) in fixtures().items():
        for chunk in (4096, 65536):
            text, _, _ = gunzip_all(emu[1], tmp_path, z, chunk, tag=name)
            assert text == t, (name, chunk)
    _check_corrupt(emu[1], tmp_path, 16384)
    z, t = fixtures()["three_members"]
    calls, fin, text, _ = run_emu(emu[1], tmp_path, z, 16384, slab=100_000, out_cap=700_000, tag="san_slabs")
    assert fin == (0, len(t), len(z), "end") and text == t
