"""The per-member inflate of fastqueeze_amd/csrc/sa_inflate.h, run on the host
by tests/cpu_emu/inflate_emu.cpp, against Python's zlib: every fixture is first
inflated with zlib.decompressobj(-15); a valid member must give zlib's bytes, a
malformed one must fail exactly where zlib raises, stops short of the stream's
end, or disagrees with the member's ISIZE / CRC-32.  The malformed set also
runs through an address + undefined-behaviour sanitizer build of the same
stand-alone program, which must report nothing.  No GPU.

The fixtures (also used by tests/test_gpu_inflate.py) are the smallest shapes
where a decoder goes wrong; see fixtures() and malformed()."""
import ctypes
import functools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import synth
from conftest import ROOT

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MEMBER_DTYPE = np.dtype([("in_off", "<u8"), ("in_len", "<u4"), ("out_off", "<u8"), ("isize", "<u4"), ("crc", "<u4")],
                        align=True)
OK, E_INPUT, E_BLOCK, E_CODES, E_DIST, E_SIZE, E_CRC = range(7)


# ---- a BGZF writer (the construction of _bgzf in tests/test_cli.py) ---------
def bgzf_member(cd: bytes, isize: int, crc: int) -> bytes:
    """One BGZF member around the raw-deflate bytes cd."""
    assert 18 + len(cd) + 8 - 1 <= 0xffff, "BSIZE does not fit"
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(cd) + 8 - 1) + cd +
            struct.pack("<II", crc, isize))


def bgzf(data: bytes, level: int = 1, chunk: int = 65280) -> bytes:
    out = bytearray()
    for i in range(0, len(data), chunk):
        part = data[i:i + chunk]
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out += bgzf_member(c.compress(part) + c.flush(), len(part), zlib.crc32(part))
    return bytes(out) + EOF_MEMBER


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


class BitWriter:
    """DEFLATE's bit order: fields lowest bit first, Huffman codes highest bit first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        self.bits(int(format(c, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def fixed_litlen(self, sym):
        if sym < 144:
            self.code(0x30 + sym, 8)
        elif sym < 256:
            self.code(0x190 + sym - 144, 9)
        elif sym < 280:
            self.code(sym - 256, 7)
        else:
            self.code(0xc0 + sym - 280, 8)

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


def zlib_verdict(cd: bytes, isize: int, crc: int):
    """The member's bytes if zlib inflates cd to the end of its stream and the
    result has the member's size and CRC-32; None otherwise."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(cd) + d.flush()
    except zlib.error:
        return None
    if not d.eof or len(out) != isize or zlib.crc32(out) != crc:
        return None
    return out


def dynamic_code_lengths(cd: bytes):
    """The literal/length and distance code lengths of cd's first block, which
    must be a dynamic one (RFC 1951, 3.2.7)."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((cd[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    bits(1)
    assert bits(2) == 2, "not a dynamic block"
    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = bits(3)
    codes, code = {}, 0
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c = ln = 0
        while (ln, c) not in codes:
            assert ln < 7
            c, ln = c << 1 | bits(1), ln + 1
        s = codes[(ln, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + bits(2))
        elif s == 17:
            lens += [0] * (3 + bits(3))
        else:
            lens += [0] * (11 + bits(7))
    return lens[:hlit], lens[hlit:hlit + hdist]


@functools.lru_cache(maxsize=None)
def _texts():
    a, _ = synth.generate(1500, paired=True, seed=77)
    assert len(a) >= 65536
    rng = np.random.default_rng(7)
    skew = np.minimum(rng.geometric(0.5, 65280 - 16) - 1, 15).astype(np.uint8).tobytes() + bytes(range(16))
    rnd = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
    return a, skew, rnd


@functools.lru_cache(maxsize=None)
def fixtures():
    """[(name, deflate bytes, data)]: the valid members (the issue's list, in its order)."""
    fq_text, skew, rnd = _texts()
    out = [("eof", b"\x03\x00", b"")]
    out.append(("stored_1", deflate(b"Q", 0), b"Q"))
    out.append(("stored_65280", deflate(fq_text[:65280], 0), fq_text[:65280]))
    out.append(("fixed", deflate(fq_text[:40000], 6, zlib.Z_FIXED), fq_text[:40000]))
    out.append(("dynamic_l9", deflate(fq_text[:65280], 9), fq_text[:65280]))
    out.append(("rle", deflate(b"A" * 65280, 6, zlib.Z_RLE), b"A" * 65280))
    out.append(("huffman_only_long_codes", deflate(skew, 6, zlib.Z_HUFFMAN_ONLY), skew))
    out.append(("random_l6", deflate(rnd, 6), rnd))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    cd = b"".join(c.compress(fq_text[i:i + 7000]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, 60000, 7000))
    out.append(("full_flush_7000", cd + c.flush(), fq_text[:63000]))
    # a stored block of 32768 bytes, then a fixed block: one match of length 258 at distance 32768
    head = fq_text[:32768]
    w = BitWriter()
    w.bits(0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(32768, 16)
    w.bits(32768 ^ 0xffff, 16)
    w.out += head
    w.bits(1, 1)
    w.bits(1, 2)
    w.fixed_litlen(285)
    w.code(29, 5)
    w.bits(32768 - 24577, 13)
    w.fixed_litlen(256)
    out.append(("dist_32768", w.done(), head + head[:258]))
    acgt = (b"ACGTTGCA" * 8192)[:65536]
    out.append(("isize_65536", deflate(acgt, 6), acgt))
    for name, cd, data in out:
        assert zlib_verdict(cd, len(data), zlib.crc32(data)) == data, name
        assert len(cd) + 26 <= 65536, name
    # the long-code fixture does have codes beyond the primary table's 10 bits (its rarest bytes
    # occur a few times in 65280: the canonical walk decodes them) and the stored fall-back is
    # what zlib chose for random bytes
    assert out[6][0] == "huffman_only_long_codes" and max(dynamic_code_lengths(out[6][1])[0]) > 10
    assert out[7][1][0] & 6 == 0 and len(out[7][1]) > 65280
    return out


@functools.lru_cache(maxsize=None)
def malformed():
    """[(name, deflate bytes, isize, crc, expected status or None)]: None = any
    non-zero status, provided zlib fails too; the seeded corruptions may also
    turn out valid (then zlib's bytes are expected)."""
    fx = {n: (cd, d) for n, cd, d in fixtures()}
    cd4, d4 = fx["dynamic_l9"]
    cd3, d3 = fx["fixed"]
    out = [("cut_short", cd4[:len(cd4) // 2], len(d4), zlib.crc32(d4), E_INPUT)]
    st = bytearray(fx["stored_1"][0])
    st[3] ^= 0x10   # NLEN
    out.append(("len_nlen", bytes(st), 1, zlib.crc32(b"Q"), E_BLOCK))
    out.append(("btype3", b"\x07\x00\x00", 1, 0, E_BLOCK))
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    w.fixed_litlen(257)
    w.code(0, 5)
    w.fixed_litlen(256)
    out.append(("match_first", w.done(), 3, 0, E_DIST))
    out.append(("isize_plus", cd3, len(d3) + 1, zlib.crc32(d3), E_SIZE))
    out.append(("isize_minus", cd3, len(d3) - 1, zlib.crc32(d3), E_SIZE))
    # a zeroed trailer in front of data: an ISIZE 0 member is inflated too, and produces a byte it has no room for
    out.append(("isize_zero", cd3, 0, 0, E_SIZE))
    out.append(("crc_wrong", cd3, len(d3), zlib.crc32(d3) ^ 0x8000, E_CRC))
    rng = np.random.default_rng(11)
    for name in ("fixed", "dynamic_l9", "full_flush_7000"):
        cd, d = fx[name]
        for k in range(200):
            at = int(rng.integers(0, len(cd)))
            b = bytearray(cd)
            b[at] ^= int(rng.integers(1, 256))
            out.append((f"{name}_corrupt{k}@{at}", bytes(b), len(d), zlib.crc32(d), None))
    for name, cd, isize, crc, want in out:
        if want is not None:
            assert zlib_verdict(cd, isize, crc) is None, name
    return out


def members_blob(members):
    """The input file of `inflate_emu members`: [(deflate bytes, isize, crc)]."""
    return struct.pack("<I", len(members)) + b"".join(struct.pack("<III", len(cd), isize, crc) + cd
                                                      for cd, isize, crc in members)


def pack_members(members):
    """One input buffer and the sa_bgzf_member array for [(deflate bytes, isize, crc)]:
    the members back to back with odd gaps, outputs back to back."""
    buf = bytearray()
    ms = np.zeros(len(members), MEMBER_DTYPE)
    out_off = 0
    for i, (cd, isize, crc) in enumerate(members):
        buf += b"\xee" * (i % 5)
        ms[i] = (len(buf), len(cd), out_off, isize, crc)
        buf += cd
        out_off += isize
    return bytes(buf), ms, out_off


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_emu")
    src = os.path.join(ROOT, "tests", "cpu_emu", "inflate_emu.cpp")
    exe, san = d / "inflate_emu", d / "inflate_emu_san"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(san), src], check=True)
    return exe, san


def _run_members(exe, tmp_path, members, tag):
    f = tmp_path / f"{tag}.bin"
    f.write_bytes(members_blob(members))
    outdir = tmp_path / f"{tag}_out"
    outdir.mkdir()
    r = subprocess.run([str(exe), "members", str(f), str(outdir)], capture_output=True)
    lines = r.stdout.decode().split("\n")[:-1]
    return r, [ln.split() for ln in lines], outdir


def test_valid_fixtures_match_zlib(emu, tmp_path):
    fx = fixtures()
    r, rows, outdir = _run_members(emu[0], tmp_path, [(cd, len(d), zlib.crc32(d)) for _, cd, d in fx], "valid")
    assert r.returncode == 0 and len(rows) == len(fx), r.stderr
    for i, ((name, cd, d), row) in enumerate(zip(fx, rows)):
        assert row[0] == "0", (name, row)
        if d:
            # the serial CRC of the output, and the CRC combined from the 64 lane shares
            assert int(row[1], 16) == int(row[2], 16) == zlib.crc32(d), (name, row)
            assert (outdir / str(i)).read_bytes() == d, name


def _check_malformed(rows, outdir):
    bad = malformed()
    assert len(rows) == len(bad)
    n_valid = 0
    for i, ((name, cd, isize, crc, want), row) in enumerate(zip(bad, rows)):
        z = zlib_verdict(cd, isize, crc)
        st = int(row[0])
        if want is not None:
            assert st == want, (name, row)
        elif z is None:
            assert st != 0, (name, row)
        else:
            n_valid += 1
            assert st == 0 and (outdir / str(i)).read_bytes() == z, (name, row)
    return n_valid


def test_malformed_fail_where_zlib_fails(emu, tmp_path):
    r, rows, outdir = _run_members(emu[0], tmp_path, [m[1:4] for m in malformed()], "bad")
    assert r.returncode == 0, r.stderr
    _check_malformed(rows, outdir)


def test_malformed_under_sanitizers(emu, tmp_path):
    """The stand-alone program built with -fsanitize=address,undefined: every
    member's input and output are heap blocks of exactly their sizes, so a read
    or write outside them, or any undefined shift or overflow, is reported."""
    r, rows, outdir = _run_members(emu[1], tmp_path, [m[1:4] for m in malformed()], "san")
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    _check_malformed(rows, outdir)
    fx = fixtures()
    r, rows, _ = _run_members(emu[1], tmp_path, [(cd, len(d), zlib.crc32(d)) for _, cd, d in fx], "san_valid")
    assert r.returncode == 0 and r.stderr == b"" and [x[0] for x in rows] == ["0"] * len(fx), r.stderr.decode()[-2000:]


# ---- sa_bgzf_scan ------------------------------------------------------------
def _scan_emu(exe, tmp_path, data, maxm, max_isize=None):
    f = tmp_path / "scan.bin"
    f.write_bytes(data)
    r = subprocess.run([str(exe), "scan", str(f), str(maxm)] + ([str(max_isize)] if max_isize is not None else []),
                       capture_output=True, check=True)
    lines = r.stdout.decode().split("\n")[:-1]
    ret, consumed, out_bytes = map(int, lines[0].split())
    return ret, consumed, out_bytes, [tuple(map(int, ln.split())) for ln in lines[1:]]


def _scan_lib(data, maxm):
    from fastqueeze_amd import build as b
    if not os.path.exists(b.LIB):
        return None
    lib = ctypes.CDLL(b.LIB)
    if not hasattr(lib, "sa_bgzf_scan"):
        return None
    lib.sa_bgzf_scan.restype = ctypes.c_int64
    lib.sa_bgzf_scan.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                 ctypes.c_void_p]
    ms = np.zeros(max(1, maxm), MEMBER_DTYPE)
    buf = np.frombuffer(data + b"\0", np.uint8)
    consumed, out_bytes = ctypes.c_uint64(0), ctypes.c_uint64(0)
    ret = lib.sa_bgzf_scan(buf.ctypes.data, len(data), ms.ctypes.data, maxm, ctypes.byref(consumed),
                           ctypes.byref(out_bytes))
    return ret, consumed.value, out_bytes.value, [tuple(int(x) for x in m) for m in ms[:max(ret, 0)]]


def test_bgzf_scan(emu, tmp_path):
    text = _texts()[0][:150000]
    whole = bgzf(text)
    want = []
    p = out = 0
    for i in range(0, len(text), 65280):
        part = text[i:i + 65280]
        bsize = struct.unpack_from("<H", whole, p + 16)[0] + 1
        want.append((p + 18, bsize - 26, out, len(part), zlib.crc32(part)))
        p += bsize
        out += len(part)
    want.append((p + 18, 2, out, 0, 0))
    assert p + 28 == len(whole)
    no_bc = bytearray(whole)
    no_bc[12:14] = b"XY"
    cut = len(whole) - 28 - 1000   # inside the third member
    cases = [("whole", whole, 16, (4, len(whole), len(text), want)),
             ("exact_max", whole, 4, (4, len(whole), len(text), want)),
             ("cut_in_member", whole[:cut], 16, (2, want[2][0] - 18, 2 * 65280, want[:2])),
             ("cut_in_header", whole[:want[2][0] - 18 + 7], 16, (2, want[2][0] - 18, 2 * 65280, want[:2])),
             ("empty", b"", 16, (0, 0, 0, [])),
             ("junk_after", whole + b"\x1f\x8bjunk", 16, -1),
             ("junk_after_long", whole + b"not a gzip member at all....", 16, -1),
             ("no_bc", bytes(no_bc), 16, -1),
             ("max_members_small", whole, 3, -3)]
    for name, data, maxm, expect in cases:
        for how, got in (("emu", _scan_emu(emu[0], tmp_path, data, maxm)), ("lib", _scan_lib(data, maxm))):
            if got is None:
                continue
            if isinstance(expect, int):
                assert got[0] == expect, (name, how, got[:3])
            else:
                assert got == expect, (name, how, got[:3])


def test_bgzf_scan_isize_limit(emu, tmp_path):
    """A member of more than 65,536 text bytes (the format's BSIZE bounds only its
    compressed size): -2 with the device kernel's limit, which sa_bgzf_scan
    passes, and walked like any other with no limit, as the host inflate wants it."""
    big = b"A" * 100_000
    cd = deflate(big)
    z = bgzf(b"ACGT" * 1000)[:-len(EOF_MEMBER)] + bgzf_member(cd, len(big), zlib.crc32(big)) + EOF_MEMBER
    first = len(z) - len(EOF_MEMBER) - (18 + len(cd) + 8)
    want = [(18, first - 26, 0, 4000, zlib.crc32(b"ACGT" * 1000)), (first + 18, len(cd), 4000, len(big), zlib.crc32(big)),
            (len(z) - 10, 2, 4000 + len(big), 0, 0)]
    assert _scan_emu(emu[0], tmp_path, z, 16, 0xffffffff) == (3, len(z), 4000 + len(big), want)
    assert _scan_emu(emu[0], tmp_path, z, 16, 100_000) == (3, len(z), 4000 + len(big), want)
    for limit in (None, 65536, 99_999):
        assert _scan_emu(emu[0], tmp_path, z, 16, limit)[0] == -2, limit
    lib = _scan_lib(z, 16)
    assert lib is None or lib[0] == -2
