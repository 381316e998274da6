"""GzStream, the gzip input of seqarc_amd (fastqueeze_amd/csrc/cli_gzstream.h):
its producer, worker, device and copier threads, its queues and its three ways
to shut down (a failure, the reader going away, the host taking over), driven by
tests/cpu_emu/gzstream_emu.cpp with host code in place of the library's device
calls, against Python's zlib.  The program is built plain, with address +
undefined-behaviour sanitizers and with the thread sanitizer, and each build is
run directly.  No GPU, nothing loaded into Python.

The stream's sizes are set so small that a file of a few hundred KB spans many
slabs, needs several device calls per slab and fills the queue; see BGZF and
GUNZIP."""
import functools
import gzip
import os
import re
import struct
import subprocess
import zlib

import pytest

import synth
import test_gunzip as tg
from conftest import ROOT
from test_inflate import EOF_MEMBER, _texts, bgzf, bgzf_member, deflate

TIMEOUT = 60
ASKS = (7, 4099, 65521, 300007, 1)   # gzstream_emu's read requests, in turn
MEMBER_TEXT = 20_000
# BGZF: members of 20,000 text bytes are ~5.6 KB, so a slab of 15,000 holds two whole members and nearly
# always ends inside the third; an output cap of 30,000 makes two device calls of such a slab; two slabs
# in flight; a queue of 10,000 is full after any one chunk, so every push but the first blocks.
BGZF = dict(slab=15_000, in_flight=2, room=0, out_cap=30_000, queue_cap=10_000)
# gunzip (the emulation's chunk is 4,096): zlib closes a block within 64 KiB of compressed bytes, and a
# slab that holds no whole block makes no progress and hands the file to the host, so 16 chunks are the
# smallest slab that keeps FASTQ on the device; room for 12 chunks of carry holds what a call cut short by
# the output cap leaves; 300,000 is the smallest cap tried that fits every first wave of fq_l6 and still
# cuts one of its calls (8 calls for 7 slabs).  With these fq_l1 / fq_l6 / fq_l9 stay on the device and
# `stored` and `runs` are taken over by the host: the split tests/test_gpu_gunzip.py asserts for the CLI.
GUNZIP = dict(slab=65_536, in_flight=2, room=49_152, out_cap=300_000, queue_cap=10_000)
SIZES = {"host": BGZF, "dev-inflate": BGZF, "dev-gunzip": GUNZIP, "both": GUNZIP}
# one wave would do all the work, or (fq_then_zeros) a block's text fits no wave's symbol range
TAKEN_OVER = ("stored", "runs", "members_30x2k", "fq_then_zeros")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzstream_emu")
    src = os.path.join(ROOT, "tests", "cpu_emu", "gzstream_emu.cpp")
    exes = {}
    for name, flags in (("plain", ["-O2", "-Wall"]),
                        ("asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                        ("tsan", ["-O1", "-g", "-fsanitize=thread"])):
        exes[name] = d / f"gzstream_emu_{name}"
        subprocess.run(["g++", "-std=c++17"] + flags + ["-o", str(exes[name]), src, "-lz", "-ldl", "-pthread"], check=True)
    return exes


def run(exe, tmp_path, data, mode, sizes=None, workers=2, limit=0, env=None, tag="x"):
    """One gzstream_emu run: (exit status, final word, text, the stream's stderr lines)."""
    s = sizes or SIZES[mode]
    f, o = tmp_path / f"{tag}.gz", tmp_path / f"{tag}.out"
    f.write_bytes(data)
    r = subprocess.run([str(exe), str(f), mode, str(workers)] +
                       [str(s[k]) for k in ("slab", "in_flight", "room", "out_cap", "queue_cap")] + [str(limit), str(o)],
                       capture_output=True, timeout=TIMEOUT, env=dict(os.environ, **(env or {})))
    log = r.stderr.decode().splitlines()
    assert all(ln.startswith("seqarc_amd: --gpu-") for ln in log), r.stderr.decode()[-3000:]   # (no sanitizer report)
    word, n = r.stdout.split()[1:]
    text = o.read_bytes()
    assert r.returncode == (1 if word == b"error" else 0) and int(n) == len(text), (r.returncode, r.stdout)
    return r.returncode, word.decode(), text, log


def ok_text(exe, tmp_path, data, mode, **kw):
    rc, word, text, log = run(exe, tmp_path, data, mode, **kw)
    assert (rc, word) == (0, "ok"), (mode, log)
    return text, log


@functools.lru_cache(maxsize=None)
def small():
    return _texts()[0]


@functools.lru_cache(maxsize=None)
def small_bgzf():
    z = bgzf(small(), chunk=MEMBER_TEXT)
    assert max(member_sizes(z)) * 2 < BGZF["slab"] < min(member_sizes(z)[:-2]) * 3
    return z


@functools.lru_cache(maxsize=None)
def gz_files():
    """{name: (gzip bytes, text)}: test_gunzip's 2 MB FASTQ at three levels, and the two
    shapes one wave would do all the work of (tests/test_gpu_gunzip.py's `stored` and `runs`)."""
    fx = {k: tg.fixtures()[k] for k in ("fq_l1", "fq_l6", "fq_l9")}
    fx["stored"] = (gzip.compress(small()[:300_000], 0, mtime=0), small()[:300_000])
    t = synth.generate(60, paired=False, seed=67)[0] * 100
    fx["runs"] = (gzip.compress(t, 6, mtime=0), t)
    fx["small_l6"] = (gzip.compress(small()[:300_000], 6, mtime=0), small()[:300_000])
    # (tg's three_members has a header CRC that is none, which zlib's gzip reading refuses)
    t = small()
    fx["three"] = (gzip.compress(t[:200_000], 6, mtime=0) + gzip.compress(t[200_000:350_000], 1, mtime=0) +
                   gzip.compress(t[350_000:], 9, mtime=0), t)
    return fx


def member_sizes(z):
    out, p = [], 0
    while p < len(z):
        out.append(struct.unpack_from("<H", z, p + 16)[0] + 1)
        p += out[-1]
    return out


def bgzf_slabs(z, slab):
    """How many slabs the BGZF reader makes of z: each is the carry and what fits behind it."""
    sizes, at, carry, n, m = member_sizes(z), 0, 0, 0, 0
    while at < len(z) or carry:
        have = carry + min(slab - carry, len(z) - at)
        at += have - carry
        while m < len(sizes) and sizes[m] <= have:
            have -= sizes[m]
            m += 1
        carry = have
        n += 1
    return n


# ---- the host paths ------------------------------------------------------------
@pytest.mark.parametrize("name", ["fq_l6", "three", "members_30x2k", "empty_between", "trailing_bytes"])
def test_host_plain(emu, tmp_path, name):
    """One member, several, and members with bytes behind them that are no member."""
    z, t = gz_files()[name] if name in gz_files() else tg.fixtures()[name]
    assert ok_text(emu["plain"], tmp_path, z, "host")[0] == t


@pytest.mark.parametrize("workers", [1, 4])
@pytest.mark.parametrize("no_libdeflate", [False, True])
def test_host_bgzf(emu, tmp_path, workers, no_libdeflate):
    env = {"SA_NO_LIBDEFLATE": "1"} if no_libdeflate else None
    assert ok_text(emu["plain"], tmp_path, small_bgzf(), "host", workers=workers, env=env)[0] == small()
    assert bgzf_slabs(small_bgzf(), BGZF["slab"]) >= 10


def test_oversized_member_inflates_on_the_host(emu, tmp_path):
    """A member of more than 65,536 text bytes: the device kernel cannot take it (the
    walk's limit for sa_bgzf_scan), the host inflate can, and does as before."""
    t = b"A" * 100_000
    z = bgzf_member(deflate(t), len(t), zlib.crc32(t)) + bgzf(small()[:50_000], chunk=MEMBER_TEXT)
    for env in (None, {"SA_NO_LIBDEFLATE": "1"}):
        assert ok_text(emu["plain"], tmp_path, z, "host", env=env)[0] == t + small()[:50_000]
    rc, word, text, _ = run(emu["plain"], tmp_path, z, "dev-inflate")
    assert (rc, word, text) == (1, "error", b"")


# ---- the device paths ----------------------------------------------------------
def _check_inflate_log(log, z):
    line = [ln for ln in log if "inflate kernel" in ln]
    assert len(line) == 1 and not any("--gpu-gunzip" in ln for ln in log), log
    want = f": {bgzf_slabs(z, BGZF['slab'])} slab(s), {len(member_sizes(z))} member(s), {len(small())} text bytes on device 0 in "
    assert want in line[0], (want, line[0])


@pytest.mark.parametrize("mode", ["dev-inflate", "both"])
def test_dev_inflate(emu, tmp_path, mode):
    text, log = ok_text(emu["plain"], tmp_path, small_bgzf(), mode, sizes=BGZF)
    assert text == small()
    _check_inflate_log(log, small_bgzf())


def test_dev_inflate_leaves_other_gzip_to_the_host(emu, tmp_path):
    z, t = gz_files()["small_l6"]
    text, log = ok_text(emu["plain"], tmp_path, z, "dev-inflate")
    assert text == t and len(log) == 1 and log[0].endswith("is gzip but not BGZF, inflating it on the host"), log


def _check_gunzip(exe, tmp_path, name, mode="dev-gunzip"):
    z, t = gz_files()[name] if name in gz_files() else tg.fixtures()[name]
    text, log = ok_text(exe, tmp_path, z, mode, tag=name)
    assert text == t, name
    summary = [ln for ln in log if "gunzip kernels" in ln]
    assert len(summary) == 1 and not any("--gpu-inflate" in ln for ln in log), log
    took_over = [ln for ln in log if "the host takes over at byte" in ln]
    assert len(took_over) == (1 if name in TAKEN_OVER else 0), (name, log)
    assert summary[0].endswith("; the host inflated the rest") == bool(took_over)
    return summary[0], took_over


@pytest.mark.parametrize("name", ["fq_l1", "fq_l6", "fq_l9", "stored", "runs", "small_l6"])
def test_dev_gunzip(emu, tmp_path, name):
    """The text is whole, on the device alone for FASTQ and finished by the host
    for the stored-only file and the file of long runs."""
    summary, _ = _check_gunzip(emu["plain"], tmp_path, name, "both" if name == "fq_l1" else "dev-gunzip")
    if name == "fq_l6":   # the output cap cut a call: more calls than slabs
        assert int(re.search(r"(\d+) call\(s\)", summary).group(1)) > -(-len(gz_files()[name][0]) // GUNZIP["slab"])


@pytest.mark.parametrize("name", ["fq_then_zeros", "three", "members_30x2k", "trailing_bytes"])
def test_dev_gunzip_shapes(emu, tmp_path, name):
    """FASTQ, then 8 MB of zeros in one member: the host takes over inside the deflate
    stream, with a window, at a bit offset, the member's CRC running.  Three members
    on the device, thirty tiny ones (taken over between two of them), and bytes after
    the last member."""
    _, took_over = _check_gunzip(emu["plain"], tmp_path, name)
    if name == "fq_then_zeros":
        assert int(took_over[0].rsplit(" ", 1)[1]) > 4096


# ---- failure: the text before the error, then -1 -------------------------------
def _bad_files():
    """[(name, bytes, modes, text, most text bytes that may be delivered)]"""
    b, t = small_bgzf(), small()
    sizes = member_sizes(b)
    bad_member = 10   # (in the fourth slab)
    assert sum(sizes[:bad_member]) > 3 * BGZF["slab"]
    flipped = bytearray(b)
    flipped[sum(sizes[:bad_member + 1]) - 8] ^= 1
    # member 3's trailer zeroed (a hole in the file): ISIZE 0 and CRC 0 in front of 20,000 bytes of text
    zeroed = bytearray(b)
    zeroed[sum(sizes[:4]) - 8:sum(sizes[:4])] = bytes(8)
    z, tz = gz_files()["small_l6"]
    bgzf_modes = ("host", "dev-inflate")
    out = [("cut_in_member", b[:-(len(EOF_MEMBER) + 100)], bgzf_modes, t, len(t) - len(t) % MEMBER_TEXT),
           ("junk_after", b + b"\x1f\x8bjunk", bgzf_modes, t, len(t)),
           ("crc_flipped", bytes(flipped), bgzf_modes, t, bad_member * MEMBER_TEXT),
           ("trailer_zeroed", bytes(zeroed), bgzf_modes + ("both",), t, 3 * MEMBER_TEXT),
           ("truncated", z[:len(z) * 2 // 3], ("host", "dev-gunzip"), tz, len(tz))]
    return out


def _check_bad(exe, tmp_path, name, data, mode, t, most):
    rc, word, text, log = run(exe, tmp_path, data, mode, tag=name)
    assert (rc, word) == (1, "error"), (name, mode, word, log)
    assert len(text) <= most and text == t[:len(text)], (name, mode, len(text))


def test_failures(emu, tmp_path):
    for name, data, modes, t, most in _bad_files():
        for mode in modes:
            _check_bad(emu["plain"], tmp_path, name, data, mode, t, most)


def test_zeroed_trailer_is_an_error_not_an_empty_member(emu, tmp_path):
    """A member with ISIZE 0 and CRC 0 is inflated like any other: with data in it
    it fails on the host pool (libdeflate and zlib) and on the device path, and the
    text before it is all that is delivered; the end-of-file marker, and one in
    the middle of the file, are the only empty members that pass."""
    name, data, _, t, most = [f for f in _bad_files() if f[0] == "trailer_zeroed"][0]
    for mode, env in (("host", None), ("host", {"SA_NO_LIBDEFLATE": "1"}), ("dev-inflate", None), ("both", None)):
        rc, word, text, log = run(emu["plain"], tmp_path, data, mode, env=env, tag=name)
        assert (rc, word) == (1, "error"), (mode, env, word, log)
        assert len(text) <= most and text == t[:len(text)], (mode, env, len(text))
    sizes = member_sizes(small_bgzf())
    eof_inside = small_bgzf()[:sum(sizes[:4])] + EOF_MEMBER + small_bgzf()[sum(sizes[:4]):]
    for mode, env in (("host", None), ("host", {"SA_NO_LIBDEFLATE": "1"}), ("dev-inflate", None)):
        assert ok_text(emu["plain"], tmp_path, eof_inside, mode, env=env, tag="eof_inside")[0] == small()


def test_corrupt_gzip_on_the_device_path(emu, tmp_path):
    for name, data, _ in tg.corrupt():
        rc, word, text, log = run(emu["plain"], tmp_path, data, "dev-gunzip", tag=name)
        assert (rc, word) == (1, "error"), (name, log)
        assert sum("the gzip stream is corrupt (status" in ln for ln in log) == 1, (name, log)
        if name != "flipped_byte":   # (a flipped byte can decode, to other text, until the CRC tells)
            assert text == tg.fq_text()[:len(text)], name


# ---- the reader goes away ------------------------------------------------------
def _reader_leaves(exe, tmp_path, names=("fq_l6", "stored")):
    """After one request the queue is full and the producer (or the copier) waits in
    push; after a few the stream is in mid-file.  The destructor returns either way."""
    files = [("host", small_bgzf(), small()), ("dev-inflate", small_bgzf(), small())]
    for n in names:
        files += [(m,) + gz_files()[n] for m in ("host", "dev-gunzip")]
    for mode, z, t in files:
        for limit in (1, 3):
            want = sum(ASKS[:limit])
            assert want < len(t)
            rc, word, text, _ = run(exe, tmp_path, z, mode, limit=limit, tag=f"leave{limit}")
            assert (rc, word) == (0, "left") and text == t[:want], (mode, limit, word, len(text))


def test_reader_goes_away(emu, tmp_path):
    _reader_leaves(emu["plain"], tmp_path)


# ---- the sanitizer builds ------------------------------------------------------
def _one_per_mode(exe, tmp_path, gunzip_names):
    assert ok_text(exe, tmp_path, small_bgzf(), "host", workers=4)[0] == small()
    assert ok_text(exe, tmp_path, tg.fixtures()["empty_between"][0], "host")[0] == tg.fixtures()["empty_between"][1]
    text, log = ok_text(exe, tmp_path, small_bgzf(), "both", sizes=BGZF)
    assert text == small()
    _check_inflate_log(log, small_bgzf())
    for name in gunzip_names:
        _check_gunzip(exe, tmp_path, name)
    for name, data, modes, t, most in _bad_files():
        for mode in modes:
            _check_bad(exe, tmp_path, name, data, mode, t, most)


def test_under_address_and_undefined_sanitizers(emu, tmp_path):
    """Every slab, output slab and chunk is a heap block of exactly its size."""
    _one_per_mode(emu["asan"], tmp_path, ("fq_l6", "stored", "runs", "fq_then_zeros"))
    _reader_leaves(emu["asan"], tmp_path)


def test_under_thread_sanitizer(emu, tmp_path):
    """The small files only (the emulated gunzip is slow under it): a device-only
    file, the two takeovers, the failures and the reader going away."""
    _one_per_mode(emu["tsan"], tmp_path, ("small_l6", "stored", "runs"))
    _reader_leaves(emu["tsan"], tmp_path, names=("small_l6", "stored"))
