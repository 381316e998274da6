"""DevInput, the compressed input of seqarc_amd --gpu-text
(fastqueeze_amd/csrc/cli_devinput.h): its file thread, pump() for BGZF and for
ordinary gzip, the takeover by the host and its ways to shut down, driven by
tests/cpu_emu/devinput_emu.cpp with host code in place of the library (a devtext
that is a heap block of exactly its capacity, gz_run over the emulation's
backend writing at its write position), against Python's zlib.  The program is
built plain, with address + undefined-behaviour sanitizers and with the thread
sanitizer, and each build is run directly.  No GPU, nothing loaded into Python.

The sizes are tests/test_gzstream.py's: slabs of 64 KiB with 48 KiB of room for
the carry keep FASTQ on the device path, and 300,000 text bytes a call fit every
first wave of fq_l6 and still cut some of its calls.  The devtext holds 400,000
bytes and is pumped to 60,000, so that every call has that room, the text moves
to the front again and again, and 30,007 bytes leave it between two pumps."""
import os
import re
import subprocess

import pytest

import test_gunzip as tg
import test_gzstream as ts
from conftest import ROOT

TIMEOUT = 60
GZIP = dict(slab=65_536, room=49_152, capacity=400_000, call_bytes=300_000, append_bytes=10_007, queue_cap=10_000,
            want=60_000, take=30_007)
# a carry larger than the room: a call that the output cap cut short leaves more than 4 KiB
SMALL_ROOM = dict(GZIP, room=4096)
# BGZF (members of 20,000 text bytes): two whole members a slab, one member a call
BGZF = dict(slab=15_000, room=0, capacity=100_000, call_bytes=30_000, append_bytes=10_007, queue_cap=10_000, want=40_000,
            take=30_007)
KEYS = ("slab", "room", "capacity", "call_bytes", "append_bytes", "queue_cap", "want", "take")
TAKEN_OVER = ("stored", "runs", "members_30x2k")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("devinput_emu")
    src = os.path.join(ROOT, "tests", "cpu_emu", "devinput_emu.cpp")
    exes = {}
    for name, flags in (("plain", ["-O2", "-Wall"]),
                        ("asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                        ("tsan", ["-O1", "-g", "-fsanitize=thread"])):
        exes[name] = d / f"devinput_emu_{name}"
        subprocess.run(["g++", "-std=c++17"] + flags + ["-o", str(exes[name]), src, "-lz", "-ldl", "-pthread"], check=True)
    return exes


def run(exe, tmp_path, data, kind, sizes, limit=0, tag="x", path=None):
    """One devinput_emu run: (exit status, final word, text, stderr lines, stats)."""
    f, o = tmp_path / f"{tag}.gz", tmp_path / f"{tag}.out"
    if path is None:
        f.write_bytes(data)
    r = subprocess.run([str(exe), str(path or f), kind] + [str(sizes[k]) for k in KEYS] + [str(limit), str(o)],
                       capture_output=True, timeout=TIMEOUT)
    log = r.stderr.decode().splitlines()
    # (no sanitizer report: every line is the input's -v output or the program's error)
    assert all(ln.startswith(("seqarc_amd: --gpu-text: ", "devinput_emu: ")) for ln in log), r.stderr.decode()[-3000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.decode().splitlines()}
    word, n = out["final"]
    text = o.read_bytes()
    assert r.returncode == (1 if word == "error" else 0) and int(n) == len(text), (r.returncode, r.stdout)
    stats = dict(zip(("calls", "members", "host_bytes", "moves"), map(int, out.get("stats", [0, 0, 0, 0]))))
    return r.returncode, word, text, log, stats


def files():
    fx = dict(ts.gz_files())
    fx["members_30x2k"] = tg.fixtures()["members_30x2k"]
    return fx


def _check_gzip(exe, tmp_path, name, sizes=GZIP, taken_over=None):
    z, t = files()[name]
    rc, word, text, log, stats = run(exe, tmp_path, z, "gzip", sizes, tag=name)
    assert (rc, word) == (0, "ok") and text == t, (name, word, len(text), log)
    took = [ln for ln in log if "the host takes over at byte" in ln]
    want_taken = name in TAKEN_OVER if taken_over is None else taken_over
    assert len(took) == (1 if want_taken else 0) and (stats["host_bytes"] > 0) == want_taken, (name, log, stats)
    line = [ln for ln in log if "sa_gunzip_run_dev" in ln]
    assert len(line) == 1 and ("the host inflated the rest" in line[0]) == want_taken, log
    assert f"{len(t)} text bytes on device 0" in line[0], line[0]
    return stats, line[0]


@pytest.mark.parametrize("name", ["fq_l1", "fq_l6", "fq_l9"])
def test_fastq_stays_on_the_device_path(emu, tmp_path, name):
    """The three 2 MB fixtures: every byte through sa_gunzip_run_dev, more calls than
    slabs where the output cap cut one, the text moved to the front many times."""
    stats, _ = _check_gzip(emu["plain"], tmp_path, name)
    assert stats["moves"] >= 4 and stats["members"] == 1
    if name == "fq_l6":
        assert stats["calls"] > -(-len(files()[name][0]) // GZIP["slab"])


@pytest.mark.parametrize("name", ["stored", "runs", "members_30x2k", "three"])
def test_takeover(emu, tmp_path, name):
    """A stored-only file, a file of enormous ratio and thirty tiny members leave the
    device path; the host's text reaches the same devtext through append and the
    text is whole.  Three ordinary members stay on the device."""
    _check_gzip(emu["plain"], tmp_path, name)


def test_carry_larger_than_the_room(emu, tmp_path):
    """With 4 KiB in front of a slab, what a call cut short by the output cap leaves
    does not fit: the host takes over in mid-stream and the text is whole."""
    stats, _ = _check_gzip(emu["plain"], tmp_path, "fq_l6", sizes=SMALL_ROOM, taken_over=True)
    assert stats["calls"] >= 1 and 0 < stats["host_bytes"] < len(files()["fq_l6"][1])


def _bad_gzip():
    z, t = files()["small_l6"]
    crc = bytearray(z)
    crc[-8] ^= 1
    stored_crc = bytearray(files()["stored"][0])   # (the host finds this one, after the takeover)
    stored_crc[-8] ^= 1
    return [("truncated", z[:len(z) * 2 // 3], t), ("crc", bytes(crc), t), ("stored_crc", bytes(stored_crc), files()["stored"][1]),
            ("stored_cut", files()["stored"][0][:200_000], files()["stored"][1])]


def _check_failures(exe, tmp_path):
    for name, data, t in _bad_gzip():
        rc, word, text, log, _ = run(exe, tmp_path, data, "gzip", GZIP, tag=name)
        assert (rc, word) == (1, "error") and text == t[:len(text)], (name, word, log)
        assert sum("read error on" in ln for ln in log) == 1, (name, log)
    # a read error: the file is a directory, which opens and does not read
    rc, word, text, log, _ = run(exe, tmp_path, None, "gzip", GZIP, path=tmp_path)
    assert (rc, word, text) == (1, "error", b"") and any("read error on" in ln for ln in log), log
    # BGZF cut inside a member, and a member's CRC flipped
    for name, data, modes, t, most in ts._bad_files():
        if "dev-inflate" in modes:
            rc, word, text, log, _ = run(exe, tmp_path, data, "bgzf", BGZF, tag=name)
            assert (rc, word) == (1, "error") and len(text) <= most and text == t[:len(text)], (name, word, log)


def test_failures(emu, tmp_path):
    """A truncated file and a wrong CRC on the device path, the same after a takeover,
    a read error, and the BGZF failures: exit status 1, and what was delivered
    before is the text's beginning."""
    _check_failures(emu["plain"], tmp_path)


def test_corrupt_set(emu, tmp_path):
    for name, data, _ in tg.corrupt():
        rc, word, text, log, _ = run(emu["plain"], tmp_path, data, "gzip", GZIP, tag=name)
        assert (rc, word) == (1, "error"), (name, log)
        if name != "flipped_byte":   # (a flipped byte can decode, to other text, until the CRC tells)
            assert text == tg.fq_text()[:len(text)], name


def _reader_leaves(exe, tmp_path, names=("fq_l6", "stored")):
    """After one pump the file thread is ahead by its slabs; after three the stored
    file's host thread waits in push on a full queue.  The destructor returns."""
    for kind, sizes, z, t in [("bgzf", BGZF, ts.small_bgzf(), ts.small())] + [("gzip", GZIP) + files()[n] for n in names]:
        for limit in (1, 3):
            rc, word, text, _, _ = run(exe, tmp_path, z, kind, sizes, limit=limit, tag=f"leave{limit}")
            assert (rc, word) == (0, "left") and text == t[:len(text)] and len(text) == limit * sizes["take"], (kind, limit, word)


def test_reader_goes_away(emu, tmp_path):
    _reader_leaves(emu["plain"], tmp_path)


def _check_bgzf(exe, tmp_path):
    z, t = ts.small_bgzf(), ts.small()
    rc, word, text, log, stats = run(exe, tmp_path, z, "bgzf", BGZF, tag="bgzf")
    assert (rc, word) == (0, "ok") and text == t, (word, log)
    line = [ln for ln in log if "sa_inflate_members_dev" in ln]
    assert len(line) == 1 and f": {len(ts.member_sizes(z))} member(s), {len(t)} text bytes in " in line[0], log
    assert stats["members"] == len(ts.member_sizes(z)) and stats["moves"] >= 4 and stats["host_bytes"] == 0


def test_bgzf(emu, tmp_path):
    """A BGZF input through the moved DevInput: every member, the -v line as before."""
    _check_bgzf(emu["plain"], tmp_path)


def test_under_address_and_undefined_sanitizers(emu, tmp_path):
    """Every slab and the devtext are heap blocks of exactly their sizes."""
    for name in ("fq_l6", "stored", "runs", "members_30x2k"):
        _check_gzip(emu["asan"], tmp_path, name)
    _check_gzip(emu["asan"], tmp_path, "fq_l6", sizes=SMALL_ROOM, taken_over=True)
    _check_bgzf(emu["asan"], tmp_path)
    _check_failures(emu["asan"], tmp_path)
    _reader_leaves(emu["asan"], tmp_path)


def test_under_thread_sanitizer(emu, tmp_path):
    """The small files only (the emulated gunzip is slow under it): a device-only
    file, the takeovers, the failures and the reader going away."""
    for name in ("small_l6", "stored", "runs"):
        _check_gzip(emu["tsan"], tmp_path, name)
    # (a carry larger than the room: 150,000 text bytes a call cut the first call of the 300,000-byte text)
    _check_gzip(emu["tsan"], tmp_path, "small_l6", sizes=dict(SMALL_ROOM, call_bytes=150_000), taken_over=True)
    _check_bgzf(emu["tsan"], tmp_path)
    _check_failures(emu["tsan"], tmp_path)
    _reader_leaves(emu["tsan"], tmp_path, names=("small_l6", "stored"))
