"""The forged DEFLATE corpus of tests/deflate_forge.py through both device
inflaters: k_inflate_bgzf (fq.Inflater: inflate_into, inflate_to) and the five
k_gz_* kernels (fq.Gunzipper), against Python's zlib.  These are streams in the
dialects of encoders other than zlib -- 15-bit literal, length and distance
codes behind the primary tables, single-code and empty distance alphabets,
header shapes zlib never writes, streams that end on the last bit of the input
-- and one or more stream per rejection rule of sa_inflate.h's header, each
with its status.  tests/test_deflate_forge.py runs the same bytes through the
host emulations first, under sanitizers too; invalid streams end with a status
by design.  Outputs are canary-filled: no byte outside a member's own range,
or past the text a call reports, may change."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_forge as df
import test_deflate_forge as tdf
import test_inflate as ti
from conftest import ROOT
from test_gpu_gunzip import _run_all, gz   # noqa: F401  (the gunzipper at 32 KiB chunks, and the call loop over a canary-filled array)

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu

CANARY = 0x5c


@pytest.fixture(scope="module")
def inflater():
    f = fq.Inflater(0)
    yield f
    f.close()


def _valid():
    """The valid members, and one that ends on the last bit of its last byte once
    more at the end: the input buffer ends with it, nothing behind it."""
    fx = df.valid()
    return fx + [v for v in fx if v[0] == "ends_on_last_bit_eob15_match"]


def _mixed():
    """The invalid set among the valid members, unlike shapes next to each other:
    [(name, deflate bytes, isize, crc, expected bytes or status)]."""
    fx, bad = _valid(), df.invalid()
    out = []
    for i in range(max(len(fx), len(bad))):
        if i < len(bad):
            name, cd, isize, crc, st, _ = bad[i]
            out.append((name, cd, isize, crc, st))
        name, cd, d = fx[(i * 7) % len(fx)]   # (7 and the list's length are coprime: every valid member occurs)
        out.append((name, cd, len(d), zlib.crc32(d), d))
    assert {m[0] for m in out} >= {v[0] for v in fx}
    return out


def _check_mixed(rc, status, out, ms, mixed):
    expect = np.full(out.size, CANARY, np.uint8)
    assert rc == sum(1 for m in mixed if isinstance(m[4], int)) == int(np.count_nonzero(status))
    for (name, _, _, _, want), m, st in zip(mixed, ms, status):
        a, b = int(m["out_off"]), int(m["out_off"]) + int(m["isize"])
        if isinstance(want, int):
            assert st == want, (name, int(st), want)
            expect[a:b] = out[a:b]   # (a failed member's own range is undefined)
        else:
            assert st == 0, (name, int(st))
            expect[a:b] = np.frombuffer(want, np.uint8)
    assert np.array_equal(out, expect)


def test_valid_members_one_call(inflater):
    fx = _valid()
    buf, ms, total = ti.pack_members([(cd, len(d), zlib.crc32(d)) for _, cd, d in fx])
    assert int(ms[-1]["in_off"]) + int(ms[-1]["in_len"]) == len(buf)
    out = np.full(total, CANARY, np.uint8)
    rc, status = inflater.inflate_into(buf, ms, out)
    assert rc == 0 and not status.any(), [(fx[i][0], int(status[i])) for i in np.flatnonzero(status)]
    for (name, _, d), m in zip(fx, ms):
        assert out[int(m["out_off"]):int(m["out_off"]) + len(d)].tobytes() == d, name


def test_invalid_among_valid(inflater):
    """The return value counts the bad members, each reports its listed status,
    every valid member is right and no byte outside a bad member's own range is touched."""
    mixed = _mixed()
    buf, ms, total = ti.pack_members([m[1:4] for m in mixed])
    out = np.full(total, CANARY, np.uint8)
    rc, status = inflater.inflate_into(buf, ms, out)
    _check_mixed(rc, status, out, ms, mixed)


def test_three_waves_reuse_tables_and_window(monkeypatch):
    """SA_INFL_GRID=3: every wave takes a third of the mixed list in turn, so a
    15-bit table follows a single-code table follows a fixed block follows a
    header that was rejected half-read: a stale table entry or window byte shows."""
    monkeypatch.setenv("SA_INFL_GRID", "3")
    mixed = _mixed()
    buf, ms, total = ti.pack_members([m[1:4] for m in mixed])
    out = np.full(total, CANARY, np.uint8)
    f = fq.Inflater(0)
    try:
        assert f.grid == 3
        rc, status = f.inflate_into(buf, ms, out)
    finally:
        f.close()
    _check_mixed(rc, status, out, ms, mixed)


@pytest.mark.parametrize("flipped", [False, True])
def test_seeded_members(inflater, flipped):
    """768 forged members in one call, and the same with one bit flipped each in
    another: zlib's verdict decides, as on the host."""
    members, verdicts = tdf._seeded_members(flipped)
    buf, ms, total = ti.pack_members(members)
    out = np.full(total, CANARY, np.uint8)
    expect = np.full(total, CANARY, np.uint8)
    rc, status = inflater.inflate_into(buf, ms, out)
    assert rc == sum(1 for z in verdicts if z is None) == int(np.count_nonzero(status))
    for i, (z, m, st) in enumerate(zip(verdicts, ms, status)):
        a, b = int(m["out_off"]), int(m["out_off"]) + int(m["isize"])
        assert (st == 0) == (z is not None), (i, int(st))
        expect[a:b] = out[a:b] if z is None else np.frombuffer(z, np.uint8)
    assert np.array_equal(out, expect)


def test_valid_members_into_devtext(inflater):
    """inflate_to at a write position off the 16-byte grid: take + fetch give the
    members' text in order."""
    fx = _valid()
    buf, ms, total = ti.pack_members([(cd, len(d), zlib.crc32(d)) for _, cd, d in fx])
    lead = b"@lead\nAC\n+\nII\n"[:13]
    dt = fq.DevText(total + (128 << 10))   # (room for the mixed list below)
    try:
        dt.append(lead)
        rc, status = inflater.inflate_to(dt, buf, ms)
        assert rc == 0 and not status.any(), status
        assert dt.avail == len(lead) + total
        blk = dt.take(dt.avail)
        assert blk.fetch() == (lead + b"".join(d for _, _, d in fx), None)
        blk.close()
        # the mixed list: the statuses, and nothing is appended
        mixed = _mixed()
        buf, ms, _ = ti.pack_members([m[1:4] for m in mixed])
        rc, status = inflater.inflate_to(dt, buf, ms)
        assert rc == sum(1 for m in mixed if isinstance(m[4], int)) and dt.avail == 0
        assert [int(s) for s in status] == [m[4] if isinstance(m[4], int) else 0 for m in mixed]
    finally:
        dt.close()


# ---- the gzip path ---------------------------------------------------------------
@pytest.fixture(scope="module")
def gz_exe(tmp_path_factory):
    """tests/cpu_emu/gunzip_emu.cpp, plain: the emulation whose counts the device must reproduce."""
    exe = tmp_path_factory.mktemp("gunzip_emu") / "gunzip_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpu_emu", "gunzip_emu.cpp")],
                   check=True)
    return exe


@pytest.mark.parametrize("name", ["long_codes", "header_shapes", "odd_dist_alphabets"])
def test_gz_streams(gz, gz_exe, tmp_path, name):
    """zlib's text with status 0; the chunks, confirmed waves and skipped false
    candidates of every call are the emulation's for the same bytes and chunk size
    (the same logic on the same input: an equality), and more than one wave is
    confirmed: the text does not come from wave 0 alone.  Then in slabs of
    100,000 compressed bytes through the state."""
    z, t = df.gz_streams()[name]
    assert gz.gunzip(z) == t, gz.calls
    assert all(c["status"] == 0 for c in gz.calls)
    got = [(c["chunks"], c["waves_confirmed"], c["false_skipped"]) for c in gz.calls]
    print(name, got)
    assert got == tdf.gz_emu_calls(gz_exe, tmp_path, name, gz.chunk)
    assert sum(c[1] for c in got) >= 2
    rc, out, n = _run_all(gz, z, len(t) + 4096, slab=100_000)
    assert rc == 0 and n == len(t) and out[:n].tobytes() == t and (out[n:] == CANARY).all()


def test_gz_invalid_blocks(gz):
    """A block that breaks a rule, in the second chunk of a stream and deep in one:
    the status the emulation gives (tests/test_deflate_forge.py pins it to the
    rule's at this chunk size), the stream's text before it, the canary past it."""
    cap = df.GZ_TEXT + 4096
    for name, z, want, t in df.gz_invalid():
        rc, out, n = _run_all(gz, z, cap)
        assert rc == want, (name, rc, gz.last_info)
        assert out[:n].tobytes() == t[:n] and (out[n:] == CANARY).all(), name
