"""The lane-per-message MD5 (k_md5_lanes) on the CPU: tests/cpu_emu/md5_lanes_emu.cpp
runs the logic of fastqueeze_amd/csrc/sa_md5_lanes.h -- the host's grouping of
a batch's messages into chain waves, each lane's loads, its tail and padding
blocks from guarded reads, the [block][word][lane] LDS image, the chain with a
lane past its last block keeping its state -- and every digest must equal
hashlib.md5.  The program is built twice, plainly and with
-fsanitize=address,undefined (every message a heap block of exactly its
length, so a read at or past ptr + len is reported), and both builds run
stand-alone.  Also here: SA_MD5_LANES through parse_knobs / plan_paths.  No GPU."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 1000, 65539]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("md5_lanes_emu")
    src = os.path.join(ROOT, "tests", "cpu_emu", "md5_lanes_emu.cpp")
    exe, san = d / "md5_lanes_emu", d / "md5_lanes_emu_san"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(san), src], check=True)
    return str(exe), str(san)


def _messages(lengths, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]


def _run(exe, tmp_path, tag, msgs):
    """-> (order, {task: (wave, lane, digest hex)})"""
    f = tmp_path / f"{tag}.bin"
    f.write_bytes(struct.pack("<I", len(msgs)) + b"".join(struct.pack("<I", len(m)) for m in msgs) + b"".join(msgs))
    r = subprocess.run([exe, "digests", str(f)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[0].split()[0] == "order"
    order = [int(x) for x in lines[0].split()[1:]]
    rows = {}
    for ln in lines[1:]:
        t, w, l, dg = ln.split()
        rows[int(t)] = (int(w), int(l), dg)
    return order, rows


def _check(exe, tmp_path, tag, msgs):
    order, rows = _run(exe, tmp_path, tag, msgs)
    n = len(msgs)
    # the grouping: by length, longest first, stable; every task exactly once; 64 consecutive tasks a wave
    assert order == sorted(range(n), key=lambda i: -len(msgs[i])), tag
    assert sorted(order) == list(range(n)) and sorted(rows) == list(range(n)), tag
    for s, t in enumerate(order):
        assert rows[t][:2] == (s // 64, s % 64), (tag, t)
    # every digest at its task's own index
    for t, m in enumerate(msgs):
        assert rows[t][2] == hashlib.md5(m).hexdigest(), (tag, t, len(m))
    return order, rows


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_each_length_alone_and_all_in_one_wave(emu, tmp_path, which):
    exe = emu[which]
    for n in LENGTHS:                                  # a one-lane wave per length
        _check(exe, tmp_path, f"len{n}", _messages([n], n))
    # one wave that mixes them all (twice, in two orders): lanes end at different
    # blocks, one- and two-block padding side by side, equal lengths in neighbouring lanes
    mixed = LENGTHS + LENGTHS[::-1]
    order, rows = _check(exe, tmp_path, "mixed", _messages(mixed, 77))
    assert len(mixed) <= 64 and {rows[t][0] for t in rows} == {0}
    assert order[:2] == [13, 14] and order[-2:] == [0, 27]   # the two longest first, the two empty ones last


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
@pytest.mark.parametrize("ntasks", [3, 64, 65, 207])
def test_grouping(emu, tmp_path, which, ntasks):
    """3, 64, 65 and 207 tasks (207: the shape of a 69-block batch -- per block a
    short ID message and two equal longer ones): ties keep task order, the last
    wave is partly filled, every padding residue occurs."""
    rng = np.random.default_rng(ntasks)
    lens = []
    for b in range((ntasks + 2) // 3):
        n = int(rng.integers(300, 700))
        lens += [int(rng.integers(0, 130)), n, n]
    lens = lens[:ntasks]
    order, rows = _check(emu[which], tmp_path, f"g{ntasks}", _messages(lens, 1000 + ntasks))
    assert max(w for w, _, _ in rows.values()) == (ntasks - 1) // 64
    ties = [(a, b) for a, b in zip(order, order[1:]) if lens[a] == lens[b]]
    assert ties and all(a < b for a, b in ties)


def _knobs(exe, env):
    r = subprocess.run([exe, "knobs"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    w = r.stdout.split()
    return dict(zip(w[0::2], map(int, w[1::2])))


def test_knob_sa_md5_lanes(emu):
    """SA_MD5_LANES unset / "1": the lane kernel, reported as path 1; "0" and "x"
    (atoi: 0): k_md5<false>, path 3; SA_MD5_PIPE=1 goes before it (path 2); MD5 off: 0."""
    exe = emu[0]
    assert _knobs(exe, {}) == dict(md5_lanes=1, md5_pipe=0, path=1, path_off=0)
    assert _knobs(exe, {"SA_MD5_LANES": "1"}) == dict(md5_lanes=1, md5_pipe=0, path=1, path_off=0)
    assert _knobs(exe, {"SA_MD5_LANES": "0"}) == dict(md5_lanes=0, md5_pipe=0, path=3, path_off=0)
    assert _knobs(exe, {"SA_MD5_LANES": "x"}) == dict(md5_lanes=0, md5_pipe=0, path=3, path_off=0)
    assert _knobs(exe, {"SA_MD5_PIPE": "1"})["path"] == 2
    assert _knobs(exe, {"SA_MD5_PIPE": "1", "SA_MD5_LANES": "0"})["path"] == 2
