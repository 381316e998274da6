"""k_md5_lanes (one MD5 message per lane of a chain wave) on the GPU: batches
whose messages -- per block its IDs, bases and qualities -- fill the chain
waves in the ways that matter, every encoded block compared byte for byte with
oracle_py.encode_block (MD5 on), and the kernel that ran asserted from
Encoder.paths() (sa_last_paths).  tests/test_md5_lanes.py runs the same logic
on the CPU."""
import functools

import numpy as np
import pytest

import oracle_py
import synth

import fastqueeze_amd as fq

pytestmark = pytest.mark.gpu


def _one_read_block(i, n):
    """One block of one read: n bases, an ID whose length varies with i."""
    rng = np.random.default_rng(1000 + i)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
    qual = rng.integers(40, 74, n, dtype=np.uint8).tobytes()
    name = b"r%d" % i + b"x" * ((7 * i) % 61)
    return fq.parse_se(b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n")


@functools.lru_cache(maxsize=None)
def _input(name):
    if name == "B140":      # 420 messages in 7 waves: 1..140 bases (every padding residue), a 36-lane last wave
        return [_one_read_block(i, i + 1) for i in range(140)]
    if name == "UNEQUAL":   # a block of ~300 KB of bases beside one-read blocks: one wave, very unequal lengths
        big = fq.blocks_from_fastq(synth.generate(2000, paired=False, seed=31)[0])
        assert len(big) == 1 and big[0].seq.size >= 250_000
        return [_one_read_block(i, 3 * i + 1) for i in range(5)] + big + [_one_read_block(i, 64 * i) for i in range(5, 10)]
    if name == "ONE":       # 3 lanes
        return [_one_read_block(0, 100)]
    if name == "B22":       # 66 messages: a full wave and a 2-lane wave
        return [_one_read_block(i, 50 + 9 * i) for i in range(22)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name, md5):
    return [oracle_py.encode_block(b, 3, 2, md5, 0, 0.0) for b in _input(name)]


def _run(monkeypatch, env, name, md5, path):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = fq.Encoder(0)
    try:
        got = e.encode(_input(name), fq.Config(md5=md5))
        paths = e.paths()
    finally:
        e.close()
    want = _want(name, md5)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: block {i} differs from the oracle ({len(g)} vs {len(w)} B)"
    assert paths["md5"] == path, paths["md5"]


def test_inputs():
    assert len(_input("B140")) == 140 and [int(b.seq.size) for b in _input("B140")] == list(range(1, 141))
    assert len({int(b.names.size) for b in _input("B140")}) > 30
    assert len(_input("B22")) * 3 == 66 and len(_input("ONE")) * 3 == 3


@pytest.mark.parametrize("name", ["B140", "UNEQUAL", "ONE", "B22"])
def test_lane_kernel(monkeypatch, name):
    _run(monkeypatch, {}, name, True, "plain")


@pytest.mark.parametrize("env,path", [({"SA_MD5_LANES": "0"}, "wave"), ({"SA_MD5_PIPE": "1"}, "pipe")],
                         ids=["lanes0", "pipe"])
def test_wave_kernels_by_knob(monkeypatch, env, path):
    _run(monkeypatch, env, "B140", True, path)


def test_md5_off(monkeypatch):
    _run(monkeypatch, {}, "B140", False, None)
