"""bench.py's host side without a GPU: what a plain run and --full select, the
--dump-outputs arrays, and the pooled generator / threaded parse against the
one-batch-at-a-time path they replace (same bytes, same blocks)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import fastqueeze_amd as fq  # noqa: E402


def test_plain_run_is_the_headline_alone():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup) == (7, 3) and not a.full and a.dump_outputs is None
    assert a.no_verify and not a.text_leg and a.cpu_seconds == 0
    assert (a.e2e_batches, a.ont_leg, a.se_leg, a.hash_leg, a.ingest_devices) == (0, 0, 0, 0, 0)
    f = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full"])
    assert (f.steps, f.warmup) == (7, 3) and not f.no_verify and f.text_leg and f.cpu_seconds > 0
    assert f.e2e_batches == f.batches and f.ont_leg and f.se_leg and f.hash_leg and f.ingest_devices


def test_dump_outputs_arrays(tmp_path):
    rng = np.random.default_rng(5)
    outs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1000, 1, 70_000)]
    digs = [hashlib.sha256(o).digest() for o in outs]
    bench.dump_outputs(str(tmp_path / "a"), outs, digs, 0, 1)
    sizes = np.load(tmp_path / "a" / "block_sizes.npy")
    digests = np.load(tmp_path / "a" / "block_digests.npy")
    sample = np.load(tmp_path / "a" / "bytes_sample.npy")
    assert sizes.dtype == np.float64 and sizes.tolist() == [1000, 1, 70_000]
    assert digests.dtype == np.float64 and digests.shape == (3, 5)
    assert [int(x) for x in digests[2]] == [int.from_bytes(digs[2][6 * k:6 * k + 6], "big") for k in range(5)]
    # fewer bytes than the sample holds: every byte, in order
    assert sample.dtype == np.float32 and np.array_equal(sample, np.frombuffer(b"".join(outs), np.uint8))
    # more: the same seeded positions every time, each value the byte at its position
    big = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (3 << 20, 5, 2 << 20)]
    bd = [hashlib.sha256(o).digest() for o in big]
    bench.dump_outputs(str(tmp_path / "b"), big, bd, 0, 1)
    bench.dump_outputs(str(tmp_path / "c"), big, bd, 1, 2)
    s1 = np.load(tmp_path / "b" / "bytes_sample.npy")
    s2 = np.load(tmp_path / "c" / "bytes_sample_rank1.npy")
    assert s1.shape == (bench.DUMP_SAMPLE,) and np.array_equal(s1, s2)
    allb = np.frombuffer(b"".join(big), np.uint8)
    at = np.sort(np.random.default_rng(2024).integers(0, allb.size, bench.DUMP_SAMPLE))
    assert np.array_equal(s1, allb[at])
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 64 << 20


def test_pooled_generator_and_threaded_parse_match_the_serial_path():
    # two chunks per batch (250,000 + 10,000 reads), two batches, single-end
    args = bench.parse_args(["--se", "--pairs", "260000", "--batches", "2"])
    new = list(bench.batch_texts([0, 1], args, 2))
    for g, (t1, t2) in enumerate(new):
        o1, o2 = bench.batch_text(g, args, 1)
        assert t2 is None and o2 is None and bytes(t1) == o1
    got = bench.cut_and_parse(new[1][0], None, 8 << 20, 3)
    want = fq.blocks_from_fastq(bytes(new[1][0]), None, 8 << 20)
    assert len(got) == len(want) > 3
    for x, y in zip(got, want):
        assert x.text_bytes == y.text_bytes and (x.text1, x.text2) == (y.text1, y.text2)
        for f in ("names", "name_lens", "seq", "seq_lens", "qual"):
            assert np.array_equal(getattr(x, f), getattr(y, f)), f
    # paired: the cut of both files and the mates' interleaving
    t1, t2 = bench.batch_text(0, bench.parse_args(["--pairs", "30000"]), 1)
    got = bench.cut_and_parse(t1, t2, 4 << 20, 3)
    want = fq.blocks_from_fastq(t1, t2, 4 << 20)
    assert len(got) == len(want) > 3
    for x, y in zip(got, want):
        assert (x.text_bytes, x.text1, x.text2) == (y.text_bytes, y.text1, y.text2)
        for f in ("names", "name_lens", "seq", "seq_lens", "qual"):
            assert np.array_equal(getattr(x, f), getattr(y, f)), f
