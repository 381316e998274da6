"""The forged DEFLATE corpus of tests/deflate_forge.py -- streams in the
dialects of encoders other than zlib, and one or more stream per rejection
rule of sa_inflate.h's header -- through the host emulations of both device
inflaters: tests/cpu_emu/inflate_emu.cpp (k_inflate_bgzf's per-member code) and
tests/cpu_emu/gunzip_emu.cpp (the speculative gzip path), plain and built with
address + undefined-behaviour sanitizers, against Python's zlib.  The forge has
asserted zlib's verdict on every stream before anything here runs.  No GPU;
tests/test_gpu_deflate_forge.py runs the same bytes through the kernels."""
import zlib

import pytest

import deflate_forge as df
import test_gunzip as tg
import test_inflate as ti
from test_gunzip import emu as gz_emu   # noqa: F401  (the fixtures that build the two stand-alone programs, as they are)
from test_inflate import emu   # noqa: F401


def _valid_members():
    return [(cd, len(d), zlib.crc32(d)) for _, cd, d in df.valid()]


def _check_valid(r, rows, outdir):
    fx = df.valid()
    assert r.returncode == 0 and len(rows) == len(fx), r.stderr
    for i, ((name, cd, d), row) in enumerate(zip(fx, rows)):
        assert row[0] == "0", (name, row)
        # the serial CRC of the output, and the CRC combined from the 64 lane shares
        assert int(row[1], 16) == int(row[2], 16) == zlib.crc32(d), (name, row)
        assert ((outdir / str(i)).read_bytes() if d else b"") == d, name   # (no file for an empty member)


def _check_invalid(r, rows):
    bad = df.invalid()
    assert r.returncode == 0 and len(rows) == len(bad), r.stderr
    for (name, cd, isize, crc, want, rule), row in zip(bad, rows):
        assert int(row[0]) == want, (name, rule, row)


def _seeded_members(flipped):
    """[(deflate bytes, isize, crc)] of all 32 seeds, and zlib's verdict on each."""
    ms = [(bad if flipped else cd, len(t), zlib.crc32(t)) for k in df.SEEDS for cd, t, bad in df.seeded(k)]
    return ms, [ti.zlib_verdict(*m) for m in ms]


def _check_seeded(r, rows, outdir, verdicts):
    assert r.returncode == 0 and len(rows) == len(verdicts), r.stderr
    n_bad = 0
    for i, (z, row) in enumerate(zip(verdicts, rows)):
        if z is None:
            n_bad += 1
            assert row[0] != "0", (i, row)
        else:
            assert row[0] == "0" and (outdir / str(i)).read_bytes() == z, (i, row)
    return n_bad


def test_every_header_rule_has_a_fixture():
    """Every rejection rule of sa_inflate.h's header comment is pinned by name."""
    rules = {v[5] for v in df.invalid()}
    assert rules >= {"HLIT > 286", "HDIST > 30", "a repeat without a previous length", "a repeat past HLIT + HDIST",
                     "a missing end-of-block code", "an over-subscribed set", "an incomplete set", "the codes 286 / 287",
                     "the distance codes 30 / 31", "input", "isize 0"}
    with open(ti.os.path.join(ti.ROOT, "fastqueeze_amd", "csrc", "sa_inflate.h")) as f:
        header = f.read().split("#pragma once")[0]
    for name in ("hlit_287", "hdist_31", "repeat_first", "repeat_past_end", "no_end_of_block", "lit_oversubscribed",
                 "dist_oversubscribed", "lit_incomplete", "dist_incomplete_two_2bit", "dist_single_code0", "dist_none",
                 "fixed_litlen_286", "fixed_dist_30"):
        assert name in header, name
        assert name in {v[0] for v in df.invalid()} | {v[0] for v in df.valid()}, name


def test_valid_members_match_zlib(emu, tmp_path):
    r, rows, outdir = ti._run_members(emu[0], tmp_path, _valid_members(), "valid")
    _check_valid(r, rows, outdir)


def test_invalid_members_give_their_statuses(emu, tmp_path):
    r, rows, _ = ti._run_members(emu[0], tmp_path, [v[1:4] for v in df.invalid()], "bad")
    _check_invalid(r, rows)


@pytest.mark.parametrize("flipped", [False, True])
def test_seeded_members_follow_zlib(emu, tmp_path, flipped):
    """768 forged members, valid by construction, and the same with one bit
    flipped each: zlib's verdict decides (most flips break the stream or its CRC;
    one in a padding bit or in a header's unused code does not)."""
    ms, verdicts = _seeded_members(flipped)
    r, rows, outdir = ti._run_members(emu[0], tmp_path, ms, "seeded")
    n_bad = _check_seeded(r, rows, outdir, verdicts)
    assert n_bad == 0 if not flipped else n_bad > 600


def test_members_under_sanitizers(emu, tmp_path):
    """The address + undefined-behaviour build: every member's input and output
    are heap blocks of exactly their sizes (an ISIZE 0 member's output has none),
    and the program must print nothing."""
    r, rows, outdir = ti._run_members(emu[1], tmp_path, _valid_members(), "san_valid")
    assert r.stderr == b"", r.stderr.decode()[-2000:]
    _check_valid(r, rows, outdir)
    r, rows, _ = ti._run_members(emu[1], tmp_path, [v[1:4] for v in df.invalid()], "san_bad")
    assert r.stderr == b"", r.stderr.decode()[-2000:]
    _check_invalid(r, rows)
    for flipped in (False, True):
        ms, verdicts = _seeded_members(flipped)
        r, rows, outdir = ti._run_members(emu[1], tmp_path, ms, f"san_seeded{int(flipped)}")
        assert r.stderr == b"", r.stderr.decode()[-2000:]
        _check_seeded(r, rows, outdir, verdicts)


# ---- the gzip path: gunzip_emu ---------------------------------------------------
DEVICE_CHUNK = 32768   # what tests/test_gpu_deflate_forge.py sets on the device


def gz_emu_calls(exe, tmp_path, name, chunk=DEVICE_CHUNK, slab=0):
    """The emulation's run of one of the three streams: its text and, per call,
    the counts the device must reproduce."""
    z, t = df.gz_streams()[name]
    calls, fin, text, _ = tg.run_emu(exe, tmp_path, z, chunk, slab=slab, tag=name)
    assert fin == (0, len(t), len(z), "end") and text == t, (name, chunk, fin, calls[-1])
    return [(c["chunks"], c["confirmed"], c["false_skipped"]) for c in calls]


@pytest.mark.parametrize("chunk", tg.CHUNKS + (DEVICE_CHUNK,))
def test_gz_streams_match_zlib(gz_emu, tmp_path, chunk):
    """The three forged gzip files: zlib's text, on the speculative path to the end
    (no handover), and not from wave 0 alone: waves that started inside forged
    blocks are confirmed, at the device's chunk size too."""
    for name, (z, t) in df.gz_streams().items():
        counts = gz_emu_calls(gz_emu[0], tmp_path, name, chunk)
        confirmed = sum(c[1] for c in counts)
        assert confirmed >= 2, (name, chunk, counts)
        # a block of 8 KiB of text is about 2.3 KB: every chunk holds a block start
        assert confirmed >= 3 * min(sum(c[0] for c in counts), len(z) // chunk) // 4, (name, chunk, counts)


@pytest.mark.parametrize("chunk", tg.CHUNKS + (DEVICE_CHUNK,))
def test_gz_invalid_blocks(gz_emu, tmp_path, chunk):
    """A block that breaks a rule of the code-length judgement, behind one chunk of
    valid blocks and deep in a stream: the rule's status, whichever wave meets it,
    and the text before it is the stream's."""
    for name, z, want, t in df.gz_invalid():
        calls, fin, text, _ = tg.run_emu(gz_emu[0], tmp_path, z, chunk, tag=name)
        assert fin[3] == "error" and fin[0] == want, (name, chunk, fin, calls[-1])
        assert text == t[:len(text)], name


def test_gz_under_sanitizers(gz_emu, tmp_path):
    """The address + undefined-behaviour build (run_emu asserts that it prints
    nothing): the three files at the smallest and the largest chunk size and in
    slabs of 100,000 compressed bytes through the state, and the invalid placements."""
    for name, (z, t) in df.gz_streams().items():
        for chunk in (4096, 65536):
            gz_emu_calls(gz_emu[1], tmp_path, name, chunk)
        gz_emu_calls(gz_emu[1], tmp_path, name, 16384, slab=100_000)
    for name, z, want, t in df.gz_invalid():
        calls, fin, text, _ = tg.run_emu(gz_emu[1], tmp_path, z, 16384, tag=name)
        assert fin[3] == "error" and fin[0] == want and text == t[:len(text)], (name, fin)
