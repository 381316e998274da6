"""The chain-per-block decoder logic (fastqueeze_amd/csrc/sa_decode_logic.h) run
on the host by tests/cpu_emu/decode_emu.cpp: the 64-lane SIMPLE_MODEL step as a
loop over the lanes, every chain decoded in slices that stop and resume through
the stored state.  A valid block must come out equal to the block that was
encoded (and to what sa_decode_block gives); a corrupt block must fail exactly
where sa_decode_block fails (return -1 or md5_ok == 0).  The program is built
twice, plainly and with -fsanitize=address,undefined, and both builds run.  Also
here: the bounded renormalisation from a constructed range-0 state, and
plan_decode.  No GPU."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_py
import synth
from conftest import ROOT, TEST1, TEST2
from test_oracle import _norm_seq

import fastqueeze_amd as fq

OK, LAYOUT, INPUT, SLOT, RANGE, PLACE, UNSUPPORTED = range(7)
EV_HIGH, EV_SWAP_63_64, EV_HALVE, EV_SWAP, EV_BASE_HALVE = 1, 2, 4, 8, 16
BIG_SLICE = 1 << 30


class Case:
    """Blocks of one config, encoded by the CPU restatement of the encoder."""

    def __init__(self, name, blocks, cfg=None, tmpl=None):
        self.name, self.blocks, self.cfg = name, blocks, cfg or fq.Config()
        self.tmpl = np.zeros(512, np.uint8) if tmpl is None else tmpl
        c = self.cfg
        self.enc = [oracle_py.encode_block(b, c.slevel, c.qlevel, c.md5, c.bin_mode, c.lossy) for b in blocks]
        self.long = [bool(b.nreads and int(b.seq_lens.max()) > 0xFFFF) for b in blocks]
        self.caps = [b.text_bytes or b.text1 + b.text2 for b in blocks]
        # what the host decoder says of each block: (its reads, md5_ok)
        self.host = [fq.decode_block(e, cap, c, self.tmpl, lg) for e, cap, lg in zip(self.enc, self.caps, self.long)]


def _read_shapes_text():
    """synth's M-style input plus the read shapes the placement and the '#' rule
    can get wrong (spliced in after M's first records, so none is the last read)."""
    m = synth.long_read_fastq(5, 510)
    extra = (b"@allhash\nACGTACGT\n+\n########\n"      # all '#'
             b"@alln\nNNNNNNNN\n+\n!!!!!!!!\n"           # all N
             b"@empty1\n\n+\n\n"
             b"@ends\nNACGTACN\n+\n!IIIIII!\n"           # N first and last; a tip read with zero exceptions
             b"@exc\nNACGNACG\n+\n5I5I5I5I\n"            # a tip read with exceptions: C at 2 and 6 as low as its Ns
             b"@empty2\n\n+\n\n")
    cut = m.index(b"\n@lr40\n") + 1
    return m[:cut] + extra + m[cut:]


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("pair_bin", "pair_tok"):      # 1: the reference test pair, PE
        t1, t2 = open(TEST1, "rb").read(), open(TEST2, "rb").read()
        blocks = fq.blocks_from_fastq(t1, t2)
        tmpl = fq.analyze_ids(blocks[0], False)
        assert tmpl[0] == 1
        return Case(name, blocks, fq.Config(bin_mode=1 if name == "pair_bin" else 0), tmpl)
    if name == "model_steps":                 # 2: qualities uniform over all 94 values
        rng = np.random.default_rng(2)
        recs = [b"@u%d\n%s\n+\n%s\n" % (i, rng.choice(np.frombuffer(b"ACGT", np.uint8), 100).tobytes(),
                                        rng.integers(33, 127, 100, dtype=np.uint8).tobytes()) for i in range(300)]
        return Case(name, fq.blocks_from_fastq(b"".join(recs)))
    if name == "const_qual":                  # 3: > 8,190 hits of one quality context
        rng = np.random.default_rng(3)
        recs = [b"@c%d\n%s\n+\n%s\n" % (i, rng.choice(np.frombuffer(b"ACGT", np.uint8), 150).tobytes(), b"F" * 150)
                for i in range(64)]
        return Case(name, fq.blocks_from_fastq(b"".join(recs)))
    if name == "poly_a":                      # 3: > 242 hits of one base context
        rng = np.random.default_rng(4)
        recs = [b"@a%d\n%s\n+\n%s\n" % (i, b"A" * 120, rng.integers(40, 70, 120, dtype=np.uint8).tobytes())
                for i in range(16)]
        return Case(name, fq.blocks_from_fastq(b"".join(recs)))
    if name == "shapes":                      # 4: read shapes
        return Case(name, fq.blocks_from_fastq(_read_shapes_text()))
    if name.startswith("level_"):             # 5: levels, on one small PE block
        a, b = synth.generate(400, paired=True, seed=3)
        kw = {"level_q1": {"qlevel": 1}, "level_q2": {"qlevel": 2}, "level_q3": {"qlevel": 3}, "level_s3": {"slevel": 3},
              "level_s4": {"slevel": 4}, "level_s9": {"slevel": 9}, "level_s8": {"slevel": 8},
              "level_nomd5": {"md5": False}}[name]
        return Case(name, fq.blocks_from_fastq(a, b), fq.Config(**kw))
    if name == "long":                        # 5: a read > 65,535 bp
        c = Case(name, fq.blocks_from_fastq(synth.generate(3, read_len=70000, seed=5)[0]))
        assert c.long == [True]
        return c
    if name == "groups":                      # 7: five unequal blocks
        a, b = synth.generate(1300, paired=True, seed=9)
        blocks = fq.blocks_from_fastq(a, b, 150_000)[:5]
        blocks[1], blocks[3] = blocks[3], fq.blocks_from_fastq(synth.generate(90, seed=10)[0])[0]
        assert len(blocks) == 5 and len({b.nreads for b in blocks}) > 1
        return Case(name, blocks)
    raise KeyError(name)


VALID = ["pair_bin", "pair_tok", "model_steps", "const_qual", "poly_a", "shapes", "level_q1", "level_q2", "level_q3",
         "level_s3", "level_s4", "level_s9", "level_nomd5", "long", "groups"]   # (+ level_s8: 4 GiB of base contexts)


# ---- the encap layout, to corrupt one stream of a block ----------------------
def encaps(block: bytes):
    """{id: (offset of the size4, payload offset, size)} of a no-reference block's streams."""
    assert block[0] == 0x81
    at, out = 5 + 6, {}          # past "81 <size4>" and the count encap "81 84 <le32>"
    assert block[5] == 0x81 and block[6] == 0x84
    while at < len(block):
        sid = block[at] & 0x7f
        size = struct.unpack_from(">I", block, at + 1)[0] & 0x0fffffff
        out[sid] = (at + 1, at + 5, size)
        at += 5 + size
    assert at == len(block)
    return out


def _resize(block: bytes, sid: int, new_size: int) -> bytes:
    """Stream sid cut to new_size bytes, its size4 and the block's rewritten."""
    hdr, pay, size = encaps(block)[sid]
    b = bytearray(block[:pay + new_size] + block[pay + size:])
    for at, delta in ((hdr, new_size - size), (1, new_size - size)):
        old = struct.unpack_from(">I", b, at)[0]
        struct.pack_into(">I", b, at, (old & 0xf0000000) | ((old & 0x0fffffff) + delta))
    return bytes(b)


def _flip(block: bytes, sid: int) -> bytes:
    _, pay, size = encaps(block)[sid]
    b = bytearray(block)
    b[pay + 16 + (size - 16) // 2] ^= 0x5a   # (past the stream's 16-byte digest)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """[(name, block bytes, cap, host verdict)]: the 'shapes' block with one
    stream damaged; verdict: sa_decode_block fails (returns -1 or md5_ok == 0)."""
    c = case("shapes")
    good, cap = c.enc[0], c.caps[0]
    e = encaps(good)
    out = [("qual_cut", _resize(good, 7, e[7][2] // 2)), ("seq_cut", _resize(good, 6, e[6][2] // 2)),
           ("qual_flip", _flip(good, 7)), ("seq_flip", _flip(good, 6))]
    b = bytearray(good)          # one more max-quality symbol than reads with the tip flag set
    cnt = struct.unpack_from("<I", b, e[24][1])[0]
    struct.pack_into("<I", b, e[24][1], cnt + 1)
    out.append(("side_count", bytes(b)))
    res = []
    for name, blk in out:
        try:
            _, ok = fq.decode_block(blk, cap, c.cfg, c.tmpl)
            failed = not ok
        except fq.SeqArcError:
            failed = True
        res.append((name, blk, cap, failed))
    return res


def equal_to_input(blk, got) -> bool:
    """got (a Block) holds exactly the reads that were encoded (bases as a decoder returns them)."""
    return (np.array_equal(got.name_lens, blk.name_lens) and np.array_equal(got.seq_lens, blk.seq_lens) and
            got.names.tobytes() == blk.names.tobytes() and np.array_equal(got.seq, _norm_seq(blk.seq)) and
            got.qual.tobytes() == blk.qual.tobytes())


# ---- the emulation -------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_emu")
    src = os.path.join(ROOT, "tests", "cpu_emu", "decode_emu.cpp")
    exe, san = d / "decode_emu", d / "decode_emu_san"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(san), src], check=True)
    return exe, san


def run_emu(exe, tmp_path, tag, cfg, tmpl, slice_, blocks):
    """blocks: [(bytes, long_reads, cap)] -> (process, rows of ints, outdir)."""
    f = tmp_path / f"{tag}.bin"
    f.write_bytes(struct.pack("<iiiiII", cfg.slevel, cfg.qlevel, 1 if cfg.md5 else 0, 1 if cfg.bin_mode else 0, slice_,
                              len(blocks)) + np.ascontiguousarray(tmpl, np.uint8).tobytes() +
                  b"".join(struct.pack("<III", len(e), 1 if lg else 0, cap) + e for e, lg, cap in blocks))
    outdir = tmp_path / f"{tag}_out"
    outdir.mkdir()
    r = subprocess.run([str(exe), "blocks", str(f), str(outdir)], capture_output=True)
    rows = [[int(x) for x in ln.split()] for ln in r.stdout.decode().split("\n")[:-1]]
    return r, rows, outdir


def _emu_block(outdir, i, cap):
    rd = lambda ext, dt: np.fromfile(outdir / f"{i}.{ext}", dt)
    return fq.Block(rd("names", np.uint8), rd("nl", np.uint16), rd("seq", np.uint8), rd("sl", np.int32),
                    rd("qual", np.uint8), cap)


def _check_valid(exe, tmp_path, name, slice_, tag):
    c = case(name)
    r, rows, outdir = run_emu(exe, tmp_path, tag, c.cfg, c.tmpl, slice_, list(zip(c.enc, c.long, c.caps)))
    assert r.returncode == 0 and r.stderr == b"" and len(rows) == len(c.blocks), r.stderr.decode()[-2000:]
    ev = 0
    for i, (blk, row, (hblk, hok)) in enumerate(zip(c.blocks, rows, c.host)):
        assert row[0] == blk.nreads and row[1] == OK, (name, i, row)
        got = _emu_block(outdir, i, c.caps[i])
        assert equal_to_input(blk, got), (name, i)
        assert got.seq.tobytes() == hblk.seq.tobytes() and got.qual.tobytes() == hblk.qual.tobytes(), (name, i)
        assert bool(row[2]) == hok, (name, i, row)
        ev |= row[3]
    return ev, rows


@pytest.mark.parametrize("name", VALID)
def test_valid_blocks_equal_the_input(emu, tmp_path, name):
    ev, _ = _check_valid(emu[0], tmp_path, name, BIG_SLICE, "v")
    if name == "model_steps":   # symbols found in list entries >= 64, bubble swaps across the 63 / 64 entry pair
        assert ev & EV_HIGH and ev & EV_SWAP_63_64, ev
    if name == "const_qual":
        assert ev & EV_HALVE, ev
    if name == "poly_a":
        assert ev & EV_BASE_HALVE, ev


def test_slevel8_plain_build(emu, tmp_path):
    """4^15 base contexts (4 GiB): the plain build only."""
    _check_valid(emu[0], tmp_path, "level_s8", BIG_SLICE, "s8")


@pytest.mark.parametrize("slice_", [61, 1])
def test_slices_resume_everywhere(emu, tmp_path, slice_):
    """Resume points at every position class (the start of a read, inside a '#' run,
    before a skipped N, at the last symbol): the stored state carries the chain."""
    _, rows = _check_valid(emu[0], tmp_path, "shapes", slice_, f"sl{slice_}")
    total = int(case("shapes").blocks[0].seq_lens.sum())
    assert rows[0][5] == max(1, -(-total // slice_)) and 1 < rows[0][4] <= rows[0][5], rows[0]


def _check_corrupt(exe, tmp_path, tag):
    c = case("shapes")
    bad = corrupt_cases()
    blocks = [(c.enc[0], False, c.caps[0])] + [(blk, False, cap) for _, blk, cap, _ in bad]
    r, rows, outdir = run_emu(exe, tmp_path, tag, c.cfg, c.tmpl, 4096, blocks)
    assert r.returncode == 0 and r.stderr == b"" and len(rows) == len(blocks), r.stderr.decode()[-2000:]
    assert rows[0][:3] == [c.blocks[0].nreads, OK, int(c.host[0][1])]
    for (name, _, _, host_failed), row in zip(bad, rows[1:]):
        assert (row[0] < 0 or row[2] == 0) == host_failed, (name, row)
        assert (row[0] < 0) == (row[1] != OK), (name, row)
    return {name: row for (name, _, _, _), row in zip(bad, rows[1:])}


def test_corrupt_blocks_fail_where_the_host_decoder_fails(emu, tmp_path):
    rows = _check_corrupt(emu[0], tmp_path, "bad")
    assert all(f for _, _, _, f in corrupt_cases())   # (each of these damages does break the block)
    assert rows["qual_cut"][1] in (INPUT, SLOT, PLACE) and rows["side_count"][1] == LAYOUT, rows


def test_under_sanitizers(emu, tmp_path):
    """The address + undefined-behaviour build: every payload, output and table is a
    heap block of exactly its size, so a read or write outside one is reported."""
    _check_corrupt(emu[1], tmp_path, "san_bad")
    for name in ("shapes", "model_steps", "const_qual", "poly_a", "level_q3", "level_s9", "level_s4", "long", "groups"):
        _check_valid(emu[1], tmp_path, name, BIG_SLICE, f"san_{name}")
    _check_valid(emu[1], tmp_path, "shapes", 61, "san_sl61")
    r = subprocess.run([str(emu[1]), "range0"], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.split() == [b"4", b"8"], (r.stdout, r.stderr)


def test_bounded_renormalisation(emu):
    """A squeeze that leaves range 0: the host decoder's loop would not return
    from that state; here it ends after 8 rounds (8 bytes read) with SA_DEC_RANGE."""
    r = subprocess.run([str(emu[0]), "range0"], capture_output=True, check=True)
    assert r.stdout.split() == [str(RANGE).encode(), b"8"]


# ---- plan_decode ---------------------------------------------------------------
def _plan(exe, slevel, qlevel, free, cap, blocks):
    args = [str(exe), "plan", str(slevel), str(qlevel), str(free), str(cap)] + [str(x) for b in blocks for x in b]
    lines = subprocess.run(args, capture_output=True, check=True).stdout.decode().split("\n")[:-1]
    keys = ("qual_table", "seq_table", "budget", "max_block", "inflight", "unsupported")
    return dict(zip(keys, map(int, lines[0].split()))), [tuple(map(int, ln.split())) for ln in lines[1:]]


def test_plan_decode(emu):
    exe = emu[0]
    blk = (9 << 20, 22 << 20, 1 << 16, 150_000)   # encoded bytes, bases, side bytes, reads: a 50 MiB block
    gib = 1 << 30
    p2, per2 = _plan(exe, 3, 2, 256 * gib, 0, [blk] * 5000)
    p3, per3 = _plan(exe, 3, 3, 256 * gib, 0, [blk] * 5000)
    assert p2["qual_table"] == (1 << 16) * 288 and p3["qual_table"] == (1 << 20) * 288
    assert per3[0][0] - per2[0][0] == p3["qual_table"] - p2["qual_table"]
    assert p2["seq_table"] == 4 * 4 ** 10
    # the block's own arrays are all there: payloads, lengths, side arrays, both outputs
    assert per2[0][0] >= blk[0] + 4 * blk[3] + blk[2] + p2["qual_table"] + p2["seq_table"] + 2 * blk[1]
    assert per2[0][0] < blk[0] + 4 * blk[3] + blk[2] + p2["qual_table"] + p2["seq_table"] + 2 * blk[1] + 4096
    p8, per8 = _plan(exe, 8, 2, 256 * gib, 0, [blk] * 2000)
    p9, _ = _plan(exe, 9, 2, 256 * gib, 0, [blk] * 2000)
    assert p8["seq_table"] == 4 * gib and p9["seq_table"] == 4
    # in flight: what the budget (7/8 of the free bytes) holds, at most the blocks there are, at most the cap
    assert p2["budget"] == 224 * gib and p2["inflight"] == p2["budget"] // per2[0][0] and p2["unsupported"] == 0
    assert 2000 < p2["inflight"] < 5000 and 500 < p3["inflight"] == p3["budget"] // per3[0][0] < 1000
    assert 1 < p8["inflight"] == p8["budget"] // per8[0][0] < 60
    small, _ = _plan(exe, 3, 2, gib, 0, [blk] * 2000)
    assert small["inflight"] == (gib - gib // 8) // per2[0][0] and 1 <= small["inflight"] < 20
    assert _plan(exe, 3, 2, 256 * gib, 0, [blk] * 3)[0]["inflight"] == 3
    assert _plan(exe, 3, 2, 256 * gib, 2, [blk] * 2000)[0]["inflight"] == 2
    # one block that does not fit on its own is unsupported; the others still run
    huge = (9 << 20, 600 << 20, 1 << 16, 150_000)
    p, per = _plan(exe, 3, 2, gib, 0, [blk, huge, blk])
    assert [u for _, u in per] == [0, 1, 0] and p["unsupported"] == 1 and p["inflight"] == 2
    p, per = _plan(exe, 8, 2, gib, 0, [blk])
    assert per[0][1] == 1 and p["inflight"] == 0 and p["unsupported"] == 1
