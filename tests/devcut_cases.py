"""Inputs of the device block cut's tests, shared by tests/test_devcut.py (the
CPU emulation of sa_devcut.h) and tests/test_gpu_devtext.py (k_dt_cut): the
synthetic pair, the golden pair and the hand-built cases, and the host cut they
are compared with.  Nothing here expects a particular length: the lengths must
be the host functions', whatever they are; only the reason a cut stops (`end`)
and, where it follows from the case's construction, the block count are stated."""
from __future__ import annotations

import functools
import os

import synth

MORE, DONE, FULL, NONE = 1, 2, 3, 4   # SA_CUT_*

BLOCK_SIZES = [8192, 65536, 65537, 1048576, 3000001]
# the host cut's block counts at BLOCK_SIZES (sa_cut_next_pe / sa_cut_next_se of mate 1)
SYNTH_PE = [3637, 440, 440, 28, 10]
SYNTH_SE = [1819, 219, 219, 14, 5]
GOLDEN_PE = [589, 73, 73, 5, 2]
PIECE = 300_001
PIECE_CAP = 3 << 20

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def synth_pair() -> tuple[bytes, bytes]:
    a, b = synth.generate(40_000, paired=True, seed=65)
    assert len(a) == len(b) == 14_297_154
    return a, b


@functools.lru_cache(maxsize=None)
def golden_pair() -> tuple[bytes, bytes]:
    with open(os.path.join(GOLDEN, "ERR2755197_test_1.fq"), "rb") as f:
        a = f.read()
    with open(os.path.join(GOLDEN, "ERR2755197_test_2.fq"), "rb") as f:
        b = f.read()
    return a, b


def first_line(t1: bytes) -> bytes:
    at = t1.find(b"\n")
    return t1 if at < 0 else t1[:at + 1]


def rec(name: bytes, seq: bytes, qual: bytes) -> bytes:
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


# a 32-byte record whose header is the first line of the hand-built texts
PLAIN = rec(b"ABCDEFGH", b"ACGTACGTA", b"IIIIIIIII")
assert len(PLAIN) == 32


def cases() -> list[dict]:
    """name, t1, t2 (None: single-end), bs, eof, max_blocks, and what is known of
    the answer: end (of one cut call that may cut every block), blocks (or None)."""
    out = []

    def add(name, t1, t2, bs, eof=True, max_blocks=4096, end=None, blocks=None, nocarry_differs=False):
        out.append(dict(name=name, t1=t1, t2=t2, bs=bs, eof=eof, max_blocks=max_blocks, end=end, blocks=blocks,
                        nocarry_differs=nocarry_differs))

    plain = PLAIN * 300
    # a quality line that begins with '@': a candidate that matches one byte
    qat = rec(b"ABCDEFGH", b"ACGTACGTA", b"@IIIIIIII") * 300
    add("qual_at_pe", qat, qat, 2000, end=DONE)
    add("qual_at_se", qat, None, 1000, end=DONE)
    # ... '@' plus six bytes of the first line: a false header
    fh = (PLAIN * 3 + rec(b"ABCDEFGH", b"ACGTACGTA", b"@ABCDEFII")) * 80
    add("false_header_pe", fh, fh, 1500)
    add("false_header_se", fh, None, 777)
    # A hit that exists only because the match counter is carried from one
    # candidate to the next.  Tail records: the quality line "@zzzzzzGH\n" ends
    # with three matches (G, H, newline at the first line's places), the header
    # "@ABzzzzzz" begins with three: 3 + 3 > 5 at the header, where a counter
    # reset per candidate finds nothing and goes on to the last plain header.
    tail = rec(b"ABzzzzzz", b"ACGTACGTA", b"@zzzzzzGH")
    carry = PLAIN * 20 + tail * 6 + PLAIN * 20
    add("carry_pe", carry, carry, 2 * 24 * 32, eof=False, max_blocks=1, end=FULL, blocks=1, nocarry_differs=True)
    add("carry_se", carry, None, 24 * 32, eof=False, max_blocks=1, end=FULL, blocks=1, nocarry_differs=True)
    # "\n@" across a tile edge: 128 records of 32 bytes are one 4 KiB tile, so every
    # 128th record's last newline is a tile's last byte and its '@' the next tile's first
    add("straddle_pe", plain, plain, 2 * (4096 + 16), end=DONE)
    add("straddle_se", plain, None, 4096 + 16, end=DONE)
    add("one_tile_window_pe", plain, plain, 8192, end=DONE)
    # ... and with a first record one byte longer the newline is a tile's first byte
    shifted = rec(b"ABCDEFGHX", b"ACGTACGTA", b"IIIIIIIII") + PLAIN * 299
    add("newline_first_of_tile_pe", shifted, shifted, 2 * (4096 + 16), end=DONE)
    add("newline_first_of_tile_se", shifted, None, 4096 + 1, end=DONE)
    # mates with different newline counts in their windows (mate 2's reads are longer)
    long2 = rec(b"ABCDEFGH", b"ACGTACGTA" * 3, b"IIIIIIIII" * 3) * 300
    add("different_counts_pe", plain, long2, 3000, end=DONE)
    add("different_counts_swapped_pe", long2, plain, 3000, end=DONE)
    # a walk back over several newlines: the window's last records' names share at
    # most five consecutive bytes with the first line (carried newline included)
    odd = rec(b"ABCxEFGy", b"ACGTACGTA", b"IIIIIIIII")
    walk = PLAIN * 30 + odd * 5 + PLAIN * 30
    add("walk_back_pe", walk, walk, 2 * 34 * 32 + 20, eof=False, max_blocks=1, end=FULL, blocks=1)
    add("walk_back_se", walk, None, 34 * 32 + 20, eof=False, max_blocks=1, end=FULL, blocks=1)
    # text without a final newline
    add("no_final_newline_pe", plain[:-1], plain[:-1], 3000, end=DONE)
    add("no_final_newline_se", plain[:-1], None, 3000, end=DONE)
    # one mate empty at eof, the other a full window
    add("one_mate_empty", plain, b"", 2000, end=NONE, blocks=0)
    # a window with no header at all: the walk runs down to the window's start
    bare = b"ACGTACGTAC\n" * 3000
    add("no_header_pe", bare, bare, 20000, end=NONE, blocks=0)
    add("no_header_se", bare, None, 20000, end=NONE, blocks=0)
    # (the window begins with a newline and nothing matches: the host walk ends on that newline)
    lead = b"\n" + b"ACGTACGTAC\n" * 300
    add("leading_newline_pe", lead, lead, 2000)
    # both inputs short
    add("both_short_eof", PLAIN * 5, PLAIN * 4, 100000, end=DONE, blocks=1)
    add("both_short_not_eof", PLAIN * 5, PLAIN * 4, 100000, eof=False, end=MORE, blocks=0)
    add("short_se_eof", PLAIN * 5, None, 100000, end=DONE, blocks=1)
    add("short_se_not_eof", PLAIN * 5, None, 100000, eof=False, end=MORE, blocks=0)
    # max_blocks reached
    add("max_blocks_pe", plain, plain, 2000, max_blocks=3, end=FULL, blocks=3)
    add("max_blocks_se", plain, None, 1000, max_blocks=3, end=FULL, blocks=3)
    return out


def host_cut(fq, t1: bytes, t2: bytes | None, bs: int, eof: bool, max_blocks: int):
    """Repeated fq.cut_next_se / fq.cut_next_pe over the texts: ([(len1, len2)], end)."""
    first = first_line(t1)
    p1 = p2 = 0
    out = []
    while True:
        a1, a2 = len(t1) - p1, (len(t2) - p2 if t2 is not None else 0)
        if a1 == 0 and a2 == 0 and eof:
            return out, DONE
        if len(out) >= max_blocks:
            return out, FULL
        if t2 is None:
            r = fq.cut_next_se(memoryview(t1)[p1:], eof, bs, first)
            if r is None:
                return out, (MORE if a1 < bs and not eof else NONE)
            r = (r, 0)
        else:
            half = (bs & 0xffffffff) >> 1
            r = fq.cut_next_pe(memoryview(t1)[p1:], eof, memoryview(t2)[p2:], eof, bs, first)
            if r is None:
                return out, (MORE if (a1 < half or a2 < half) and not eof else NONE)
        out.append(r)
        p1 += r[0]
        p2 += r[1]
