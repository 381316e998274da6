// sa_devcut.h -- the reader's block cut (cultPEbuf@0x432180, getEndPos@0x4320c0;
// fastq_host.cpp: sa_cut_next_se / sa_cut_next_pe_nl) over text that lies in
// device memory, as plain C++ for host and device.  sa_devtext.hip's kernels
// (k_dt_count, k_dt_cut) and the CPU emulation (tests/cpu_emu/devcut_emu.cpp)
// call the same functions.
//
// The text of one input is a linear buffer with a 16-byte-aligned base whose
// bytes up to the 16-byte boundary after `wr` are readable.  Its newlines are
// counted once per DC_TILE-byte tile of the buffer (tile t: bytes [t x 4096,
// (t + 1) x 4096), the tile that holds `wr` up to `wr`): a tile's count is
// final once the tile lies wholly below `wr`, and only those are read here;
// the partial tiles at both ends of a window are counted from their bytes.
//
// Lanes: the functions are written for ONE wave of DC_LANES lanes in lockstep.
// A lane object gives the two collectives they need, ballot(f) and sum(f) over
// f(lane); every other value, and so every branch, is the same in all lanes.
// On the device the object is the wave (DcWaveLanes), on the host a loop over
// the lanes (DcLoopLanes).
//
// Loops: every loop is bounded by the bytes or tiles of a window, the first
// line's length, the 64 bits of a ballot or max_blocks; the comment at each
// loop says which.  Nothing waits for another wave.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/seqarc_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SDC_HD __host__ __device__ inline
#else
#define SDC_HD inline
#endif

namespace sa {

constexpr uint32_t DC_TILE = 4096;   // (= PARSE_TILE: 256 threads x 16 bytes)
constexpr uint32_t DC_LANES = 64;

struct DcLoopLanes {   // the host's wave: the lanes one after the other
    template <class F> uint64_t ballot(F f) const
    {
        uint64_t m = 0;
        for (uint32_t l = 0; l < DC_LANES; l++)
            if (f(l)) m |= 1ull << l;
        return m;
    }
    template <class F> uint32_t sum(F f) const
    {
        uint32_t s = 0;
        for (uint32_t l = 0; l < DC_LANES; l++) s += f(l);
        return s;
    }
};

#if defined(__HIPCC__)
struct DcWaveLanes {   // one wave of 64 (k_dt_cut: __launch_bounds__(64))
    uint32_t lane;
    template <class F> __host__ __device__ uint64_t ballot(F f) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return __ballot(f(lane) ? 1 : 0);
#else
        (void)f;
        return 0;
#endif
    }
    template <class F> __host__ __device__ uint32_t sum(F f) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        uint32_t v = f(lane);
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
        return v;
#else
        (void)f;
        return 0;
#endif
    }
};
#endif

// One input's text as the cut sees it.
struct DcSide {
    const uint8_t* text;     // the buffer's base
    const uint32_t* tiles;   // newlines per tile of the buffer
    uint64_t pos;            // where the next block starts
    uint64_t wr;             // the end of the text
    int32_t eof;             // the text up to wr is the rest of the input
    int32_t pad_;
};

// Newlines among the 16 bytes at `at` (a multiple of 16) that lie in [lo, hi); hi > at.
SDC_HD uint32_t dc_mask16(const uint8_t* text, uint64_t at, uint64_t lo, uint64_t hi)
{
    struct alignas(16) V {
        uint32_t w[4];
    } v;
    __builtin_memcpy(&v, __builtin_assume_aligned(text + at, 16), 16);
    uint32_t m = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t x = v.w[k] ^ 0x0a0a0a0au;   // '\n' bytes are the zero bytes of x
        for (int j = 0; j < 4; j++)
            if (((x >> (8 * j)) & 0xffu) == 0) m |= 1u << (4 * k + j);
    }
    if (at < lo) m &= lo - at >= 16 ? 0u : ~0u << (uint32_t)(lo - at);
    if (at + 16 > hi) m &= (1u << (uint32_t)(hi - at)) - 1u;
    return m;
}

// k_dt_count: thread `th` of the 256 that count tile `tile` of a text that ends at wr
SDC_HD uint32_t dc_tile_thread_count(const uint8_t* text, uint64_t tile, uint64_t wr, uint32_t th)
{
    const uint64_t at = tile * DC_TILE + 16ull * th;
    return at < wr ? (uint32_t)__builtin_popcount(dc_mask16(text, at, 0, wr)) : 0u;
}

// newlines in text[lo, hi), from the bytes
template <class L> SDC_HD uint32_t dc_count_bytes(const L& ln, const uint8_t* text, uint64_t lo, uint64_t hi)
{
    if (lo >= hi) return 0;
    uint32_t n = 0;
    // 1 KiB a step: bounded by the range's bytes (the callers pass less than two tiles)
    for (uint64_t p = lo & ~15ull; p < hi; p += 16ull * DC_LANES)
        n += ln.sum([&](uint32_t l) -> uint32_t {
            const uint64_t at = p + 16ull * l;
            return at < hi ? (uint32_t)__builtin_popcount(dc_mask16(text, at, lo, hi)) : 0u;
        });
    return n;
}

// newlines in [lo, hi) of a side: whole tiles from their counts, the partial tiles from their bytes
template <class L> SDC_HD uint32_t dc_range_count(const L& ln, const DcSide& s, uint64_t lo, uint64_t hi)
{
    const uint64_t t0 = (lo + DC_TILE - 1) / DC_TILE, t1 = hi / DC_TILE;
    if (t0 >= t1) return dc_count_bytes(ln, s.text, lo, hi);
    uint32_t n = dc_count_bytes(ln, s.text, lo, t0 * DC_TILE) + dc_count_bytes(ln, s.text, t1 * DC_TILE, hi);
    n += ln.sum([&](uint32_t l) -> uint32_t {
        uint32_t c = 0;
        for (uint64_t t = t0 + l; t < t1; t += DC_LANES) c += s.tiles[t];   // bounded by the window's tiles
        return c;
    });
    return n;
}

// The newline of text[a, b) that has `back` newlines of the range after it: its
// position, or -1 with `back` lowered by the range's newlines.
template <class L> SDC_HD int64_t dc_select_from_end(const L& ln, const uint8_t* text, uint64_t a, uint64_t b, uint64_t& back)
{
    // 64 bytes a step from the end, bit l of the ballot the byte at e - 1 - l: bounded by the range's bytes
    for (uint64_t e = b; e > a; e = e - a > DC_LANES ? e - DC_LANES : a) {
        const uint64_t m = ln.ballot([&](uint32_t l) -> bool { return e - a > l && text[e - 1 - l] == '\n'; });
        const uint32_t c = (uint32_t)__builtin_popcountll(m);
        if (back >= c) {
            back -= c;
            continue;
        }
        uint64_t mm = m;
        for (uint64_t i = 0; i < back; i++) mm &= mm - 1;   // back < c <= 64
        return (int64_t)(e - 1 - (uint64_t)__builtin_ctzll(mm));
    }
    return -1;
}

// nl_from_end of fastq_host.cpp over [lo, hi) of a side: a tile search from the
// end over the tile counts, then the select inside the tile
template <class L> SDC_HD int64_t dc_nl_from_end(const L& ln, const DcSide& s, uint64_t lo, uint64_t hi, uint64_t back)
{
    const uint64_t t0 = (lo + DC_TILE - 1) / DC_TILE, t1 = hi / DC_TILE;
    if (t0 >= t1) return dc_select_from_end(ln, s.text, lo, hi, back);
    const int64_t r = dc_select_from_end(ln, s.text, t1 * DC_TILE, hi, back);
    if (r >= 0) return r;
    uint64_t t = t1;
    while (t > t0) {   // 64 tiles a step from the end: bounded by the window's tiles
        const uint64_t nt = t - t0 < DC_LANES ? t - t0 : DC_LANES;
        const uint32_t c64 = ln.sum([&](uint32_t l) -> uint32_t { return l < nt ? s.tiles[t - 1 - l] : 0u; });
        if (back >= c64) {
            back -= c64;
            t -= nt;
            continue;
        }
        for (uint64_t i = 0; i < nt; i++, t--) {   // the newline is in one of these nt tiles
            const uint32_t c = s.tiles[t - 1];
            if (back < c) return dc_select_from_end(ln, s.text, (t - 1) * DC_TILE, t * DC_TILE, back);
            back -= c;
        }
        return -1;   // (tile counts that disagree with their sum)
    }
    return dc_select_from_end(ln, s.text, lo, t0 * DC_TILE, back);
}

// end_pos of fastq_host.cpp (getEndPos@0x4320c0) over the window data[0, avail):
// from n down, the first "\n@" with pos + 1 < avail at which the consecutive
// match counter against the first line passes five.  The counter is carried
// from one candidate to the next and reset only by a mismatch; `carry` = false
// resets it at every candidate, which the binary does not (the emulation shows
// an input where the two differ).
template <class L>
SDC_HD int64_t dc_end_pos(const L& ln, const uint8_t* data, uint64_t avail, int64_t n, const uint8_t* first, uint64_t flen,
                          bool carry = true)
{
    if (n <= 0 || flen == 0) return 0;
    uint32_t run = 0;
    // positions n down to 1, 64 a step, bit l of the ballot the position p - l: bounded by n < the window's bytes
    for (int64_t p = n; p > 0; p -= DC_LANES) {
        uint64_t cand = ln.ballot([&](uint32_t l) -> bool {
            const int64_t pos = p - (int64_t)l;
            return pos > 0 && (uint64_t)pos + 1 < avail && data[pos] == '\n' && data[pos + 1] == '@';
        });
        while (cand) {   // the step's candidates from the highest position down: at most 64
            const int64_t pos = p - (int64_t)__builtin_ctzll(cand);
            cand &= cand - 1;
            if (!carry) run = 0;
            for (uint64_t kb = 0; kb < flen; kb += DC_LANES) {   // the header, 64 bytes a step: bounded by flen
                const uint32_t w = flen - kb < DC_LANES ? (uint32_t)(flen - kb) : DC_LANES;
                uint64_t m = ln.ballot([&](uint32_t l) -> bool {
                    const uint64_t at = (uint64_t)pos + 1 + kb + l;
                    return l < w && at < avail && data[at] == first[kb + l];
                });
                uint32_t left = w;
                while (left) {   // the runs of matches in the step's bits: each turn takes at least one of `left`
                    uint32_t lead = ~m == 0 ? 64u : (uint32_t)__builtin_ctzll(~m);
                    if (lead > left) lead = left;
                    if (run + lead > 5) return pos;
                    if (lead == left) {
                        run += lead;
                        break;
                    }
                    run = 0;
                    m = lead + 1 >= 64 ? 0 : m >> (lead + 1);
                    left -= lead + 1;
                }
            }
        }
    }
    return 0;
}

// The next block at the sides' positions: 0 and its lengths, or why there is
// none (SA_CUT_MORE / SA_CUT_DONE / SA_CUT_NONE).  s2 = nullptr: single-end.
// What sa_cut_next_se / sa_cut_next_pe return for the same bytes, avail and eof.
template <class L>
SDC_HD int dc_cut_block(const L& ln, const DcSide& s1, const DcSide* s2, uint64_t bs, const uint8_t* first, uint64_t flen,
                        uint64_t& l1, uint64_t& l2, bool carry = true)
{
    const uint64_t avail1 = s1.wr - s1.pos;
    l1 = l2 = 0;
    if (!s2) {
        if (avail1 == 0 && s1.eof) return SA_CUT_DONE;
        if (avail1 < bs) {   // the short read of the file's last buffer
            if (!s1.eof) return SA_CUT_MORE;
            l1 = avail1;
            return 0;
        }
        if (flen >= bs) return SA_CUT_NONE;
        const int64_t e = dc_end_pos(ln, s1.text + s1.pos, bs, (int64_t)(bs - flen), first, flen, carry);
        if (e <= 0) return SA_CUT_NONE;
        l1 = (uint64_t)e + 1;
        return 0;
    }
    const uint64_t avail2 = s2->wr - s2->pos;
    if (avail1 == 0 && avail2 == 0 && s1.eof && s2->eof) return SA_CUT_DONE;
    const uint64_t half = (uint64_t)((uint32_t)bs >> 1);
    if ((avail1 < half && !s1.eof) || (avail2 < half && !s2->eof)) return SA_CUT_MORE;
    const uint64_t a1 = avail1 < half ? avail1 : half, a2 = avail2 < half ? avail2 : half;
    if (a1 < half && a2 < half) {   // both reads short: the last block takes the rest
        l1 = avail1;
        l2 = avail2;
        return 0;
    }
    const uint64_t k1 = dc_range_count(ln, s1, s1.pos, s1.pos + a1), k2 = dc_range_count(ln, *s2, s2->pos, s2->pos + a2);
    const uint64_t k = k1 < k2 ? k1 : k2;
    if (k < 2) return SA_CUT_NONE;
    const uint64_t j = k - 2;
    const int64_t pj_abs = dc_nl_from_end(ln, s1, s1.pos, s1.pos + a1, k1 - 1 - j);
    if (pj_abs < 0) return SA_CUT_NONE;
    const int64_t pj = pj_abs - (int64_t)s1.pos;
    const int64_t pos = dc_end_pos(ln, s1.text + s1.pos, a1, pj, first, flen, carry);
    // The host walks back from newline j to the newline at pos, lowering j by
    // one per newline, and gives up when it passes pos or runs out.  pos <= pj;
    // pos > 0 is a newline (a candidate of end_pos), pos = 0 (no hit) is one
    // only if the window begins with it.  So the walk ends at pos exactly when
    // data[pos] is a newline, and then j has dropped by the newlines in [pos, pj).
    if (pos == 0 && s1.text[s1.pos] != '\n') return SA_CUT_NONE;
    const uint64_t jj = j - dc_range_count(ln, s1, s1.pos + (uint64_t)pos, s1.pos + (uint64_t)pj);
    const int64_t q = dc_nl_from_end(ln, *s2, s2->pos, s2->pos + a2, k2 - 1 - jj);
    if (q < 0) return SA_CUT_NONE;
    l1 = (uint64_t)pos + 1;
    l2 = (uint64_t)(q - (int64_t)s2->pos) + 1;
    return 0;
}

// As many blocks as the text holds, block 0 at the sides' positions and each
// further one where the last ended: their lengths, the count, and in *end why
// the cut stopped.
template <class L>
SDC_HD uint32_t dc_cut_blocks(const L& ln, DcSide s1, DcSide s2, bool pe, uint64_t bs, const uint8_t* first, uint64_t flen,
                              uint64_t* len1, uint64_t* len2, uint32_t max_blocks, int32_t* end, bool carry = true)
{
    uint32_t nb = 0;
    for (;;) {   // bounded by max_blocks
        uint64_t l1, l2;
        const bool done = pe ? s1.wr == s1.pos && s2.wr == s2.pos && s1.eof && s2.eof : s1.wr == s1.pos && s1.eof;
        if (!done && nb >= max_blocks) {
            *end = SA_CUT_FULL;
            return nb;
        }
        const int why = dc_cut_block(ln, s1, pe ? &s2 : nullptr, bs, first, flen, l1, l2, carry);
        if (why) {
            *end = why;
            return nb;
        }
        len1[nb] = l1;
        len2[nb] = l2;
        s1.pos += l1;
        s2.pos += l2;
        ++nb;
    }
}

}  // namespace sa
