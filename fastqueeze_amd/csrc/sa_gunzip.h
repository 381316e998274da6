// sa_gunzip.h -- ordinary gzip (gzip, pigz, concatenated members) inflated in
// parallel by two-stage speculation, written once as host+device functions on
// top of sa_inflate.h.  sa_gunzip.hip runs it one wave per chunk of compressed
// bytes; tests/cpu_emu/gunzip_emu.cpp drives the same functions sequentially
// (lane 0 of 1) against zlib before they run on the GPU.
//
//   find     gz_find_first: the first bit position of a chunk at which a
//            non-final dynamic block can start (gz_candidate).  Chunk 0 is the
//            call's known start.
//   spec     gz_wave: decode from a start, block after block, into uint16_t
//            symbols: < 256 a byte; 0x8000 | j byte j of the unknown 32 KiB
//            window before the start (j = 32767: the byte just before it).  A
//            wave stops where a block boundary IS the next start (GZ_MET).
//   chain    gz_chain_*: wave 0 is confirmed; a wave is confirmed when a
//            confirmed wave met its start.  Each confirmed wave's true window
//            follows from its predecessor's (gz_window_next).
//   resolve  text[off_j + i] = s < 256 ? s : window_j[s & 0x7fff]
//   crc      CRC-32 of the text in tasks of <= 64 KiB (crc32_share), combined
//            on the host per member (gz_crc_combine) and compared with the
//            trailers (GzAccount).
//
// Bit positions are absolute bit offsets into the call's input (< 2^31: a call
// takes at most GZ_MAX_IN bytes).
//
// Bounds, by construction:
//   input   as sa_inflate.h (InflBits); gz_bits57 and gz_header_len read
//           in[i] only with i < in_len.
//   symbols a wave's symbols reach global memory only in gz_flush, whose range
//           [fl, to) has to <= sp <= cap (a literal is produced only when
//           sp < cap, a match or stored block only when it fits: GZ_FULL).
//   ring    indices are masked with GZ_RING - 1.
//   loops   each symbol consumes >= 1 bit or ends its block, each block >= 3
//           bits, a member >= 18 bytes; the finder's loop is bounded by to_bit;
//           the chain visits strictly increasing wave indices.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "sa_inflate.h"

namespace sa {

constexpr uint32_t GZ_RING = 32768;          // symbols of the LDS ring: DEFLATE's window
constexpr uint32_t GZ_SPAN = 4096;           // unflushed symbols that trigger a flush
constexpr uint32_t GZ_MAX_BREAKS = 8;        // member ends one wave records
constexpr uint32_t GZ_MAX_IN = 1u << 28;     // bytes of one call's input (bit positions < 2^31)
constexpr uint32_t GZ_NONE = 0xffffffffu;    // no candidate in a chunk
constexpr uint32_t GZ_MET = SA_GZ_MET, GZ_FULL = SA_GZ_FULL, GZ_END = SA_GZ_END, GZ_BREAKS = SA_GZ_BREAKS,
                   GZ_OUTCAP = SA_GZ_OUTCAP;

struct GzBreak { uint32_t sym_off, crc, isize; };   // a member ended after sym_off symbols of the wave
// What a wave leaves.  Everything before its last boundary is good if the wave is confirmed.
struct GzWaveRes {
    uint32_t stop;        // GZ_MET, GZ_FULL, GZ_END, GZ_BREAKS or an SA_INFL_* status
    uint32_t met;         // GZ_MET: the index of the start it stopped at
    uint32_t lb_bit;      // last boundary: its bit position (a member header's: 8 x its byte)
    uint32_t lb_sym;      // ... the symbols produced before it
    uint32_t lb_header;   // ... 1: a member header (or the end of the input) stands there
    uint32_t lb_breaks;   // ... the breaks before it (all that were recorded)
    uint32_t skipped;     // starts the wave decoded past: false candidates
    uint32_t nsym;        // symbols flushed (>= lb_sym)
    GzBreak br[GZ_MAX_BREAKS];
};

// ---- block finder ----------------------------------------------------------
// 57 bits from bit position p (the bits past the input are zeros)
SAI_HD uint64_t gz_bits57(const uint8_t* in, uint32_t in_len, uint32_t p)
{
    const uint32_t at = p >> 3;
    uint64_t w = 0;
    if (at + 8 <= in_len) {
        __builtin_memcpy(&w, in + at, 8);
    } else {
        for (uint32_t i = 0; i < 8 && at + i < in_len; i++) w |= (uint64_t)in[at + i] << (8 * i);
    }
    return w >> (p & 7u);
}

// Tests 1-3 of a candidate, per lane, no tables: BFINAL = 0 and BTYPE = 2;
// HLIT <= 29 and HDIST <= 29; the code-length code complete and not
// over-subscribed (Kraft sum of its HCLEN + 4 lengths, in units of 2^-7, is 128:
// what infl_build asks of it).
SAI_HD bool gz_precheck(const uint8_t* in, uint32_t in_len, uint32_t p)
{
    const uint64_t h = gz_bits57(in, in_len, p);
    if ((h & 7u) != 4u) return false;
    if (((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
    const uint32_t ncode = (uint32_t)((h >> 13) & 15u) + 4;
    if ((uint64_t)p + 17 + 3 * ncode > 8ull * in_len) return false;
    const uint64_t c = gz_bits57(in, in_len, p + 17);   // 19 x 3 bits
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < ncode; i++) {
        const uint32_t l = (uint32_t)(c >> (3 * i)) & 7u;
        kraft += l ? 128u >> l : 0u;
    }
    return kraft == 128u;
}

// the bit buffer at bit position p (p <= 8 in_len)
SAI_HD InflBits gz_bits_at(const uint8_t* in, uint32_t in_len, uint32_t p)
{
    InflBits b{in, in_len, p >> 3, 0, 0, 0, 0xffffffffu};
    infl_refill(b);
    uint32_t v;
    (void)infl_take(b, p & 7u, v);   // (fewer bits than that: nothing is left, and the next take fails)
    return b;
}

SAI_HD uint32_t gz_bitpos(const InflBits& b) { return 8u * b.ip - b.bits; }

// Test 4, by the whole wave (p is wave-uniform): infl_dynamic as it stands.
SAI_HD bool gz_candidate(const uint8_t* in, uint32_t in_len, uint32_t p, InflTabs& t, uint32_t lane, uint32_t nl)
{
    if (!gz_precheck(in, in_len, p)) return false;
    InflBits b = gz_bits_at(in, in_len, p);
    uint32_t v, nlen, ndist;
    if (!infl_take(b, 3, v)) return false;
    return infl_dynamic(b, t, nlen, ndist, lane, nl) == 0;
}

// the lanes (bit i: lane i) for which ok holds; one lane on the host
SAI_HD uint64_t gz_ballot(bool ok)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(ok);
#else
    return ok ? 1u : 0u;
#endif
}

// The first candidate in [from_bit, to_bit), or GZ_NONE.  The nl lanes test nl
// consecutive positions a step (tests 1-3); the survivors go through test 4 one
// at a time, lowest first.  Bounded by to_bit: the outer loop advances nl bits a
// step, the inner one clears one bit of the mask a step.
SAI_HD uint32_t gz_find_first(const uint8_t* in, uint32_t in_len, uint32_t from_bit, uint32_t to_bit, InflTabs& t,
                              uint32_t lane, uint32_t nl)
{
    for (uint32_t base = from_bit; base < to_bit; base += nl) {
        const uint32_t p = base + lane;
        uint64_t mask = gz_ballot(p < to_bit && gz_precheck(in, in_len, p));
        while (mask) {
            const uint32_t k = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1;
            if (gz_candidate(in, in_len, base + k, t, lane, nl)) return base + k;
        }
    }
    return GZ_NONE;
}

// ---- gzip member header ----------------------------------------------------
// The header at in[at..): 0 ok (hlen), 1 the input ends inside it, 2 not a gzip header.
SAI_HD uint32_t gz_header_len(const uint8_t* in, uint32_t in_len, uint32_t at, uint32_t& hlen)
{
    const uint32_t left = in_len - at;   // at <= in_len
    if ((left > 0 && in[at] != 0x1f) || (left > 1 && in[at + 1] != 0x8b) || (left > 2 && in[at + 2] != 8) ||
        (left > 3 && (in[at + 3] & 0xe0)))
        return 2;
    if (left < 10) return 1;
    const uint32_t flg = in[at + 3];
    uint32_t p = at + 10;
    if (flg & 4u) {   // FEXTRA
        if (in_len - p < 2) return 1;
        const uint32_t xlen = in[p] | (uint32_t)in[p + 1] << 8;
        p += 2;
        if (in_len - p < xlen) return 1;
        p += xlen;
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1) {   // FNAME, FCOMMENT: zero-terminated (bounded by in_len)
        if (!(flg & f)) continue;
        while (p < in_len && in[p]) p++;
        if (p == in_len) return 1;
        p++;
    }
    if (flg & 2u) {   // FHCRC
        if (in_len - p < 2) return 1;
        p += 2;
    }
    hlen = p - at;
    return 0;
}

// ---- speculative wave ------------------------------------------------------
// ring[fl & .., to & ..) to out[fl, to): whole 8-symbol vectors (16 bytes: out
// and the ring are 16-byte aligned and fl is a multiple of 8), then -- the last
// flush only -- the symbols left.  to <= cap: the caller's.
SAI_HD void gz_flush(const uint16_t* ring, uint16_t* out, uint32_t& fl, uint32_t to, uint32_t lane, uint32_t nl)
{
    struct alignas(16) Vec { uint32_t w[4]; };
    const uint32_t v1 = to >> 3;
    for (uint32_t v = (fl >> 3) + lane; v < v1; v += nl) {
        Vec x;
        __builtin_memcpy(&x, __builtin_assume_aligned(ring + ((v << 3) & (GZ_RING - 1)), 16), 16);
        __builtin_memcpy(__builtin_assume_aligned(out + ((size_t)v << 3), 16), &x, 16);
    }
    for (uint32_t i = (v1 << 3) + lane; i < to; i += nl) out[i] = ring[i & (GZ_RING - 1)];
    fl = to & ~7u;
}

// The symbols of one Huffman block.  sp: symbols produced; a match may reach
// back `sp - brk + init` symbols (brk: sp at the last member break; init: the
// history before the wave that still counts).
// INVARIANT of the ring: symbol i lives in ring[i mod 32768] until symbol
// i + 32768 is produced.  A flush runs as soon as GZ_SPAN symbols are unflushed,
// and one step produces at most 258 (a stored block goes in pieces of GZ_SPAN),
// so unflushed + 258 <= 2 GZ_SPAN + 258 -- far below 32768: nothing unflushed is
// overwritten, and the 32768 symbols a match may read are all there.  A match at
// distance 32768 reads and writes the same slot: in a lockstep wave each lane
// loads before it stores, and the value does not change.
SAI_HD uint32_t gz_block(InflBits& b, const InflTabs& t, uint32_t nlsym, uint32_t ndsym, uint16_t* ring, uint16_t* out,
                         uint32_t cap, uint32_t& sp, uint32_t& fl, uint32_t brk, uint32_t init, uint32_t lane, uint32_t nl)
{
    constexpr uint32_t M = GZ_RING - 1;
    for (;;) {   // >= 1 bit a step, or the block ends
        infl_refill(b);
        uint32_t sym;
        uint32_t st = infl_sym(b, t.lit, INFL_LBITS, t.lsorted, nlsym, t.lcnt, sym);
        if (st) return st;
        if (sym < 256) {
            if (sp >= cap) return GZ_FULL;
            ring[sp & M] = (uint16_t)sym;   // (every lane stores the same symbol)
            sp++;
        } else {
            if (sym == 256) return 0;
            if (sym >= 286) return SA_INFL_CODES;
            sym -= 257;
            uint32_t len, v;
            if (sym < 8) {
                len = 3 + sym;
            } else if (sym == 28) {
                len = 258;
            } else {
                const uint32_t xb = (sym - 4) >> 2;
                if (!infl_take(b, xb, v)) return SA_INFL_INPUT;
                len = 3 + ((4 + (sym & 3u)) << xb) + v;
            }
            uint32_t ds;
            st = infl_sym(b, t.dst, INFL_DBITS, t.dsorted, ndsym, t.dcnt, ds);
            if (st) return st;
            if (ds >= 30) return SA_INFL_CODES;
            uint32_t dist;
            if (ds < 4) {
                dist = 1 + ds;
            } else {
                const uint32_t xb = (ds - 2) >> 1;
                if (!infl_take(b, xb, v)) return SA_INFL_INPUT;
                dist = 1 + ((2 + (ds & 1u)) << xb) + v;
            }
            if (dist > GZ_RING || dist > sp - brk + init) return SA_INFL_DIST;
            if (len > cap - sp) return GZ_FULL;   // (sp <= cap)
            // the source [sp - dist, sp) is complete before the copy: symbol i of an
            // overlapping match is source symbol i mod dist.  Markers are copied as they are.
            const uint32_t s0 = sp - dist;   // (mod 2^32: masked below)
            if (dist >= len) {
                for (uint32_t i = lane; i < len; i += nl) ring[(sp + i) & M] = ring[(s0 + i) & M];
            } else if (dist == 1) {
                const uint16_t c = ring[s0 & M];
                for (uint32_t i = lane; i < len; i += nl) ring[(sp + i) & M] = c;
            } else {
                for (uint32_t i = lane; i < len; i += nl) ring[(sp + i) & M] = ring[(s0 + i % dist) & M];
            }
            sp += len;
        }
        if (sp - fl >= GZ_SPAN) gz_flush(ring, out, fl, sp & ~7u, lane, nl);
    }
}

// Decodes from starts[self], one block after another, until a stop (GzWaveRes).
//   known       the call's start (self == 0): the window is win[32768 - win_len ..
//               32768), real bytes; at_header: a member header stands at the start
//               (win_len = 0).  Otherwise a candidate: the window is markers.
//   starts      the call's starts, strictly ascending (starts[0]: the known one)
//   out, cap    the wave's symbol range (16-byte aligned; cap a multiple of 8)
// At every block boundary: (a) the boundary is recorded, (b) starts below the
// position are skipped (they were false), (c) a start AT the position stops the
// wave with GZ_MET, (d) after a final block the trailer is read, a break is
// recorded and the next member's header parsed.
// The result goes to *res by lane 0's plain stores.
SAI_HD void gz_wave(const uint8_t* in, uint32_t in_len, const uint32_t* starts, uint32_t nstarts, uint32_t self, bool known,
                    bool at_header, const uint8_t* win, uint32_t win_len, uint16_t* ring, InflTabs& t, uint16_t* out,
                    uint32_t cap, GzWaveRes* res, uint32_t lane, uint32_t nl)
{
    constexpr uint32_t M = GZ_RING - 1;
    if (known) {
        for (uint32_t j = lane; j < GZ_RING; j += nl) ring[j] = j >= GZ_RING - win_len ? win[j] : 0;
    } else {
        for (uint32_t j = lane; j < GZ_RING; j += nl) ring[j] = (uint16_t)(0x8000u | j);
    }
    const uint32_t start = starts[self];
    uint32_t sp = 0, fl = 0, brk = 0, init = known ? win_len : GZ_RING, nbr = 0, nx = self + 1, skipped = 0;
    uint32_t lb_bit = start, lb_sym = 0, lb_header = at_header ? 1u : 0u, lb_breaks = 0, met = 0, stop;
    bool need_header = at_header;
    InflBits b = gz_bits_at(in, in_len, start);
    for (;;) {   // a block or a member header a step: >= 3 bits, bounded by 8 in_len
        if (need_header) {
            const uint32_t at = lb_bit >> 3;
            if (at == in_len) { stop = GZ_END; break; }
            uint32_t hlen = 0;
            const uint32_t h = gz_header_len(in, in_len, at, hlen);
            if (h == 1) { stop = SA_INFL_INPUT; break; }
            // bytes that are no member after a member end the stream, as gzread has it
            if (h == 2) { stop = nbr || !known ? GZ_END : (uint32_t)SA_INFL_HEADER; break; }
            b = gz_bits_at(in, in_len, 8u * (at + hlen));
            need_header = false;
        }
        const uint32_t pos = gz_bitpos(b);
        lb_bit = pos;   // (a)
        lb_sym = sp;
        lb_header = 0;
        lb_breaks = nbr;
        while (nx < nstarts && starts[nx] < pos) {   // (b)  (bounded by nstarts)
            nx++;
            skipped++;
        }
        if (nx < nstarts && starts[nx] == pos) {   // (c)
            stop = GZ_MET;
            met = nx;
            break;
        }
        infl_refill(b);
        uint32_t hdr, v;
        if (!infl_take(b, 3, hdr)) { stop = SA_INFL_INPUT; break; }
        const uint32_t type = hdr >> 1;
        uint32_t st = 0;
        if (type == 0) {
            (void)infl_take(b, b.bits & 7u, v);   // to the byte boundary
            infl_refill(b);
            if (!infl_take(b, 32, v)) { stop = SA_INFL_INPUT; break; }
            const uint32_t n = v & 0xffffu;
            if (n != ((v >> 16) ^ 0xffffu)) { stop = SA_INFL_BLOCK; break; }
            const uint32_t at = b.ip - (b.bits >> 3);   // the bytes still in the bit buffer lie before ip
            if (n > in_len - at) { stop = SA_INFL_INPUT; break; }
            if (n > cap - sp) { stop = GZ_FULL; break; }
            for (uint32_t done = 0; done < n;) {   // the bytes as literal symbols, a span at a time
                const uint32_t piece = n - done < GZ_SPAN ? n - done : GZ_SPAN;
                for (uint32_t i = lane; i < piece; i += nl) ring[(sp + i) & M] = in[at + done + i];
                sp += piece;
                done += piece;
                if (sp - fl >= GZ_SPAN) gz_flush(ring, out, fl, sp & ~7u, lane, nl);
            }
            b.ip = at + n;
            b.hold = 0;
            b.bits = 0;
        } else if (type == 3) {
            st = SA_INFL_BLOCK;
        } else {
            uint32_t nlsym = 288, ndsym = 32;
            if (type == 1) infl_fixed(t, lane, nl);
            else st = infl_dynamic(b, t, nlsym, ndsym, lane, nl);
            if (!st) st = gz_block(b, t, nlsym, ndsym, ring, out, cap, sp, fl, brk, init, lane, nl);
        }
        if (st) { stop = st; break; }
        if (hdr & 1u) {   // (d) the member's trailer
            (void)infl_take(b, b.bits & 7u, v);
            const uint32_t at = b.ip - (b.bits >> 3);
            if (in_len - at < 8) { stop = SA_INFL_INPUT; break; }
            const uint32_t crc = in[at] | (uint32_t)in[at + 1] << 8 | (uint32_t)in[at + 2] << 16 | (uint32_t)in[at + 3] << 24;
            const uint32_t isz = in[at + 4] | (uint32_t)in[at + 5] << 8 | (uint32_t)in[at + 6] << 16 | (uint32_t)in[at + 7] << 24;
            if (lane == 0) res->br[nbr] = GzBreak{sp, crc, isz};   // (nbr < GZ_MAX_BREAKS: the wave stops at the eighth)
            nbr++;
            brk = sp;
            init = 0;
            lb_bit = 8u * (at + 8);
            lb_sym = sp;
            lb_header = 1;
            lb_breaks = nbr;
            need_header = true;
            if (nbr == GZ_MAX_BREAKS) { stop = at + 8 == in_len ? GZ_END : GZ_BREAKS; break; }
        }
    }
    gz_flush(ring, out, fl, sp, lane, nl);
    if (lane == 0) {
        res->stop = stop;
        res->met = met;
        res->lb_bit = lb_bit;
        res->lb_sym = lb_sym;
        res->lb_header = lb_header;
        res->lb_breaks = lb_breaks;
        res->skipped = skipped;
        res->nsym = sp;
    }
}

// ---- chain -----------------------------------------------------------------
// The true window after a confirmed wave: the last 32768 of window ++ symbols
// (both windows right-aligned in 32768 bytes); a wave that produced fewer than
// 32768 symbols shifts the old window in.  The lanes split the bytes.
SAI_HD void gz_window_next(const uint8_t* win, const uint16_t* sym, uint32_t nsym, uint8_t* nwin, uint32_t lane, uint32_t nl)
{
    for (uint32_t i = lane; i < GZ_RING; i += nl) {
        const uint32_t q = nsym + i;   // index in window ++ symbols of byte i of the last 32768
        uint8_t c;
        if (q < GZ_RING) {
            c = win[q];
        } else {
            const uint16_t s = sym[q - GZ_RING];
            c = s < 256 ? (uint8_t)s : win[s & 0x7fffu];
        }
        nwin[i] = c;
    }
}

// the real bytes of the window after a wave that used nsym symbols up to its boundary
SAI_HD uint32_t gz_win_len_next(uint32_t win_len, const GzWaveRes& r)
{
    const uint64_t n = r.lb_breaks ? (uint64_t)(r.lb_sym - r.br[r.lb_breaks - 1].sym_off) : (uint64_t)win_len + r.lb_sym;
    return n < GZ_RING ? (uint32_t)n : GZ_RING;
}

// What the chain leaves: the confirmed waves in order, their text offsets and window lengths.
struct GzChainEnd {
    uint32_t nconf;       // confirmed waves (order[0..nconf))
    uint32_t end_wave;    // the wave that ended the prefix
    uint32_t end_why;     // its stop, or GZ_OUTCAP: the text up to it fills out_cap
    uint32_t end_bit;     // where the next call starts
    uint32_t end_header;  // ... 1: at a member header
    uint32_t end_slot;    // the window slot that holds the next call's window
    uint32_t end_win_len;
    uint32_t skipped;     // false candidates the confirmed waves decoded past
    uint64_t text;        // bytes of text of the prefix
};

// One step of the chain at wave j (confirmed), all scalars; the caller derives
// the window (gz_window_next into slot `next_slot`) when it returns true.
// Returns false when the prefix ended before j (out_cap).
struct GzChainStep { uint32_t next_slot, next_len; bool last; };
SAI_HD bool gz_chain_step(const GzWaveRes& r, uint32_t j, uint32_t nw, const uint32_t* starts, uint32_t win_len, uint64_t out_cap,
                          bool first_header, GzChainEnd& e, GzChainStep& s)
{
    if (e.text + r.lb_sym > out_cap) {
        e.end_wave = j;
        e.end_why = GZ_OUTCAP;
        e.end_bit = starts[j];
        e.end_header = j == 0 && first_header;
        e.end_slot = j;   // (j's own window)
        e.end_win_len = win_len;
        return false;
    }
    e.nconf++;
    e.text += r.lb_sym;
    e.skipped += r.skipped;
    s.next_len = gz_win_len_next(win_len, r);
    s.last = r.stop != GZ_MET || r.met <= j || r.met >= nw;   // (met > j always: the chain only moves forward)
    s.next_slot = s.last ? nw : r.met;
    if (s.last) {
        e.end_wave = j;
        e.end_why = r.stop == GZ_MET ? (uint32_t)SA_INFL_BLOCK : r.stop;
        e.end_bit = r.lb_bit;
        e.end_header = r.lb_header;
        e.end_slot = nw;
        e.end_win_len = s.next_len;
    }
    return true;
}

// a text byte; bad: a marker that points before the window's real bytes
SAI_HD uint8_t gz_resolve_sym(uint16_t s, const uint8_t* win, uint32_t win_len, bool& bad)
{
    if (s < 256) return (uint8_t)s;
    const uint32_t j = s & 0x7fffu;
    if (j < GZ_RING - win_len) bad = true;
    return win[j];
}

// ---- CRC-32 of pieces of any length ------------------------------------------
// x^(8 n) mod P
SAI_HD uint32_t gz_crc_xpow8(uint64_t n)
{
    uint32_t sq = 1u << 23;   // x^8
    uint32_t p = 1u << 31;    // x^0
    for (; n; n >>= 1) {      // <= 64 steps
        if (n & 1u) p = crc32_mul(sq, p);
        sq = crc32_mul(sq, sq);
    }
    return p;
}

// CRC-32 of A ++ B from CRC-32(A), CRC-32(B) and B's length: zlib's crc32_combine
SAI_HD uint32_t gz_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    return crc32_mul(gz_crc_xpow8(len_b), crc_a) ^ crc_b;
}

// ---- the call's host side (shared by sa_gunzip_run and the emulation) -------
struct GzPlan {
    std::vector<uint32_t> starts, cap;   // per wave: start bit, symbols of its range
    std::vector<uint64_t> base;          // ... the range's first symbol (a multiple of 8)
    uint64_t total = 0;                        // symbols of all ranges
    uint32_t candidates = 0;
};

// Compacts the finder's per-chunk candidates (cand[0] is unused: chunk 0 is the
// known start at start0) and sizes each wave's symbol range: ratio x (compressed
// bytes up to the next start) + 64 Ki symbols, a multiple of 8.  A wave counts
// at most GZ_RANGE_CHUNKS chunks of compressed bytes: a start lies in nearly
// every chunk, and where none does for longer (stored or fixed blocks only) the
// wave stops GZ_FULL at a block boundary and the next call goes on from there --
// or the caller's host path does.
constexpr uint32_t GZ_RANGE_CHUNKS = 4;
constexpr uint32_t GZ_RANGE_MIN = 1u << 20;   // ... and at least 1 MiB of them (small chunks: a block is many chunks long)
inline void gz_plan(const uint32_t* cand, uint32_t nchunks, uint32_t chunk, uint32_t start0, uint32_t in_len, uint32_t ratio,
                    GzPlan& p)
{
    p.starts.assign(1, start0);
    for (uint32_t k = 1; k < nchunks; k++)
        if (cand[k] != GZ_NONE && cand[k] > p.starts.back()) p.starts.push_back(cand[k]);
    p.candidates = (uint32_t)p.starts.size() - 1;
    const size_t nw = p.starts.size();
    p.base.resize(nw);
    p.cap.resize(nw);
    p.total = 0;
    for (size_t j = 0; j < nw; j++) {
        const uint64_t end = j + 1 < nw ? p.starts[j + 1] : 8ull * in_len;
        const uint64_t bytes = std::min<uint64_t>((end - p.starts[j]) / 8 + 1, std::max<uint64_t>((uint64_t)GZ_RANGE_CHUNKS * chunk, GZ_RANGE_MIN));
        uint64_t c = (uint64_t)ratio * bytes + 65536;
        c = std::min<uint64_t>((c + 7) & ~7ull, 1u << 30);
        p.base[j] = p.total;
        p.cap[j] = (uint32_t)c;
        p.total += c;
    }
}

// The members of the confirmed prefix: text pieces cut at the breaks, in CRC
// tasks of <= 64 KiB; after the tasks' CRCs are known, walk() combines them per
// member onto the state's running CRC and length and compares with the trailers.
struct GzAccount {
    struct Task { uint64_t off; uint32_t len; };
    struct Item { uint32_t task_or_break; GzBreak br; bool is_break; };
    std::vector<Task> tasks;
    std::vector<Item> items;
    uint64_t at = 0;   // text consumed into tasks
    void piece_to(uint64_t end)
    {
        while (at < end) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(end - at, 64 * INFL_CRC_CHUNK);
            items.push_back(Item{(uint32_t)tasks.size(), GzBreak{}, false});
            tasks.push_back(Task{at, n});
            at += n;
        }
    }
    // a confirmed wave: its text offset and its result
    void wave(uint64_t text_off, const GzWaveRes& r)
    {
        for (uint32_t k = 0; k < r.lb_breaks && k < GZ_MAX_BREAKS; k++) {
            piece_to(text_off + r.br[k].sym_off);
            items.push_back(Item{0, r.br[k], true});
        }
        piece_to(text_off + r.lb_sym);
    }
    // 0, or SA_INFL_CRC / SA_INFL_SIZE of the first member that fails; crc / len: the running member's
    uint32_t walk(const uint32_t* task_crc, uint32_t& crc, uint64_t& len, uint32_t& members) const
    {
        for (const Item& it : items) {
            if (!it.is_break) {
                const Task& t = tasks[it.task_or_break];
                crc = len ? gz_crc_combine(crc, task_crc[it.task_or_break], t.len) : task_crc[it.task_or_break];
                len += t.len;
                continue;
            }
            if ((len ? crc : 0u) != it.br.crc) return SA_INFL_CRC;
            if ((uint32_t)len != it.br.isize) return SA_INFL_SIZE;
            members++;
            crc = 0;
            len = 0;
        }
        return 0;
    }
};

// The CRC-32 of data[0..len), len <= 64 KiB, as the 64 lanes' shares combine (the
// emulation's form of k_gz_crc; tab: the byte table).
inline uint32_t gz_crc_task(const uint8_t* data, uint32_t len, const uint32_t* tab)
{
    if (!len) return 0;
    uint32_t x = 0;
    for (uint32_t lane = 0; lane < 64; lane++) x ^= crc32_share(data, len, lane, crc32_chunk_shift(63 - lane), tab);
    return ~x;
}

// One call (sa_gunzip_run's body), over a backend that runs the stages: the
// kernels of sa_gunzip.hip, or the emulation's sequential loops.
//   bool upload(in, in_len, state)                      the input, and the state's window into slot 0
//   bool find(nchunks, chunk, cand)                     cand[k]: chunk k's first candidate or GZ_NONE (k >= 1)
//   bool spec(plan, at_header, win_len)                 a wave per start
//   bool chain(plan, win_len, out_cap, first_header, end, order, woff, wwl, res)
//   bool resolve(plan, order, woff, wwl, res, out, text) the text into out[0..text)
//   bool crc(tasks, out, crcs)                          the CRC-32 of each task's bytes
//   bool window(slot, dst)                              a window slot's 32768 bytes
//   bool finish(info, bad)                              the three above are complete (they may only
//                                                       have been queued); bad: a marker pointed before
//                                                       a window's real bytes; the kernel times
template <class Backend>
int gz_run(Backend& be, const uint8_t* in, uint64_t in_bytes, int eof, sa_gunzip_state* st, uint8_t* out, uint64_t out_cap,
           uint64_t* out_bytes, uint64_t* in_used, sa_gunzip_info* info, uint32_t chunk, uint32_t ratio, std::string& err)
{
    sa_gunzip_info inf{};
    *out_bytes = 0;
    *in_used = 0;
    if (info) *info = inf;
    if (st->ended) return 0;
    if (in_bytes > GZ_MAX_IN) {
        err = "sa_gunzip_run: more than 256 MiB of input in one call";
        return -1;
    }
    if (st->bit > 7 || st->win_len > GZ_RING || (!st->in_stream && (st->bit || st->win_len))) {
        err = "sa_gunzip_run: the state is not one a call left";
        return -1;
    }
    if (!in_bytes) {
        if (eof && st->in_stream) {
            inf.status = inf.end_why = SA_INFL_INPUT;
            if (info) *info = inf;
            return SA_INFL_INPUT;
        }
        return 0;
    }
    const uint32_t in_len = (uint32_t)in_bytes;
    const uint32_t nchunks = (in_len + chunk - 1) / chunk;
    const bool first_header = !st->in_stream;
    std::vector<uint32_t> cand(nchunks, GZ_NONE);
    GzPlan plan;
    GzChainEnd end{};
    std::vector<uint32_t> order, wwl;
    std::vector<uint64_t> woff;
    std::vector<GzWaveRes> res;
    if (!be.upload(in, in_len, st) || !be.find(nchunks, chunk, cand.data())) return -1;
    gz_plan(cand.data(), nchunks, chunk, st->in_stream ? st->bit : 0u, in_len, ratio, plan);
    if (!be.spec(plan, first_header, st->win_len) || !be.chain(plan, st->win_len, out_cap, first_header, end, order, woff, wwl, res))
        return -1;
    inf.chunks = nchunks;
    inf.candidates = plan.candidates;
    inf.waves_confirmed = end.nconf;
    inf.false_skipped = end.skipped;
    inf.end_wave = end.end_wave;
    inf.end_why = end.end_why;
    if (!end.nconf) {
        err = "sa_gunzip_run: out_cap is too small for the first wave's text";
        if (info) *info = inf;
        return -2;
    }
    GzAccount acc;
    for (uint32_t k = 0; k < end.nconf; k++) acc.wave(woff[k], res[order[k]]);
    bool bad = false;
    std::vector<uint32_t> crcs(acc.tasks.size());
    if (!be.resolve(plan, order, woff, wwl, res, out, end.text) || !be.crc(acc.tasks, out, crcs) ||
        !be.window(end.end_slot, st->window) || !be.finish(inf, bad))
        return -1;
    *out_bytes = end.text;
    *in_used = end.end_bit >> 3;
    uint32_t crc = st->crc;
    uint64_t len = st->len;
    uint32_t status = bad ? (uint32_t)SA_INFL_DIST : acc.walk(crcs.data(), crc, len, inf.members_ended);
    st->in_stream = end.end_header ? 0u : 1u;
    st->bit = end.end_header ? 0u : end.end_bit & 7u;
    st->win_len = end.end_header ? 0u : end.end_win_len;
    st->crc = crc;
    st->len = len;
    if (!status) {
        const uint32_t why = end.end_why;
        if (why == SA_INFL_INPUT) status = eof ? why : 0u;   // (not at the end of the file: more input decides)
        else if (why < GZ_MET) status = why;
        else if (why == GZ_END && *in_used < in_bytes) st->ended = 1;   // bytes that are no member: the stream is over
    }
    inf.status = status;
    if (info) *info = inf;
    return (int)status;
}

}  // namespace sa
