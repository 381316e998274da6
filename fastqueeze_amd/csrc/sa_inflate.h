// sa_inflate.h -- raw-DEFLATE (RFC 1951) inflate of one BGZF member, written
// once as host+device functions.  sa_inflate.hip runs it one wave per member
// (every lane executes the same symbol loop; `lane` / `nl` only split the table
// fills, the match copies and the CRC); tests/cpu_emu/inflate_emu.cpp drives the
// same functions sequentially (lane 0 of 1) against zlib before they run on the
// GPU.
//
// Bounds, by construction:
//   input   every refill reads in[ip] with ip < in_len (the 8-byte loads only
//           when ip + 8 <= in_len); bits past the end are zeros and are never
//           consumed: a code or an extra field longer than the bits left is
//           SA_INFL_INPUT.
//   output  a literal is stored only when op < isize, a match only when
//           op + len <= isize, a stored block likewise; otherwise SA_INFL_SIZE.
//   window  a match's distance is checked against op (SA_INFL_DIST).
//   tables  primary indices are masked to the table size; the canonical walk
//           indexes sorted[] below the number of coded symbols (<= the array).
//   loops   the symbol loop consumes >= 1 bit per iteration (every code has
//           length >= 1) or ends the block; the block loop consumes >= 3 bits
//           per block; the bit count left is bounded by 8 x in_len.
// The code-length judgement is zlib's (inflate.c / inftrees.c): HLIT > 286,
// HDIST > 30, a repeat without a previous length or past HLIT + HDIST, a missing
// end-of-block code, an over-subscribed set, and an incomplete set other than
// a single one-bit code (no distance codes at all is allowed) are rejected; so
// are the codes 286 / 287 and the distance codes 30 / 31 when they are used.
// Each rule is pinned by a hand-built stream of tests/deflate_forge.py, on the
// host emulation and on the device, with its status:
//   HLIT > 286                      hlit_287, hlit_288
//   HDIST > 30                      hdist_31, hdist_32
//   a repeat without a previous     repeat_first
//   a repeat past HLIT + HDIST      repeat_past_end, repeat_16_past_end
//   a missing end-of-block code     no_end_of_block, hclen_4_all_zero
//   an over-subscribed set          lit_oversubscribed, dist_oversubscribed, cl_oversubscribed
//   an incomplete set               lit_incomplete, lit_one_2bit_code, dist_incomplete_two_2bit,
//                                   dist_incomplete_one_2bit, cl_incomplete, dist_unused_code_used
//   ... but one 1-bit code, or none dist_single_code0, dist_single_code29, dist_none, empty_dynamic (valid)
//   the codes 286 / 287             fixed_litlen_286, fixed_litlen_287
//   the distance codes 30 / 31      fixed_dist_30, fixed_dist_31
// A member whose ISIZE is 0 is inflated like any other (isize0_dynamic_l9,
// isize0_stored, isize0_fixed): with no room in the window its first byte is
// SA_INFL_SIZE, so only a stream that ends having produced nothing is an empty
// member.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/seqarc_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// (inlined into the kernel: the tables and the window keep their LDS address space)
#define SAI_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SAI_HD inline
#endif

namespace sa {

constexpr uint32_t INFL_LBITS = 10;       // primary literal/length table: 2^10 entries
constexpr uint32_t INFL_DBITS = 9;        // primary distance table
constexpr uint32_t INFL_MAX_ISIZE = 65536;
constexpr uint32_t INFL_CRC_CHUNK = 1024; // bytes per lane of the parallel CRC (64 lanes x 1 KiB = 64 KiB)

// Decode tables of the block being read.  An entry of a primary table is
// (symbol << 4 | code length), 0 where no code of at most the table's width
// ends: the canonical walk over cnt / sorted decodes those (and finds the
// unused codes of an incomplete set).
struct InflTabs {
    uint16_t lit[1u << INFL_LBITS];
    uint16_t dst[1u << INFL_DBITS];   // (the code-length code's table while a dynamic header is read)
    uint16_t lsorted[288];
    uint16_t dsorted[32];
    uint16_t lcnt[16];
    uint16_t dcnt[16];
    uint16_t work[32];    // infl_build: next sorted slot and next code of each length
    uint8_t lens[352];    // 286 + 30 code lengths of a dynamic block; [320, 339): the code-length code's
};

struct InflBits {
    const uint8_t* in;
    uint32_t in_len;
    uint32_t ip;      // next input byte
    uint64_t hold;    // bits not yet consumed, first bit lowest; zeros above `bits` at the end of the input
    uint32_t bits;    // valid bits in hold
    uint64_t pre;     // in[pre_at .. pre_at + 8), loaded one refill ahead (pre_at + 8 <= in_len), or pre_at = ~0
    uint32_t pre_at;
};

// At least 48 valid bits -- more than a literal/length + distance pair with its
// extra bits (15 + 5 + 15 + 13), a stored block's header or any field of a
// dynamic header takes -- or every bit the input has left.  The 8-byte word of
// a refill was loaded by the refill before it, so that the symbols decoded in
// between cover the load's latency; a refill after a stored block moved ip
// loads its own.
SAI_HD void infl_refill(InflBits& b)
{
    if (b.bits >= 48) return;
    if (b.ip + 8 <= b.in_len) {
        uint64_t w;
        if (b.pre_at == b.ip) w = b.pre;
        else __builtin_memcpy(&w, b.in + b.ip, 8);   // (little-endian hosts and the device)
        b.hold |= w << b.bits;
        b.ip += (63 - b.bits) >> 3;
        b.bits |= 56;
        if (b.ip + 8 <= b.in_len) {
            __builtin_memcpy(&b.pre, b.in + b.ip, 8);
            b.pre_at = b.ip;
        }
        return;
    }
    while (b.bits <= 56 && b.ip < b.in_len) {
        b.hold |= (uint64_t)b.in[b.ip++] << b.bits;
        b.bits += 8;
    }
}

// n <= 32 bits; false: the input has fewer left
SAI_HD bool infl_take(InflBits& b, uint32_t n, uint32_t& v)
{
    if (n > b.bits) return false;
    v = (uint32_t)(b.hold & ((1ull << n) - 1));
    b.hold >>= n;
    b.bits -= n;
    return true;
}

SAI_HD uint32_t infl_rev(uint32_t code, uint32_t len)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// Builds the tables of one code from lens[0..n) (n <= 288 and <= the size of
// sorted[]).  codes_type: the code-length code, whose set must be complete.
// false: zlib's inflate_table would reject the set.
// (Every lane runs the same statements on the same values, so a plain store or
// an increment of a shared counter is the same store from every lane; only the
// loops over `lane` split work.  The per-length counters live in the tables'
// memory, not in indexed registers.)
// ASSUMPTION of every lane-split loop in this file (these fills, the match and
// stored-block copies): the nl lanes are ONE wave running in lockstep
// (k_inflate_bgzf: __launch_bounds__(64), one wave per workgroup), whose LDS
// accesses the hardware performs in issue order, so what one lane stores a
// later instruction of any lane loads -- with plain accesses and no fence; the
// accesses may alias, so the compiler keeps their order.  A workgroup of more
// than one wave sharing a window or tables would need barriers here.
SAI_HD bool infl_build(const uint8_t* lens, uint32_t n, uint16_t* tab, uint32_t tbits, uint16_t* sorted, uint16_t* cnt,
                       uint16_t* work, bool codes_type, uint32_t lane, uint32_t nl)
{
    uint16_t* count = cnt;
    uint16_t* offs = work;
    uint16_t* next = work + 16;
    for (uint32_t l = 0; l < 16; l++) count[l] = 0;
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = lens[s] & 15u;
        count[l] = (uint16_t)(count[l] + 1);
    }
    uint32_t maxl = 15;
    while (maxl > 0 && count[maxl] == 0) maxl--;
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left <<= 1;
        left -= (int32_t)count[l];
        if (left < 0) return false;   // over-subscribed
    }
    count[0] = 0;
    if (maxl == 0) {
        if (codes_type) return false;   // (every length would read as 0: no end-of-block code)
    } else if (left > 0 && (codes_type || maxl != 1)) {
        return false;   // incomplete
    }
    offs[0] = 0;
    offs[1] = 0;
    next[0] = 0;
    uint32_t code = 0;
    for (uint32_t l = 1; l < 16; l++) {
        if (l > 1) offs[l] = (uint16_t)(offs[l - 1] + count[l - 1]);
        code = (code + count[l - 1]) << 1;
        next[l] = (uint16_t)code;   // (a code of l bits: < 2^l in a set that is not over-subscribed)
    }
    const uint32_t tsize = 1u << tbits;
    for (uint32_t j = lane; j < tsize; j += nl) tab[j] = 0;
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = lens[s] & 15u;
        if (!l) continue;
        const uint32_t at = offs[l];
        offs[l] = (uint16_t)(at + 1);
        if (at < n) sorted[at] = (uint16_t)s;
        const uint32_t c = next[l];
        next[l] = (uint16_t)(c + 1);
        if (l <= tbits) {
            const uint16_t e = (uint16_t)(s << 4 | l);
            for (uint32_t j = infl_rev(c, l) + (lane << l); j < tsize; j += nl << l) tab[j] = e;
        }
    }
    return true;
}

// One symbol of a code.  0: ok (sym, consumed); otherwise the status.
SAI_HD uint32_t infl_sym(InflBits& b, const uint16_t* tab, uint32_t tbits, const uint16_t* sorted, uint32_t nsorted,
                         const uint16_t* cnt, uint32_t& sym)
{
    const uint32_t e = tab[(uint32_t)b.hold & ((1u << tbits) - 1)];
    uint32_t len = e & 15u;
    sym = e >> 4;
    if (!e) {
        // canonical walk, one bit a step (codes longer than the table, unused codes)
        uint32_t code = 0, first = 0, index = 0;
        len = 0;
        for (uint32_t l = 1; l < 16; l++) {
            code |= (uint32_t)(b.hold >> (l - 1)) & 1u;
            const uint32_t c = cnt[l];
            if (code < first + c) {
                const uint32_t at = index + (code - first);
                if (at >= nsorted) return SA_INFL_CODES;
                sym = sorted[at];
                len = l;
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (!len) return b.bits < 15 ? SA_INFL_INPUT : SA_INFL_CODES;   // no code: the set is incomplete
    }
    if (len > b.bits) return SA_INFL_INPUT;
    b.hold >>= len;
    b.bits -= len;
    return 0;
}

// The dynamic block's header: HLIT, HDIST, HCLEN, the code-length code and the
// literal/length + distance lengths (one run: a repeat may cross from the one
// alphabet into the other), then both tables.
SAI_HD uint32_t infl_dynamic(InflBits& b, InflTabs& t, uint32_t& nlen, uint32_t& ndist, uint32_t lane, uint32_t nl)
{
    uint32_t v;
    infl_refill(b);
    if (!infl_take(b, 14, v)) return SA_INFL_INPUT;
    nlen = (v & 31u) + 257;
    ndist = ((v >> 5) & 31u) + 1;
    const uint32_t ncode = ((v >> 10) & 15u) + 4;
    if (nlen > 286 || ndist > 30) return SA_INFL_CODES;
    // the order of the code-length code's lengths, 5 bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const uint64_t olo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 |
                         10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t ohi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    uint8_t* cl = t.lens + 320;
    for (uint32_t i = 0; i < 19; i++) cl[i] = 0;
    for (uint32_t i = 0; i < ncode; i++) {
        infl_refill(b);
        if (!infl_take(b, 3, v)) return SA_INFL_INPUT;
        const uint32_t o = (uint32_t)((i < 12 ? olo >> (5 * i) : ohi >> (5 * (i - 12))) & 31u);
        if (o < 19) cl[o] = (uint8_t)v;
    }
    if (!infl_build(cl, 19, t.dst, 7, t.dsorted, t.dcnt, t.work, true, lane, nl)) return SA_INFL_CODES;
    const uint32_t total = nlen + ndist;   // <= 316
    uint32_t have = 0;
    while (have < total) {
        infl_refill(b);
        uint32_t sym;
        const uint32_t st = infl_sym(b, t.dst, 7, t.dsorted, 19, t.dcnt, sym);
        if (st) return st;
        if (sym < 16) {
            t.lens[have++] = (uint8_t)sym;
            continue;
        }
        uint32_t len = 0, rep;
        if (sym == 16) {
            if (have == 0) return SA_INFL_CODES;
            len = t.lens[have - 1];
            if (!infl_take(b, 2, v)) return SA_INFL_INPUT;
            rep = 3 + v;
        } else if (sym == 17) {
            if (!infl_take(b, 3, v)) return SA_INFL_INPUT;
            rep = 3 + v;
        } else {
            if (!infl_take(b, 7, v)) return SA_INFL_INPUT;
            rep = 11 + v;
        }
        if (have + rep > total) return SA_INFL_CODES;
        while (rep--) t.lens[have++] = (uint8_t)len;
    }
    if (t.lens[256] == 0) return SA_INFL_CODES;   // no end-of-block code
    if (!infl_build(t.lens, nlen, t.lit, INFL_LBITS, t.lsorted, t.lcnt, t.work, false, lane, nl)) return SA_INFL_CODES;
    if (!infl_build(t.lens + nlen, ndist, t.dst, INFL_DBITS, t.dsorted, t.dcnt, t.work, false, lane, nl)) return SA_INFL_CODES;
    return 0;
}

SAI_HD void infl_fixed(InflTabs& t, uint32_t lane, uint32_t nl)
{
    for (uint32_t i = 0; i < 288; i++) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (uint32_t i = 288; i < 320; i++) t.lens[i] = 5;
    (void)infl_build(t.lens, 288, t.lit, INFL_LBITS, t.lsorted, t.lcnt, t.work, false, lane, nl);
    (void)infl_build(t.lens + 288, 32, t.dst, INFL_DBITS, t.dsorted, t.dcnt, t.work, false, lane, nl);
}

// The symbols of one Huffman block into win[op..).  nlsym / ndsym: the coded
// symbols of each alphabet (the bound of sorted[]).
SAI_HD uint32_t infl_block(InflBits& b, const InflTabs& t, uint32_t nlsym, uint32_t ndsym, uint8_t* win, uint32_t isize,
                           uint32_t& op, uint32_t lane, uint32_t nl)
{
    for (;;) {
        infl_refill(b);   // >= 48 bits or all that is left: a literal/length + distance pair takes <= 48
        uint32_t sym;
        uint32_t st = infl_sym(b, t.lit, INFL_LBITS, t.lsorted, nlsym, t.lcnt, sym);
        if (st) return st;
        if (sym < 256) {
            if (op >= isize) return SA_INFL_SIZE;
            win[op++] = (uint8_t)sym;   // (every lane stores the same byte)
            continue;
        }
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
        if (dist > op) return SA_INFL_DIST;
        if (len > isize - op) return SA_INFL_SIZE;   // (op <= isize)
        // the source [op - dist, op) is complete before the copy and is not written by it:
        // byte i of an overlapping match is source byte i mod dist
        const uint8_t* src = win + (op - dist);
        uint8_t* dstp = win + op;
        if (dist >= len) {
            for (uint32_t i = lane; i < len; i += nl) dstp[i] = src[i];
        } else if (dist == 1) {
            const uint8_t c = src[0];
            for (uint32_t i = lane; i < len; i += nl) dstp[i] = c;
        } else {
            for (uint32_t i = lane; i < len; i += nl) dstp[i] = src[i % dist];
        }
        op += len;
    }
}

// Inflates in[0..in_len) into win[0..isize).  Returns 0 when the stream ends
// (its final block's end-of-block code) with exactly isize bytes written; the
// input may have bytes left over, as for zlib.  The CRC is the caller's.
SAI_HD uint32_t infl_member(const uint8_t* in, uint32_t in_len, uint8_t* win, uint32_t isize, InflTabs& t, uint32_t lane,
                            uint32_t nl)
{
    InflBits b{in, in_len, 0, 0, 0, 0, 0xffffffffu};
    uint32_t op = 0;
    for (;;) {
        infl_refill(b);
        uint32_t hdr;
        if (!infl_take(b, 3, hdr)) return SA_INFL_INPUT;
        const uint32_t type = hdr >> 1;
        if (type == 0) {
            uint32_t v;
            (void)infl_take(b, b.bits & 7u, v);   // to the byte boundary
            infl_refill(b);
            if (!infl_take(b, 32, v)) return SA_INFL_INPUT;
            const uint32_t n = v & 0xffffu;
            if (n != ((v >> 16) ^ 0xffffu)) return SA_INFL_BLOCK;
            // the bytes still in the bit buffer are the input's bytes before ip
            const uint32_t at = b.ip - (b.bits >> 3);
            if (n > in_len - at) return SA_INFL_INPUT;   // (at <= ip <= in_len)
            if (n > isize - op) return SA_INFL_SIZE;
            for (uint32_t i = lane; i < n; i += nl) win[op + i] = in[at + i];
            op += n;
            b.ip = at + n;
            b.hold = 0;
            b.bits = 0;
        } else if (type == 3) {
            return SA_INFL_BLOCK;
        } else {
            uint32_t nlsym = 288, ndsym = 32;
            if (type == 1) {
                infl_fixed(t, lane, nl);
            } else {
                const uint32_t st = infl_dynamic(b, t, nlsym, ndsym, lane, nl);
                if (st) return st;
            }
            const uint32_t st = infl_block(b, t, nlsym, ndsym, win, isize, op, lane, nl);
            if (st) return st;
        }
        if (hdr & 1u) break;
    }
    return op == isize ? 0 : SA_INFL_SIZE;
}

// ---- CRC-32 (IEEE 802.3, reflected: gzip's) --------------------------------
constexpr uint32_t CRC_POLY = 0xedb88320u;

SAI_HD uint32_t crc32_entry(uint32_t i)   // entry i of the byte table
{
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}

// a(x) b(x) mod P, reflected (0x80000000 is 1): zlib's multmodp
SAI_HD uint32_t crc32_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 INFL_CRC_CHUNK k) mod P
SAI_HD uint32_t crc32_chunk_shift(uint32_t k)
{
    uint32_t sq = 1u << 30;   // x^1
    for (uint32_t i = 0; i < 13; i++) sq = crc32_mul(sq, sq);   // x^(2^13) = x^(8 x 1024)
    uint32_t p = 1u << 31;                                      // x^0
    for (; k; k >>= 1) {
        if (k & 1u) p = crc32_mul(sq, p);
        sq = crc32_mul(sq, sq);
    }
    return p;
}

// Lane `lane` of 64's share of the member's CRC-32: the member is laid, right
// aligned, over 64 chunks of INFL_CRC_CHUNK bytes; the lane runs the register
// over the data bytes of chunk `lane` (from zero -- leading zeros leave a zero
// register alone -- or from 0xffffffff in the chunk that holds the member's
// first byte) and shifts it to the end of the message with `shift` =
// crc32_chunk_shift(63 - lane).  The XOR of the 64 shares, inverted, is the
// CRC.  tab: the 256-entry byte table.
// (On the device the 64 lanes read data[lane x 1024 + i]: a 1 KiB stride, one
// LDS bank for all of them, so each of the 1,024 steps is a serialised read --
// about 1 % of the kernel at its present rate; an interleaved layout is due
// once the symbol loop is faster.)
SAI_HD uint32_t crc32_share(const uint8_t* data, uint32_t isize, uint32_t lane, uint32_t shift, const uint32_t* tab)
{
    const uint32_t pad = 64 * INFL_CRC_CHUNK - isize;   // isize <= 65536
    const uint32_t c0 = lane * INFL_CRC_CHUNK, c1 = c0 + INFL_CRC_CHUNK;
    if (c1 <= pad) return 0;
    uint32_t crc = c0 <= pad ? 0xffffffffu : 0u;
    const uint32_t from = (c0 <= pad ? pad : c0) - pad, to = c1 - pad;   // to <= isize
    for (uint32_t i = from; i < to; i++) crc = tab[(crc ^ data[i]) & 0xffu] ^ (crc >> 8);
    return lane == 63 ? crc : crc32_mul(crc, shift);
}

// ---- BGZF member walk (host) --------------------------------------------------
// The walk over a slab's members: sa_bgzf_scan's body, and what GzStream's two
// BGZF paths call (cli_gzstream.h).  max_isize: a member of more text bytes is
// -2 (INFL_MAX_ISIZE for the device kernel; the host inflate takes any).  ms may
// be null (the members are counted).
inline int64_t bgzf_scan(const uint8_t* buf, uint64_t have, sa_bgzf_member* ms, uint64_t max_members, uint64_t* consumed,
                         uint64_t* out_bytes, uint32_t max_isize = INFL_MAX_ISIZE)
{
    uint64_t p = 0, total = 0, n = 0;
    while (p < have) {
        const uint8_t* h = buf + p;
        const uint64_t left = have - p;
        // what is there of the fixed header must be a gzip member with an extra field
        if (h[0] != 0x1f || (left > 1 && h[1] != 0x8b) || (left > 2 && h[2] != 8) || (left > 3 && !(h[3] & 4))) return -1;
        if (left < 18) break;   // cut inside the header
        const uint64_t xlen = h[10] | (uint64_t)h[11] << 8;
        uint64_t bsize = 0;
        for (uint64_t x = 12; x + 4 <= 12 + xlen && x + 4 <= left;) {   // the 'BC' subfield
            const uint64_t sl = h[x + 2] | (uint64_t)h[x + 3] << 8;
            if (h[x] == 'B' && h[x + 1] == 'C' && sl == 2 && x + 6 <= 12 + xlen && x + 6 <= left) bsize = (h[x + 4] | (uint64_t)h[x + 5] << 8) + 1;
            x += 4 + sl;
        }
        if (!bsize) {
            if (12 + xlen > left) break;   // the extra field is cut: more input decides
            return -1;                     // no 'BC': not BGZF
        }
        if (bsize < 12 + xlen + 8) return -1;
        if (bsize > left) break;   // the member continues past the slab
        const uint8_t* t = h + bsize - 8;
        const uint32_t crc = (uint32_t)(t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24);
        const uint32_t isize = (uint32_t)(t[4] | t[5] << 8 | t[6] << 16 | (uint32_t)t[7] << 24);
        if (isize > max_isize) return -2;
        if (n >= max_members) return -3;
        if (ms) ms[n] = sa_bgzf_member{p + 12 + xlen, (uint32_t)(bsize - 12 - xlen - 8), total, isize, crc};
        n++;
        total += isize;
        p += bsize;
    }
    if (consumed) *consumed = p;
    if (out_bytes) *out_bytes = total;
    return (int64_t)n;
}

}  // namespace sa
