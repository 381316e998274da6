// sa_decode_logic.h -- the two serial chains of a block decode (QUAL:
// SIMPLE_MODEL<95> per quality context, SEQ: BASE_MODEL per k-mer context), the
// N / IUPAC placement between them and the memory plan of a decoder that holds
// many blocks on the device at once, written as host+device functions: plain
// C++ that compiles for both.  What is restated here is sa_decode_block's code
// (arc_decode.cpp / arc_decode_host.h): RangeIn, SModel::decode, the quality
// context, the placement walk and the base loop.  tests/cpu_emu/decode_emu.cpp
// drives these functions on the host with the 64 lanes as a loop; no kernel
// uses them yet ("Block decode for the device").
//
// The wave abstraction W (LoopOps in decode_emu.cpp; on a device: one wave):
//   W::N                  lanes a W object holds registers for (64 in the
//                         emulation; 1 on a device: the executing lane's)
//   w.each(f)             f(lane, k) for every lane; k indexes the register arrays
//   w.scan(in, out)       out = exclusive prefix sum of in over the lanes; returns the total
//   w.first(a, v)         the lowest lane whose a == v, or 64
//   w.get(a, lane)        a of that lane, the same value in every lane
//   w.ld8 / w.ld32        one load, the same value in every lane (lane 0's)
//   w.st8 / w.st32        one store, from lane 0
//   w.fill(p, n, v)       n bytes v from p on, split over the lanes
// Values that are the same in every lane (the coder state, positions, contexts)
// are plain variables: on a device the compiler can keep them in scalar registers.
//
// Memory rule of the QUAL model: lane i owns list entries i and i + 64 (freq and
// sym) of every context, lane 0 also the bubble counter.  A lane loads and stores
// only what it owns; the bubble swap crosses lanes through w.get.  One wave works
// on a block's table, and each address is touched by one lane in program order,
// so the table needs no fence.
//
// Bounds, by construction:
//   input   every coded byte is read through dec_byte (pos < in_len); past the
//           end the chain ends with SA_DEC_INPUT.
//   loops   the renormalisation runs at most DEC_RENORM_MAX rounds
//           (SA_DEC_RANGE: a squeeze can leave range 0, from which the host
//           decoder's loop would not return); a slice decodes at most `slice`
//           symbols; every other loop is bounded by a read's length or the
//           read count.
//   tables  the quality context is masked to the table's size, the base
//           context to 4^k - 1; list indices are lane numbers.
//   output  positions are off + i with i < lens[r], off the sum of the lengths
//           before r: inside the block's `bases` bytes the host sized.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/seqarc_amd.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SAD_HD inline
#endif
// a value every lane holds alike, said so to the compiler (a scalar register on a device)
#if defined(__HIP_DEVICE_COMPILE__)
#define SAD_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define SAD_UNI(x) ((uint32_t)(x))
#endif

namespace sa {

// (why a block's chain ended: SA_DEC_* of include/seqarc_amd.h)

constexpr uint32_t DEC_LANES = 64;
constexpr uint32_t DEC_QSYM = 95;          // SIMPLE_MODEL<95>: symbol 94 = "the rest of the read is '#'"
// one quality context in global memory: 95 x u16 freq, 95 x u8 sym, the bubble
// counter (the total is the sum of the freqs: the step's prefix sum gives it)
constexpr uint32_t DEC_QM_FREQ = 0, DEC_QM_SYM = 190, DEC_QM_BUB = 285, DEC_QM_STRIDE = 288;
constexpr uint32_t DEC_RENORM_MAX = 8;
// events of a model step (the emulation counts them; tests rest on shapes that hit them)
constexpr uint32_t DEC_EV_HIGH = 1, DEC_EV_SWAP_63_64 = 2, DEC_EV_HALVE = 4, DEC_EV_SWAP = 8, DEC_EV_BASE_HALVE = 16;

// Everything a chain needs to stop after a slice and resume in the next launch.
struct DecChain {
    uint64_t low, code;          // coder
    uint32_t range, pos;         // pos: the input cursor
    uint32_t status, done;       // SA_DEC_*; done: the chain has ended (all reads, or a status)
    uint64_t off;                // output offset of read r
    uint32_t r, i;               // read index, position in the read
    uint32_t q1, q2, delta, last;   // QUAL: the context's inputs and the last context
    uint32_t ctx;                // SEQ
    uint32_t started;
};
static_assert(sizeof(DecChain) == 72, "DecChain is copied between host and device as it is");

SAD_HD void dec_fail(DecChain& c, uint32_t st)
{
    if (!c.status) c.status = st;
}

// ---- carry-less range decoder (RangeIn of arc_decode_host.h) ----
SAD_HD uint32_t dec_byte(DecChain& c, const uint8_t* in, uint32_t in_len)
{
    if (c.pos < in_len) return SAD_UNI(in[c.pos++]);
    dec_fail(c, SA_DEC_INPUT);
    return 0;
}

SAD_HD void dec_coder_start(DecChain& c, const uint8_t* in, uint32_t in_len)
{
    c.low = 0;
    c.code = 0;
    c.range = 0xffffffffu;
    c.pos = 0;
    for (int k = 0; k < 8; k++) c.code = (c.code << 8) | dec_byte(c, in, in_len);
}

// slot of the next symbol in [0, tot).  code - low fits 32 bits in every valid
// state; if it does not, (code - low) / scale >= tot because scale = range / tot
// <= 2^32 / tot: the high word decides and the division is 32-bit.
SAD_HD uint32_t dec_slot(DecChain& c, uint32_t tot, uint32_t& scale)
{
    scale = tot ? c.range / tot : 0;
    const uint64_t d = c.code - c.low;
    if ((d >> 32) || !scale) {
        dec_fail(c, SA_DEC_SLOT);
        return 0;
    }
    const uint32_t v = (uint32_t)d / scale;
    if (v >= tot) {
        dec_fail(c, SA_DEC_SLOT);
        return 0;
    }
    return v;
}

SAD_HD void dec_consume(DecChain& c, const uint8_t* in, uint32_t in_len, uint32_t scale, uint32_t cum, uint32_t freq)
{
    c.low += (uint32_t)(cum * scale);
    c.range = scale * freq;
    for (uint32_t round = 0; c.range < (1u << 24); round++) {
        if (round == DEC_RENORM_MAX) {   // range 0 after a squeeze
            dec_fail(c, SA_DEC_RANGE);
            return;
        }
        if ((c.low ^ (c.low + c.range)) >> 56) c.range = ((uint32_t)c.low | 0xffffffu) - (uint32_t)c.low;
        c.code = (c.code << 8) | dec_byte(c, in, in_len);
        c.range <<= 8;
        c.low <<= 8;
    }
}

// ---- SIMPLE_MODEL<95> over the lanes ----
template <class W> struct SmRegs {
    uint32_t f0[W::N], f1[W::N];   // freq of entries lane and lane + 64 (0 where lane + 64 >= 95)
    uint32_t s0[W::N], s1[W::N];   // their symbols
    uint32_t bub[W::N];            // lane 0: the bubble counter
};

// a fresh context: sym = index, freq 1, bubble 0 (SModel::reset(95)); entry e of context m
SAD_HD void sm_init_entry(uint8_t* m, uint32_t e)
{
    reinterpret_cast<uint16_t*>(m + DEC_QM_FREQ)[e] = 1;
    m[DEC_QM_SYM + e] = (uint8_t)e;
    if (e == 0) m[DEC_QM_BUB] = m[DEC_QM_BUB + 1] = m[DEC_QM_BUB + 2] = 0;
}

template <class W> SAD_HD void sm_load(W& w, const uint8_t* m, SmRegs<W>& R)
{
    w.each([&](uint32_t l, uint32_t k) {
        const uint16_t* f = reinterpret_cast<const uint16_t*>(m + DEC_QM_FREQ);
        R.f0[k] = f[l];
        R.s0[k] = m[DEC_QM_SYM + l];
        const bool two = l + DEC_LANES < DEC_QSYM;
        R.f1[k] = two ? f[l + DEC_LANES] : 0u;
        R.s1[k] = two ? m[DEC_QM_SYM + l + DEC_LANES] : 0u;
        R.bub[k] = l == 0 ? m[DEC_QM_BUB] : 0u;
    });
}

// One symbol of context m (its entries in R): SModel::decode.  Returns the
// symbol; on a status the chain ends and the value is not used.
template <class W>
SAD_HD uint32_t sm_step(W& w, uint8_t* m, SmRegs<W>& R, DecChain& c, const uint8_t* in, uint32_t in_len, uint32_t& ev)
{
    uint32_t pk[W::N], x[W::N], hit[W::N], d0[W::N], d1[W::N];
    // both halves of the list in one scan: the freqs' sum is < 2^16, so the low half never carries
    w.each([&](uint32_t, uint32_t k) { pk[k] = R.f0[k] | R.f1[k] << 16; });
    const uint32_t tpk = w.scan(pk, x);
    const uint32_t t0 = tpk & 0xffffu, tot = t0 + (tpk >> 16);
    uint32_t scale;
    const uint32_t v = dec_slot(c, tot, scale);
    if (c.status) return 0;
    w.each([&](uint32_t, uint32_t k) {
        hit[k] = (x[k] & 0xffffu) + R.f0[k] > v ? 1u : t0 + (x[k] >> 16) + R.f1[k] > v ? 2u : 0u;
    });
    uint32_t own = w.first(hit, 1u), slot = 0;
    if (own >= DEC_LANES) {
        own = w.first(hit, 2u);
        slot = 1;
        if (own >= DEC_LANES) {   // (v < tot = the sum of the freqs: does not happen)
            dec_fail(c, SA_DEC_SLOT);
            return 0;
        }
    }
    const uint32_t idx = own + slot * DEC_LANES;
    const uint32_t xo = w.get(x, own);
    const uint32_t cum = slot ? t0 + (xo >> 16) : xo & 0xffffu;
    // (the slot is chosen per value, never per array: the registers stay registers)
    uint32_t fs[W::N], ss[W::N], fps[W::N], sps[W::N];
    w.each([&](uint32_t, uint32_t k) {
        const uint32_t f0 = R.f0[k], f1 = R.f1[k], s0 = R.s0[k], s1 = R.s1[k];
        fs[k] = slot ? f1 : f0;
        ss[k] = slot ? s1 : s0;
    });
    const uint32_t fr = w.get(fs, own);
    const uint32_t sym = w.get(ss, own);
    dec_consume(c, in, in_len, scale, cum, fr);
    if (c.status) return sym;
    if (idx >= DEC_LANES) ev |= DEC_EV_HIGH;
    // +8, the halving above 0xffe0: every lane on its own entries
    const bool halve = tot + 8 > 0xffe0u;
    if (halve) ev |= DEC_EV_HALVE;
    w.each([&](uint32_t l, uint32_t k) {
        d0[k] = l == own && !slot;
        d1[k] = l == own && slot;
        R.f0[k] += d0[k] ? 8u : 0u;
        R.f1[k] += d1[k] ? 8u : 0u;
        const uint32_t f0 = R.f0[k], f1 = R.f1[k];
        R.f0[k] = halve ? f0 - (f0 >> 1) : f0;
        R.f1[k] = halve ? f1 - (f1 >> 1) : f1;
        d0[k] |= halve;
        d1[k] |= halve && l + DEC_LANES < DEC_QSYM;
    });
    // every 16th update: entry idx against idx - 1 (63 / 64: lane 63's first slot against lane 0's second)
    const uint32_t b = (w.get(R.bub, 0) + 1) & 15u;
    if (b == 0 && idx > 0) {
        const uint32_t pown = idx == DEC_LANES ? DEC_LANES - 1 : own - 1, pslot = idx == DEC_LANES ? 0u : slot;
        w.each([&](uint32_t, uint32_t k) {
            const uint32_t f0 = R.f0[k], f1 = R.f1[k], s0 = R.s0[k], s1 = R.s1[k];
            fs[k] = slot ? f1 : f0;
            fps[k] = pslot ? f1 : f0;
            sps[k] = pslot ? s1 : s0;
        });
        const uint32_t fi = w.get(fs, own), si = sym;
        const uint32_t fp = w.get(fps, pown), sp = w.get(sps, pown);
        if (fi > fp) {
            ev |= idx == DEC_LANES ? (DEC_EV_SWAP | DEC_EV_SWAP_63_64) : DEC_EV_SWAP;
            w.each([&](uint32_t l, uint32_t k) {
                // (values chosen, not places, so the registers stay registers; entries idx and idx - 1 differ)
                const bool a0 = l == own && !slot, a1 = l == own && slot;
                const bool b0 = l == pown && !pslot, b1 = l == pown && pslot;
                const uint32_t f0 = R.f0[k], f1 = R.f1[k], s0 = R.s0[k], s1 = R.s1[k];
                R.f0[k] = a0 ? fp : b0 ? fi : f0;
                R.s0[k] = a0 ? sp : b0 ? si : s0;
                R.f1[k] = a1 ? fp : b1 ? fi : f1;
                R.s1[k] = a1 ? sp : b1 ? si : s1;
                d0[k] |= a0 || b0;
                d1[k] |= a1 || b1;
            });
        }
    }
    w.each([&](uint32_t l, uint32_t k) {
        uint16_t* f = reinterpret_cast<uint16_t*>(m + DEC_QM_FREQ);
        if (d0[k]) { f[l] = (uint16_t)R.f0[k]; m[DEC_QM_SYM + l] = (uint8_t)R.s0[k]; }
        if (d1[k]) { f[l + DEC_LANES] = (uint16_t)R.f1[k]; m[DEC_QM_SYM + l + DEC_LANES] = (uint8_t)R.s1[k]; }
        if (l == 0) { R.bub[k] = b; m[DEC_QM_BUB] = (uint8_t)b; }
    });
    return sym;
}

SAD_HD uint32_t dec_qual_contexts(int32_t qlevel) { return qlevel > 2 ? 0x100000u : 0x10000u; }

// the context the next quality is read with (decode_block's update; i = the position of s)
SAD_HD uint32_t dec_qual_ctx(DecChain& c, uint32_t s, uint32_t i, int32_t qlevel, uint32_t mask)
{
    uint32_t ctx = (((c.q1 > c.q2 ? c.q1 : c.q2) << 6) + s) & 0xfffu;
    if (qlevel > 1) {
        ctx += c.q1 == c.q2 ? 0x1000u : 0u;
        c.delta += c.q1 > s ? c.q1 - s : 0u;
        ctx += ((c.delta <= 56u ? c.delta : 56u) & 0xf8u) << 10;
        if (qlevel > 2) ctx += i <= 0x6fu ? ((i + 15u) & 0x78u) << 13 : 0xf0000u;
    }
    c.q2 = c.q1;
    c.q1 = s;
    return ctx & mask;
}

SAD_HD void dec_next_read(DecChain& c, uint32_t len, uint32_t seed)
{
    c.off += len;
    c.r++;
    c.i = 0;
    c.q1 = c.q2 = 0;
    c.delta = 5;
    c.last = 0;
    c.ctx = seed;
}

// At most `slice` quality symbols of a block; Q: the block's qualities, models:
// its contexts (dec_qual_contexts x DEC_QM_STRIDE bytes, initialised).
template <class W>
SAD_HD void dec_qual_slice(W& w, DecChain& c, const uint8_t* in, uint32_t in_len, const uint32_t* lens, uint32_t n,
                           uint8_t* Q, uint8_t* models, int32_t qlevel, uint32_t slice, uint32_t& ev)
{
    const uint32_t mask = dec_qual_contexts(qlevel) - 1;
    if (!c.started) {
        c.started = 1;
        c.off = 0;
        c.r = 0;
        dec_next_read(c, 0, 0);
        c.r = 0;
        dec_coder_start(c, in, in_len);
    }
    SmRegs<W> R;
    uint32_t cur = ~0u, count = 0;
    while (!c.status && c.r < n) {
        const uint32_t L = SAD_UNI(lens[c.r]);
        if (c.i >= L) {
            dec_next_read(c, L, 0);
            continue;
        }
        if (count >= slice) return;
        const uint32_t at = c.last & mask;
        uint8_t* m = models + (size_t)at * DEC_QM_STRIDE;
        if (cur != at) {   // (the entries of the context just used are still in R)
            sm_load(w, m, R);
            cur = at;
        }
        const uint32_t s = sm_step(w, m, R, c, in, in_len, ev);
        count++;
        if (c.status) break;
        if (s == DEC_QSYM - 1) {   // the stripped trailing '#' run
            w.fill(Q + c.off + c.i, L - c.i, (uint8_t)'#');
            c.i = L;
            continue;
        }
        w.st8(Q + c.off + c.i, (uint8_t)(s + 33));
        c.last = dec_qual_ctx(c, s, c.i, qlevel, mask);
        c.i++;
    }
    c.done = 1;
}

// ---- BASE_MODEL chain ----
SAD_HD uint32_t dec_seq_mask(int32_t slevel)   // 4^k - 1, k = slevel + 7; slevel 9: (2k) & 31 == 0, one context
{
    return (1u << ((2 * (slevel + 7)) & 31)) - 1u;
}

// At most `slice` positions of a block's bases; S: the block's bases, zero but
// for what the placement wrote (those positions are skipped); tab: 4 x (mask + 1)
// counts, all 3 at the start.
template <class W>
SAD_HD void dec_seq_slice(W& w, DecChain& c, const uint8_t* in, uint32_t in_len, const uint32_t* lens, uint32_t n,
                          uint8_t* S, uint8_t* tab, uint32_t mask, uint32_t slice, uint32_t& ev)
{
    const uint32_t seed = 0x7616c7u & mask;
    if (!c.started) {
        c.started = 1;
        c.off = 0;
        c.r = 0;
        dec_next_read(c, 0, seed);
        c.r = 0;
        dec_coder_start(c, in, in_len);
    }
    uint32_t count = 0;
    while (!c.status && c.r < n) {
        const uint32_t L = SAD_UNI(lens[c.r]);
        if (c.i >= L) {
            dec_next_read(c, L, seed);
            continue;
        }
        if (count >= slice) return;
        count++;
        uint8_t* out = S + c.off + c.i;
        if (w.ld8(out)) {   // an N / IUPAC base the placement put there: no symbol, the context stays
            c.i++;
            continue;
        }
        uint32_t* mp = reinterpret_cast<uint32_t*>(tab + (size_t)(c.ctx & mask) * 4);
        const uint32_t word = w.ld32(mp);
        uint32_t m[4] = {word & 0xffu, (word >> 8) & 0xffu, (word >> 16) & 0xffu, word >> 24};
        uint32_t tot = m[0] + m[1] + m[2] + m[3];
        if (tot > 253) {   // halve before the symbol is read
            ev |= DEC_EV_BASE_HALVE;
            for (int j = 0; j < 4; j++) m[j] -= m[j] >> 1;
            tot = m[0] + m[1] + m[2] + m[3];
        }
        uint32_t scale;
        const uint32_t v = dec_slot(c, tot, scale);
        if (c.status) break;
        uint32_t cum = 0, b = 0;
        while (b < 3 && cum + m[b] <= v) cum += m[b++];
        dec_consume(c, in, in_len, scale, cum, m[b]);
        if (c.status) break;
        m[b]++;
        w.st32(mp, m[0] | m[1] << 8 | m[2] << 16 | m[3] << 24);
        w.st8(out, (uint8_t)"ACGT"[b]);
        c.ctx = ((c.ctx << 2) + b) & mask;
        c.i++;
    }
    c.done = 1;
}

// ---- N / IUPAC placement (decode_block's walk, strict form) ----
// A tip read's candidate positions (quality <= its max) read
// N^g1 B N^g2 B ... N^gE B N...: gaps g, E = its exception count.  The character
// goes straight into the zero-initialised bases.  Only the tip reads are walked:
// read t lies at tip_off[t] and has tip_len[t] bases.  0 or SA_DEC_PLACE.
SAD_HD uint32_t dec_place(const uint8_t* Q, uint8_t* S, uint32_t ntip, const uint64_t* tip_off, const uint32_t* tip_len,
                          const uint8_t* maxq, const uint64_t* exc, const uint64_t* gaps, uint64_t ngaps,
                          const uint8_t* chs, uint64_t nchs)
{
    uint64_t ig = 0, ic = 0;
    for (uint32_t t = 0; t < ntip; t++) {
        const int mq = (int)maxq[t] + 33;
        const uint64_t E = exc[t];
        uint64_t e = 0, rem = ~0ull;
        if (E) {
            if (ig >= ngaps) return SA_DEC_PLACE;
            rem = gaps[ig];
        }
        const uint8_t* q = Q + tip_off[t];
        uint8_t* s = S + tip_off[t];
        const uint32_t L = tip_len[t];
        for (uint32_t i = 0; i < L; i++) {
            if ((int)(int8_t)q[i] > mq) continue;
            if (e < E && rem == 0) {
                e++;
                ig++;
                rem = ~0ull;
                if (e < E) {
                    if (ig >= ngaps) return SA_DEC_PLACE;
                    rem = gaps[ig];
                }
            } else {
                if (ic >= nchs) return SA_DEC_PLACE;
                const uint8_t sc = chs[ic++];
                s[i] = (uint8_t)"NMRYKSWHBVD"[sc < 11 ? sc : 0];
                rem--;
            }
        }
    }
    return ic == nchs ? 0u : (uint32_t)SA_DEC_PLACE;
}

// ---- memory plan ----
struct DecBlockSize {
    uint64_t enc_bytes;    // the encoded block (its two payloads are uploaded)
    uint64_t bases;        // sum of the read lengths
    uint64_t side_bytes;   // the tip / gap / character arrays of the placement
    uint32_t nreads;
    uint32_t pad;
};
struct DecPlan {
    uint64_t qual_table, seq_table;   // per block, from the levels
    uint64_t budget;                  // the share of the device's free bytes the decoder takes
    uint64_t max_block;               // the largest supported block's bytes
    uint32_t inflight;                // blocks a group holds (0: no block fits)
    uint32_t unsupported;             // blocks that exceed the budget on their own
};
constexpr uint64_t DEC_PAD = 64;   // every per-block array starts on a 64-byte boundary

SAD_HD uint64_t dec_pad(uint64_t v) { return (v + DEC_PAD - 1) & ~(DEC_PAD - 1); }

// Pure: from the config, the blocks' sizes and the device's free bytes, each
// block's device bytes (per_block[i]; unsupported[i] = 1 where one block
// exceeds the budget: the host decodes it) and how many blocks go in flight.
// cap: an upper limit on the blocks in flight (SA_DEC_INFLIGHT), 0 = none.
inline DecPlan plan_decode(const sa_cfg& cfg, uint32_t nblocks, const DecBlockSize* bs, uint64_t free_bytes, uint32_t cap,
                           uint64_t* per_block, uint8_t* unsupported)
{
    DecPlan p{};
    p.qual_table = (uint64_t)dec_qual_contexts(cfg.qlevel) * DEC_QM_STRIDE;
    p.seq_table = 4ull * ((uint64_t)dec_seq_mask(cfg.slevel) + 1);
    p.budget = free_bytes - free_bytes / 8;
    uint32_t ok = 0;
    for (uint32_t i = 0; i < nblocks; i++) {
        const uint64_t b = dec_pad(bs[i].enc_bytes) + dec_pad(4ull * bs[i].nreads) + dec_pad(bs[i].side_bytes) + p.qual_table +
                           dec_pad(p.seq_table) + 2 * dec_pad(bs[i].bases) + 4 * DEC_PAD;   // (+ chains, descriptor, status)
        if (per_block) per_block[i] = b;
        const bool un = b > p.budget;
        if (unsupported) unsupported[i] = un;
        if (un) {
            p.unsupported++;
        } else {
            ok++;
            if (b > p.max_block) p.max_block = b;
        }
    }
    if (ok) {
        const uint64_t fit = p.budget / p.max_block;
        p.inflight = (uint32_t)(fit < ok ? fit : ok);
        if (cap && p.inflight > cap) p.inflight = cap;
    }
    return p;
}

// ---- a block of a group (sa_decoder.h lays the groups out) ----
// Byte offsets into the group's arena, each on a DEC_PAD boundary and checked by
// the host against the arena's size before any launch (dec_desc_ok).
struct DecDesc {
    uint64_t qin, sin, lens;                          // uploaded: the two payloads, n x u32 lengths
    uint64_t tip_off, tip_len, maxq, exc, gaps, chs;  // uploaded: the placement's side arrays
    uint64_t Q, S;                                    // outputs: total bytes each (S is zeroed over dec_pad(total))
    uint64_t models, tab;                             // the QUAL and SEQ tables
    uint64_t total, ngaps, nchs;
    uint32_t qin_len, sin_len, n, ntip;
};
static_assert(sizeof(DecDesc) == 144, "DecDesc is copied to the device as it is");

template <class W>
SAD_HD void dec_block_qual(W& w, uint8_t* base, const DecDesc& d, DecChain& c, int32_t qlevel, uint32_t slice, uint32_t& ev)
{
    dec_qual_slice(w, c, base + d.qin, d.qin_len, reinterpret_cast<const uint32_t*>(base + d.lens), d.n, base + d.Q, base + d.models,
                   qlevel, slice, ev);
}

// The placement once the QUAL chain is over; the block's status so far (a QUAL
// chain that has not ended after its launches is SA_DEC_STUCK).  A status ends
// the SEQ chain before it starts.
SAD_HD uint32_t dec_block_place(uint8_t* base, const DecDesc& d, const DecChain& qc, DecChain& sc)
{
    uint32_t st = qc.status ? qc.status : !qc.done ? (uint32_t)SA_DEC_STUCK : 0u;
    if (!st)
        st = dec_place(base + d.Q, base + d.S, d.ntip, reinterpret_cast<const uint64_t*>(base + d.tip_off),
                       reinterpret_cast<const uint32_t*>(base + d.tip_len), base + d.maxq, reinterpret_cast<const uint64_t*>(base + d.exc),
                       reinterpret_cast<const uint64_t*>(base + d.gaps), d.ngaps, base + d.chs, d.nchs);
    if (st) {
        sc.status = st;
        sc.done = 1;
    }
    return st;
}

template <class W>
SAD_HD void dec_block_seq(W& w, uint8_t* base, const DecDesc& d, DecChain& c, uint32_t mask, uint32_t slice, uint32_t& ev)
{
    dec_seq_slice(w, c, base + d.sin, d.sin_len, reinterpret_cast<const uint32_t*>(base + d.lens), d.n, base + d.S, base + d.tab, mask,
                  slice, ev);
}

}  // namespace sa
