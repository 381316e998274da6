// sa_decoder.h -- the driver of the many-blocks decoder (sa_decode_blocks): plain
// host C++ over a small table of backend calls, written like gz_run over
// GzDevice.  sa_decode.hip fills the table with the kernels (DecDevice);
// tests/cpu_emu/decoder_emu.cpp fills it with dec_*_slice<LoopOps> on the host.
//
// A call: dec_prepass on every block (host threads), plan_decode, groups of at
// most `inflight` supported blocks in input order, and per group
//   alloc, upload, init, L x qual_slice, chains, place, L x seq_slice, chains, download
// then dec_md5_verify (host threads).
//
// NO UNBOUNDED WAITS.  L = max(1, ceil(the group's largest symbol count / slice))
// is computed before the group's first launch and the launches are a counted
// for loop: a chain decodes `slice` symbols a launch and has at most `total` of
// them (a block without symbols still takes one launch, which ends its chain).
// The chain states are read after the last launch, never in between; a chain
// that is then neither done nor failed gives its block SA_DEC_STUCK and nothing
// more is launched for it.  No loop here or in a backend asks the device
// whether it has finished.
//
// The backend (a duck-typed struct, every call false + an error text on failure):
//   uint64_t free_bytes()                       the device memory the plan may count on
//   bool alloc(arena, up, out, nb, &h_up, &h_out)
//                                               the group's arena (upload region at 0, `up` bytes; output region
//                                               behind it, `out` bytes; the tables behind that) and the two
//                                               page-locked staging buffers, recycled between groups
//   bool upload(desc, nb, up)                   h_up and the descriptors to the device
//   bool init(nb, out_off, out, qual_table, seq_table)
//                                               fresh tables, zeroed outputs, chain states and status words
//   bool qual_slice(nb, qlevel, slice)          one launch: every chain of the group that is not done, `slice` symbols
//   bool place(nb)                              dec_block_place per block, into the status words
//   bool seq_slice(nb, mask, slice)
//   bool chains(which, c, status, nb)           which 0: the QUAL states; 1: the SEQ states and the status words.
//                                               One transfer, synchronised.
//   bool download(out_off, out)                 the output region into h_out, synchronised
//   bool finish(info)                           adds the group's phase times to info
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "arc_decode_host.h"
#include "sa_decode_logic.h"

namespace sadec {

using namespace sa;

// SA_DEC_SLICE: symbols a launch (unmeasured default);
// SA_DEC_INFLIGHT: a cap on the blocks of a group, 0 = what the memory plan gives
struct DecKnobs {
    uint32_t slice = 1u << 18;
    uint32_t inflight = 0;
};

template <class GetEnv> inline DecKnobs parse_dec_knobs(GetEnv get)
{
    DecKnobs k;
    if (const char* e = get("SA_DEC_SLICE")) k.slice = (uint32_t)std::min<long long>(std::max<long long>(atoll(e), 1), 1ll << 30);
    if (const char* e = get("SA_DEC_INFLIGHT")) k.inflight = (uint32_t)std::min<long long>(std::max<long long>(atoll(e), 0), 65535);
    return k;
}

// f(i) for i < n on up to `threads` host threads (each takes the next index: bounded by n)
template <class F> inline void dec_parallel(uint32_t n, int threads, F f)
{
    const uint32_t nt = (uint32_t)std::min<int64_t>(std::max(threads, 1), n);
    if (nt <= 1) {
        for (uint32_t i = 0; i < n; i++) f(i);
        return;
    }
    std::atomic<uint32_t> next{0};
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nt; t++)
        th.emplace_back([&]() {
            for (uint32_t i = next++; i < n; i = next++) f(i);
        });
    for (auto& x : th) x.join();
}

// the six side arrays of a block's placement, as the device holds them
inline uint64_t dec_side_bytes(const sadh::DecPre& p)
{
    return dec_pad(8 * p.tip_off.size()) + dec_pad(4 * p.tip_len.size()) + dec_pad(p.side.maxq.size()) + dec_pad(8 * p.side.exc.size()) +
           dec_pad(8 * p.side.gaps.size()) + dec_pad(p.side.chs.size());
}

// every array of the descriptor inside the arena, on its boundary (sizes from the descriptor's own counts)
inline bool dec_desc_ok(const DecDesc& d, uint64_t arena, uint64_t qual_table, uint64_t seq_table)
{
    auto in = [&](uint64_t off, uint64_t bytes) { return off % DEC_PAD == 0 && off <= arena && bytes <= arena - off; };
    return in(d.qin, d.qin_len) && in(d.sin, d.sin_len) && in(d.lens, 4ull * d.n) && in(d.tip_off, 8ull * d.ntip) &&
           in(d.tip_len, 4ull * d.ntip) && in(d.maxq, d.ntip) && in(d.exc, 8ull * d.ntip) && d.ngaps <= arena / 8 &&
           in(d.gaps, 8 * d.ngaps) && in(d.chs, d.nchs) && d.total <= arena && in(d.Q, d.total) && in(d.S, dec_pad(d.total)) &&
           in(d.models, qual_table) && in(d.tab, seq_table);
}

struct DecGroup {
    std::vector<uint32_t> blocks;   // indices into the call's arrays, in input order
    std::vector<DecDesc> desc;
    uint64_t up = 0, out = 0, arena = 0;
    uint64_t launches = 0;
};

// the arena of a group: [uploads of every block][Q, S of every block][tables of every block]
inline void dec_layout(DecGroup& g, const std::vector<sadh::DecPre>& pre, const DecPlan& plan, uint32_t slice)
{
    const uint32_t nb = (uint32_t)g.blocks.size();
    g.desc.assign(nb, DecDesc{});
    uint64_t at = 0, most = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += dec_pad(bytes);
        return o;
    };
    for (uint32_t k = 0; k < nb; k++) {
        const sadh::DecPre& p = pre[g.blocks[k]];
        DecDesc& d = g.desc[k];
        d.qin_len = p.qual_len;
        d.sin_len = p.seq_len;
        d.n = p.n;
        d.ntip = (uint32_t)p.tip_off.size();
        d.total = p.total;
        d.ngaps = p.side.gaps.size();
        d.nchs = p.side.chs.size();
        d.qin = take(d.qin_len);
        d.sin = take(d.sin_len);
        d.lens = take(4ull * d.n);
        d.tip_off = take(8ull * d.ntip);
        d.tip_len = take(4ull * d.ntip);
        d.maxq = take(d.ntip);
        d.exc = take(8ull * d.ntip);
        d.gaps = take(8 * d.ngaps);
        d.chs = take(d.nchs);
        most = std::max(most, p.total);
    }
    g.up = at;
    for (uint32_t k = 0; k < nb; k++) {
        g.desc[k].Q = take(g.desc[k].total);
        g.desc[k].S = take(g.desc[k].total);
    }
    g.out = at - g.up;
    for (uint32_t k = 0; k < nb; k++) {
        g.desc[k].models = take(plan.qual_table);
        g.desc[k].tab = take(plan.seq_table);
    }
    g.arena = at;
    g.launches = std::max<uint64_t>(1, (most + slice - 1) / slice);
}

// a block's uploads into the staging buffer (the upload region starts at the arena's offset 0)
inline void dec_stage(uint8_t* h_up, const DecDesc& d, const sadh::DecPre& p)
{
    auto put = [&](uint64_t off, const void* src, uint64_t bytes) {
        if (bytes) memcpy(h_up + off, src, bytes);
    };
    put(d.qin, p.qual, d.qin_len);
    put(d.sin, p.seq, d.sin_len);
    put(d.lens, p.len.data(), 4ull * d.n);
    put(d.tip_off, p.tip_off.data(), 8ull * d.ntip);
    put(d.tip_len, p.tip_len.data(), 4ull * d.ntip);
    put(d.maxq, p.side.maxq.data(), d.ntip);
    put(d.exc, p.side.exc.data(), 8ull * d.ntip);
    put(d.gaps, p.side.gaps.data(), 8 * d.ngaps);
    put(d.chs, p.side.chs.data(), d.nchs);
}

// sa_decode_blocks.  Returns the number of blocks with a status, or -1 (err says why).
template <class Backend>
inline int dec_run(Backend& be, const uint8_t* const* in, const uint64_t* len, const int32_t* long_reads, uint32_t n, const sa_cfg* cfg,
                   const uint8_t* tmpl, int threads, sa_decoded* out, uint32_t* status, const DecKnobs& kn, sa_decode_info& info,
                   std::string& err)
{
    info = sa_decode_info{};
    info.slice = kn.slice;
    if (!n) return 0;
    if (cfg->lossy > 0.0) {   // (-l: the placement is lenient there and the qualities carry no digest; the host decodes)
        for (uint32_t i = 0; i < n; i++) status[i] = SA_DEC_UNSUPPORTED;
        info.unsupported = n;
        return (int)n;
    }
    std::vector<sadh::DecPre> pre(n);
    dec_parallel(n, threads, [&](uint32_t i) {
        out[i].md5_ok = 1;
        status[i] = in[i] && sadh::dec_prepass(in[i], len[i], cfg, tmpl, long_reads ? long_reads[i] : 0, &out[i], pre[i])
                        ? (uint32_t)SA_DEC_OK
                        : (uint32_t)SA_DEC_LAYOUT;
    });
    // the plan over the blocks that passed (their device bytes: what dec_layout takes of the arena)
    std::vector<uint32_t> ok;
    std::vector<DecBlockSize> bs;
    for (uint32_t i = 0; i < n; i++) {
        if (status[i]) continue;
        ok.push_back(i);
        bs.push_back({dec_pad(pre[i].qual_len) + dec_pad(pre[i].seq_len), pre[i].total, dec_side_bytes(pre[i]), pre[i].n, 0});
    }
    int bad = (int)(n - ok.size());
    if (ok.empty()) return bad;
    std::vector<uint64_t> per(ok.size());
    std::vector<uint8_t> un(ok.size());
    const DecPlan plan = plan_decode(*cfg, (uint32_t)ok.size(), bs.data(), be.free_bytes(), kn.inflight, per.data(), un.data());
    info.inflight = plan.inflight;
    std::vector<DecGroup> groups;
    for (size_t k = 0; k < ok.size(); k++) {
        if (un[k] || !plan.inflight) {
            status[ok[k]] = SA_DEC_UNSUPPORTED;
            info.unsupported++;
            bad++;
            continue;
        }
        if (groups.empty() || groups.back().blocks.size() >= plan.inflight) groups.emplace_back();
        groups.back().blocks.push_back(ok[k]);
    }
    std::vector<DecChain> qc, sc;
    std::vector<uint32_t> st;
    for (DecGroup& g : groups) {
        const uint32_t nb = (uint32_t)g.blocks.size();
        dec_layout(g, pre, plan, kn.slice);
        for (const DecDesc& d : g.desc)
            if (!dec_desc_ok(d, g.arena, plan.qual_table, plan.seq_table)) {
                err = "sa_decode_blocks: a block's arrays lie outside the group's allocation";
                return -1;
            }
        uint8_t *h_up = nullptr, *h_out = nullptr;
        if (!be.alloc(g.arena, g.up, g.out, nb, &h_up, &h_out)) return -1;
        dec_parallel(nb, threads, [&](uint32_t k) { dec_stage(h_up, g.desc[k], pre[g.blocks[k]]); });
        if (!be.upload(g.desc.data(), nb, g.up) || !be.init(nb, g.up, g.out, plan.qual_table, plan.seq_table)) return -1;
        for (uint64_t l = 0; l < g.launches; l++)   // counted: never "until done"
            if (!be.qual_slice(nb, cfg->qlevel, kn.slice)) return -1;
        qc.assign(nb, DecChain{});
        sc.assign(nb, DecChain{});
        st.assign(nb, 0);
        if (!be.chains(0, qc.data(), nullptr, nb) || !be.place(nb)) return -1;
        for (uint64_t l = 0; l < g.launches; l++)   // counted
            if (!be.seq_slice(nb, dec_seq_mask(cfg->slevel), kn.slice)) return -1;
        if (!be.chains(1, sc.data(), st.data(), nb) || !be.download(g.up, g.out) || !be.finish(info)) return -1;
        info.groups++;
        info.qual_launches += (uint32_t)g.launches;
        info.seq_launches += (uint32_t)g.launches;
        for (uint32_t k = 0; k < nb; k++) {
            // the QUAL chain's end or the placement (the status word), then the SEQ chain's
            uint32_t s = qc[k].status ? qc[k].status : !qc[k].done ? (uint32_t)SA_DEC_STUCK : st[k];
            if (!s) s = sc[k].status ? sc[k].status : !sc[k].done ? (uint32_t)SA_DEC_STUCK : 0u;
            status[g.blocks[k]] = s;
            bad += s != 0;
        }
        dec_parallel(nb, threads, [&](uint32_t k) {
            const uint32_t i = g.blocks[k];
            const DecDesc& d = g.desc[k];
            if (status[i] || !d.total) return;
            memcpy(out[i].qual, h_out + (d.Q - g.up), d.total);
            memcpy(out[i].seq, h_out + (d.S - g.up), d.total);
        });
    }
    if (cfg->md5)
        dec_parallel(n, threads, [&](uint32_t i) {
            if (!status[i])
                out[i].md5_ok = sadh::dec_md5_verify(&out[i], pre[i].name_total, pre[i].total, true, pre[i].dg_id, pre[i].dg_q, pre[i].dg_s);
        });
    return bad;
}

}  // namespace sadec
