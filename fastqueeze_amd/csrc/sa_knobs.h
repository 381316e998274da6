// sa_knobs.h -- every SA_* environment knob of the engine (sa_engine.hip) in one
// table: EngineKnobs is parsed once when a context is created, RunKnobs at the
// top of every run.  Host-only (no HIP header): tests/cpu_emu sweeps the
// parsing on the CPU (tests/test_plan.py).  The comments carry each knob's
// measured A/B history.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace sa {

// Constants of sa_kernels.hip / sa_logic.h the host planning needs; the engine
// static_asserts each against the kernels' own.
namespace host_k {
constexpr int SORT_MIN_DB = 7, SORT_MAX_DB = 9;
constexpr uint32_t WQ_CHUNK = 64;
constexpr uint32_t KEY_SLACK = 128;
constexpr uint32_t AUX_DENSE_BITS = 17;
constexpr uint32_t SEQ_HALVE_J = 242;
constexpr uint32_t LONG_RUN = 512;
constexpr uint32_t RB_CHUNK = 8192, RB_CHUNK_DEFAULT = 7904;
}  // namespace host_k

using GetEnv = const char* (*)(const char*);   // std::getenv in the product

struct EngineKnobs {
    // the dense AUX sort (k_aux_presence / k_aux_dense: one 9-bit pass over the
    // blocks' dense model ids instead of two over the 17-bit ids).  SA_AUX_DENSE=0:
    // off.  This is the context's initial flag: sa_ctx::aux_dense is the state
    // (a batch with more than 512 models in a block turns it off).
    bool aux_dense = true;
    uint32_t chain_prio = 1;   // s_setprio 3 in the latency-bound chain kernels (SA_CHAIN_PRIO=0: off)
    uint32_t md5_prio = 1;     // ... and in k_md5 (SA_MD5_PRIO; off the critical path); unset: chain_prio
    bool prep_fused = false;   // (set at all) name columns in k_prep_sq16 (A/B)
    bool prep_wave = false;    // (set at all) k_prep_sq instead of k_prep_sq16
    bool emit_wave = false;    // (set at all) k_emit_sq for SEQ / QUAL / N-IUPAC
    // records per chunk in the L passes (SA_L_CHUNK=16: 56 VGPRs, 8 waves per
    // SIMD, half a line per chunk; 32: 88 VGPRs, 5 waves, a whole line)
    uint32_t l_chunk = 32;
    // the L passes at issue priority 2 (they are on the batch's critical path,
    // the other contexts' fronts beside them are not always; SA_L_PRIO=1, A/B)
    uint32_t l_prio = 0;
    bool seq_unpacked = false;   // SA_SEQ_PACK=0: unpacked SEQ keys at every k
    // k_prep_sq16 / k_emit_sq16 with the round-4 static grid stride instead of
    // reads taken from a counter (WaveReads; SA_FRONT_STATIC=1, A/B)
    bool front_static = false;
    // reads a front wave takes from the counter at a time (WaveReads): 0 = by the
    // batch's mean read length (front_wq_chunk), SA_WQ_CHUNK=n to fix it (A/B;
    // 64 was the only value until round 6)
    uint32_t wq_chunk_env = 0;
    // pass R with one chain per lane in the VALU (k_coder_rl: the scalar units
    // stay free for the front kernels of the other batches) instead of one
    // chain per wave on the scalar unit (k_coder_rv); SA_RV_LANES=1 / 0.  Off:
    // pass R 1,835-1,864 against 679-689 ms under the bench's load, the bench
    // 7,971-8,064 against 16,849-16,908 MB/s (r5k)
    bool rv_lanes = false;
    // the SEQ space sorted by the context's low 8-9 bits only and replayed per
    // bucket with the models in LDS (k_replay_seq_bkt, contexts of <= 22 bits);
    // SA_SEQ_BUCKET=0: the full sort and k_replay_seq.  By the low bits the
    // bench gained 1-3 % (r5k: 17,039 / 17,349 against 16,908 / 16,849 MB/s,
    // SEQ sort + replay 84 against 88-98 ms); by the top bits it had lost
    // (r5e-r5h: 14.9-15.4 against 15.9-16.8 GB/s)
    bool seq_bucket = true;
    // the bucket replay's records in sorted order (coalesced stores), then put
    // in stream order by a gather through the sort's inverse permutation, which
    // the bucket pass writes in stream order instead of the positions
    // (k_seq_unpermute); SA_SEQ_INV=0: one scattered 4-byte store per symbol
    bool seq_inv = true;
    // SA_BKT_DB=8 / 9 / 10: the bucket pass's digit bits (default 8 for contexts
    // of <= 20 bits, 9 above; 10 with the inverse-permutation pass only)
    int bkt_db_env = 0;
    // SA_PREP_ROW=64: a whole wave per read (round 6; for long reads the ONT
    // batch's prep+scan measured the same as with 16-lane rows under load, r6l:
    // 44.2 / 46.4 against 44.9 / 41.4 ms, so 16 stays the default)
    int prep_row = 0;
    // the bucket replay's largest digits first (k_bkt_order); SA_BKT_LPT=0: digit order
    bool bkt_lpt = true;
    // SA_BKT_PROBE=file: per bucket-replay wave its clocks and steps, appended
    // to file (the front waits for the replay to read them back: diagnostics)
    const char* bkt_probe = nullptr;
    // workgroups per CU of the grid-stride wave-per-read kernels (SA_WAVE_GRID, at least 1)
    uint32_t wg_per_cu = 8;
    // k_md5<true> reads the next block's words while the chain runs: 148 VGPRs instead
    // of 60, which costs the co-resident front kernels more than it saves (r2x:
    // 11.6 vs 12.9 GB/s), so SA_MD5_PIPE=1 only
    bool md5_pipe = false;
    // k_md5_lanes: one message per lane of a chain wave (the bench batch's 207
    // messages in 4 chain waves) instead of k_md5's wave per message, whose 64
    // lanes all run the same chain; SA_MD5_LANES=0: k_md5<false> (A/B, fallback).
    // SA_MD5_PIPE=1 goes before it.  The 207 chain waves at chain priority
    // took vector issue from the front kernels and L passes on their SIMDs:
    // the bench 21,289-21,635 against 19,217-19,498 MB/s, three alternating
    // runs each; front span 129 against 161 ms, L1..L3 39 against 69 ms, MD5
    // itself 250 against 294 ms a batch (profiles/md5_lanes_ab.json)
    bool md5_lanes = true;
    // The waits between a context's streams happen on the host thread (which
    // has nothing else to do then) instead of as barrier packets: the boxes run
    // with four hardware queues per process (GPU_MAX_HW_QUEUES=4), so the
    // contexts' streams share queues, and a barrier waiting for this batch's
    // front or long runs held up every other context's work queued behind it
    // (pass R, L passes).  SA_HOST_WAITS=0: device-side waits, for A/B.
    bool host_waits = true;
    // pass-R placement (k_coder_rv): four chains per workgroup, one per SIMD, and
    // enough unused LDS that a CU holds one pass-R workgroup (SA_CODER_WAVES: 1
    // or 2, else 4; SA_CODER_LDS: 0..160 KiB)
    uint32_t coder_waves = 4;
    uint32_t coder_lds = 82 * 1024;
    // the pass-R step order (k_coder_rv<V>): 5 = the 24 v_readlane of eight steps
    // issued together ahead of their SALU steps (r4z3: pass R 671-675 against
    // 767-776 ms, the bench +3-5 %); 0 = a step's three v_readlane ahead of it.
    // The batched moves hold the vector unit of their SIMD longer, and batches
    // of long reads (mean > 1000 bp), whose fronts are VALU-heavy and set the
    // pace, ran 11 % slower with them (r4z5: ONT shape 7,187 / 7,281 against
    // 8,081 / 8,260 MB/s), so those keep 0.  SA_RV_VARIANT=0 / 5: one for all.
    // Round 6: 6 = the operands through SMEM from a per-wave ring the lanes fill
    // (k_coder_rv<6>, coder_rg_chain): the chain itself is faster (r6b: one
    // context alone 504 against 630 ms; under the bench's load 626-644 against
    // 665-691) but it issues 10 SALU per symbol instead of 8 and holds its SIMD's
    // scalar issue ~90 % of the time, so the kernels that share those SIMDs
    // slow (L passes 89 against 52 ms, prep 16 against 10) and the bench lost
    // 3 % (r6b / r6c: 16,623-16,904 against 17,281-17,493 MB/s).  On the tree
    // with the full-segment L passes the bench is level (r6m: 19,301 / 19,237
    // against 19,437 / 19,279) and the command line, whose batches' latency
    // sets its pace, faster: 42.8 GB in 3.47 / 3.53 s against 4.22 / 3.89 s
    // (r6o); and in r6q the bench too (19,339 / 19,422 against 18,386 /
    // 18,851 MB/s), so 6 is the default for short-read batches since round 6.
    int rv_variant = -1;
    // (default variant, A/B) 6 only while at most SA_RV_V6_MAX other contexts of
    // the device are in pass R, else 5; -1: 5 always.  Unset: 6 always -- the
    // limit measured no better (r6q: bench 19,106 / 19,264 with 2, 18,386 /
    // 18,851 with -1, 19,339 / 19,422 without; 42.8 GB in 5.02 / 4.28 s with 2,
    // 4.44 / 4.11 with -1, 4.35 / 4.17 without)
    int rv_v6_max = 1 << 30;
    // pass R's wait for records the long runs have not written (SA_RV_WAIT_MS, default 20 s: the
    // long runs take ~0.4 s; a wave that waits longer gives up and the batch fails with E_CODER),
    // in ticks of the 100 MHz clock, at most 4e9
    uint32_t rv_wait_ticks = 2000000000u;
    bool test_skip_long = false;   // (set at all; tests: starve pass R)
    // pass R: the chains under RV_LONG_SYMS symbols share this many waves
    // (k_coder_rv; SA_RV_SHORT_WAVES=0: a wave per chain)
    uint32_t rv_short_waves = 32;
    bool trace = false;   // (set at all) SA_TRACE: phase timing on, per sub-batch host timings
    // SA_RV_PROBE=file: per pass-R wave its timing and placement, appended to
    // the file per batch (diagnostics, k_coder_rv)
    const char* rv_probe = nullptr;
    // SA_RB_APPLY=1: the round-4 second full walk (k_rb_apply) instead of k_rb_true + k_rb_fill (A/B)
    bool rb_apply_walk = false;
    // SA_RB_FIX_SERIAL=1: the entries by k_rb_fix (a lane per block, chunk by
    // chunk) instead of k_rb_fix_w (a wave per block, 64 chunks a step; A/B)
    bool rb_fix_serial = false;
    // k_rb_spec on n workgroups per CU taking 64 chunks at a time from a
    // counter (round 6: n = 2, the ONT batch's prep+scan 25.0 / 26.4 against
    // 28.6 / 29.7 ms with one grid of a lane per chunk, r6z8; 4: no gain);
    // SA_RB_SPEC_WG=n to change, 0 = the one grid
    uint32_t rb_spec_wg = 2;
    // R-Block chunk length, also the stride of the per-chunk arrays (opens,
    // vals): SA_RB_CHUNK=n, a multiple of 32 up to RB_CHUNK.  Not a power of
    // two: the lanes of k_rb_spec walk their chunks in step, so at 8192 every
    // lane's load and store of a step fell on addresses 8 KiB apart (round 6)
    uint32_t rb_chunk = host_k::RB_CHUNK_DEFAULT;
    // The long AUX model runs replay on every SA_LONG_CU_EVERY-th CU (st4,
    // latency-bound) while the SEQ path (st3, throughput) runs on the others
    // without sharing a SIMD; 1: both on all CUs.  SA_LONG_LDS: the LDS per
    // long-run workgroup, i.e. how many share a CU.
    int long_cu_every = 4;
    uint32_t long_lds = 0;
    // (A/B, round 5) SA_RV_CUS=n (1..5, with every = 4): pass R and the L passes
    // (st3) on n of each 8 CUs only, the front (st) on the others -- the scalar
    // units of the front's CUs free of chain waves (k_coder_rl showed the
    // fronts 2-3x faster beside a pass R that leaves the scalar units alone)
    int rv_cus = 0;
    // k_replay_aux_long workgroups: 0 = what the long-run CUs hold at once (6 per
    // CU); SA_LONG_GRID overrides (at least 1; round 2 used 2048)
    uint32_t long_grid_env = 0;
    // SA_L_CU_EVERY=N (N >= 2): the L passes of the coder (L1 / L2 / L3) on a
    // stream of their own, masked to every N-th CU, after the host has seen
    // pass R end (the L passes are throughput kernels: on pass R's CUs they
    // take the whole GPU for ~40 ms per batch and the other batches' front
    // kernels beside them run ~3x slower, round 4 r4c trace).  1 (A/B, round 6):
    // that stream on the front's CUs.  0: after pass R on its stream (st3).
    int l_cu_every = 0;
};

inline EngineKnobs parse_knobs(GetEnv get)
{
    auto num = [&](const char* n, int unset) { const char* e = get(n); return e ? std::atoi(e) : unset; };
    auto is_set = [&](const char* n) { return get(n) != nullptr; };
    auto nonzero = [&](const char* n) { return num(n, 0) != 0; };        // on when set and not 0
    auto unless_zero = [&](const char* n) { return num(n, 1) != 0; };    // off when set and 0
    EngineKnobs k;
    k.aux_dense = unless_zero("SA_AUX_DENSE");
    k.chain_prio = unless_zero("SA_CHAIN_PRIO") ? 1u : 0u;
    k.md5_prio = is_set("SA_MD5_PRIO") ? (nonzero("SA_MD5_PRIO") ? 1u : 0u) : k.chain_prio;
    k.prep_fused = is_set("SA_PREP_FUSED");
    k.prep_wave = is_set("SA_PREP_WAVE");
    k.emit_wave = is_set("SA_EMIT_WAVE");
    k.l_chunk = num("SA_L_CHUNK", 32) == 16 ? 16u : 32u;
    k.l_prio = nonzero("SA_L_PRIO") ? 1u : 0u;
    k.seq_unpacked = !unless_zero("SA_SEQ_PACK");
    k.front_static = nonzero("SA_FRONT_STATIC");
    k.wq_chunk_env = (uint32_t)num("SA_WQ_CHUNK", 0);
    k.rv_lanes = nonzero("SA_RV_LANES");
    k.seq_bucket = unless_zero("SA_SEQ_BUCKET");
    k.seq_inv = unless_zero("SA_SEQ_INV");
    k.bkt_db_env = num("SA_BKT_DB", 0);
    k.prep_row = num("SA_PREP_ROW", 0);
    k.bkt_lpt = unless_zero("SA_BKT_LPT");
    k.bkt_probe = get("SA_BKT_PROBE");
    k.wg_per_cu = (uint32_t)std::max(1, num("SA_WAVE_GRID", 8));
    k.md5_pipe = nonzero("SA_MD5_PIPE");
    k.md5_lanes = unless_zero("SA_MD5_LANES");
    k.host_waits = unless_zero("SA_HOST_WAITS");
    const int w = num("SA_CODER_WAVES", 4);
    k.coder_waves = (w == 1 || w == 2) ? (uint32_t)w : 4u;
    k.coder_lds = (uint32_t)std::min(std::max(num("SA_CODER_LDS", 82 * 1024), 0), 160 * 1024);
    k.rv_variant = num("SA_RV_VARIANT", -1);
    k.rv_v6_max = num("SA_RV_V6_MAX", 1 << 30);
    if (is_set("SA_RV_WAIT_MS"))
        k.rv_wait_ticks = (uint32_t)std::min<uint64_t>(100000ull * (uint64_t)std::max(1, num("SA_RV_WAIT_MS", 1)),
                                                       4000000000ull);
    k.test_skip_long = is_set("SA_TEST_SKIP_LONG");
    k.rv_short_waves = (uint32_t)num("SA_RV_SHORT_WAVES", 32);
    k.trace = is_set("SA_TRACE");
    k.rv_probe = get("SA_RV_PROBE");
    k.rb_apply_walk = nonzero("SA_RB_APPLY");
    k.rb_fix_serial = nonzero("SA_RB_FIX_SERIAL");
    k.rb_spec_wg = (uint32_t)std::max(0, num("SA_RB_SPEC_WG", 2));
    const uint32_t rc = (uint32_t)num("SA_RB_CHUNK", (int)host_k::RB_CHUNK_DEFAULT);
    k.rb_chunk = rc >= 32 && rc <= host_k::RB_CHUNK && rc % 32 == 0 ? rc : host_k::RB_CHUNK;
    k.long_cu_every = std::max(1, num("SA_LONG_CU_EVERY", 4));
    k.long_lds = (uint32_t)num("SA_LONG_LDS", 0);
    k.rv_cus = num("SA_RV_CUS", 0);
    k.long_grid_env = is_set("SA_LONG_GRID") ? (uint32_t)std::max(1, num("SA_LONG_GRID", 1)) : 0u;
    k.l_cu_every = num("SA_L_CU_EVERY", 0);
    return k;
}

// What a run reads when it starts (the tests set these after the context exists).
struct RunKnobs {
    uint64_t payload_slack = 4096;   // SA_PAYLOAD_SLACK: bytes on top of a stream's exact cap (tests: the fallback)
    bool find_runs = false;          // (set at all) SA_FIND_RUNS: k_find_runs after the one dense pass (A/B)
    bool aln_trace = false;          // (set at all) SA_ALN_TRACE: the reference path's progress on stderr
    uint64_t batch_bases = ~0ull;    // SA_BATCH_BASES: bases per sub-batch of sa_encode_blocks (tests)
    // SA_SORT_MIN_DB (7..9; 8: round 1's floor, for A/B): no sort pass of fewer
    // digit bits.  Read once per process: the engine fills it from its first read.
    int sort_min_db = host_k::SORT_MIN_DB;
};

inline int parse_sort_min_db(GetEnv get)
{
    const char* e = get("SA_SORT_MIN_DB");
    return e ? std::max(7, std::min(9, std::atoi(e))) : host_k::SORT_MIN_DB;
}

inline RunKnobs parse_run_knobs(GetEnv get, int sort_min_db)
{
    RunKnobs r;
    if (const char* e = get("SA_PAYLOAD_SLACK")) r.payload_slack = std::strtoull(e, nullptr, 10);
    r.find_runs = get("SA_FIND_RUNS") != nullptr;
    r.aln_trace = get("SA_ALN_TRACE") != nullptr;
    if (const char* e = get("SA_BATCH_BASES")) {
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v > 0) r.batch_bases = v;
    }
    r.sort_min_db = sort_min_db;
    return r;
}

}  // namespace sa
