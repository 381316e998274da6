// sa_plan.h -- host-side layout of a batch after the per-read count scan:
// symbol spaces, sort segments, coder tasks and the final output arena.
// And, before any of it is known, which kernels the batch will run
// (plan_paths, plan_totals): the engine launches what these decide.
// Shared by the engine (sa_engine.hip) and the CPU decomposition test.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/seqarc_amd.h"
#include "sa_device.h"
#include "sa_knobs.h"

namespace sa {

inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

struct SortPlan {
    std::vector<SortSeg> segs;
    std::vector<uint32_t> tile_seg;
    uint64_t total = 0;
};

inline SortPlan plan_sort(const std::vector<uint64_t>& counts)
{
    SortPlan p;
    uint64_t base = 0;
    uint32_t tile = 0;
    for (size_t s = 0; s < counts.size(); s++) {
        SortSeg g{};
        g.base = base;
        g.count = (uint32_t)counts[s];
        g.ntiles = (uint32_t)((counts[s] + SORT_TILE - 1) / SORT_TILE);
        g.tile0 = tile;
        for (uint32_t t = 0; t < g.ntiles; t++) p.tile_seg.push_back((uint32_t)s);
        tile += g.ntiles;
        base += (uint64_t)g.ntiles * SORT_TILE;
        p.segs.push_back(g);
    }
    p.total = base;
    return p;
}

// The SEQ bucket replay (k_replay_seq_bkt): one sort pass over the context's
// low `db` bits, then a wave per (block, digit) replays the bucket with the
// models of the remaining high `sb` context bits in LDS.
struct BktPlan {
    int db, sb;
};

// contexts the bucket replay takes (packed keys only): 12..22 bits, Slevel <= 4
inline bool bkt_applies(int seq_bits) { return seq_bits >= 12 && seq_bits <= 22; }

// dynamic LDS of a k_replay_seq_bkt wave holding sb context bits
inline uint32_t bkt_lds_bytes(int sb) { return 5u * ((1u << sb) + 64u); }

constexpr uint32_t BKT_LDS_MAX = 65536;   // what a launch gets without raising the kernel's limit

// The digit width for contexts of seq_bits bits.  db_env (SA_BKT_DB, 0: unset)
// is taken when it is 8 / 9 (10 with the inverse-permutation pass, seq_inv),
// leaves a wave at least 4 context bits and fits its models in BKT_LDS_MAX
// (8 at 22 bits would need 82,240 B: refused); otherwise the default, 8 up to
// 20 bits and 9 above.
inline BktPlan plan_bkt(int seq_bits, int db_env, bool seq_inv)
{
    int db = seq_bits <= 20 ? 8 : 9;
    if (db_env >= 8 && db_env <= (seq_inv ? 10 : 9) && seq_bits - db_env >= 4 &&
        bkt_lds_bytes(seq_bits - db_env) <= BKT_LDS_MAX)
        db = db_env;
    return BktPlan{db, seq_bits - db};
}

// Digit widths of a sort over bits [lo, hi): the fewest passes of at most
// max_db bits, widths as even as possible and at least min_db (a digit may
// reach above hi: those key bits are 0, or 1 in the pad keys, which sort last
// anyway).
inline std::vector<int> sort_digits(int lo, int hi, int max_db, int min_db)
{
    std::vector<int> w;
    if (hi <= lo) return w;
    const int bits = hi - lo, passes = (bits + max_db - 1) / max_db;
    for (int p = 0, done = 0; p < passes; p++) {
        const int d = (bits - done + (passes - p) - 1) / (passes - p);
        w.push_back(std::max(d, min_db));
        done += d;
    }
    return w;
}

// the digit widths of a sort, first pass in the low four bits (sa_paths)
inline uint32_t pack_digits(const std::vector<int>& w)
{
    uint32_t p = 0;
    for (size_t i = 0; i < w.size() && i < 8; i++) p |= (uint32_t)w[i] << (4 * i);
    return p;
}

// histogram words per tile of a sort over bits [lo, hi)
inline uint64_t sort_hist_per_tile(int lo, int hi, int max_db, int min_db)
{
    int m = 0;
    for (int d : sort_digits(lo, hi, max_db, min_db)) m = std::max(m, d);
    return 1ull << m;
}

// Reads per take of the front kernels' read counter: ~64 reads' worth of
// 150 bp (about 10 KB of bases) a take, so short-read batches keep WQ_CHUNK
// and long-read batches take one wave's four reads at a time; a multiple of
// four (the rows of a wave).
inline uint32_t front_wq_chunk(const EngineKnobs& k, uint64_t seq_bytes, uint32_t nreads)
{
    if (k.wq_chunk_env) return std::max<uint32_t>(4, std::min<uint32_t>(1024, k.wq_chunk_env & ~3u));
    const uint64_t mean = nreads ? std::max<uint64_t>(1, seq_bytes / nreads) : 1;
    const uint64_t c = (uint64_t)host_k::WQ_CHUNK * 150 / mean;
    return (uint32_t)std::max<uint64_t>(4, std::min<uint64_t>(host_k::WQ_CHUNK, c) & ~3ull);
}

// ---- which kernels a batch runs, decided before anything is launched ----
struct PathCfg {
    int slevel, qlevel;
    bool lossy, md5;
};
struct BatchShape {
    uint32_t nreads;
    uint64_t seq_bytes;
    uint32_t nblocks;
    bool reference;   // the reference (HASH index) path
    bool aux_dense;   // the context's dense flag when the batch starts
};

struct PathPlan {
    // k <= 14: the SEQ key carries the base in its low two bits and the values
    // are the stream position, i.e. the index (the emitter writes no values, the
    // first sort pass computes them); k = 15 fills all 32 key bits (a key could
    // equal the sort pad) and order 0 has no sort pass, so they keep values
    // position << 2 | base (SA_SEQ_PACK=0: always)
    int seq_bits;       // NS = 1 << seq_bits (x86 shl masks the count)
    uint32_t ns, seq_sh;
    // contexts of <= 22 bits (Slevel <= 4): one sort pass over the context's low
    // 8 (9) bits, the high bkt.sb bits replayed per bucket with the models in LDS
    // (k_replay_seq_bkt); longer contexts: the full sort and k_replay_seq
    bool seq_bkt, seq_inv;
    // (SA_BKT_DB: one more digit bit halves the models a replay wave holds in
    // LDS -- 2^12 contexts in 20 KB instead of 2^13 in 40 KB at 22 bits --
    // for twice the waves per CU; 10 bits with the inverse-permutation pass only;
    // plan_bkt refuses a width whose models do not fit the launch's LDS)
    BktPlan bkt;
    int seq_lo, seq_hi, seq_max_db;   // (the bucket pass sorts by the context's LOW bits)
    std::vector<int> seq_dg;          // the SEQ sort's digit widths (the bucket sort: one pass)
    bool bkt_lpt;                     // the bucket replay's largest digits first (k_bkt_order)
    int aux_bits;
    uint32_t prep, emit;      // SA_PATH_PREP_* / SA_PATH_EMIT_* (0: a batch without reads)
    bool front_counter;       // k_prep_sq16 / k_emit_sq16 take their reads from a counter
    bool report_counter;      // ... and one of them runs (sa_paths::front_counter)
    uint32_t wqc;             // reads a take (front_wq_chunk)
    bool dege_counter;        // k_emit_sq's listed reads from a counter (one a take) for long-read batches
    bool dege_maxq;           // the prep leaves the N / IUPAC maxq (not k_prep_sq: k_emit's serial path)
    int rv_batch;             // pass R's variant (see EngineKnobs::rv_variant)
    uint32_t md5;             // sa_paths::md5: 0 none, 1 k_md5_lanes, 2 k_md5<true>, 3 k_md5<false>
    bool aux_dense;
    bool skip_long;           // (SA_TEST_SKIP_LONG) no k_replay_aux_long: pass R starves
    // -l R (a batch with qualities): k_rb_spec from a counter on rb_spec_wg
    // workgroups per CU (0: one grid); k_rb_fix_w, not k_rb_fix; k_rb_apply's
    // walk instead of k_rb_true + k_rb_fill; the chunk length and array stride
    bool rblock, rb_fix_wave, rb_apply_walk;
    uint32_t rb_spec_wg, rb_chunk;
};

inline PathPlan plan_paths(const EngineKnobs& k, const RunKnobs& rk, const PathCfg& cfg, const BatchShape& sh)
{
    PathPlan p{};
    const int kk = cfg.slevel + 7;
    p.seq_bits = (2 * kk) & 31;
    p.ns = 1u << p.seq_bits;
    p.seq_sh = (p.ns > 1 && p.seq_bits <= 28 && !k.seq_unpacked) ? 2u : 0u;
    p.seq_bkt = k.seq_bucket && p.seq_sh == 2 && bkt_applies(p.seq_bits);
    p.seq_inv = p.seq_bkt && k.seq_inv;
    p.bkt = plan_bkt(p.seq_bits, k.bkt_db_env, k.seq_inv);
    p.seq_max_db = p.seq_bkt ? std::max(p.bkt.db, host_k::SORT_MAX_DB) : host_k::SORT_MAX_DB;
    p.seq_lo = (int)p.seq_sh;
    p.seq_hi = p.ns > 1 ? (int)p.seq_sh + (p.seq_bkt ? p.seq_bits - p.bkt.sb : p.seq_bits) : 0;
    p.seq_dg = sort_digits(p.seq_lo, p.seq_hi, p.seq_max_db, rk.sort_min_db);
    p.bkt_lpt = k.bkt_lpt;
    p.aux_bits = cfg.qlevel > 2 ? 21 : 17;
    if (sh.nreads) {
        p.prep = k.prep_fused ? SA_PATH_PREP_FUSED : k.prep_wave ? SA_PATH_PREP_WAVE
                 : k.prep_row == 64 ? SA_PATH_PREP_ROW64 : SA_PATH_PREP_ROW16;
        p.emit = k.emit_wave ? SA_PATH_EMIT_WAVE : SA_PATH_EMIT_ROW16;
    }
    p.front_counter = !k.front_static;
    // (k_prep_sq and k_emit_sq walk a static stride whatever the knob says)
    p.report_counter = sh.nreads && p.front_counter && !(k.prep_wave && k.emit_wave);
    p.wqc = front_wq_chunk(k, sh.seq_bytes, sh.nreads);
    p.dege_counter = !k.front_static && p.wqc < host_k::WQ_CHUNK;
    p.dege_maxq = !k.prep_wave;
    p.rv_batch = k.rv_variant == 0 || k.rv_variant == 5 || k.rv_variant == 6
                     ? k.rv_variant
                     : (sh.nreads && sh.seq_bytes / sh.nreads > 1000 ? 0 : 6);
    p.md5 = cfg.md5 ? (k.md5_pipe ? 2u : k.md5_lanes ? 1u : 3u) : 0u;
    p.aux_dense = sh.aux_dense;
    p.skip_long = k.test_skip_long;
    p.rblock = cfg.lossy && sh.seq_bytes > 0;
    p.rb_fix_wave = !k.rb_fix_serial;
    p.rb_apply_walk = k.rb_apply_walk;
    p.rb_spec_wg = k.rb_spec_wg;
    p.rb_chunk = k.rb_chunk;
    return p;
}

// What depends on the totals of the count scan: the padded sizes of the two
// symbol spaces (SortPlan::total) and the batch's N / IUPAC bases.
struct TotalsPlan {
    bool dense;          // the dense AUX sort (17 model bits, the context's flag on)
    int aux_passes;      // odd: the emit writes the front scratch, even: the context's buffer (ping-pong)
    // element counts; slack: the replay loops read up to 2 chunks past a run's
    // end, pass R one 16-record chunk past a stream's last full segment
    uint64_t stot, atot, max_long, max_seq_long, max_short;
    uint64_t seq_hist_per_tile, aux_hist_per_tile;
    uint32_t seq_digits, aux_digits_raw;   // pack_digits (sa_paths)
    bool dege_list;      // k_dege_list + the listed k_emit_sq
};

inline TotalsPlan plan_totals(const EngineKnobs& k, const RunKnobs& rk, const PathPlan& p, const BatchShape& sh,
                              uint64_t seq_total, uint64_t aux_total, uint64_t n_ch)
{
    TotalsPlan t{};
    const int a_lo = (int)AUX_SYM_BITS, a_hi = (int)AUX_SYM_BITS + p.aux_bits, mx = host_k::SORT_MAX_DB;
    t.dense = p.aux_dense && p.aux_bits == (int)host_k::AUX_DENSE_BITS && aux_total;
    t.aux_passes = t.dense ? 1 : (int)sort_digits(a_lo, a_hi, mx, rk.sort_min_db).size();
    t.stot = seq_total + host_k::KEY_SLACK;
    t.atot = aux_total + host_k::KEY_SLACK;
    t.max_long = aux_total / host_k::LONG_RUN + 1;
    t.max_seq_long = seq_total / (host_k::SEQ_HALVE_J + 1) + 1;
    // at most one run per (block, model) and per symbol
    t.max_short = std::max<uint64_t>(std::min<uint64_t>(aux_total, (uint64_t)sh.nblocks << p.aux_bits), 1);
    t.seq_hist_per_tile = 1;
    for (int d : p.seq_dg) t.seq_hist_per_tile = std::max<uint64_t>(t.seq_hist_per_tile, 1ull << d);
    t.aux_hist_per_tile = sort_hist_per_tile(a_lo, a_hi, mx, rk.sort_min_db);
    t.seq_digits = seq_total ? pack_digits(p.seq_dg) : 0u;
    t.aux_digits_raw = pack_digits(sort_digits(a_lo, a_hi, mx, rk.sort_min_db));
    t.dege_list = sh.nreads && p.emit == SA_PATH_EMIT_ROW16 && p.dege_maxq && n_ch;
    return t;
}

// sa_paths (sa_last_paths) from the plan: everything the host decides without
// the device's answers.  What becomes known later is reported there: aux_sort /
// aux_digits / aux_runs / aux_nmod_max of a dense batch and aux_dense_next
// (after the model counts), pass R's and the L passes' fields (the coder),
// exact_rerun.  front_masked, long_grid: the context's (from its CU masks).
inline void report_paths(sa_paths& P, const EngineKnobs& k, const PathPlan& p, const TotalsPlan& t, uint64_t seq_total,
                         uint64_t aux_total, bool front_masked, uint32_t long_grid)
{
    P.md5 = p.md5;
    P.wg_per_cu = k.wg_per_cu;
    P.prep = p.prep;
    P.emit = p.emit;
    P.front_counter = p.report_counter ? 1u : 0u;
    P.dege_list = t.dege_list ? 1u : 0u;
    if (p.rblock) {
        P.rblock = 1;
        P.rb_spec_counter = p.rb_spec_wg > 0 ? 1u : 0u;
        P.rb_fix_wave = p.rb_fix_wave ? 1u : 0u;
        P.rb_apply_walk = p.rb_apply_walk ? 1u : 0u;
        P.rb_chunk = p.rb_chunk;
    }
    P.seq_packed = p.seq_sh == 2 ? 1u : 0u;
    P.seq_digits = t.seq_digits;
    if (seq_total) P.seq_replay = p.seq_bkt ? SA_PATH_SEQ_BUCKET : SA_PATH_SEQ_FULL;
    if (seq_total && p.seq_bkt && p.seq_dg.size() == 1) {
        P.bkt_inv = p.seq_inv ? 1u : 0u;
        P.bkt_lpt = p.bkt_lpt ? 1u : 0u;
        P.bkt_db = (uint32_t)p.seq_dg[0];
        P.bkt_sb = (uint32_t)p.bkt.sb;
    }
    if (aux_total && !t.dense) {
        P.aux_sort = SA_PATH_AUX_RAW;
        P.aux_digits = t.aux_digits_raw;
        P.aux_runs = SA_PATH_RUNS_FIND;
    }
    P.host_waits = k.host_waits ? 1u : 0u;
    P.front_masked = front_masked ? 1u : 0u;
    P.long_grid = long_grid;
}

// The dense AUX sort once the blocks' model counts are back: 9 digit bits up
// to 512 models a block, else all AUX_DENSE_BITS (two passes and a copy); one
// 9-bit pass gives the run lists from its scan (k_runs_dense; SA_FIND_RUNS=1:
// k_find_runs, A/B).
struct DensePlan {
    int dbits;
    bool runs_from_hist;
};
inline DensePlan plan_dense(uint32_t dmax, const RunKnobs& rk)
{
    const int dbits = dmax > 512 ? (int)host_k::AUX_DENSE_BITS : 9;
    return DensePlan{dbits, dbits == 9 && !rk.find_runs};
}

struct BatchPlan {
    SortPlan seq, aux;
    std::vector<CoderTask> tasks;
    std::vector<uint64_t> task_out_base;
    std::vector<AsmBlock> asmb;
    uint64_t total_segs = 0;
    uint64_t payload_bytes = 0;
    uint64_t final_bytes = 0;
};

constexpr uint32_t NO_TASK = 0xffffffffu;   // AsmBlock::task of a stream the layout does not have

// totals: per block, the NCOL column sums of k_scan_reads.  atot (reference
// path only): per block the NACOL sums of the alignment columns, whose streams
// follow the others in the AUX space; mis_model: the Mis stream's model (0: no
// symbols).  Fills the symbol space fields of every DevBlock.  Returns false if
// a block is too large.
inline bool plan_batch(std::vector<DevBlock>& blocks, const std::vector<uint32_t>& totals, BatchPlan& bp,
                       const std::vector<uint32_t>* atot = nullptr, uint32_t mis_model = 0)
{
    const size_t nbk = blocks.size();
    std::vector<uint64_t> seq_counts(nbk), aux_counts(nbk);
    for (size_t b = 0; b < nbk; b++) {
        DevBlock& d = blocks[b];
        const uint32_t* t = &totals[b * NCOL];
        const uint32_t sc[NAUX] = {t[C_LEN], t[C_NAME], t[C_QUAL], t[C_TIP], t[C_CH], t[C_MAXQ], t[C_NCNT], t[C_NPOS]};
        uint64_t a = 0;
        for (int s = 0; s < NSTREAM; s++) d.sbase[s] = d.scount[s] = 0;
        for (int s = 0; s < NAUX; s++) {
            d.sbase[s] = (uint32_t)a;
            d.scount[s] = sc[s];
            a += sc[s];
        }
        if (atot) {
            const uint32_t* at = &(*atot)[b * NACOL];
            for (int k = 0; k < NACOL; k++) {
                const int s = ST_ORD + k;
                d.sbase[s] = (uint32_t)a;
                d.scount[s] = (k == A_MIS && !mis_model) ? 0u : at[k];
                a += d.scount[s];
            }
            d.align_count = at[A_REV];
        }
        // (< 2^30 keys per space: the sort scatter's 32-bit byte offsets in a segment)
        if (a >= (1ull << 30) || t[C_SEQ] >= (1u << 30)) return false;
        d.n_aux = (uint32_t)a;
        d.n_seq = t[C_SEQ];
        for (int s = 0; s < NSTREAM; s++) d.vcount[s] = 0;
        d.vcount[ST_TIP] = d.nreads;
        d.vcount[ST_CH] = t[C_CH];
        d.vcount[ST_MAXQ] = t[C_MAXQ];
        d.vcount[ST_NCNT] = t[C_MAXQ];
        d.vcount[ST_NPOS] = t[C_NPOSV];
        seq_counts[b] = d.n_seq;
        aux_counts[b] = d.n_aux;
    }
    bp.seq = plan_sort(seq_counts);
    bp.aux = plan_sort(aux_counts);
    bp.tasks.clear();
    bp.task_out_base.clear();
    AsmBlock none{};
    for (int s = 0; s < NSTREAM; s++) none.task[s] = NO_TASK;
    bp.asmb.assign(nbk, none);
    uint64_t payload = 0, fin = 0, segs = 0;
    // coder tasks: every block's SEQ stream first (tasks [0, nbk)), then the AUX
    // streams (tasks [nbk, 9 nbk)), so the two groups can be coded on two streams
    auto add_task = [&](size_t b, int s) {
        const DevBlock& d = blocks[b];
        CoderTask tk{};
        if (s == ST_SEQ) {
            tk.space = 0;
            tk.rec_base = d.seq_sym_base;
            tk.n = d.n_seq;
        } else {
            tk.space = 1;
            tk.rec_base = d.aux_sym_base + d.sbase[s];
            tk.n = d.scount[s];
        }
        tk.nseg = tk.n ? (tk.n + SEG_SYMS - 1) / SEG_SYMS : 1;
        tk.seg_base = segs;
        segs += tk.nseg;
        // each symbol narrows the range by at most 2^16 (tot <= 0xffe0):
        // <= 2 output bytes per symbol, plus the 8-byte flush
        const uint64_t cap = 2ull * tk.n + 64;
        tk.out_cap = (uint32_t)std::min<uint64_t>(cap, 0xffffffffull);
        tk.out_base = payload;
        payload = align_up(payload + tk.out_cap, 16);
        bp.asmb[b].task[s] = (uint32_t)bp.tasks.size();
        bp.tasks.push_back(tk);
        bp.task_out_base.push_back(tk.out_base);
    };
    for (size_t b = 0; b < nbk; b++) {
        DevBlock& d = blocks[b];
        d.seq_sym_base = bp.seq.segs[b].base;
        d.aux_sym_base = bp.aux.segs[b].base;
        add_task(b, ST_SEQ);
    }
    const int nst = atot ? NSTREAM : ST_SEQ + 1;   // (the alignment streams: reference path only)
    for (size_t b = 0; b < nbk; b++)
        for (int s = 0; s < nst; s++)
            if (s != ST_SEQ) add_task(b, s);
    for (size_t b = 0; b < nbk; b++) {
        const DevBlock& d = blocks[b];
        uint64_t blk_out = 64 + 2 + d.name_bytes + (atot ? 96 : 0);   // headers, counts, MD5s, ID-bin first ID
        for (int s = 0; s < NSTREAM; s++)
            if (bp.asmb[b].task[s] != NO_TASK) blk_out += bp.tasks[bp.asmb[b].task[s]].out_cap + 32;
        for (int f = 0; f < 3; f++) bp.asmb[b].md5_task[f] = (uint32_t)(3 * b + f);
        bp.asmb[b].out_base = fin;
        fin = align_up(fin + blk_out, 16);
    }
    bp.total_segs = segs;
    bp.payload_bytes = payload;
    bp.final_bytes = fin;
    return true;
}

}  // namespace sa
