// sa_engine.hip -- host orchestration of the gfx950 block encoder and the C-ABI
// (include/seqarc_amd.h).  Replaces EncapFqzComp::doFqzEncode@0x42d2d0 for a
// batch of blocks: all blocks of a batch are encoded concurrently, every
// stream of every block on its own range-coder lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <optional>
#include <sys/mman.h>
#include <unistd.h>
#include <cerrno>
#include <string>
#include <thread>
#include <vector>

#include "../../include/seqarc_amd.h"
#include "sa_align_host.h"
#include "sa_kernels.hip"
#include "sa_plan.h"

using namespace sa;

namespace {

std::atomic<uint32_t> g_grows{0};   // buffer re-allocations (each hipFree synchronises the device)
std::atomic<uint64_t> g_alloc_ns{0};  // host time in hipMalloc / hipFree (SA_TRACE)
// (sa_set_reserve) a context whose batches grow -- the command line's ramp of
// first batches -- allocates for its full batch from the first one: a
// re-allocation's hipFree would synchronise the device under the other contexts
thread_local double g_reserve_scale = 1.0;

struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap && p) return hipSuccess;
        const auto t0 = std::chrono::steady_clock::now();
        if (p) {
            (void)hipFree(p);
            g_grows++;
        }
        p = nullptr;
        // slack for the next, slightly larger batch: a re-allocation's hipFree
        // synchronises the whole device, stalling every other context on it
        // (the reserve scale gets the same slack on top: a full batch of the
        // command line's ramp can need a little more than scale x a ramp batch,
        // e.g. the exact payload arena, and a grow then stalled every context
        // for 1.5 s, round 3 g3m)
        const size_t scaled = g_reserve_scale > 1.0 ? (size_t)((double)bytes * g_reserve_scale) : bytes;
        size_t want = std::max(scaled + scaled / 16, cap + cap / 16);
        want = std::max<size_t>(want, 256);
        hipError_t e = hipMalloc(&p, want);
        cap = e == hipSuccess ? want : 0;
        g_alloc_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now() - t0).count();
        return e;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct ReserveScope {   // g_reserve_scale for one call on a batch of nbk blocks
    explicit ReserveScope(uint32_t reserve_blocks, uint32_t nbk)
    {
        g_reserve_scale = reserve_blocks > nbk && nbk ? (double)reserve_blocks / nbk : 1.0;
    }
    ~ReserveScope() { g_reserve_scale = 1.0; }
};

// Device time of each phase of the last sa_run, from HIP events on the stream
// the phase runs on.  MD5 runs on its own stream concurrently with the
// others; "total" is the wall time of the whole batch.
const char* kPhaseNames[] = {"prep+scan", "emit", "sort_seq", "sort_aux", "replay_seq", "replay_aux", "coder_r",
                             "coder_l", "md5", "assemble", "total"};
enum { PH_PREP, PH_EMIT, PH_SORT_SEQ, PH_SORT_AUX, PH_REPLAY_SEQ, PH_REPLAY_AUX, PH_CODER_R, PH_CODER_L, PH_MD5,
       PH_ASM, PH_TOTAL, PH_N };

}  // namespace

// The front scratch of a device: buffers only the throughput-bound front of a
// batch uses (count columns, name prefix/suffix, the SEQ sort's key/value ping
// pong, one half of the AUX sort's, histograms, run lists of the front), shared
// by the contexts of one device that are created together (sa_create_shared).
// Their fronts run one at a time -- they are throughput-bound, two at once only
// slow each other -- while each context's latency-bound part (long model runs,
// range-coder chains, MD5) overlaps the next context's front.  `mu` is held
// while a context enqueues its front; its stream first waits for `ev_free`,
// recorded after the previous front's last kernel.
struct FrontShare {
    int refs = 0;
    // the front is taken in arrival order (a ticket lock): std::mutex lets a
    // returning thread barge in, and in the command line's pipeline some
    // contexts waited 2+ s for their turn while others went again (r3b trace)
    std::mutex mu;
    std::condition_variable turn_cv;
    uint64_t next_ticket = 0, serving = 0;
    hipEvent_t ev_free = nullptr;
    bool have_ev = false;
    std::atomic<int> tails{0};   // contexts of the device inside coder_run (pass R in flight)
    DBuf d_seq_k[2], d_seq_v[2], d_auxs_k, d_auxs_v;
    DBuf d_bkt_spare;   // (k_replay_seq_bkt: the inactive lanes' record stores)
    DBuf d_bkt_order;   // (k_bkt_order: the digits, largest first)
    DBuf d_hist_seq, d_hist_aux, d_segs_seq, d_segs_aux, d_tile_seq, d_tile_aux, d_seq_longs, d_nseq_long, d_short_at;
    std::vector<DBuf*> buffers()
    {
        return {&d_seq_k[0], &d_seq_k[1], &d_seq_v[0], &d_seq_v[1], &d_auxs_k, &d_auxs_v, &d_hist_seq, &d_hist_aux,
                &d_segs_seq, &d_segs_aux, &d_tile_seq, &d_tile_aux, &d_seq_longs, &d_nseq_long, &d_short_at,
                &d_bkt_spare, &d_bkt_order};
    }
    uint64_t held_bytes()
    {
        uint64_t h = 0;
        for (DBuf* b : buffers()) h += b->cap;
        return h;
    }
};
std::mutex g_share_mu;   // FrontShare::refs

// RAII turn on a FrontShare's front (FIFO)
struct FrontTurn {
    FrontShare* F = nullptr;
    hipStream_t st = nullptr;   // the stream the holder enqueues its front on
    bool held = false;
    bool freed = false;         // F->ev_free recorded after this front's last kernel
    FrontTurn(FrontShare* f, hipStream_t s) : F(f), st(s)
    {
        std::unique_lock<std::mutex> lk(F->mu);
        const uint64_t t = F->next_ticket++;
        F->turn_cv.wait(lk, [&] { return F->serving == t; });
        held = true;
    }
    void unlock()
    {
        if (!held) return;
        // an early exit (error) after front kernels were queued: the next front
        // must still wait for them before it reuses the shared scratch
        if (!freed && hipEventRecord(F->ev_free, st) == hipSuccess) {
            F->have_ev = true;
            freed = true;
        }
        {
            std::lock_guard<std::mutex> g(F->mu);
            F->serving++;
        }
        F->turn_cv.notify_all();
        held = false;
    }
    ~FrontTurn() { unlock(); }
};

// A batch of parsed blocks resident in HBM (names, bases, qualities and the
// per-read offsets), read-only while it is encoded: any number of contexts of
// its device may encode it, one after the other or concurrently.
struct sa_input {
    int device = 0;
    std::vector<DevBlock> blocks;   // layout fields only (the symbol spaces are per run)
    uint32_t nblocks = 0, nreads = 0;
    uint64_t names_bytes = 0, seq_bytes = 0, text_bytes = 0;
    DBuf d_names, d_seq, d_qual, d_read_block, d_name_off, d_name_len, d_seq_off, d_seq_len;
    std::vector<uint32_t> h_read_block, h_name_off, h_seq_off, h_seq_len;
    std::vector<uint16_t> h_name_len;
    // sa_stage_text: the texts and the device parse's scratch (sa_parse.hip)
    DBuf d_text, d_tile_text, d_tile_cnt, d_tile_base, d_ptexts, d_ntiles, d_text_nl, d_pblocks, d_btot, d_perr, d_nl,
        d_src;
    DBuf d_text_b;   // (round 6) the second text arena of sa_text_upload / sa_text_parse (slot 1)
    ~sa_input()
    {
        for (DBuf* b : {&d_names, &d_seq, &d_qual, &d_read_block, &d_name_off, &d_name_len, &d_seq_off, &d_seq_len,
                        &d_text, &d_tile_text, &d_tile_cnt, &d_tile_base, &d_ptexts, &d_ntiles, &d_text_nl, &d_pblocks,
                        &d_btot, &d_perr, &d_nl, &d_src, &d_text_b})
            b->release();
    }
};

struct sa_ctx {
    const EngineKnobs knobs;   // every SA_* knob read when the context is created (sa_knobs.h)
    explicit sa_ctx(const EngineKnobs& k) : knobs(k), aux_dense(k.aux_dense), timing(k.trace) {}

    int device = 0;
    // main/AUX, MD5, SEQ path (CU-masked), long AUX runs (CU-masked, disjoint);
    // st5: the L passes' own stream (SA_L_CU_EVERY, else null: st3)
    hipStream_t st = nullptr, st2 = nullptr, st3 = nullptr, st4 = nullptr, st5 = nullptr;
    // (round 6) sa_text_upload's copies: a stream of their own, made on first
    // use (from whichever thread uploads), so the next batch's texts go to the
    // device while this context's kernels run
    hipStream_t st_copy = nullptr;
    std::mutex copy_mu;
    std::string upload_err;   // sa_text_upload_dev's error text, under copy_mu (never c->err: sa_run may be running)
    // the dense AUX sort's flag (EngineKnobs::aux_dense to begin with).  The
    // emit's target buffer depends on the number of passes, so the batch follows
    // this context's previous one: a batch with more than 512 models in a block
    // sorts in two dense passes and a copy, and turns it off.
    bool aux_dense;
    DBuf d_aux_bm, d_aux_tab, d_aux_nmod;
    uint32_t* h_aux_nmod = nullptr;   // (pinned)
    size_t h_aux_nmod_cap = 0;
    hipEvent_t ev_r_done = nullptr, ev_dense = nullptr;
    hipEvent_t ev_fork = nullptr, ev_fork_seq = nullptr, ev_md5_done = nullptr;
    hipEvent_t ev_seq_done = nullptr, ev_long_done = nullptr;
    // the AUX record array is all zero between batches (pass R's unwritten-record
    // test): zeroed in the tail of the batch that used it (st3, after the L
    // passes), not in the front turn; prs_zero_cap = its bytes known zero,
    // ev_prs_zero = that tail memset
    hipEvent_t ev_prs_zero = nullptr;
    size_t prs_zero_cap = 0;
    void* prs_zero_p = nullptr;
    bool prs_zero_pending = false;
    bool front_masked = false;   // (SA_RV_CUS: the front's stream on the CUs pass R leaves)
    uint32_t reserve_blocks = 0;   // sa_set_reserve: the batch size to allocate for
    bool front_warm = false;       // a batch ran: its buffers exist (run_input's `early`)
    int rv_batch = 5;   // the current batch's pass-R variant (PathPlan::rv_batch, SA_RV_V6_MAX)
    uint32_t long_grid = 0;   // k_replay_aux_long workgroups (EngineKnobs::long_grid_env)
    std::string err;
    bool timing;
    // pinned host mailbox for the run's small copies (plans, task lists, count
    // and length read-backs): a pageable copy goes through the runtime's
    // staging path, which the other contexts' bulk copies hold up; bump
    // allocation, reset at the start of a run (no copy of the previous run is
    // in flight then); D2H copies land in it and reach their destination at the
    // next sync_d2h
    uint8_t* mail = nullptr;
    size_t mail_cap = 0, mail_used = 0, mail_high = 16u << 20;   // (16 MiB from the first run on)
    std::vector<uint8_t*> mail_retired;   // outgrown mailboxes, freed in the destructor
    struct Pending {
        void* dst;
        const void* src;
        size_t n;
    };
    std::vector<Pending> pending;
    uint32_t n_cu = 256;
    uint32_t coder_restarts = 0;
    uint64_t max_stream_syms = 0, total_stream_syms = 0;
    hipEvent_t ev_beg[PH_N] = {}, ev_end[PH_N] = {};
    float ph_ms[PH_N];
    float align_kernel_ms = 0.f;   // sa_hash_align: the aligner kernel of the last call (variant 0)
    DBuf d_bkt_probe, d_probe;   // SA_BKT_PROBE / SA_RV_PROBE
    uint32_t probe_waves = 0;
    DBuf d_ring;   // pass R's per-wave operand rings (k_coder_rv<6>)

    // the batch sa_stage uploads (sa_run encodes it); blocks = the working copy
    // of the batch being encoded (its symbol spaces filled by plan_batch)
    sa_input own;
    std::vector<DevBlock> blocks;

    // work
    FrontShare* fs = nullptr;   // front scratch, possibly shared with other contexts of the device
    DBuf d_blocks, d_totals, d_err;
    DBuf d_auxp_k, d_auxp_v, d_prs_seq, d_prs_aux, d_cum_seq, d_cum_aux;   // d_auxp: the sorted AUX keys/values
    DBuf d_task_ends;
    DBuf d_tasks, d_out_len, d_payload, d_md5tasks, d_digests, d_asm, d_asm_copies, d_task_out_base, d_final, d_final_len;
    DBuf d_longs, d_huge_sorted, d_nlong;
    DBuf d_ck, d_maps, d_low_at, d_off_at, d_first_sq;
    DBuf d_list_ids[2], d_list_gbase[2], d_list_run[2];
    DBuf d_dege_list;   // the reads with N / IUPAC bases (k_dege_list -> k_emit_sq)
    DBuf d_qual_q, d_rb_chunks, d_rb_ck0, d_rb_opens, d_rb_spec, d_rb_entry, d_rb_guess, d_rb_tab;   // -l (rblock)
    DBuf d_rb_vals, d_rb_info;   // (round 5: run values per chunk byte, RbInfo per chunk)
    std::vector<uint32_t> rb_tab_host;   // the R decision tables (RbTab) of rb_tab_r
    double rb_tab_r = -1.0;
    bool rb_tab_sent = false;
    // reference path: per read the alignment of both carried states, status, the
    // alignment columns, the SEQ skip flags (sa_hash.hip, align_front)
    // per-read counts of every column (k_prep, k_prep_sq16 -> k_scan_reads ->
    // the emitters), name prefix / suffix, the per-block running name maximum,
    // the N / IUPAC maxq: this context's own (the prep runs before its front turn)
    DBuf d_counts, d_name_p, d_name_s, d_maxlen, d_dege_maxq;
    DBuf d_al_ret[2], d_al_rev[2], d_al_pos[2], d_al_mp[2], d_al_mt[2], d_al_st, d_al_sel, d_al_scr, d_acounts, d_atot,
        d_seq_skip;
    // the last aligned batch's block plans (a re-run of the same batch -- the
    // exact-payload fallback -- reuses them instead of passing the chain again)
    const sa_input* al_input = nullptr;
    uint64_t al_batch = 0;
    std::vector<uint32_t> al_plan;   // per block: order count, win, ibits, insert bits

    // last run
    std::vector<uint64_t> final_base, final_len;
    bool have_output = false;
    // what the host chose for the last run (sa_last_paths): report_paths from
    // the plan, the rest where the device's answer is known; paths_r: pass R's
    // first launch of the run is in it
    sa_paths paths{};
    bool paths_r = false;

    std::vector<DBuf*> work_buffers()
    {
        return {&d_blocks, &d_totals, &d_err, &d_auxp_k, &d_auxp_v, &d_prs_seq, &d_prs_aux, &d_cum_seq, &d_cum_aux,
                &d_task_ends, &d_tasks, &d_out_len, &d_payload, &d_md5tasks, &d_digests, &d_asm, &d_asm_copies, &d_task_out_base,
                &d_final, &d_final_len, &d_longs, &d_huge_sorted, &d_nlong, &d_ck, &d_maps, &d_low_at, &d_off_at,
                &d_dege_list, &d_qual_q, &d_rb_chunks, &d_rb_ck0, &d_rb_opens, &d_rb_spec, &d_rb_entry, &d_rb_guess, &d_rb_tab, &d_rb_vals, &d_rb_info, &d_first_sq,
                &d_list_ids[0], &d_list_gbase[0], &d_list_run[0], &d_list_ids[1], &d_list_gbase[1], &d_list_run[1],
                &d_al_ret[0], &d_al_rev[0], &d_al_pos[0], &d_al_mp[0], &d_al_mt[0], &d_al_ret[1], &d_al_rev[1],
                &d_al_pos[1], &d_al_mp[1], &d_al_mt[1], &d_al_st, &d_al_sel, &d_al_scr, &d_acounts, &d_atot,
                &d_seq_skip, &d_counts, &d_name_p, &d_name_s, &d_maxlen, &d_dege_maxq, &d_probe, &d_bkt_probe, &d_ring, &d_aux_bm,
                &d_aux_tab, &d_aux_nmod};
    }
    uint64_t held_bytes()
    {
        uint64_t h = own.d_names.cap + own.d_seq.cap + own.d_qual.cap;
        for (DBuf* b : work_buffers()) h += b->cap;
        return h;   // (the front scratch: front_bytes)
    }
    // every event of the context (created by sa_create, destroyed here); timed: a phase's
    struct Ev {
        hipEvent_t* e;
        bool timed;
    };
    std::vector<Ev> events()
    {
        std::vector<Ev> v;
        for (hipEvent_t* e : {&ev_fork, &ev_fork_seq, &ev_md5_done, &ev_seq_done, &ev_long_done, &ev_prs_zero, &ev_r_done,
                              &ev_dense})
            v.push_back(Ev{e, false});
        for (int i = 0; i < PH_N; i++) {
            v.push_back(Ev{&ev_beg[i], true});
            v.push_back(Ev{&ev_end[i], true});
        }
        return v;
    }

    ~sa_ctx()
    {
        if (fs) {
            std::lock_guard<std::mutex> g(g_share_mu);
            if (--fs->refs == 0) {
                for (DBuf* b : fs->buffers()) b->release();
                if (fs->ev_free) (void)hipEventDestroy(fs->ev_free);
                delete fs;
            }
            fs = nullptr;
        }
        for (DBuf* b : work_buffers()) b->release();
        for (const Ev& ev : events())
            if (*ev.e) (void)hipEventDestroy(*ev.e);
        if (mail) (void)hipHostFree(mail);
        for (uint8_t* m : mail_retired) (void)hipHostFree(m);
        for (hipStream_t s : {st, st2, st3, st4, st5, st_copy})
            if (s) (void)hipStreamDestroy(s);
        if (h_aux_nmod) (void)hipHostFree(h_aux_nmod);
    }
};

#define SA_CHECK(ctx, expr)                                                              \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);              \
            return -1;                                                                   \
        }                                                                                \
    } while (0)

namespace {

// ---- the pinned mailbox (sa_ctx::mail) ----
// Starts a run's use of the mailbox: grows it (to the previous runs' high-water
// mark) while nothing of this context is in flight.
int mail_reset(sa_ctx* c)
{
    c->pending.clear();
    c->mail_used = 0;
    const size_t want = std::max<size_t>(c->mail_high + c->mail_high / 8, 1u << 20);
    if (want > c->mail_cap) {
        // the old one is retired, not freed: hipHostFree waits for the whole
        // device, i.e. for every other context's work in flight
        if (c->mail) c->mail_retired.push_back(c->mail);
        c->mail = nullptr;
        c->mail_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&c->mail), want, hipHostMallocDefault) != hipSuccess) {
            c->mail = nullptr;
            return 0;   // (copies fall back to pageable memory)
        }
        c->mail_cap = want;
    }
    return 0;
}

uint8_t* mail_take(sa_ctx* c, size_t n)
{
    const size_t at = align_up(c->mail_used, 64);
    c->mail_high = std::max(c->mail_high, at + n);
    if (!c->mail || at + n > c->mail_cap) return nullptr;
    c->mail_used = at + n;
    return c->mail + at;
}

// host -> device through the mailbox (the source may be reused at once)
hipError_t h2d(sa_ctx* c, void* dst, const void* src, size_t n, hipStream_t st)
{
    if (!n) return hipSuccess;
    uint8_t* m = mail_take(c, n);
    if (!m) return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st);
    std::memcpy(m, src, n);
    return hipMemcpyAsync(dst, m, n, hipMemcpyHostToDevice, st);
}

// device -> host through the mailbox: `dst` holds the bytes after sync_d2h
hipError_t d2h(sa_ctx* c, void* dst, const void* src, size_t n, hipStream_t st)
{
    if (!n) return hipSuccess;
    uint8_t* m = mail_take(c, n);
    if (!m) return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st);
    c->pending.push_back(sa_ctx::Pending{dst, m, n});
    return hipMemcpyAsync(m, src, n, hipMemcpyDeviceToHost, st);
}

hipError_t sync_d2h(sa_ctx* c, hipStream_t st)
{
    const hipError_t e = hipStreamSynchronize(st);
    for (const sa_ctx::Pending& p : c->pending) std::memcpy(p.dst, p.src, p.n);
    c->pending.clear();
    return e;
}

// sa_knobs.h's copies of the kernels' constants
static_assert(host_k::SORT_MIN_DB == SORT_MIN_DB && host_k::SORT_MAX_DB == SORT_MAX_DB &&
                  host_k::WQ_CHUNK == WQ_CHUNK && host_k::KEY_SLACK == KEY_SLACK &&
                  host_k::AUX_DENSE_BITS == AUX_DENSE_BITS && host_k::SEQ_HALVE_J == SEQ_HALVE_J &&
                  host_k::LONG_RUN == LONG_RUN && host_k::RB_CHUNK == RB_CHUNK &&
                  host_k::RB_CHUNK_DEFAULT == RB_CHUNK_DEFAULT,
              "sa_knobs.h: host_k differs from the kernels' constants");

// ---- the environment: read here and nowhere else (and SA_SYNC in sa_create) ----
const char* env_get(const char* name) { return std::getenv(name); }

int sort_min_db()   // SA_SORT_MIN_DB: once per process
{
    static const int v = parse_sort_min_db(env_get);
    return v;
}

RunKnobs run_knobs() { return parse_run_knobs(env_get, sort_min_db()); }

// grid of a wave-per-read, grid-stride kernel (EMIT_WAVES waves per workgroup):
// 8 workgroups per CU, fewer for a small batch
uint32_t wave_grid(const sa_ctx* c, uint32_t nreads)
{
    return std::max<uint32_t>(1, std::min<uint32_t>((nreads + EMIT_WAVES - 1) / EMIT_WAVES, c->knobs.wg_per_cu * c->n_cu));
}

// sa_plan.h's sort_digits / sort_hist_per_tile with the process's SA_SORT_MIN_DB
std::vector<int> sort_digits(int lo, int hi, int max_db = SORT_MAX_DB)
{
    return sa::sort_digits(lo, hi, max_db, sort_min_db());
}
uint64_t sort_hist_per_tile(int lo, int hi, int max_db = SORT_MAX_DB)
{
    return sa::sort_hist_per_tile(lo, hi, max_db, sort_min_db());
}

template <int DB>
void sort_pass(hipStream_t st, const SortView& sv, const uint32_t* kin, const uint32_t* vin, uint32_t* kout,
               uint32_t* vout, uint32_t shift, bool wide, bool inv = false)
{
    const dim3 hgrid((sv.ntiles + HIST_TILES - 1) / HIST_TILES);
    if (sv.dense)
        hipLaunchKernelGGL((k_sort_hist<DB, true>), hgrid, dim3(SORT_THREADS), 0, st, sv, kin, shift);
    else
        hipLaunchKernelGGL((k_sort_hist<DB, false>), hgrid, dim3(SORT_THREADS), 0, st, sv, kin, shift);
    hipLaunchKernelGGL(k_sort_scan<DB>, dim3(sv.nsegs), dim3(1024), 0, st, sv);
    // (vin = nullptr: the values are the elements' index, IDX)
    auto scatter = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(sv.ntiles), dim3(SORT_THREADS), 0, st, sv, kin, vin, kout, vout, shift); };
    if (wide) {
        if (vin) scatter(k_sort_scatter<DB, true, false, false>);
        else scatter(k_sort_scatter<DB, true, false, true>);
    } else if (sv.dense) {
        if (vin) scatter(k_sort_scatter<DB, false, true, false>);
        else scatter(k_sort_scatter<DB, false, true, true>);
    } else if (inv) {   // (one pass over implicit values: run_sort checks)
        scatter(k_sort_scatter<DB, false, false, true, true>);
    } else {
        if (vin) scatter(k_sort_scatter<DB, false, false, false>);
        else scatter(k_sort_scatter<DB, false, false, true>);
    }
}

// sorts keys by bits [lo, hi) (bits below lo ride along); the result is in
// keys[result_buf] / vals[result_buf]
// index_vals: the input values are each element's index in its segment and are
// not read (the first pass computes them)
// dense: the AUX space by dense model ids (k_aux_dense's tables; bits
// [lo, hi) of the dense id)
int run_sort(sa_ctx* c, hipStream_t st, const SortPlan& plan, DBuf& segs, DBuf& tiles, DBuf& hist,
             DBuf* const* keys, DBuf* const* vals, int lo, int hi, int& result_buf, bool index_vals = false,
             const uint64_t* dense = nullptr, bool inv_vals = false, int max_db = SORT_MAX_DB)
{
    result_buf = 0;
    if (plan.total && hi <= lo && index_vals) {
        c->err = "internal: a sort without passes over implicit values";
        return -1;
    }
    if (plan.total == 0 || hi <= lo) return 0;
    SortView sv{};
    sv.segs = segs.as<SortSeg>();
    sv.tile_seg = tiles.as<uint32_t>();
    sv.hist = hist.as<uint32_t>();
    sv.total = plan.total;
    sv.ntiles = (uint32_t)plan.tile_seg.size();
    sv.nsegs = (uint32_t)plan.segs.size();
    sv.dense = dense;
    // a segment of >= 2^30 keys needs 64-bit offsets in the scatter (the HASH
    // index of a genome > 2^31 bases: one segment of all its seeds)
    bool wide = false;
    for (const SortSeg& g : plan.segs) {
        wide |= (uint64_t)g.ntiles * SORT_TILE >= (1ull << 30);
        if ((uint64_t)g.ntiles * SORT_TILE >= (1ull << 32)) {
            c->err = "sort segment of 2^32 keys or more";
            return -1;
        }
    }
    if (inv_vals && (!index_vals || wide || dense || sort_digits(lo, hi, max_db).size() != 1)) {
        c->err = "internal: an inverse-permutation sort that is not one plain pass over implicit values";
        return -1;
    }
    if (wide && dense) {
        c->err = "internal: a dense sort of a segment of 2^30 keys or more";
        return -1;
    }
    int cur = 0, shift = lo;
    for (const int db : sort_digits(lo, hi, max_db)) {
        const uint32_t* kin = keys[cur]->as<uint32_t>();
        const uint32_t* vin = index_vals && shift == lo ? nullptr : vals[cur]->as<uint32_t>();
        uint32_t* kout = keys[cur ^ 1]->as<uint32_t>();
        uint32_t* vout = vals[cur ^ 1]->as<uint32_t>();
        if (db == 7) sort_pass<7>(st, sv, kin, vin, kout, vout, (uint32_t)shift, wide, inv_vals);
        else if (db == 8) sort_pass<8>(st, sv, kin, vin, kout, vout, (uint32_t)shift, wide, inv_vals);
        else if (db == 9) sort_pass<9>(st, sv, kin, vin, kout, vout, (uint32_t)shift, wide, inv_vals);
        else if (db == 10 && inv_vals) sort_pass<10>(st, sv, kin, vin, kout, vout, (uint32_t)shift, false, true);
        else {
            c->err = "internal: no sort pass of this digit width";
            return -1;
        }
        shift += db;
        cur ^= 1;
    }
    SA_CHECK(c, hipGetLastError());
    result_buf = cur;
    return 0;
}

void ev_begin(sa_ctx* c, int ph, hipStream_t st);
void ev_finish(sa_ctx* c, int ph, hipStream_t st);

// -l R: the R-Block pre-pass (rblock@0x426c10) of every block's qualities into
// d_qual_q, which the QUAL stream then codes (speculative chunks, one carry
// lane per block, chunk replay; sa_logic.h).  The staged qualities stay
// untouched: the N/IUPAC side streams use them, and the batch can be re-run.
int run_rblock(sa_ctx* c, const PathPlan& K, double ratio, uint64_t seq_bytes, BatchView& bv)
{
    hipStream_t st = c->st;
    std::vector<RbChunk> ck;
    std::vector<uint32_t> ck0;
    for (const DevBlock& d : c->blocks) {
        ck0.push_back((uint32_t)ck.size());
        for (uint64_t o = 0; o < d.seq_bytes; o += K.rb_chunk) {
            const uint32_t len = (uint32_t)std::min<uint64_t>(K.rb_chunk, d.seq_bytes - o);
            uint32_t fl = (o == 0 ? RB_FIRST : 0u) | (o + len == d.seq_bytes ? RB_LAST : 0u);
            ck.push_back(RbChunk{d.seq_base + o, len, fl});
        }
    }
    ck0.push_back((uint32_t)ck.size());
    const uint32_t nck = (uint32_t)ck.size(), nbk = (uint32_t)c->blocks.size();
    SA_CHECK(c, c->d_qual_q.ensure(seq_bytes + 64));
    bv.qual_q = c->d_qual_q.as<uint8_t>();
    if (!nck) return 0;
    SA_CHECK(c, c->d_rb_chunks.ensure(sizeof(RbChunk) * nck));
    SA_CHECK(c, c->d_rb_ck0.ensure(4ull * (nbk + 1)));
    SA_CHECK(c, c->d_rb_opens.ensure(4ull * RB_WORDS * nck));
    SA_CHECK(c, c->d_rb_spec.ensure(sizeof(RbRun) * nck));
    SA_CHECK(c, c->d_rb_entry.ensure(sizeof(RbRun) * nck));
    SA_CHECK(c, c->d_rb_guess.ensure(sizeof(RbRun) * nck));
    SA_CHECK(c, h2d(c, c->d_rb_chunks.p, ck.data(), sizeof(RbChunk) * nck, st));
    SA_CHECK(c, h2d(c, c->d_rb_ck0.p, ck0.data(), 4ull * (nbk + 1), st));
    // the decision tables of this R (rebuilt when R changes)
    if (c->rb_tab_r != ratio || c->rb_tab_host.empty()) {
        c->rb_tab_host.assign(2 * RB_TAB_WORDS, 0u);
        rb_tab_build(ratio, c->rb_tab_host.data(), c->rb_tab_host.data() + RB_TAB_WORDS);
        c->rb_tab_r = ratio;
        c->rb_tab_sent = false;
    }
    if (!c->d_rb_tab.p) c->rb_tab_sent = false;
    SA_CHECK(c, c->d_rb_tab.ensure(8ull * RB_TAB_WORDS));
    if (!c->rb_tab_sent) {   // (through the mailbox, once per R)
        SA_CHECK(c, h2d(c, c->d_rb_tab.p, c->rb_tab_host.data(), 8ull * RB_TAB_WORDS, st));
        c->rb_tab_sent = true;
    }
    const uint32_t* tab = c->d_rb_tab.as<uint32_t>();
    const RbChunk* dck = c->d_rb_chunks.as<RbChunk>();
    const uint32_t rgrid = (nck + RB_THREADS - 1) / RB_THREADS;
    const bool walk = K.rb_apply_walk;
    if (!walk) {
        SA_CHECK(c, c->d_rb_vals.ensure((uint64_t)RB_CHUNK * nck));
        SA_CHECK(c, c->d_rb_info.ensure(sizeof(RbInfo) * nck));
    }
    uint8_t* vals = walk ? nullptr : c->d_rb_vals.as<uint8_t>();
    RbInfo* info = walk ? nullptr : c->d_rb_info.as<RbInfo>();
    const uint32_t cs = K.rb_chunk;   // (the arrays' stride per chunk: bytes, opens words * 32)
    // (rb_spec_wg workgroups per CU taking chunks from a counter; 0: one grid)
    uint32_t* wq_spec = K.rb_spec_wg > 0 ? c->d_err.as<uint32_t>() + ERR_WQ_SPEC : nullptr;
    const uint32_t sgrid = wq_spec ? std::max<uint32_t>(1, std::min<uint32_t>(rgrid, K.rb_spec_wg * c->n_cu)) : rgrid;
    hipLaunchKernelGGL(k_rb_spec, dim3(sgrid), dim3(RB_THREADS), 0, st, bv.qual, dck, nck, tab,
                       c->d_rb_opens.as<uint32_t>(), c->d_rb_spec.as<RbRun>(), vals, info, cs, wq_spec);
    hipLaunchKernelGGL(k_rb_guess, dim3(rgrid), dim3(RB_THREADS), 0, st, bv.qual, dck, nck, tab,
                       c->d_rb_opens.as<uint32_t>(), c->d_rb_spec.as<RbRun>(), c->d_rb_guess.as<RbRun>(), cs);
    if (!K.rb_fix_wave)
        hipLaunchKernelGGL(k_rb_fix, dim3((nbk + 63) / 64), dim3(64), 0, st, bv.qual, dck, c->d_rb_ck0.as<uint32_t>(),
                           nbk, tab, c->d_rb_opens.as<uint32_t>(), c->d_rb_spec.as<RbRun>(),
                           c->d_rb_guess.as<RbRun>(), c->d_rb_entry.as<RbRun>(), cs);
    else
        hipLaunchKernelGGL(k_rb_fix_w, dim3(nbk), dim3(64), 0, st, bv.qual, dck, c->d_rb_ck0.as<uint32_t>(), nbk, tab,
                           c->d_rb_opens.as<uint32_t>(), c->d_rb_spec.as<RbRun>(), c->d_rb_guess.as<RbRun>(),
                           c->d_rb_entry.as<RbRun>(), cs);
    if (walk) {
        hipLaunchKernelGGL(k_rb_apply, dim3(rgrid), dim3(RB_THREADS), 0, st, bv.qual, c->d_qual_q.as<uint8_t>(), dck,
                           nck, tab, c->d_rb_entry.as<RbRun>());
    } else {
        hipLaunchKernelGGL(k_rb_true, dim3(rgrid), dim3(RB_THREADS), 0, st, bv.qual, dck, nck, tab,
                           c->d_rb_opens.as<uint32_t>(), vals, info, c->d_rb_entry.as<RbRun>(), cs);
        hipLaunchKernelGGL(k_rb_fill, dim3(nck), dim3(RB_WORDS), 0, st, c->d_qual_q.as<uint8_t>(), dck,
                           c->d_rb_opens.as<uint32_t>(), vals, info, cs);
    }
    SA_CHECK(c, hipGetLastError());
    return 0;
}

int coder_buffers(sa_ctx* c, size_t ntasks, uint64_t total_segs, CoderView& cv)
{
    const uint64_t nsegs = std::max<uint64_t>(total_segs, 1);
    SA_CHECK(c, c->d_ck.ensure(nsegs * 4));
    SA_CHECK(c, c->d_maps.ensure(nsegs * sizeof(LowMap)));
    SA_CHECK(c, c->d_low_at.ensure(nsegs * 8));
    SA_CHECK(c, c->d_off_at.ensure(nsegs * 4));
    SA_CHECK(c, c->d_first_sq.ensure(4 * std::max<size_t>(ntasks, 1)));
    for (int g = 0; g < 2; g++) {
        SA_CHECK(c, c->d_list_ids[g].ensure(4 * std::max<size_t>(ntasks, 1)));
        SA_CHECK(c, c->d_list_gbase[g].ensure(8 * (ntasks + 1)));
        SA_CHECK(c, c->d_list_run[g].ensure(sizeof(CoderRun) * std::max<size_t>(ntasks, 1)));
    }
    cv.ck_r = c->d_ck.as<uint32_t>();
    cv.maps = c->d_maps.as<LowMap>();
    cv.low_at = c->d_low_at.as<uint64_t>();
    cv.off_at = c->d_off_at.as<uint32_t>();
    cv.first_sq = c->d_first_sq.as<uint32_t>();
    return 0;
}

// Uploads the list of one round (tasks ids + start states) into list slot `slot`.
int coder_list(sa_ctx* c, hipStream_t st, int slot, const std::vector<CoderTask>& tasks,
               const std::vector<uint32_t>& ids, const std::vector<CoderRun>& runs, std::vector<uint64_t>& gbase,
               TaskList& tl)
{
    const size_t cnt = ids.size();
    gbase.assign(cnt + 1, 0);
    for (size_t i = 0; i < cnt; i++) gbase[i + 1] = gbase[i] + (tasks[ids[i]].nseg - runs[i].start_seg);
    if (cnt) {
        SA_CHECK(c, h2d(c, c->d_list_ids[slot].p, ids.data(), 4 * cnt, st));
        SA_CHECK(c, h2d(c, c->d_list_gbase[slot].p, gbase.data(), 8 * (cnt + 1), st));
        SA_CHECK(c, h2d(c, c->d_list_run[slot].p, runs.data(), sizeof(CoderRun) * cnt, st));
    }
    tl = TaskList{c->d_list_ids[slot].as<uint32_t>(), c->d_list_gbase[slot].as<uint64_t>(),
                  c->d_list_run[slot].as<CoderRun>(), (uint32_t)cnt, 0u, gbase[cnt]};
    return 0;
}

// pass R: chains of at least RV_LONG_SYMS symbols get a wave each; the others
// share rv_short_waves waves (k_coder_rv; SA_RV_SHORT_WAVES=0: a wave per chain)
constexpr uint32_t RV_LONG_SYMS = 1u << 21;

int coder_launch_r(sa_ctx* c, hipStream_t st, TaskList tl, const CoderView& cv, int ph, uint32_t nlong)
{
    if (!tl.count) return 0;
    const EngineKnobs& K = c->knobs;
    uint32_t waves = tl.count;
    tl.nlong = tl.count;
    if (K.rv_short_waves && nlong + K.rv_short_waves < tl.count) {
        tl.nlong = nlong;
        waves = nlong + K.rv_short_waves;
    }
    if (!c->paths_r) {   // (the run's first pass R; the restarts' lists are short)
        c->paths_r = true;
        c->paths.pass_r = K.rv_lanes ? SA_PATH_R_LANES : c->rv_batch == 6 ? SA_PATH_R_V6 : c->rv_batch == 5 ? SA_PATH_R_V5 : SA_PATH_R_V0;
        c->paths.r_short_shared = tl.nlong != tl.count ? 1u : 0u;
        c->paths.r_waves = K.rv_lanes ? (uint32_t)RL_WAVES : K.coder_waves;
        c->paths.chain_prio = K.chain_prio;
    }
    if (ph >= 0) ev_begin(c, ph, st);
    tl.wait_ticks = K.rv_wait_ticks;
    if (K.rv_lanes) {   // a chain per lane, 64 per workgroup, longest first
        hipLaunchKernelGGL(k_coder_rl, dim3((tl.count + 63) / 64), dim3(64 * RL_WAVES), 0, st, cv.tasks, tl, cv.prs[0],
                           cv.prs[1], cv.ck_r, c->d_err.as<uint32_t>(), K.chain_prio);
        if (ph >= 0) ev_finish(c, ph, st);
        return 0;
    }
    const uint32_t grid = (waves + K.coder_waves - 1) / K.coder_waves;
    uint64_t* probe = nullptr;
    if (K.rv_probe && ph >= 0 && c->d_probe.ensure(32ull * grid * K.coder_waves) == hipSuccess) {
        probe = c->d_probe.as<uint64_t>();
        c->probe_waves = grid * K.coder_waves;
        (void)hipMemsetAsync(probe, 0, 32ull * c->probe_waves, st);
    }
    // (V = 6) a 2 KiB ring per wave, sized for 1024 waves from the start (a
    // re-allocation's hipFree would synchronise the device)
    if (c->rv_batch == 6 &&
        c->d_ring.ensure(4ull * RING_DW * std::max<uint32_t>(1024u, grid * K.coder_waves)) != hipSuccess) {
        c->err = "pass R: cannot allocate the operand ring";
        return -1;
    }
    hipLaunchKernelGGL(c->rv_batch == 6   ? k_coder_rv<6>
                       : c->rv_batch == 5 ? k_coder_rv<5>
                                          : k_coder_rv<0>,
                       dim3(grid), dim3(64 * K.coder_waves), K.coder_lds, st, cv.tasks, tl, cv.prs[0], cv.prs[1],
                       cv.ck_r, c->d_err.as<uint32_t>(), K.chain_prio, probe, c->d_ring.as<uint32_t>());
    if (ph >= 0) ev_finish(c, ph, st);
    return 0;
}

// SA_RV_PROBE: one line per pass-R wave of this batch: context, batch, wave,
// start / end (us on the 100 MHz clock, absolute), shader MHz over the wave,
// XCC, SE, CU, SIMD, wave slot, chains
void write_rv_probe(sa_ctx* c, const std::vector<uint64_t>& p)
{
    static std::mutex mu;
    static uint64_t batch = 0;
    std::lock_guard<std::mutex> g(mu);
    FILE* f = std::fopen(c->knobs.rv_probe, "a");
    if (!f) return;
    const uint64_t b = batch++;
    for (size_t w = 0; w + 3 < p.size(); w += 4) {
        const uint64_t t0 = p[w], t1 = p[w + 1], cyc = p[w + 2], id = p[w + 3];
        if (!t1) continue;
        const uint32_t hw = (uint32_t)id;
        const double us = (double)(t1 - t0) / 100.0;
        std::fprintf(f, "%p %llu %zu %.1f %.1f %.0f xcc %u se %u cu %u simd %u slot %u chains %u sh %u hwid %08x\n",
                     (void*)c, (unsigned long long)b, w / 4, (double)t0 / 100.0, (double)t1 / 100.0,
                     us > 0 ? (double)cyc / us : 0.0, (unsigned)((id >> 32) & 0xff), (hw >> 13) & 7u,
                     (hw >> 8) & 15u, (hw >> 4) & 3u, hw & 15u, (unsigned)(id >> 40), (hw >> 12) & 1u, hw);
    }
    std::fclose(f);
}

// SA_BKT_PROBE: reads the bucket replay's probe back (the front waits for the
// replay: diagnostics) and appends one line per wave: block, digit (its rank
// with k_bkt_order, `ranked`), start / end (us, 100 MHz), cycles, steps, shared
// steps, xcc
int dump_bkt_probe(sa_ctx* c, hipStream_t st, const uint64_t* bprobe, uint32_t bgrid, uint32_t nbk, int db, bool ranked)
{
    std::vector<uint64_t> pr(4ull * bgrid);
    SA_CHECK(c, hipMemcpyAsync(pr.data(), bprobe, 32ull * bgrid, hipMemcpyDeviceToHost, st));
    SA_CHECK(c, hipStreamSynchronize(st));
    FILE* f = std::fopen(c->knobs.bkt_probe, "a");
    if (!f) return 0;
    for (uint32_t w = 0; w < bgrid; w++) {
        const uint64_t* q = &pr[4ull * w];
        if (!q[1]) continue;
        std::fprintf(f, "%u %u %.2f %.2f %llu %llu %llu %llu\n", ranked ? w % nbk : w >> db,
                     ranked ? w / nbk : w & ((1u << db) - 1), (double)q[0] / 100.0, (double)q[1] / 100.0,
                     (unsigned long long)q[2], (unsigned long long)(q[3] & 0xffffff),
                     (unsigned long long)((q[3] >> 24) & 0xffffff), (unsigned long long)(q[3] >> 48));
    }
    std::fclose(f);
    return 0;
}

void coder_launch_l12(sa_ctx* c, hipStream_t st, const TaskList& tl, const CoderView& cv)
{
    if (!tl.count) return;
    const uint32_t lgrid = (uint32_t)((tl.total_segs + 255) / 256);
    hipLaunchKernelGGL(c->knobs.l_chunk == 16 ? k_coder_l1<16> : k_coder_l1<32>, dim3(lgrid), dim3(256), 0, st, cv, tl);
    hipLaunchKernelGGL(k_coder_l2, dim3(tl.count), dim3(L2_THREADS), 0, st, cv, tl);
}

void coder_launch_l3(sa_ctx* c, hipStream_t st, const TaskList& tl, const CoderView& cv)
{
    if (!tl.count) return;
    const uint32_t lgrid = (uint32_t)((tl.total_segs + 255) / 256);
    hipLaunchKernelGGL(c->knobs.l_chunk == 16 ? k_coder_l3<16> : k_coder_l3<32>, dim3(lgrid), dim3(256), 0, st, cv, tl);
}

// Range coder driver (DESIGN.md "Coder"): pass R of every listed chain (on st,
// longest first), then -- once `before_l` (the long model runs) is done -- L1
// and L2.  With `exact`, the payload arena is then sized from the streams'
// real byte counts (k_task_ends; a stream's out_cap gets 1/64 + 4 KiB of slack
// for squeeze restarts) instead of the 2-bytes-per-symbol bound the plan
// carries: tasks' out_base / out_cap, d_tasks and the payload are set here.
// Then L3, and the streams whose exact coding squeezed before their last
// segment restart after that segment from the state L3 computed, until none
// does.  out_len: every stream's bytes.  Returns 0, -1 on error, 2 when a
// stream outgrew its slack (the caller re-runs with exact = false).
int coder_run(sa_ctx* c, std::vector<CoderTask>& tasks, CoderView& cv, hipStream_t st, int ph_r, int ph_l,
              hipEvent_t before_l, bool exact, uint64_t payload_slack, std::vector<uint32_t>& out_len,
              uint64_t& payload_bytes)
{
    out_len.assign(tasks.size(), 0);
    if (tasks.empty()) return 0;
    c->coder_restarts = 0;
    c->paths_r = false;
    c->paths.l_chunk = c->knobs.l_chunk;
    c->paths.l_stream = c->st5 ? 1u : 0u;
    std::vector<uint64_t> gb;
    TaskList tl;
    uint32_t nlong = 0;
    {
        std::vector<uint32_t> ids;
        for (uint32_t t = 0; t < (uint32_t)tasks.size(); t++) ids.push_back(t);
        // longest streams first: a pass-R workgroup's chains are of similar length
        std::stable_sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t b) { return tasks[a].n > tasks[b].n; });
        std::vector<CoderRun> runs(ids.size(), CoderRun{0ull, 0xffffffffu, 0u, 0u, 0u});
        if (coder_list(c, st, 0, tasks, ids, runs, gb, tl)) return -1;
        for (const uint32_t t : ids) nlong += tasks[t].n >= RV_LONG_SYMS ? 1u : 0u;
    }
    if (coder_launch_r(c, st, tl, cv, c->timing ? ph_r : -1, nlong)) return -1;
    if (c->st5) {   // (SA_L_CU_EVERY) the L passes on their own CUs once pass R is done
        SA_CHECK(c, hipEventRecord(c->ev_r_done, st));
        SA_CHECK(c, hipEventSynchronize(c->ev_r_done));
        st = c->st5;
    }
    if (before_l) {
        if (c->knobs.host_waits) SA_CHECK(c, hipEventSynchronize(before_l));   // (see EngineKnobs::host_waits)
        else SA_CHECK(c, hipStreamWaitEvent(st, before_l, 0));
    }
    if (c->timing && ph_l >= 0) ev_begin(c, ph_l, st);
    coder_launch_l12(c, st, tl, cv);
    SA_CHECK(c, hipGetLastError());
    if (exact) {
        SA_CHECK(c, c->d_task_ends.ensure(4 * tasks.size()));
        hipLaunchKernelGGL(k_task_ends, dim3((tl.count + 255) / 256), dim3(256), 0, st, cv, tl,
                           c->d_task_ends.as<uint32_t>());
        std::vector<uint32_t> ends(tasks.size());
        uint32_t perr[4] = {0, 0, 0, 0};
        SA_CHECK(c, d2h(c, ends.data(), c->d_task_ends.p, 4 * tasks.size(), st));
        SA_CHECK(c, d2h(c, perr, c->d_err.p, 16, st));
        std::vector<uint64_t> probe;
        if (c->knobs.rv_probe && c->probe_waves) {
            probe.resize(4ull * c->probe_waves);
            SA_CHECK(c, d2h(c, probe.data(), c->d_probe.p, 32ull * c->probe_waves, st));
        }
        SA_CHECK(c, sync_d2h(c, st));
        if (!probe.empty()) write_rv_probe(c, probe);
        if (perr[0] & E_CODER) {   // (pass R gave up on unwritten records: L3 is not run on them)
            c->err = "range coder: pass R timed out waiting for model records (E_CODER)";
            return -1;
        }
        uint64_t payload = 0;
        for (size_t t = 0; t < tasks.size(); t++) {
            const uint64_t cap = (uint64_t)ends[t] + ends[t] / 64 + payload_slack;
            tasks[t].out_cap = (uint32_t)std::min<uint64_t>(cap, tasks[t].out_cap);
            tasks[t].out_base = payload;
            payload = align_up(payload + tasks[t].out_cap, 16);
        }
        payload_bytes = payload;
        SA_CHECK(c, c->d_payload.ensure(std::max<uint64_t>(payload, 16)));
        cv.out = c->d_payload.as<uint8_t>();
        SA_CHECK(c, h2d(c, c->d_tasks.p, tasks.data(), sizeof(CoderTask) * tasks.size(), st));
    }
    coder_launch_l3(c, st, tl, cv);
    if (c->timing && ph_l >= 0) ev_finish(c, ph_l, st);
    SA_CHECK(c, hipGetLastError());
    std::vector<uint32_t> first_sq(tasks.size());
    for (int round = 0;; round++) {
        SA_CHECK(c, d2h(c, first_sq.data(), cv.first_sq, 4 * tasks.size(), st));
        SA_CHECK(c, d2h(c, out_len.data(), cv.out_len, 4 * tasks.size(), st));
        SA_CHECK(c, sync_d2h(c, st));
        std::vector<uint32_t> ids;
        for (size_t t = 0; t < tasks.size(); t++) {
            const uint32_t k = first_sq[t];
            if (k != 0xffffffffu && k + 1 < tasks[t].nseg) ids.push_back((uint32_t)t);
        }
        if (ids.empty()) break;
        // the exact end state L3 left at each restarted stream's squeezed
        // segment: all copies queued on st, one wait
        std::vector<LowMap> endst(ids.size());
        std::vector<uint32_t> off(ids.size());
        for (size_t i = 0; i < ids.size(); i++) {
            const uint64_t sg = tasks[ids[i]].seg_base + first_sq[ids[i]];
            SA_CHECK(c, d2h(c, &endst[i], cv.maps + sg, sizeof(LowMap), st));
            SA_CHECK(c, d2h(c, &off[i], cv.off_at + sg, 4, st));
        }
        SA_CHECK(c, hipMemsetAsync(cv.first_sq, 0xff, 4 * tasks.size(), st));
        SA_CHECK(c, sync_d2h(c, st));
        std::vector<CoderRun> runs;
        for (size_t i = 0; i < ids.size(); i++)
            runs.push_back(CoderRun{endst[i].B, endst[i].s, first_sq[ids[i]] + 1, off[i] + endst[i].nbytes, 0u});
        if (round > 1000) {
            c->err = "range coder: too many restarts";
            return -1;
        }
        c->coder_restarts += (uint32_t)ids.size();
        if (coder_list(c, st, 0, tasks, ids, runs, gb, tl)) return -1;
        if (coder_launch_r(c, st, tl, cv, -1, 0)) return -1;
        coder_launch_l12(c, st, tl, cv);
        coder_launch_l3(c, st, tl, cv);
        SA_CHECK(c, hipGetLastError());
    }
    for (size_t t = 0; t < tasks.size(); t++)
        if (out_len[t] > tasks[t].out_cap) {
            if (exact) return 2;
            c->err = "range coder output overflowed its buffer";
            return -1;
        }
    return 0;
}

void ev_begin(sa_ctx* c, int ph, hipStream_t st)
{
    if (c->timing) (void)hipEventRecord(c->ev_beg[ph], st);
}
void ev_finish(sa_ctx* c, int ph, hipStream_t st)
{
    if (c->timing) (void)hipEventRecord(c->ev_end[ph], st);
}

}  // namespace

extern "C" {

const char* sa_version(void) { return "seqarc_amd 0.1 (gfx950)"; }

sa_ctx* sa_create(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "seqarc_amd: device %d is %s, this library is built for gfx950 only\n", device,
                     prop.gcnArchName);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    // SA_SYNC=block: host waits sleep instead of spinning (the command line sets
    // it: five encoder threads spinning on their streams took the CPU share the
    // reader needs); only effective before the device's first use in the process
    if (const char* e = std::getenv("SA_SYNC")) {
        if (!std::strcmp(e, "block")) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
        else if (!std::strcmp(e, "spin")) (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
        (void)hipGetLastError();   // (hipErrorSetOnActiveProcess when the device is in use already)
    }
    std::unique_ptr<sa_ctx> c(new sa_ctx(parse_knobs(env_get)));   // (a failed create: the destructor cleans up)
    const EngineKnobs& K = c->knobs;
    if (K.coder_lds > 64 * 1024)   // pass R's unused LDS (k_coder_rv): above what a launch gets by default
        for (const void* f : {reinterpret_cast<const void*>(&k_coder_rv<0>), reinterpret_cast<const void*>(&k_coder_rv<5>),
                              reinterpret_cast<const void*>(&k_coder_rv<6>)})
            if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)K.coder_lds) != hipSuccess) {
                std::fprintf(stderr, "seqarc_amd: cannot reserve %u B of LDS for pass R\n", K.coder_lds);
                return nullptr;
            }
    c->device = device;
    c->n_cu = (uint32_t)prop.multiProcessorCount;
    // st carries the critical path (AUX symbols -> QUAL coder chain).  While the
    // long AUX model runs replay (latency-bound, st4: every 4th CU), the SEQ path
    // (throughput, st3: the other CUs) runs beside them without sharing a SIMD.
    const int ncu = prop.multiProcessorCount, every = K.long_cu_every;
    std::vector<uint32_t> m_long((ncu + 31) / 32, 0u), m_seq(m_long.size(), 0u);
    for (int cu = 0; cu < ncu; cu++)
        ((cu % every) == 0 || every == 1 ? m_long : m_seq)[cu / 32] |= 1u << (cu % 32);
    if (every == 1) m_seq = m_long;   // (st3: the coder chains; st4: the long model runs)
    std::vector<uint32_t> m_front;   // (see EngineKnobs::rv_cus)
    if (every == 4 && K.rv_cus >= 1 && K.rv_cus <= 5) {
        m_front.assign(m_long.size(), 0u);
        std::fill(m_seq.begin(), m_seq.end(), 0u);
        static const int order[6] = {1, 5, 2, 6, 3, 7};   // (the non-long CUs of each 8, spread)
        for (int cu = 0; cu < ncu; cu++) {
            bool r = false;
            for (int k = 0; k < K.rv_cus; k++) r |= (cu % 8) == order[k];
            (r ? m_seq : m_front)[cu / 32] |= 1u << (cu % 32);
        }
    }
    uint32_t ncu_long = 0;
    for (uint32_t w : m_long) ncu_long += (uint32_t)__builtin_popcount(w);
    c->long_grid = K.long_grid_env ? K.long_grid_env : std::max(1u, 6u * ncu_long);
    c->front_masked = !m_front.empty();
    auto masked = [](hipStream_t* s, const std::vector<uint32_t>& m) {   // (no mask: all CUs)
        return m.empty() ? hipStreamCreateWithFlags(s, hipStreamNonBlocking)
                         : hipExtStreamCreateWithCUMask(s, (uint32_t)m.size(), m.data());
    };
    if (masked(&c->st, m_front) != hipSuccess || masked(&c->st2, m_long) != hipSuccess ||
        masked(&c->st3, m_seq) != hipSuccess || masked(&c->st4, m_long) != hipSuccess)
        return nullptr;
    if (K.l_cu_every == 1) {   // (A/B, round 6) the L passes on the front's CUs (all of them without SA_RV_CUS)
        if (masked(&c->st5, m_front) != hipSuccess) return nullptr;
    } else if (K.l_cu_every >= 2) {
        std::vector<uint32_t> m_l(m_long.size(), 0u);
        for (int cu = 0; cu < ncu; cu++)   // (offset: not the long runs' CUs when n = 4)
            if (cu % K.l_cu_every == K.l_cu_every / 2) m_l[cu / 32] |= 1u << (cu % 32);
        if (masked(&c->st5, m_l) != hipSuccess) return nullptr;
    }
    for (const sa_ctx::Ev& ev : c->events()) {
        if (ev.e == &c->ev_r_done && !c->st5) continue;   // (only the L passes' own stream waits for it)
        if ((ev.timed ? hipEventCreate(ev.e) : hipEventCreateWithFlags(ev.e, hipEventDisableTiming)) != hipSuccess)
            return nullptr;
    }
    c->fs = new FrontShare();
    c->fs->refs = 1;
    if (hipEventCreateWithFlags(&c->fs->ev_free, hipEventDisableTiming) != hipSuccess) return nullptr;
    return c.release();
}

sa_ctx* sa_create_shared(int device, sa_ctx* peer)
{
    if (!peer || peer->device != device) return nullptr;
    sa_ctx* c = sa_create(device);
    if (!c) return nullptr;
    std::lock_guard<std::mutex> g(g_share_mu);
    FrontShare* own = c->fs;
    c->fs = peer->fs;
    c->fs->refs++;
    for (DBuf* b : own->buffers()) b->release();
    if (own->ev_free) (void)hipEventDestroy(own->ev_free);
    delete own;
    return c;
}

uint64_t sa_front_bytes(const sa_ctx* c) { return c && c->fs ? c->fs->held_bytes() : 0; }

void sa_destroy(sa_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    delete ctx;
}

const char* sa_last_error(const sa_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

void sa_set_timing(sa_ctx* ctx, int on)
{
    if (ctx) ctx->timing = on != 0;
}

int sa_host_register(void* p, uint64_t bytes)
{
    if (!p || !bytes) return -1;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? 0 : -1;
}

int sa_host_unregister(void* p)
{
    if (!p) return -1;
    return hipHostUnregister(p) == hipSuccess ? 0 : -1;
}

uint64_t sa_output_bound(const sa_block* b)
{
    uint64_t nb = 0, nn = 0;
    for (uint32_t r = 0; r < b->nreads; r++) {
        nb += (uint64_t)(b->seq_lens[r] > 0 ? b->seq_lens[r] : 0);
        nn += b->name_lens[r];
    }
    // coded symbols per stream: len <= 5 per read, names <= 3 per read + the
    // name bytes, quals <= bases + 1 per read, tip / max-qual 1 per read, N/IUPAC
    // chars <= bases, exception counts <= 33 per read (kModel), gaps <= bases
    // (1 + bits(g) symbols per g + 1 bases), bases; each symbol narrows the
    // range by < 2^16 (<= 2 bytes); + per stream flush and header, the MD5s and
    // the ID-bin first ID
    // (+ 140 per read: the reference path's alignment symbols, <= 64 position
    // bits, <= 63 x 17 mismatch bits and types at maxmis 7 ...)
    const uint64_t syms = 3 * nb + nn + (45ull + 140ull) * b->nreads;
    return 2 * syms + 9 * 96 + 4096 + 0x10000;
}

}  // extern "C"

namespace {

// Uploads a batch of parsed blocks into `in` (its buffers grow as needed) on
// stream st and waits for the copies.  Returns 0 or -1 with err set.
int input_upload(sa_input* I, const sa_block* in, int n, hipStream_t st, std::string& err)
{
#define IN_CHECK(expr)                                                                   \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return -1;                                                                   \
        }                                                                                \
    } while (0)
    if (n < 0 || (n > 0 && !in)) {
        err = "invalid block list";
        return -1;
    }
    I->nblocks = (uint32_t)n;
    I->blocks.assign((size_t)n, DevBlock{});
    uint64_t nb = 0, sb = 0, tb = 0;
    uint32_t nr = 0;
    for (int b = 0; b < n; b++) {
        DevBlock& d = I->blocks[(size_t)b];
        d.nreads = in[b].nreads;
        d.read0 = nr;
        uint64_t ln = 0, ls = 0;
        for (uint32_t r = 0; r < in[b].nreads; r++) {
            if (in[b].seq_lens[r] < 0) {
                err = "negative read length";
                return -1;
            }
            ln += in[b].name_lens[r];
            ls += (uint64_t)in[b].seq_lens[r];
            if (in[b].seq_lens[r] > 0xffff) d.len_long = 1;   // getBlockRead@0x411d2a
        }
        if (ls >= (1ull << 30) || ln >= (1ull << 32)) {
            err = "block too large (a reference block is 50 MiB of FASTQ)";
            return -1;
        }
        if ((uint64_t)nr + in[b].nreads >= (1ull << 31)) {
            err = "too many reads in one batch";
            return -1;
        }
        d.name_base = nb;
        d.seq_base = sb;
        d.name_bytes = ln;
        d.seq_bytes = ls;
        nb = align_up(nb + ln, 16);
        sb = align_up(sb + ls, 16);
        tb += ln + 2 * ls;
        nr += in[b].nreads;
    }
    I->nreads = nr;
    I->names_bytes = nb;
    I->seq_bytes = sb;
    I->text_bytes = tb;
    I->h_read_block.resize(nr);
    I->h_name_off.resize(nr);
    I->h_name_len.resize(nr);
    I->h_seq_off.resize(nr);
    I->h_seq_len.resize(nr);
    for (int b = 0; b < n; b++) {
        const DevBlock& d = I->blocks[(size_t)b];
        uint32_t no = 0, so = 0;
        for (uint32_t r = 0; r < d.nreads; r++) {
            const uint32_t g = d.read0 + r;
            I->h_read_block[g] = (uint32_t)b;
            I->h_name_off[g] = no;
            I->h_name_len[g] = in[b].name_lens[r];
            I->h_seq_off[g] = so;
            I->h_seq_len[g] = (uint32_t)in[b].seq_lens[r];
            no += in[b].name_lens[r];
            so += (uint32_t)in[b].seq_lens[r];
        }
    }
    IN_CHECK(I->d_names.ensure(nb + 64));   // (k_prep_sq16 reads whole dwords past a name)
    IN_CHECK(I->d_seq.ensure(sb + 64));   // (k_prep_sq16 reads whole dwords past a read)
    IN_CHECK(I->d_qual.ensure(sb + 64));
    const size_t nr4 = (size_t)std::max<uint32_t>(nr, 1) * 4;
    IN_CHECK(I->d_read_block.ensure(nr4));
    IN_CHECK(I->d_name_off.ensure(nr4));
    IN_CHECK(I->d_name_len.ensure(nr4));
    IN_CHECK(I->d_seq_off.ensure(nr4));
    IN_CHECK(I->d_seq_len.ensure(nr4));
    for (int b = 0; b < n; b++) {
        const DevBlock& d = I->blocks[(size_t)b];
        if (d.name_bytes)
            IN_CHECK(hipMemcpyAsync(I->d_names.as<uint8_t>() + d.name_base, in[b].names, d.name_bytes,
                                    hipMemcpyHostToDevice, st));
        if (d.seq_bytes) {
            IN_CHECK(hipMemcpyAsync(I->d_seq.as<uint8_t>() + d.seq_base, in[b].seq, d.seq_bytes,
                                    hipMemcpyHostToDevice, st));
            IN_CHECK(hipMemcpyAsync(I->d_qual.as<uint8_t>() + d.seq_base, in[b].qual, d.seq_bytes,
                                    hipMemcpyHostToDevice, st));
        }
    }
    if (nr) {
        IN_CHECK(hipMemcpyAsync(I->d_read_block.p, I->h_read_block.data(), nr * 4ull, hipMemcpyHostToDevice, st));
        IN_CHECK(hipMemcpyAsync(I->d_name_off.p, I->h_name_off.data(), nr * 4ull, hipMemcpyHostToDevice, st));
        IN_CHECK(hipMemcpyAsync(I->d_name_len.p, I->h_name_len.data(), nr * 2ull, hipMemcpyHostToDevice, st));
        IN_CHECK(hipMemcpyAsync(I->d_seq_off.p, I->h_seq_off.data(), nr * 4ull, hipMemcpyHostToDevice, st));
        IN_CHECK(hipMemcpyAsync(I->d_seq_len.p, I->h_seq_len.data(), nr * 4ull, hipMemcpyHostToDevice, st));
    }
    IN_CHECK(hipStreamSynchronize(st));
#undef IN_CHECK
    return 0;
}

}  // namespace

extern "C" {

void sa_alloc_stats(uint32_t* grows, double* alloc_ms)
{
    if (grows) *grows = g_grows.load();
    if (alloc_ms) *alloc_ms = g_alloc_ns.load() / 1e6;
}

void sa_set_reserve(sa_ctx* c, uint32_t blocks)
{
    if (c) c->reserve_blocks = blocks;
}

int sa_stage(sa_ctx* c, const sa_block* in, int n)
{
    const ReserveScope reserve(c ? c->reserve_blocks : 0, n > 0 ? (uint32_t)n : 0);
    if (!c) return -1;
    SA_CHECK(c, hipSetDevice(c->device));
    c->have_output = false;
    return input_upload(&c->own, in, n, c->st, c->err);
}

sa_input* sa_input_create(int device, const sa_block* in, int n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
    sa_input* I = new sa_input();
    I->device = device;
    std::string err;
    const int rc = input_upload(I, in, n, st, err);
    (void)hipStreamDestroy(st);
    if (rc) {
        std::fprintf(stderr, "seqarc_amd: sa_input_create: %s\n", err.c_str());
        delete I;
        return nullptr;
    }
    return I;
}

void sa_input_destroy(sa_input* in)
{
    if (!in) return;
    (void)hipSetDevice(in->device);
    delete in;
}

int sa_run(sa_ctx* c, const sa_cfg* cfg)
{
    if (!c) return -1;
    return sa_run_input(c, &c->own, cfg);
}

}  // extern "C"

// The reference (HASH index) path of a batch: doAlignEncode@0x42d4c0 instead of
// doFqzEncode@0x42d2d0 (sa_run_input_aligned).
struct AlignReq {
    const sa_hash_index* ix;
    sa_align_cfg cfg;
    sa_align_chain* chain;
    uint64_t batch;   // the batch's place in the chain (UINT64_MAX: the chain's next)
};
// sa_hash.hip: aligns the batch, follows the carried state through it (after
// the chain's previous batch), plans its blocks (c->blocks: order count, insert
// window), counts and scans the alignment columns (atot: per block NACOL sums)
// and sets the BatchView / AlignView fields of the path
int align_front(sa_ctx* c, const sa_input* I, BatchView& bv, const AlignReq& rq, std::vector<uint32_t>& atot,
                AlignView& av);
void align_chain_fail(sa_align_chain* ch);

namespace {

// One batch on its way through run_input's stages: what they share.  The
// stages return 0, -1 (c->err set), or 2 from the coder (see run_input).
struct Batch {
    const sa_input* I;
    const sa_cfg* cfg;
    const AlignReq* al;   // the reference path (nullptr: no reference)
    bool exact;
    RunKnobs rk;
    PathPlan pp;          // decided before the first launch (plan_paths)
    TotalsPlan tp{};      // ... and once the count scan's totals are back (plan_totals)
    uint32_t nbk = 0, nr = 0;
    bool early = false;   // the context's first batch: the turn is taken after its own allocations
    bool trace = false;   // SA_ALN_TRACE on the reference path
    // the turn on the device's front scratch: RAII, so a stage that returns
    // early inside the turn releases it
    std::optional<FrontTurn> turn;
    BatchView bv{};
    AlignView alv{};
    std::vector<uint32_t> aln_tot;
    std::vector<uint32_t> tot;   // per block the NCOL column sums (k_scan_reads)
    BatchPlan bp;                // (its tasks' out_base / out_cap: the coder's when exact)
    uint64_t payload = 0;
    CoderView cv{};
    // the sorts' ping-pong tables and where their results are
    DBuf *skb[2] = {}, *svb[2] = {}, *akb[2] = {}, *avb[2] = {};
    int seq_sorted = 0, aux_sorted = 0;
    SortView svs{}, sva{};
    std::vector<uint32_t> out_len;
};

// the words of d_err work is taken from (nullptr: the kernel's static path)
uint32_t* err_word(sa_ctx* c, uint32_t word, bool on) { return on ? c->d_err.as<uint32_t>() + word : nullptr; }

// ---- checks, the plan, BatchView, the reference path, the turn (a warm
//      context), the MD5 fork ----
int batch_begin(sa_ctx* c, Batch& B)
{
    const sa_input* I = B.I;
    const sa_cfg* cfg = B.cfg;
    SA_CHECK(c, hipSetDevice(c->device));
    c->have_output = false;
    c->paths = sa_paths{};
    c->paths.aux_dense_next = c->aux_dense ? 1u : 0u;
    if (mail_reset(c)) return -1;
    c->blocks = I->blocks;
    const uint32_t nbk = B.nbk = I->nblocks, nr = B.nr = I->nreads;
    if (nbk == 0) {
        c->final_base.clear();
        c->final_len.clear();
        c->have_output = true;
        return 0;
    }
    if (cfg->slevel < 0 || cfg->slevel > 9 || cfg->qlevel < 0 || cfg->qlevel > 3) {
        c->err = "unsupported slevel/qlevel";
        return -1;
    }
    const bool lossy = cfg->lossy > 0.0;   // -l R: param+0x1870 / +0x1878
    B.rk = run_knobs();
    B.pp = plan_paths(c->knobs, B.rk, PathCfg{cfg->slevel, cfg->qlevel, lossy, cfg->md5 != 0},
                      BatchShape{nr, I->seq_bytes, nbk, B.al != nullptr, c->aux_dense});
    c->rv_batch = B.pp.rv_batch;
    hipStream_t st = c->st;
    FrontShare* F = c->fs;

    SA_CHECK(c, c->d_blocks.ensure(sizeof(DevBlock) * nbk));
    SA_CHECK(c, h2d(c, c->d_blocks.p, c->blocks.data(), sizeof(DevBlock) * nbk, st));
    BatchView& bv = B.bv;
    bv.blocks = c->d_blocks.as<DevBlock>();
    bv.nblocks = nbk;
    bv.nreads_total = nr;
    bv.read_block = I->d_read_block.as<uint32_t>();
    bv.names = I->d_names.as<uint8_t>();
    bv.seq = I->d_seq.as<uint8_t>();
    bv.qual = I->d_qual.as<uint8_t>();
    bv.qual_q = bv.qual;
    bv.lossy = lossy ? 1 : 0;
    bv.name_off = I->d_name_off.as<uint32_t>();
    bv.name_len = I->d_name_len.as<uint16_t>();
    bv.seq_off = I->d_seq_off.as<uint32_t>();
    bv.seq_len = I->d_seq_len.as<uint32_t>();
    bv.seq_mask = B.pp.ns - 1;
    bv.qlevel = cfg->qlevel;
    bv.bin_mode = cfg->bin_mode ? 1 : 0;
    bv.md5 = cfg->md5 ? 1 : 0;
    // reference path: the reads are aligned (and the batch placed in the
    // align_info chain) before the front is taken: the chain may wait for
    // the batch before this one, which another context runs
    if (B.al && align_front(c, I, bv, *B.al, B.aln_tot, B.alv)) {
        align_chain_fail(B.al->chain);
        return -1;
    }
    B.trace = B.al && B.rk.aln_trace;
    // the front (prep up to the short model runs) holds the device's front
    // scratch.  (The prep before the turn, overlapping another context's
    // front, measured slower: 12.6 vs 13.9 GB/s, round 3 g3i -- the front
    // kernels are throughput-bound together.)  A context's first batch is the
    // exception: its prep touches no front scratch, and its own buffers (~34
    // GB for a 69-block batch) are allocated from the plan -- hipMalloc of
    // tens of GB takes ~0.3 s, which inside the turn held up every other
    // context (the command line's first batches: 1.4 s of allocations in
    // series, round 4 r4c).  So the first batch preps, plans and allocates
    // first, then takes its turn (batch_plan_and_buffers).
    B.early = !c->front_warm;
    if (!B.early) B.turn.emplace(F, st);
    if (B.trace && !B.early) fprintf(stderr, "[align] front turn taken\n");
    SA_CHECK(c, c->d_counts.ensure((size_t)std::max<uint32_t>(nr, 1) * NCOL * 4));
    SA_CHECK(c, c->d_dege_maxq.ensure((size_t)std::max<uint32_t>(nr, 1)));
    SA_CHECK(c, c->d_totals.ensure((size_t)nbk * NCOL * 4));
    SA_CHECK(c, c->d_name_p.ensure((size_t)std::max<uint32_t>(nr, 1) * 2));
    SA_CHECK(c, c->d_name_s.ensure((size_t)std::max<uint32_t>(nr, 1) * 2));
    SA_CHECK(c, c->d_maxlen.ensure((size_t)std::max<uint32_t>(nr, 1) * 2));
    SA_CHECK(c, c->d_err.ensure(ERR_BYTES));   // (its words: sa_device.h)
    SA_CHECK(c, hipMemsetAsync(c->d_err.p, 0, ERR_BYTES, st));

    ev_begin(c, PH_TOTAL, st);
    // ---- MD5 of every block's IDs/bases/quals (calcBlockMd5@0x414d90) on st2,
    //      concurrent with everything up to the assembly ----
    std::vector<Md5Task> md5t;
    for (uint32_t b = 0; b < nbk; b++) {
        const DevBlock& d = c->blocks[b];
        md5t.push_back(Md5Task{I->d_names.as<uint8_t>() + d.name_base, d.name_bytes});
        md5t.push_back(Md5Task{I->d_seq.as<uint8_t>() + d.seq_base, d.seq_bytes});
        md5t.push_back(Md5Task{I->d_qual.as<uint8_t>() + d.seq_base, d.seq_bytes});
    }
    if (B.pp.md5) {
        // the task table, then (k_md5_lanes) the tasks' order: longest first,
        // 64 consecutive ones to a chain wave (sa_md5_lanes.h)
        const uint32_t nt = (uint32_t)md5t.size();
        const size_t task_bytes = sizeof(Md5Task) * md5t.size();
        std::vector<uint8_t> up(task_bytes + (B.pp.md5 == 1 ? 4 * md5t.size() : 0));
        memcpy(up.data(), md5t.data(), task_bytes);
        if (B.pp.md5 == 1) {
            const std::vector<uint32_t> order = md5l::lane_order(nt, [&](uint32_t i) { return md5t[i].len; });
            memcpy(up.data() + task_bytes, order.data(), 4 * order.size());
        }
        SA_CHECK(c, c->d_md5tasks.ensure(up.size()));
        SA_CHECK(c, c->d_digests.ensure(16 * md5t.size()));
        SA_CHECK(c, hipEventRecord(c->ev_fork, st));
        SA_CHECK(c, hipStreamWaitEvent(c->st2, c->ev_fork, 0));
        SA_CHECK(c, h2d(c, c->d_md5tasks.p, up.data(), up.size(), c->st2));
        ev_begin(c, PH_MD5, c->st2);
        if (B.pp.md5 == 1)
            hipLaunchKernelGGL(k_md5_lanes, dim3(md5l::wave_count(nt)), dim3(128), 0, c->st2, c->d_md5tasks.as<Md5Task>(),
                               reinterpret_cast<const uint32_t*>(c->d_md5tasks.as<uint8_t>() + task_bytes), nt,
                               c->d_digests.as<uint32_t>(), c->knobs.md5_prio);
        else
            hipLaunchKernelGGL(B.pp.md5 == 2 ? k_md5<true> : k_md5<false>, dim3(nt), dim3(128), 0, c->st2,
                               c->d_md5tasks.as<Md5Task>(), nt, c->d_digests.as<uint32_t>(), c->knobs.md5_prio);
        ev_finish(c, PH_MD5, c->st2);
        SA_CHECK(c, hipGetLastError());
        SA_CHECK(c, hipEventRecord(c->ev_md5_done, c->st2));
    } else {
        SA_CHECK(c, c->d_digests.ensure(16 * md5t.size()));
    }
    if (!B.early && F->have_ev) SA_CHECK(c, hipStreamWaitEvent(st, F->ev_free, 0));   // the previous front is done with it
    return 0;
}

// ---- prep, scan, the totals and the error word back ----
int front_prep(sa_ctx* c, Batch& B)
{
    const PathPlan& p = B.pp;
    hipStream_t st = c->st;
    const uint32_t nr = B.nr;
    const BatchView& bv = B.bv;
    uint32_t* d_err = c->d_err.as<uint32_t>();
    uint32_t* counts = c->d_counts.as<uint32_t>();
    uint32_t* wq_prep = err_word(c, ERR_WQ_PREP, p.front_counter);
    ev_begin(c, PH_PREP, st);
    if (bv.lossy && run_rblock(c, p, B.cfg->lossy, B.I->seq_bytes, B.bv)) return -1;
    // k_prep (names, lengths: lane per read -- a grid-stride variant with 8
    // workgroups per CU measured slower: k_prep 1.2 -> 1.7 ms, k_emit 6.8 -> 9.4)
    // and k_prep_sq16 (SEQ / QUAL / N-IUPAC columns: a row per read).
    // SA_PREP_FUSED=1: k_prep_sq16 takes the name columns too (row-parallel
    // prefix / suffix) -- measured no faster under load (prep 38 vs 32 ms, same
    // GB/s, round 3 g3r / g3s); SA_PREP_WAVE=1: round 2's wave-per-read k_prep_sq
    if (p.prep && p.prep != SA_PATH_PREP_FUSED)
        hipLaunchKernelGGL(k_prep, dim3((nr + 255) / 256), dim3(256), 0, st, bv, counts, c->d_name_p.as<int16_t>(),
                           c->d_name_s.as<int16_t>(), d_err);
    switch (p.prep) {
    case SA_PATH_PREP_FUSED:
        hipLaunchKernelGGL(wq_prep ? k_prep_sq16<true> : k_prep_sq16<false>, dim3(wave_grid(c, (nr + 3) / 4)),
                           dim3(256), 0, st, bv, counts, d_err, c->d_dege_maxq.as<uint8_t>(),
                           c->d_name_p.as<int16_t>(), c->d_name_s.as<int16_t>(), wq_prep, p.wqc);
        break;
    case SA_PATH_PREP_WAVE:
        hipLaunchKernelGGL(k_prep_sq, dim3(wave_grid(c, nr)), dim3(64 * EMIT_WAVES), 0, st, bv, counts, d_err);
        break;
    case SA_PATH_PREP_ROW64:
        hipLaunchKernelGGL((wq_prep ? k_prep_sq16<true, 64> : k_prep_sq16<false, 64>), dim3(wave_grid(c, nr)),
                           dim3(256), 0, st, bv, counts, d_err, c->d_dege_maxq.as<uint8_t>(), nullptr, nullptr,
                           wq_prep, p.wqc);
        break;
    case SA_PATH_PREP_ROW16:
        hipLaunchKernelGGL(wq_prep ? k_prep_sq16<true> : k_prep_sq16<false>, dim3(wave_grid(c, (nr + 3) / 4)),
                           dim3(256), 0, st, bv, counts, d_err, c->d_dege_maxq.as<uint8_t>(), nullptr, nullptr,
                           wq_prep, p.wqc);
        break;
    default: break;   // (a batch without reads)
    }
    hipLaunchKernelGGL(k_scan_reads, dim3(B.nbk), dim3(1024), 0, st, bv, counts, c->d_totals.as<uint32_t>(),
                       c->d_maxlen.as<uint16_t>());
    SA_CHECK(c, hipGetLastError());
    ev_finish(c, PH_PREP, st);
    B.tot.assign((size_t)B.nbk * NCOL, 0);
    uint32_t herr[ERR_WORDS];
    SA_CHECK(c, d2h(c, B.tot.data(), c->d_totals.p, B.tot.size() * 4, st));
    SA_CHECK(c, d2h(c, herr, c->d_err.p, 4 * ERR_WORDS, st));
    SA_CHECK(c, sync_d2h(c, st));
    if (herr[0]) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "input rejected (error bits 0x%x)", herr[0]);
        c->err = buf;
        return -1;
    }
    return 0;
}

// ---- layout of the symbol spaces, coder tasks, md5 tasks, outputs; the
//      context's own buffers; then (inside the turn) the shared front scratch ----
int batch_plan_and_buffers(sa_ctx* c, Batch& B)
{
    hipStream_t st = c->st;
    FrontShare* F = c->fs;
    const uint32_t nbk = B.nbk;
    BatchPlan& bp = B.bp;
    if (!plan_batch(c->blocks, B.tot, bp, B.al ? &B.aln_tot : nullptr, B.alv.mis_model)) {
        c->err = "block symbol space too large";
        return -1;
    }
    const SortPlan& ps = bp.seq;
    const SortPlan& pa = bp.aux;
    const std::vector<CoderTask>& tasks = bp.tasks;
    c->max_stream_syms = c->total_stream_syms = 0;
    for (const CoderTask& tk : tasks) {
        c->max_stream_syms = std::max<uint64_t>(c->max_stream_syms, tk.n);
        c->total_stream_syms += tk.n;
    }
    uint64_t n_ch = 0;   // N / IUPAC bases in the batch
    for (uint32_t b = 0; b < nbk; b++) n_ch += B.tot[(size_t)b * NCOL + C_CH];
    const TotalsPlan& t = B.tp = plan_totals(c->knobs, B.rk, B.pp, BatchShape{B.nr, B.I->seq_bytes, nbk, B.al != nullptr, c->aux_dense},
                                             ps.total, pa.total, n_ch);
    report_paths(c->paths, c->knobs, B.pp, t, ps.total, pa.total, c->front_masked, c->long_grid);
    B.payload = bp.payload_bytes;

    // this context's own buffers
    SA_CHECK(c, c->d_auxp_k.ensure(t.atot * 4));
    SA_CHECK(c, c->d_auxp_v.ensure(t.atot * 4));
    SA_CHECK(c, c->d_prs_seq.ensure(t.stot * sizeof(PRec)));
    SA_CHECK(c, c->d_prs_aux.ensure(t.atot * sizeof(PRec)));
    SA_CHECK(c, c->d_cum_aux.ensure(t.atot * 2));
    SA_CHECK(c, c->d_longs.ensure(t.max_long * sizeof(LongRun)));
    SA_CHECK(c, c->d_huge_sorted.ensure((pa.total / HUGE_RUN + 1) * sizeof(LongRun)));
    SA_CHECK(c, c->d_nlong.ensure(16));   // RunLists counters: short, huge, long, queue
    SA_CHECK(c, c->d_tasks.ensure(sizeof(CoderTask) * tasks.size()));
    SA_CHECK(c, c->d_out_len.ensure(4 * tasks.size()));
    if (!B.exact) SA_CHECK(c, c->d_payload.ensure(std::max<uint64_t>(B.payload, 16)));
    SA_CHECK(c, c->d_asm.ensure(sizeof(AsmBlock) * nbk));
    SA_CHECK(c, c->d_asm_copies.ensure(4ull * ASM_COPY_WORDS * nbk));
    SA_CHECK(c, c->d_task_out_base.ensure(8 * tasks.size()));
    SA_CHECK(c, c->d_final_len.ensure(8 * nbk));
    if (coder_buffers(c, tasks.size(), bp.total_segs, B.cv)) return -1;
    if (B.early) {   // (see batch_begin): now the turn, and the previous front's end on the device
        B.turn.emplace(F, st);
        if (B.trace) fprintf(stderr, "[align] front turn taken\n");
        if (F->have_ev) SA_CHECK(c, hipStreamWaitEvent(st, F->ev_free, 0));
    }
    // the device's front scratch (shared by its contexts: inside the turn)
    for (int i = 0; i < 2; i++) {
        SA_CHECK(c, F->d_seq_k[i].ensure(t.stot * 4));
        SA_CHECK(c, F->d_seq_v[i].ensure(t.stot * 4));
    }
    SA_CHECK(c, F->d_auxs_k.ensure(t.atot * 4));
    SA_CHECK(c, F->d_auxs_v.ensure(t.atot * 4));
    // AUX sort ping-pong: the sorted keys/values must land in this context's
    // buffers (the long model runs read them after the front scratch is released)
    const bool odd = t.aux_passes % 2;
    B.akb[0] = odd ? &F->d_auxs_k : &c->d_auxp_k;
    B.akb[1] = odd ? &c->d_auxp_k : &F->d_auxs_k;
    B.avb[0] = odd ? &F->d_auxs_v : &c->d_auxp_v;
    B.avb[1] = odd ? &c->d_auxp_v : &F->d_auxs_v;
    for (int i = 0; i < 2; i++) {
        B.skb[i] = &F->d_seq_k[i];
        B.svb[i] = &F->d_seq_v[i];
    }
    SA_CHECK(c, F->d_seq_longs.ensure(t.max_seq_long * 8));
    SA_CHECK(c, F->d_nseq_long.ensure(4));
    SA_CHECK(c, F->d_short_at.ensure(t.max_short * 8));
    SA_CHECK(c, F->d_hist_seq.ensure(std::max<uint64_t>(ps.tile_seg.size(), 1) * 4 * t.seq_hist_per_tile));
    SA_CHECK(c, F->d_hist_aux.ensure(std::max<uint64_t>(pa.tile_seg.size(), 1) * 4 * t.aux_hist_per_tile));
    SA_CHECK(c, F->d_segs_seq.ensure(sizeof(SortSeg) * nbk));
    SA_CHECK(c, F->d_segs_aux.ensure(sizeof(SortSeg) * nbk));
    SA_CHECK(c, F->d_tile_seq.ensure(std::max<size_t>(ps.tile_seg.size(), 1) * 4));
    SA_CHECK(c, F->d_tile_aux.ensure(std::max<size_t>(pa.tile_seg.size(), 1) * 4));

    SA_CHECK(c, h2d(c, c->d_blocks.p, c->blocks.data(), sizeof(DevBlock) * nbk, st));
    SA_CHECK(c, h2d(c, F->d_segs_seq.p, ps.segs.data(), sizeof(SortSeg) * nbk, st));
    SA_CHECK(c, h2d(c, F->d_segs_aux.p, pa.segs.data(), sizeof(SortSeg) * nbk, st));
    if (!ps.tile_seg.empty())
        SA_CHECK(c, h2d(c, F->d_tile_seq.p, ps.tile_seg.data(), ps.tile_seg.size() * 4, st));
    if (!pa.tile_seg.empty())
        SA_CHECK(c, h2d(c, F->d_tile_aux.p, pa.tile_seg.data(), pa.tile_seg.size() * 4, st));
    SA_CHECK(c, h2d(c, c->d_tasks.p, tasks.data(), sizeof(CoderTask) * tasks.size(), st));

    CoderView& cv = B.cv;
    cv.tasks = c->d_tasks.as<CoderTask>();
    cv.prs[0] = c->d_prs_seq.as<PRec>();
    cv.prs[1] = c->d_prs_aux.as<PRec>();
    cv.cum[0] = nullptr;   // packed SEQ records
    cv.cum[1] = c->d_cum_aux.as<uint16_t>();
    cv.out = c->d_payload.as<uint8_t>();
    cv.out_len = c->d_out_len.as<uint32_t>();
    cv.lprio = c->knobs.l_prio;
    B.svs = SortView{F->d_segs_seq.as<SortSeg>(), F->d_tile_seq.as<uint32_t>(), F->d_hist_seq.as<uint32_t>(),
                     ps.total, (uint32_t)ps.tile_seg.size(), nbk};
    B.sva = SortView{F->d_segs_aux.as<SortSeg>(), F->d_tile_aux.as<uint32_t>(), F->d_hist_aux.as<uint32_t>(),
                     pa.total, (uint32_t)pa.tile_seg.size(), nbk};
    return 0;
}

// ---- emit (main stream), the dense AUX sort's presence pass, the AUX record
//      array made zero ----
int front_emit(sa_ctx* c, Batch& B)
{
    const PathPlan& p = B.pp;
    hipStream_t st = c->st;
    FrontShare* F = c->fs;
    const uint32_t nbk = B.nbk, nr = B.nr, rgrid = (nr + 255) / 256;
    const BatchView& bv = B.bv;
    const SortPlan& ps = B.bp.seq;
    const SortPlan& pa = B.bp.aux;
    uint32_t* d_err = c->d_err.as<uint32_t>();
    uint32_t* counts = c->d_counts.as<uint32_t>();
    uint32_t* totals = c->d_totals.as<uint32_t>();
    uint32_t* seq_k = F->d_seq_k[0].as<uint32_t>();
    uint32_t* seq_v = F->d_seq_v[0].as<uint32_t>();
    uint32_t* aux_k = B.akb[0]->as<uint32_t>();   // (AUX values: the index, run_sort)
    uint8_t* dege_maxq = p.dege_maxq ? c->d_dege_maxq.as<uint8_t>() : nullptr;   // (k_prep_sq: k_emit's serial path)
    uint32_t* wq_emit = err_word(c, ERR_WQ_EMIT, p.front_counter);
    ev_begin(c, PH_EMIT, st);
    {
        const SortView pv_s{F->d_segs_seq.as<SortSeg>(), nullptr, nullptr, ps.total, 0u, nbk};
        const SortView pv_a{F->d_segs_aux.as<SortSeg>(), nullptr, nullptr, pa.total, 0u, nbk};
        const uint32_t pgrid = (uint32_t)(((uint64_t)(nbk + 1) * SORT_TILE + 255) / 256);
        hipLaunchKernelGGL(k_pad_keys, dim3(pgrid), dim3(256), 0, st, pv_s, seq_k, F->d_seq_k[1].as<uint32_t>());
        hipLaunchKernelGGL(k_pad_keys, dim3(pgrid), dim3(256), 0, st, pv_a, aux_k, B.akb[1]->as<uint32_t>());
    }
    SA_CHECK(c, hipMemsetAsync(c->d_first_sq.p, 0xff, 4 * B.bp.tasks.size(), st));
    if (p.emit)
        hipLaunchKernelGGL(k_emit, dim3(rgrid), dim3(256), 0, st, bv, counts, totals, c->d_name_p.as<int16_t>(),
                           c->d_name_s.as<int16_t>(), c->d_maxlen.as<uint16_t>(), seq_k, seq_v, aux_k, nullptr, d_err,
                           dege_maxq);
    if (p.emit == SA_PATH_EMIT_WAVE) {   // (SA_EMIT_WAVE=1: round 2's wave-per-read SEQ / QUAL, for A/B)
        hipLaunchKernelGGL(k_emit_sq, dim3(wave_grid(c, nr)), dim3(64 * EMIT_WAVES), 0, st, bv, counts, seq_k, seq_v,
                           aux_k, nullptr, totals, dege_maxq, p.seq_sh,
                           (uint32_t)(EMIT_SEQ | EMIT_QUAL | EMIT_DEGE), nullptr, nullptr);
    } else if (p.emit == SA_PATH_EMIT_ROW16) {
        hipLaunchKernelGGL(p.seq_sh ? (wq_emit ? k_emit_sq16<2, true> : k_emit_sq16<2, false>)
                                    : (wq_emit ? k_emit_sq16<0, true> : k_emit_sq16<0, false>),
                           dim3(wave_grid(c, (nr + 3) / 4)), dim3(256), 0, st, bv, counts, seq_k, seq_v, aux_k, nullptr,
                           wq_emit, p.wqc);
        if (B.tp.dege_list) {   // the N / IUPAC side streams of the reads that have such bases
            SA_CHECK(c, c->d_dege_list.ensure(4ull * ((uint64_t)nr + 1)));
            SA_CHECK(c, hipMemsetAsync(c->d_dege_list.p, 0, 4, st));
            hipLaunchKernelGGL(k_dege_list, dim3(std::max<uint32_t>(1, std::min<uint32_t>((nr + 255) / 256, c->n_cu * 4))),
                               dim3(256), 0, st, bv, counts, totals, c->d_dege_list.as<uint32_t>());
            hipLaunchKernelGGL(k_emit_sq, dim3(wave_grid(c, nr)), dim3(64 * EMIT_WAVES), 0, st, bv, counts, seq_k, seq_v,
                               aux_k, nullptr, totals, dege_maxq, p.seq_sh, (uint32_t)EMIT_DEGE,
                               c->d_dege_list.as<uint32_t>(), err_word(c, ERR_WQ_DEGE, p.dege_counter));
        }
    }
    if (p.emit && B.al)   // the alignment streams (AlignInfoProcess[PE], decomposeAlignInfo)
        hipLaunchKernelGGL(k_align_emit, dim3(rgrid), dim3(256), 0, st, bv, B.alv, c->d_acounts.as<uint32_t>(), aux_k);
    SA_CHECK(c, hipGetLastError());
    ev_finish(c, PH_EMIT, st);
    if (B.tp.dense) {   // the blocks' model bitmaps and rank tables; the model counts to the host
        SA_CHECK(c, c->d_aux_bm.ensure(4ull * AUX_DENSE_WORDS * nbk));
        SA_CHECK(c, c->d_aux_tab.ensure(8ull * AUX_DENSE_WORDS * nbk));
        SA_CHECK(c, c->d_aux_nmod.ensure(4ull * nbk));
        if (c->h_aux_nmod_cap < nbk) {
            if (c->h_aux_nmod) SA_CHECK(c, hipHostFree(c->h_aux_nmod));
            c->h_aux_nmod = nullptr;
            c->h_aux_nmod_cap = 0;
            SA_CHECK(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_aux_nmod), 4ull * nbk * 2, 0));
            c->h_aux_nmod_cap = 2ull * nbk;
        }
        SA_CHECK(c, hipMemsetAsync(c->d_aux_bm.p, 0, 4ull * AUX_DENSE_WORDS * nbk, st));
        hipLaunchKernelGGL(k_aux_presence, dim3((uint32_t)((pa.tile_seg.size() + PRESENCE_TILES - 1) / PRESENCE_TILES)),
                           dim3(SORT_THREADS), 0, st, B.sva, aux_k, c->d_aux_bm.as<uint32_t>());
        hipLaunchKernelGGL(k_aux_dense, dim3(nbk), dim3(256), 0, st, c->d_aux_bm.as<uint32_t>(),
                           c->d_aux_tab.as<uint64_t>(), c->d_aux_nmod.as<uint32_t>());
        SA_CHECK(c, hipGetLastError());
        SA_CHECK(c, hipMemcpyAsync(c->h_aux_nmod, c->d_aux_nmod.p, 4ull * nbk, hipMemcpyDeviceToHost, st));
        SA_CHECK(c, hipEventRecord(c->ev_dense, st));
    }
    if (c->prs_zero_p != c->d_prs_aux.p || c->prs_zero_cap < B.tp.atot * sizeof(PRec)) {
        // (a new buffer, or the last batch did not end normally: zeroed here, all of it)
        SA_CHECK(c, hipMemsetAsync(c->d_prs_aux.p, 0, c->d_prs_aux.cap, st));
    } else if (c->prs_zero_pending) {   // (the previous batch's tail memset: long done by now)
        SA_CHECK(c, hipStreamWaitEvent(st, c->ev_prs_zero, 0));
    }
    c->prs_zero_p = c->d_prs_aux.p;
    c->prs_zero_cap = 0;   // (until this batch's tail zeroes what it wrote)
    c->prs_zero_pending = false;
    return 0;
}

// ---- throughput phases on st (each fills the GPU): the SEQ sort and the
//      BASE_MODEL replay ----
int seq_sort_replay(sa_ctx* c, Batch& B)
{
    const PathPlan& p = B.pp;
    hipStream_t st = c->st;
    FrontShare* F = c->fs;
    const uint32_t nbk = B.nbk;
    const SortPlan& ps = B.bp.seq;
    const SymSink sink_seq{c->d_prs_seq.as<PRec>(), nullptr};   // packed
    ev_begin(c, PH_SORT_SEQ, st);
    if (run_sort(c, st, ps, F->d_segs_seq, F->d_tile_seq, F->d_hist_seq, B.skb, B.svb, p.seq_lo, p.seq_hi, B.seq_sorted,
                 p.seq_sh != 0, nullptr, p.seq_inv, p.seq_max_db))
        return -1;
    ev_finish(c, PH_SORT_SEQ, st);
    ev_begin(c, PH_REPLAY_SEQ, st);
    const uint32_t* sk = F->d_seq_k[B.seq_sorted].as<uint32_t>();
    uint32_t* sv = F->d_seq_v[B.seq_sorted].as<uint32_t>();
    if (ps.total && p.seq_bkt) {
        if (p.seq_dg.size() != 1) {
            c->err = "internal: the SEQ bucket sort is not one pass";
            return -1;
        }
        const uint32_t db = (uint32_t)p.seq_dg[0], sb = (uint32_t)p.bkt.sb, bgrid = nbk << db;
        const size_t lds = (size_t)5 * ((1u << sb) + 64);
        SA_CHECK(c, F->d_bkt_spare.ensure(256ull * bgrid));
        PRec* spare = F->d_bkt_spare.as<PRec>();
        const uint32_t* border = nullptr;
        if (p.bkt_lpt) {
            SA_CHECK(c, F->d_bkt_order.ensure(4ull << db));
            hipLaunchKernelGGL(k_bkt_order, dim3(1), dim3(1u << db), 0, st, B.svs, 1u << db, F->d_bkt_order.as<uint32_t>());
            border = F->d_bkt_order.as<uint32_t>();
        }
        uint64_t* bprobe = nullptr;
        if (c->knobs.bkt_probe) {
            SA_CHECK(c, c->d_bkt_probe.ensure(32ull * bgrid));
            SA_CHECK(c, hipMemsetAsync(c->d_bkt_probe.p, 0, 32ull * bgrid, st));
            bprobe = c->d_bkt_probe.as<uint64_t>();
        }
        if (p.seq_inv) {
            // records in sorted order into the other value buffer (the bucket
            // pass over implicit values never read it), then gathered through
            // the inverse permutation the pass left in d_seq_v[sorted]
            PRec* rs = F->d_seq_v[B.seq_sorted ^ 1].as<PRec>();
            hipLaunchKernelGGL(k_replay_seq_bkt<true>, dim3(bgrid), dim3(64), lds, st, B.svs, sk, nullptr,
                               SymSink{rs, nullptr}, db, sb, p.seq_sh + db, spare, bprobe, border);
            hipLaunchKernelGGL(k_seq_unpermute, dim3(8 * (uint32_t)((ps.tile_seg.size() + 7) / 8)),
                               dim3(SORT_THREADS), 0, st, B.svs, sv, rs, c->d_prs_seq.as<PRec>());
        } else {
            hipLaunchKernelGGL(k_replay_seq_bkt<false>, dim3(bgrid), dim3(64), lds, st, B.svs, sk, sv, sink_seq, db, sb,
                               p.seq_sh + db, spare, bprobe, border);
        }
        if (bprobe && dump_bkt_probe(c, st, bprobe, bgrid, nbk, (int)db, border != nullptr)) return -1;
    } else if (ps.total) {
        SA_CHECK(c, hipMemsetAsync(F->d_nseq_long.p, 0, 4, st));
        hipLaunchKernelGGL(k_replay_seq, dim3((uint32_t)ps.tile_seg.size()), dim3(SORT_THREADS), 0, st, B.svs, sk, sv,
                           sink_seq, F->d_seq_longs.as<uint64_t>(), F->d_nseq_long.as<uint32_t>(), p.seq_sh);
        hipLaunchKernelGGL(k_replay_seq_long, dim3((uint32_t)std::min<uint64_t>(B.tp.max_seq_long, 2048)), dim3(128), 0,
                           st, B.svs, sk, sv, sink_seq, F->d_seq_longs.as<uint64_t>(), F->d_nseq_long.as<uint32_t>(),
                           c->d_err.as<uint32_t>(), p.seq_sh);
    }
    SA_CHECK(c, hipGetLastError());
    ev_finish(c, PH_REPLAY_SEQ, st);
    return 0;
}

// ---- the AUX sort, the run lists and the short SIMPLE_MODEL runs on st; the
//      front is released; then the long SIMPLE_MODEL runs (latency-bound, st4:
//      CU set B), beside which pass R of every coder chain starts (coder_tail) ----
int aux_sort_runs(sa_ctx* c, Batch& B)
{
    const PathPlan& p = B.pp;
    const TotalsPlan& t = B.tp;
    hipStream_t st = c->st;
    FrontShare* F = c->fs;
    const uint32_t nbk = B.nbk;
    const SortPlan& pa = B.bp.aux;
    uint32_t* d_err = c->d_err.as<uint32_t>();
    const SymSink sink_aux{c->d_prs_aux.as<PRec>(), c->d_cum_aux.as<uint16_t>()};
    ev_begin(c, PH_SORT_AUX, st);
    bool runs_from_hist = false;   // one dense pass: the run lists from the scan (k_runs_dense)
    if (t.dense) {
        // (the counts were read back right after the emit: the SEQ sort and
        // replay queued above keep the device busy while the host waits here)
        SA_CHECK(c, hipEventSynchronize(c->ev_dense));
        uint32_t dmax = 0;
        for (uint32_t b = 0; b < nbk; b++) dmax = std::max(dmax, c->h_aux_nmod[b]);
        const DensePlan dp = plan_dense(dmax, B.rk);
        runs_from_hist = dp.runs_from_hist;
        c->paths.aux_nmod_max = dmax;
        c->paths.aux_sort = SA_PATH_AUX_DENSE1;
        c->paths.aux_digits = pack_digits(sort_digits(0, dp.dbits));
        c->paths.aux_runs = runs_from_hist ? SA_PATH_RUNS_DENSE : SA_PATH_RUNS_FIND;
        if (run_sort(c, st, pa, F->d_segs_aux, F->d_tile_aux, F->d_hist_aux, B.akb, B.avb, 0, dp.dbits, B.aux_sorted, true,
                     c->d_aux_tab.as<uint64_t>()))
            return -1;
        if (B.aux_sorted != 1) {   // (two dense passes: the result is in the front scratch)
            SA_CHECK(c, hipMemcpyAsync(c->d_auxp_k.p, F->d_auxs_k.p, t.atot * 4, hipMemcpyDeviceToDevice, st));
            SA_CHECK(c, hipMemcpyAsync(c->d_auxp_v.p, F->d_auxs_v.p, t.atot * 4, hipMemcpyDeviceToDevice, st));
            B.aux_sorted = 1;
            c->aux_dense = false;   // (this input has too many models per block for one pass)
            c->paths.aux_sort = SA_PATH_AUX_DENSE2_COPY;
        }
    } else if (run_sort(c, st, pa, F->d_segs_aux, F->d_tile_aux, F->d_hist_aux, B.akb, B.avb, AUX_SYM_BITS,
                        AUX_SYM_BITS + p.aux_bits, B.aux_sorted, true)) {
        return -1;
    }
    c->paths.aux_dense_next = c->aux_dense ? 1u : 0u;
    ev_finish(c, PH_SORT_AUX, st);
    ev_begin(c, PH_REPLAY_AUX, st);
    if (pa.total && B.akb[B.aux_sorted] != &c->d_auxp_k) {
        c->err = "internal: sorted AUX keys not in the context's buffer";
        return -1;
    }
    const uint32_t* ak = B.akb[B.aux_sorted]->as<uint32_t>();   // the sorted AUX keys / values
    const uint32_t* av = B.avb[B.aux_sorted]->as<uint32_t>();
    uint32_t* ctr = c->d_nlong.as<uint32_t>();
    const RunLists rl{F->d_short_at.as<uint64_t>(), ctr, c->d_longs.as<LongRun>(), ctr + 1, ctr + 2, t.max_long, ctr + 3,
                      c->d_huge_sorted.as<LongRun>()};
    SA_CHECK(c, hipMemsetAsync(ctr, 0, 16, st));
    if (pa.total) {
        if (runs_from_hist)
            hipLaunchKernelGGL(k_runs_dense<9>, dim3((nbk * 512u + 255) / 256), dim3(256), 0, st, B.sva, ak, rl);
        else
            hipLaunchKernelGGL(k_find_runs, dim3((uint32_t)((pa.total / FIND_ITEMS + 255) / 256)), dim3(256), 0, st,
                               B.sva, ak, rl);
        hipLaunchKernelGGL(k_sort_huge, dim3(1), dim3(1024), 0, st, rl);
        hipLaunchKernelGGL(k_replay_aux_short, dim3(SHORT_GRID), dim3(RP_THREADS), 0, st, B.sva, ak, av, sink_aux, rl,
                           d_err);
    }
    SA_CHECK(c, hipGetLastError());
    SA_CHECK(c, hipEventRecord(c->ev_fork_seq, st));
    // the front scratch is free once the kernels enqueued so far on st are done
    SA_CHECK(c, hipEventRecord(F->ev_free, st));
    F->have_ev = true;
    B.turn->freed = true;
    B.turn->unlock();
    if (c->knobs.host_waits) SA_CHECK(c, hipEventSynchronize(c->ev_fork_seq));
    else SA_CHECK(c, hipStreamWaitEvent(c->st4, c->ev_fork_seq, 0));
    if (pa.total && !p.skip_long)
        hipLaunchKernelGGL(k_replay_aux_long, dim3(c->long_grid), dim3(128), c->knobs.long_lds, c->st4, rl, ak, av, sink_aux,
                           d_err, c->knobs.chain_prio);
    SA_CHECK(c, hipGetLastError());
    SA_CHECK(c, hipEventRecord(c->ev_long_done, c->st4));
    ev_finish(c, PH_REPLAY_AUX, c->st4);
    return 0;
}

// ---- range coders: every chain in one launch on st3, longest first
//      (concurrent latency-bound launches land on shared SIMDs): pass R waits
//      per segment for records the long runs have not written yet (k_coder_r),
//      the L passes run after the long runs are done; then the AUX records
//      this batch wrote back to zero ----
int coder_tail(sa_ctx* c, Batch& B)
{
    FrontShare* F = c->fs;
    hipStream_t st3 = c->st3;
    if (!c->knobs.host_waits) SA_CHECK(c, hipStreamWaitEvent(st3, c->ev_fork_seq, 0));
    // (SA_RV_V6_MAX, see EngineKnobs::rv_v6_max) the SMEM-fed chain only when
    // few other contexts' chains are in flight
    if (c->knobs.rv_variant < 0 && c->rv_batch == 6 && F->tails.load() > c->knobs.rv_v6_max) c->rv_batch = 5;
    F->tails++;
    const int rc = coder_run(c, B.bp.tasks, B.cv, st3, PH_CODER_R, PH_CODER_L, c->ev_long_done, B.exact,
                             B.rk.payload_slack, B.out_len, B.payload);
    F->tails--;
    if (rc) return rc;
    // (in the batch's tail, after the L passes on st3)
    SA_CHECK(c, hipMemsetAsync(c->d_prs_aux.p, 0, B.tp.atot * sizeof(PRec), st3));
    SA_CHECK(c, hipEventRecord(c->ev_prs_zero, st3));
    c->prs_zero_cap = c->d_prs_aux.cap;
    c->prs_zero_pending = true;
    return 0;
}

// ---- the final arena from the streams' real sizes, the assembly (after MD5),
//      the lengths and the error word back ----
int assemble_and_finish(sa_ctx* c, Batch& B)
{
    hipStream_t st = c->st;
    const uint32_t nbk = B.nbk;
    const std::vector<CoderTask>& tasks = B.bp.tasks;
    std::vector<AsmBlock>& asmb = B.bp.asmb;
    // per block its encaps (<= 32 header bytes each), count / MD5s, and the ID-bin first ID
    uint64_t final_bytes = 0;
    std::vector<uint64_t> task_out_base(tasks.size());
    for (size_t t = 0; t < tasks.size(); t++) task_out_base[t] = tasks[t].out_base;
    c->final_base.assign(nbk, 0);
    for (uint32_t b = 0; b < nbk; b++) {
        uint64_t blk = 64 + 2 + 0x10000 + 96;
        for (int s = 0; s < NSTREAM; s++)
            if (asmb[b].task[s] != NO_TASK) blk += B.out_len[asmb[b].task[s]] + 32;
        asmb[b].out_base = final_bytes;
        c->final_base[b] = final_bytes;
        final_bytes = align_up(final_bytes + blk, 16);
    }
    SA_CHECK(c, c->d_final.ensure(std::max<uint64_t>(final_bytes, 16)));
    SA_CHECK(c, h2d(c, c->d_asm.p, asmb.data(), sizeof(AsmBlock) * nbk, st));
    SA_CHECK(c, h2d(c, c->d_task_out_base.p, task_out_base.data(), 8 * tasks.size(), st));

    if (B.pp.md5) SA_CHECK(c, hipStreamWaitEvent(st, c->ev_md5_done, 0));
    ev_begin(c, PH_ASM, st);
    AsmView asv{c->d_asm.as<AsmBlock>(), c->d_task_out_base.as<uint64_t>(), c->d_asm_copies.as<uint32_t>()};
    hipLaunchKernelGGL(k_assemble, dim3((nbk + 63) / 64), dim3(64), 0, st, B.bv, asv, c->d_out_len.as<uint32_t>(),
                       c->d_digests.as<uint32_t>(), c->d_final.as<uint8_t>(), c->d_final_len.as<uint64_t>());
    hipLaunchKernelGGL(k_assemble_copy, dim3(nbk * ASM_SLICES), dim3(256), 0, st, asv, c->d_payload.as<uint8_t>(),
                       c->d_final.as<uint8_t>());
    SA_CHECK(c, hipGetLastError());
    ev_finish(c, PH_ASM, st);
    ev_finish(c, PH_TOTAL, st);

    c->final_len.assign(nbk, 0);
    uint32_t herr[ERR_WORDS];
    SA_CHECK(c, d2h(c, c->final_len.data(), c->d_final_len.p, 8ull * nbk, st));
    SA_CHECK(c, d2h(c, herr, c->d_err.p, 4 * ERR_WORDS, st));
    SA_CHECK(c, sync_d2h(c, st));
    if (herr[0]) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "device error bits 0x%x", herr[0]);
        c->err = buf;
        return -1;
    }
    if (c->timing) {
        for (int i = 0; i < PH_N; i++) {
            c->ph_ms[i] = 0.f;
            if (i == PH_MD5 && !B.pp.md5) continue;
            (void)hipEventElapsedTime(&c->ph_ms[i], c->ev_beg[i], c->ev_end[i]);
        }
    }
    if (B.trace) fprintf(stderr, "[align] batch queued\n");
    c->have_output = true;
    c->front_warm = true;
    return 0;
}

// One encode of a resident batch; exact: the payload arena sized from the
// streams' real byte counts after L2 (else the 2-bytes-per-symbol bound).
// al: the reference path (nullptr: no reference).
// Returns 0, -1, or 2 when a stream outgrew its exact cap.
int run_input(sa_ctx* c, const sa_input* I, const sa_cfg* cfg, bool exact, const AlignReq* al = nullptr)
{
    if (!c) return -1;
    if (!I || !cfg || I->device != c->device) {
        c->err = "sa_run_input: no input, no config, or an input of another device";
        return -1;
    }
    const ReserveScope reserve(c->reserve_blocks, I->nblocks);
    Batch B{I, cfg, al, exact};
    if (const int rc = batch_begin(c, B)) return rc;
    if (!B.nbk) return 0;   // (an empty batch: done)
    for (int (*stage)(sa_ctx*, Batch&) : {front_prep, batch_plan_and_buffers, front_emit, seq_sort_replay, aux_sort_runs,
                                          coder_tail, assemble_and_finish})
        if (const int rc = stage(c, B)) return rc;
    return 0;
}

// A batch that failed part-way (E_CODER, a device error bit, a failed call)
// may still have work in flight on the context's streams -- e.g. the long-run
// replay writing d_prs_aux after pass R gave up: the next batch's full memset
// of that buffer (prs_zero_cap is 0 after a failure) must not race it.
void drain_after_error(sa_ctx* c)
{
    for (hipStream_t s : {c->st, c->st2, c->st3, c->st4, c->st5})
        if (s) (void)hipStreamSynchronize(s);
    c->prs_zero_cap = 0;
    c->prs_zero_pending = false;
}

}  // namespace

extern "C" {

int sa_run_input(sa_ctx* c, const sa_input* I, const sa_cfg* cfg)
{
    if (!c) return -1;
    int rc = run_input(c, I, cfg, true);
    if (rc == 2) {   // a stream outgrew its exact payload cap (rare): drain, re-run with the bound
        for (hipStream_t s : {c->st, c->st2, c->st3, c->st4}) SA_CHECK(c, hipStreamSynchronize(s));
        rc = run_input(c, I, cfg, false);
        c->paths.exact_rerun = 1;
    }
    if (rc) drain_after_error(c);
    return rc ? -1 : 0;
}

int sa_phase_times(const sa_ctx* c, const char** names, float* ms, int max)
{
    if (!c || !c->timing) return 0;
    int n = std::min(max, (int)PH_N);
    for (int i = 0; i < n; i++) {
        if (names) names[i] = kPhaseNames[i];
        if (ms) ms[i] = c->ph_ms[i];
    }
    return n;
}

int sa_fetch(sa_ctx* c, sa_out* out, int n)
{
    if (!c || !c->have_output) return -1;
    if ((uint32_t)n != c->final_len.size()) {
        c->err = "sa_fetch: block count mismatch";
        return -1;
    }
    SA_CHECK(c, hipSetDevice(c->device));
    for (int b = 0; b < n; b++) {
        if (c->final_len[(size_t)b] > out[b].cap) {
            c->err = "sa_fetch: output buffer too small";
            return -1;
        }
        SA_CHECK(c, hipMemcpyAsync(out[b].data, c->d_final.as<uint8_t>() + c->final_base[(size_t)b],
                                   c->final_len[(size_t)b], hipMemcpyDeviceToHost, c->st));
        out[b].size = c->final_len[(size_t)b];
    }
    SA_CHECK(c, hipStreamSynchronize(c->st));
    return 0;
}

int sa_fetch_sizes(const sa_ctx* c, uint64_t* sizes, int n)
{
    if (!c || !c->have_output || (n && !sizes) || (uint32_t)n != c->final_len.size()) return -1;
    for (int b = 0; b < n; b++) sizes[b] = c->final_len[(size_t)b];
    return 0;
}

int sa_code_records(sa_ctx* c, int nstreams, const uint32_t* lens, const uint16_t* cum, const uint16_t* freq,
                    const uint16_t* tot, uint8_t* out, uint64_t out_cap, uint64_t* out_lens)
{
    if (!c || nstreams < 0 || (nstreams && (!lens || !out || !out_lens))) return -1;
    SA_CHECK(c, hipSetDevice(c->device));
    std::vector<CoderTask> tasks((size_t)nstreams);
    uint64_t nsym = 0, payload = 0, segs = 0;
    for (int s = 0; s < nstreams; s++) {
        CoderTask& tk = tasks[(size_t)s];
        tk.rec_base = nsym;
        tk.n = lens[s];
        tk.space = 1;   // wide records
        tk.nseg = tk.n ? (tk.n + SEG_SYMS - 1) / SEG_SYMS : 1;
        tk.seg_base = segs;
        tk.out_base = payload;
        const uint64_t cap = 2ull * tk.n + 64;
        if (cap > 0xffffffffull) {
            c->err = "sa_code_records: stream too long";
            return -1;
        }
        tk.out_cap = (uint32_t)cap;
        nsym += tk.n;
        segs += tk.nseg;
        payload = align_up(payload + cap, 16);
    }
    std::vector<PRec> prs(nsym + 128, PRec{0});
    std::vector<uint16_t> cm(nsym + 128, 0);
    for (uint64_t i = 0; i < nsym; i++) {
        const uint32_t t = tot[i], f = freq[i], cu = cum[i];
        if (t < 2 || f < 1 || cu + f > t) {
            c->err = "sa_code_records: invalid (cum, freq, tot)";   // the reference abort()s
            return -1;
        }
        prs[i] = PRec{t | (f << 16)};
        cm[i] = (uint16_t)cu;
    }
    hipStream_t st = c->st;
    c->paths = sa_paths{};
    c->paths.aux_dense_next = c->aux_dense ? 1u : 0u;
    // (SA_RV_VARIANT holds here too; unset: the last batch's variant, 5 on a fresh context)
    if (c->knobs.rv_variant == 0 || c->knobs.rv_variant == 5 || c->knobs.rv_variant == 6) c->rv_batch = c->knobs.rv_variant;
    SA_CHECK(c, c->d_prs_seq.ensure(prs.size() * sizeof(PRec)));
    SA_CHECK(c, c->d_cum_seq.ensure(cm.size() * 2));
    SA_CHECK(c, c->d_tasks.ensure(sizeof(CoderTask) * std::max<size_t>(tasks.size(), 1)));
    SA_CHECK(c, c->d_out_len.ensure(4 * std::max<size_t>(tasks.size(), 1)));
    SA_CHECK(c, c->d_payload.ensure(std::max<uint64_t>(payload, 16)));
    SA_CHECK(c, hipMemcpyAsync(c->d_prs_seq.p, prs.data(), prs.size() * sizeof(PRec), hipMemcpyHostToDevice, st));
    SA_CHECK(c, hipMemcpyAsync(c->d_cum_seq.p, cm.data(), cm.size() * 2, hipMemcpyHostToDevice, st));
    if (!tasks.empty())
        SA_CHECK(c, hipMemcpyAsync(c->d_tasks.p, tasks.data(), sizeof(CoderTask) * tasks.size(), hipMemcpyHostToDevice, st));
    CoderView cv{};
    cv.tasks = c->d_tasks.as<CoderTask>();
    cv.prs[0] = cv.prs[1] = c->d_prs_seq.as<PRec>();
    cv.cum[0] = cv.cum[1] = c->d_cum_seq.as<uint16_t>();
    cv.out = c->d_payload.as<uint8_t>();
    cv.out_len = c->d_out_len.as<uint32_t>();
    c->have_output = false;
    if (coder_buffers(c, tasks.size(), segs, cv)) return -1;
    SA_CHECK(c, hipMemsetAsync(c->d_first_sq.p, 0xff, 4 * std::max<size_t>(tasks.size(), 1), st));
    std::vector<uint32_t> out_len;
    if (coder_run(c, tasks, cv, st, -1, -1, nullptr, false, 0, out_len, payload)) return -1;
    std::vector<uint32_t> ol(tasks.size());
    if (!tasks.empty())
        SA_CHECK(c, hipMemcpyAsync(ol.data(), c->d_out_len.p, 4 * tasks.size(), hipMemcpyDeviceToHost, st));
    SA_CHECK(c, hipStreamSynchronize(st));
    uint64_t o = 0;
    for (size_t s = 0; s < tasks.size(); s++) {
        if (o + ol[s] > out_cap) {
            c->err = "sa_code_records: output buffer too small";
            return -1;
        }
        SA_CHECK(c, hipMemcpyAsync(out + o, c->d_payload.as<uint8_t>() + tasks[s].out_base, ol[s], hipMemcpyDeviceToHost, st));
        out_lens[s] = ol[s];
        o += ol[s];
    }
    SA_CHECK(c, hipStreamSynchronize(st));
    return 0;
}

uint32_t sa_coder_restarts(const sa_ctx* c) { return c ? c->coder_restarts : 0; }

int sa_last_paths(const sa_ctx* c, sa_paths* out)
{
    if (!c || !out) return -1;
    *out = c->paths;
    return 0;
}

uint64_t sa_device_bytes(const sa_ctx* c) { return c ? const_cast<sa_ctx*>(c)->held_bytes() : 0; }

void sa_stream_stats(const sa_ctx* c, uint64_t* max_symbols, uint64_t* total_symbols)
{
    if (max_symbols) *max_symbols = c ? c->max_stream_syms : 0;
    if (total_symbols) *total_symbols = c ? c->total_stream_syms : 0;
}

// HBM a block needs while its batch is encoded: per SEQ symbol the
// double-buffered u32 keys and values plus the 4-byte record (20 B); per AUX
// symbol the same plus its u16 cum (22 B); per symbol up to 2 payload and 2
// final bytes; per read the count columns and the read arrays; the input.
// AUX symbols ~ qualities + name bytes + 8 per read (len, name tokens, dege).
static uint64_t block_footprint(const sa_block& b)
{
    uint64_t bases = 0, nb = 0;
    for (uint32_t r = 0; r < b.nreads; r++) {
        bases += (uint64_t)std::max(b.seq_lens[r], 0);
        nb += b.name_lens[r];
    }
    const uint64_t aux = bases + nb + 8ull * b.nreads;
    return (20 + 4) * bases + (22 + 4) * aux + (nb + 2 * bases + 16) + 64ull * b.nreads;
}

int sa_encode_blocks(sa_ctx* ctx, const sa_block* in, int n, const sa_cfg* cfg, sa_out* out)
{
    if (!ctx || !cfg || (n > 0 && (!in || !out))) return -1;
    if (n == 0) return 0;
    SA_CHECK(ctx, hipSetDevice(ctx->device));
    // Blocks are independent, so a batch larger than the HBM this context can
    // use is encoded as consecutive sub-batches (outputs keep the input order).
    // Budget: 85 % of what is free plus what this context already holds (its
    // buffers are reused).  SA_BATCH_BASES caps the bases per sub-batch (tests).
    size_t free_b = 0, total_b = 0;
    SA_CHECK(ctx, hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = (uint64_t)((double)(free_b + ctx->held_bytes()) * 0.85);
    const uint64_t cap_bases = run_knobs().batch_bases;
    int b0 = 0;
    while (b0 < n) {
        int b1 = b0;
        uint64_t bases = 0, bytes = 0;
        while (b1 < n) {
            uint64_t ls = 0;
            for (uint32_t r = 0; r < in[b1].nreads; r++) ls += (uint64_t)std::max(in[b1].seq_lens[r], 0);
            const uint64_t fb = block_footprint(in[b1]);
            if (b1 > b0 && (bases + ls > cap_bases || bytes + fb > budget)) break;
            bases += ls;
            bytes += fb;
            b1++;
        }
        const auto t0 = std::chrono::steady_clock::now();
        if (sa_stage(ctx, in + b0, b1 - b0)) return -1;
        const auto t1 = std::chrono::steady_clock::now();
        if (sa_run(ctx, cfg)) return -1;
        const auto t2 = std::chrono::steady_clock::now();
        if (sa_fetch(ctx, out + b0, b1 - b0)) return -1;
        if (ctx->knobs.trace) {   // SA_TRACE: per sub-batch host-side stage timings
            const auto t3 = std::chrono::steady_clock::now();
            auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            std::string ph;
            for (int i = 0; i < PH_N; i++) {
                char pb[48];
                std::snprintf(pb, sizeof pb, " %s %.0f", kPhaseNames[i], ctx->ph_ms[i]);
                ph += pb;
            }
            std::fprintf(stderr,
                         "seqarc_amd[%p]: %d blocks: stage %.1f ms, run %.1f ms, fetch %.1f ms, grows %u, "
                         "alloc %.1f ms (all contexts); phases ms:%s\n",
                         (void*)ctx, b1 - b0, ms(t0, t1), ms(t1, t2), ms(t2, t3), g_grows.load(),
                         g_alloc_ns.load() / 1e6, ph.c_str());
        }
        b0 = b1;
    }
    return 0;
}

}  // extern "C"

// FASTQ text parsed on the device (sa_stage_text)
#include "sa_parse.hip"
#include "sa_inflate.hip"
#include "sa_devtext.hip"
#include "sa_gunzip.hip"

// the HASH reference-index path
#include "sa_hash.hip"
