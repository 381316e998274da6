// cli_plan.h -- the command line's batch geometry as one pure function of plain
// numbers: the options, PE or SE, the block size, what is known of each input
// (size, gzip, regular file), the CliKnobs and the number of encoder contexts.
// Host-only (no HIP header, no file or device access): compress() calls it,
// tests/cpu_emu/cli_emu.cpp sweeps it on the CPU (tests/test_cli_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "cli_knobs.h"

namespace cli {

constexpr uint64_t kUnknownSize = ~0ull;
constexpr uint64_t kSegSlice = 4ull << 20;      // SegReader: the fill threads' unit of a segment
constexpr size_t kTextChunk = 16;               // TextPool: windows per page-locked arena chunk
constexpr uint64_t kWindowSlack = 64u << 10;    // a text window's slack for the carry

// the options the plan reads (the command line's Options derives from this)
struct PlanOpts {
    int batch = 32, contexts = 2, devices = 1, threads = 0;
    // --read-threads: the plain-file reader's fill threads (SegReader).  16 since
    // round 6: the whole-node ingest (--ingest-only --devices 8) 34.3 / 35.8
    // against 18.2 / 28.7 GB/s with 8 (r6s; the reader two or three batches
    // ahead instead: 21.5-25.4)
    int read_threads = 16;
    bool host_only = false, host_parse = false, ingest_only = false, ramp = false, stage_ahead = false;
    // --gpu-text applies (the command line sets it in the plan's input once it knows the inputs
    // are BGZF): the text stays on the device, so the feed is the streamed one and the reader
    // holds no page-locked windows
    bool gpu_text = false;
};

struct PlanIn : PlanOpts {
    bool pe = false;
    uint64_t bs = 50ull << 20;                  // block bytes (--block-size)
    // each input (the second only with pe): its size if it is a regular file
    // and fstat gives one, whether it is gzip
    uint64_t size[2] = {kUnknownSize, kUnknownSize};
    bool gz[2] = {false, false}, regular[2] = {false, false};
    unsigned hw_threads = 16;                   // std::thread::hardware_concurrency()
};

// the contexts the options ask for (what the plan is made with while they do not exist yet)
inline int64_t plan_contexts_asked(const PlanOpts& o) { return (int64_t)o.contexts * (o.host_only ? 1 : o.devices); }

struct BatchPlan {
    // Device parse (default): the reader's text windows are page-locked, the
    // encoder threads stage them (H2D DMA + parse in HBM) and recycle them at
    // once; only block 0 is parsed on the host, for the ID template.
    // --host-parse / --host-only: nparse parser threads build the SoA.
    bool dev_parse = true;
    int nparse = 1;
    // plain regular files (not gzip, not a pipe) are read by the segment reader
    // (SegReader), the others in per-block windows (TextPool)
    bool seg_plain = false;
    bool early_read = false;      // the reader starts before the contexts exist (seg_plain only)
    bool texts_pinned = false;    // the text windows are page-locked
    // bytes of one input the cut looks at (a block, or half of one per mate); a
    // text window (that + slack for the carry); streamed staging: bytes
    // reserved per text on the device
    uint64_t cut_window = 0, text_win = 0, tstride = 0;
    // the windows the reader will hold (two batches ahead of the staging, both
    // mates; an input that is smaller needs fewer), pinned ahead in chunks
    size_t prefill_windows = 0, prefill_chunks = 0;
    // batch k = blocks [bstart(k), bstart(k + 1)): B blocks, C contexts.
    // --ramp: the first batch of each context ramps up (B (k+1) / (C+1) blocks:
    // the first encode starts after a fraction of a batch is read, and the
    // contexts' first tails are staggered); the contexts allocate for B from
    // the start (sa_set_reserve).  Off by default since round 4: a batch's
    // latency is its longest chain's whatever its size, so the ramp's five
    // small batches cost a round of throughput (42.8 GB: 5,390 MB/s with it,
    // 6,642 without, r4m).  A plain-file input that fits one round (C batches
    // of B blocks, by its size) is dealt as C equal batches and the ramp is off
    // (round 3 g4g: with the ramp its last blocks waited for a second round of
    // batch latencies); --host-only and --ingest-only keep B.
    int64_t B = 1, C = 1;
    bool ramp = false;
    std::vector<int64_t> ramp_start{0};
    // the streamed staging (SA_CLI_STREAM) applies: each context's helper holds
    // one more batch on the device, its text already back with the reader
    bool stream_opt = false;
    // blocks read but not yet written: C batches encoding (twice with
    // stream_opt) and two ahead
    size_t max_inflight = 0;
    // the segment reader (seg_plain): batches ahead of the staging, its cut
    // window, the bytes it reads ahead, a segment's bytes, segments per file.
    // (at least a batch of windows and two segments of slack: the blocks of a
    // batch keep their segments until the batch is staged; r5i: a ring of four
    // 512 MiB segments deadlocked a 69-block batch)
    int64_t seg_ahead = 0, seg_ahead_bytes = 0;
    uint64_t seg_window = 0, seg_bytes = 0;
    int ring_segs = 0;

    int64_t bstart(int64_t k) const
    {
        const int64_t r = (int64_t)ramp_start.size() - 1;
        return k <= r ? ramp_start[(size_t)k] : ramp_start.back() + (k - r) * B;
    }
};

// nctx: the encoder contexts -- plan_contexts_asked(in) while they do not
// exist, or the number created.  Everything but B, C, the ramp, max_inflight
// and the segment ring is independent of it, so a second call with the created
// count re-plans a run whose first plan was made before the contexts existed.
inline BatchPlan plan_batches(const PlanIn& in, const CliKnobs& kn, int64_t nctx)
{
    BatchPlan p;
    const int nin = in.pe ? 2 : 1;
    const bool gz = in.gz[0] || (in.pe && in.gz[1]);
    // the inputs' sizes: all known (regular files), their sum and the largest
    bool known = true;
    uint64_t sum = 0, mx = 0;
    for (int i = 0; i < nin; i++) {
        if (!in.regular[i] || in.size[i] == kUnknownSize) known = false;   // (a pipe: size unknown)
        else sum += in.size[i], mx = std::max(mx, in.size[i]);
    }
    p.dev_parse = !in.host_parse && !in.host_only;
    p.nparse = p.dev_parse ? 1 : in.threads > 0 ? in.threads : (int)std::max(1u, std::min(16u, in.hw_threads));
    p.cut_window = in.pe ? (uint64_t)((uint32_t)in.bs >> 1) : in.bs;
    p.text_win = p.cut_window + kWindowSlack;
    p.tstride = p.cut_window + (128u << 10);
    p.texts_pinned = p.dev_parse && !in.ingest_only;
    p.seg_plain = in.read_threads > 0 && !gz && !kn.windows && known;
    p.early_read = kn.early_read && p.seg_plain;
    if (p.texts_pinned && !p.seg_plain && !in.gpu_text) {
        p.prefill_windows = (size_t)nin * (2 * (size_t)std::max(1, in.batch) + 4);
        if (known && !gz) p.prefill_windows = std::min(p.prefill_windows, (size_t)nin * (size_t)(mx / p.cut_window + 3));
        if (kn.prefill_windows_set) p.prefill_windows = (size_t)kn.prefill_windows;
        p.prefill_chunks = (p.prefill_windows + kTextChunk - 1) / kTextChunk;
    }
    p.B = std::max(1, in.batch);
    p.C = nctx;
    p.ramp = in.ramp;
    if (!in.host_only && !in.ingest_only && !gz && known && sum < (~0ull >> 2)) {
        const int64_t est = (int64_t)((sum + in.bs - 1) / in.bs) + 1;   // blocks (cut at record ends: <= bs each)
        if (est <= p.C * p.B) {   // one round
            p.ramp = false;
            p.B = (est + p.C - 1) / p.C;
        }
    }
    p.stream_opt = p.dev_parse && !in.ingest_only && !in.stage_ahead && (kn.stream || in.gpu_text);
    p.max_inflight = (size_t)p.B * ((size_t)p.C * (p.stream_opt ? 2 : 1) + 2);
    for (int64_t k = 0; p.ramp && k < p.C; k++)
        p.ramp_start.push_back(p.ramp_start.back() + std::max<int64_t>(1, p.B * (k + 1) / (p.C + 1)));
    if (p.seg_plain) {
        p.seg_ahead = kn.ahead_batches;
        p.seg_window = p.text_win;
        p.seg_ahead_bytes = (int64_t)(p.seg_ahead * p.B + 2) * (int64_t)p.cut_window;
        // segments of SA_CLI_SEG_MIB MiB (a small input: one segment), SA_CLI_SEG_SLICES=n: n slices
        uint64_t S = std::max(kSegSlice, std::min((uint64_t)kn.seg_mib << 20, (mx + kSegSlice - 1) / kSegSlice * kSegSlice));
        if (kn.seg_slices) S = kSegSlice * kn.seg_slices;
        int R = (int)std::max<int64_t>(3, (p.seg_ahead_bytes + (int64_t)S - 1) / (int64_t)S + 3);
        if (kn.ring_segs) R = kn.ring_segs;
        p.seg_bytes = S;
        p.ring_segs = std::max<int>(R, (int)(((uint64_t)p.B * p.seg_window + S - 1) / S) + 2);
    }
    return p;
}

}  // namespace cli
