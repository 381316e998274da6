// cli_knobs.h -- every SA_CLI_* environment knob of the command line
// (seqarc_cli.cpp) in one table: CliKnobs is parsed once, in main, and passed
// down (compress, the pipeline, SegReader, OutPool).  Host-only (no HIP
// header): tests/cpu_emu/cli_emu.cpp sweeps the parsing on the CPU
// (tests/test_cli_plan.py).  The comments carry each knob's measured A/B
// history.  (The engine's SA_* knobs: sa_knobs.h.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace cli {

using GetEnv = const char* (*)(const char*);   // std::getenv in the product

struct CliKnobs {
    // ---- the plain-file reader (SegReader) ----
    // SA_CLI_WINDOWS (set at all): plain regular files through the per-block
    // window reader (TextPool) as gzip inputs and pipes are, not the segment reader
    bool windows = false;
    // segments of at most SA_CLI_SEG_MIB MiB (at least 4; a small input: one
    // segment).  512 until round 5, 256 since: the ring is unmapped at the end,
    // ~25 GB/s of page-locked memory, and while device work runs the unmapping
    // stalls it -- a smaller ring costs less of both (r5x)
    int seg_mib = 256;
    // SA_CLI_SEG_SLICES=n: segments of n 4 MiB slices (at least 1) whatever the
    // input's size, for the tests (0: unset)
    uint64_t seg_slices = 0;
    // (A/B) SA_CLI_RING_SEGS=n: n segments per file (at least 3; 0: unset).  The
    // ring is page-locked once, at ~12 GB/s for the whole process
    // (hipHostRegister does not scale with threads,
    // profiles/round5_r5a_ingest_probe.txt): a smaller ring costs less of it
    // before the first pass over it completes
    int ring_segs = 0;
    // the reader runs SA_CLI_AHEAD_BATCHES batches of windows (at least 1) ahead
    // of the staging.  One since round 5, two before: the contexts take batches
    // as fast as the reader cuts them until all are busy, then the device sets
    // the pace
    int64_t ahead_batches = 1;
    // the segments' page-locked memory is released on up to SA_CLI_FREE_THREADS
    // threads (at least 1): releasing ~10 GB of segments one by one took
    // ~0.47 s past the last encode (r5m)
    int free_threads = 8;
    // SA_CLI_RING_FREE=0 (A/B): the ring is left to the process exit instead of
    // being released as soon as every block is staged
    bool ring_free = true;
    // The plain-file reader starts before the device contexts exist (round 5):
    // creating five contexts takes ~0.35 s, which the reader's first batch then
    // overlaps instead of following.  SA_CLI_EARLY_READ=0: contexts first (A/B)
    bool early_read = true;

    // ---- the text windows (TextPool) ----
    // (A/B) SA_CLI_PREFILL_WINDOWS=n: the prefill thread pins n windows (strtoull
    // as it comes) instead of the two batches the reader will hold
    bool prefill_windows_set = false;
    uint64_t prefill_windows = 0;

    // ---- the encoders ----
    // (round 6) the device parse, streamed: sa_text_upload per block as it is
    // cut + sa_text_parse per batch, the next batch uploaded by a helper thread
    // meanwhile.  SA_CLI_STREAM=1 (A/B; off by default): the reader ran faster
    // with it (17.8 GB read in 0.69 against 0.92 s, 42.8 GB in 1.84 against
    // 2.39 s) but the device pipeline slower -- pass R 744-1,019 against
    // 605-694 ms a batch, the run's end 2.28 / 4.46 against 2.08-2.14 /
    // 3.48-3.59 s (r6e, one box): with every batch on the device at once the
    // fronts queue up all the same and the concurrent uploads slow the chains
    bool stream = false;
    // SA_CLI_PREFETCH=0 (A/B): the streamed path takes its next batch after the
    // current one instead of beside it
    bool prefetch = true;
    // (round 6) the device-parse path sizes each block's output buffer by its
    // encoded size (sa_fetch_sizes after sa_run) instead of its output bound:
    // the pool held ~270 buffers of ~180 MB of address space for ~7 MB blocks,
    // whose teardown was most of the exit (r6z).  SA_CLI_OUT_EXACT=0: the bound (A/B)
    bool out_exact = true;
    // the encoded blocks' host buffers are recycled (OutPool, round 5).
    // SA_CLI_OUT_POOL=0: a fresh buffer per block (A/B)
    bool out_pool = true;
    // one hardware queue per stream: SA_CLI_HWQ=n queues per context (at least
    // 1; 0: unset -- four, five with SA_CLI_STREAM's copy stream; A/B)
    int hwq = 0;

    // ---- tests and diagnostics ----
    // SA_CLI_TEST_OUT=n: --host-only gives each block n bytes of filler (strtoull
    // as it comes), so the archive writer runs without a device
    uint64_t test_out = 0;
    // SA_CLI_EXIT_PROBE=1: what the exit would tear down (the output pool's
    // buffers, then the contexts) is torn down and timed before it
    bool exit_probe = false;
};

inline CliKnobs parse_cli_knobs(GetEnv env)
{
    CliKnobs k;
    auto off_if_zero = [&](const char* n) { const char* e = env(n); return !(e && std::atoi(e) == 0); };
    auto on_if_nonzero = [&](const char* n) { const char* e = env(n); return e && std::atoi(e) != 0; };
    k.windows = env("SA_CLI_WINDOWS") != nullptr;
    if (const char* e = env("SA_CLI_SEG_MIB")) k.seg_mib = std::max(4, std::atoi(e));
    if (const char* e = env("SA_CLI_SEG_SLICES")) k.seg_slices = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    if (const char* e = env("SA_CLI_RING_SEGS")) k.ring_segs = std::max(3, std::atoi(e));
    if (const char* e = env("SA_CLI_AHEAD_BATCHES")) k.ahead_batches = std::max(1, std::atoi(e));
    if (const char* e = env("SA_CLI_FREE_THREADS")) k.free_threads = std::max(1, std::atoi(e));
    k.ring_free = off_if_zero("SA_CLI_RING_FREE");
    k.early_read = off_if_zero("SA_CLI_EARLY_READ");
    if (const char* e = env("SA_CLI_PREFILL_WINDOWS")) {
        k.prefill_windows_set = true;
        k.prefill_windows = std::strtoull(e, nullptr, 10);
    }
    k.stream = on_if_nonzero("SA_CLI_STREAM");
    k.prefetch = off_if_zero("SA_CLI_PREFETCH");
    k.out_exact = off_if_zero("SA_CLI_OUT_EXACT");
    k.out_pool = off_if_zero("SA_CLI_OUT_POOL");
    if (const char* e = env("SA_CLI_HWQ")) k.hwq = std::max(1, std::atoi(e));
    if (const char* e = env("SA_CLI_TEST_OUT")) k.test_out = std::strtoull(e, nullptr, 10);
    k.exit_probe = on_if_nonzero("SA_CLI_EXIT_PROBE");
    return k;
}

// GPU_MAX_HW_QUEUES for a process of `contexts` contexts per device: four
// queues per context (five with the streamed staging's copy stream, round 6)
// and four to spare, at most 32
inline int plan_hw_queues(const CliKnobs& k, int contexts) { return std::min(32, (k.hwq ? k.hwq : k.stream ? 5 : 4) * contexts + 4); }

}  // namespace cli
