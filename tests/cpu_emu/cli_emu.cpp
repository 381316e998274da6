// cli_emu -- the command line's knob table (cli_knobs.h) and batch plan
// (cli_plan.h) as a stand-alone program, for tests/test_cli_plan.py:
//
//   cli_emu --knobs                 every CliKnobs field under this environment
//   cli_emu --plan key=value ...    plan_batches for the PlanIn the keys describe
//                                   (nctx=N: the context count; default: the
//                                   count the options ask for), under this
//                                   environment's knobs; "--" starts another plan
//
// One line of `name value` pairs, integers only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../fastqueeze_amd/csrc/cli_knobs.h"
#include "../../fastqueeze_amd/csrc/cli_plan.h"

static const char* env(const char* n) { return std::getenv(n); }

static void put(const char* n, unsigned long long v) { printf("%s %llu ", n, v); }
static void puts64(const char* n, long long v) { printf("%s %lld ", n, v); }

static int knobs()
{
    const cli::CliKnobs k = cli::parse_cli_knobs(env);
    put("windows", k.windows);
    puts64("seg_mib", k.seg_mib);
    put("seg_slices", k.seg_slices);
    puts64("ring_segs", k.ring_segs);
    puts64("ahead_batches", k.ahead_batches);
    puts64("free_threads", k.free_threads);
    put("ring_free", k.ring_free);
    put("early_read", k.early_read);
    put("prefill_windows_set", k.prefill_windows_set);
    put("prefill_windows", k.prefill_windows);
    put("stream", k.stream);
    put("prefetch", k.prefetch);
    put("out_exact", k.out_exact);
    put("out_pool", k.out_pool);
    puts64("hwq", k.hwq);
    put("test_out", k.test_out);
    put("exit_probe", k.exit_probe);
    for (int c : {1, 2, 5, 8}) put(("queues_c" + std::to_string(c)).c_str(), (unsigned long long)cli::plan_hw_queues(k, c));
    printf("\n");
    return 0;
}

static int plan(int first, int argc, char** argv)   // the keys argv[first .. argc)
{
    cli::PlanIn in;
    long long nctx = -1;
    for (int i = first; i < argc; i++) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string key(argv[i], (size_t)(eq - argv[i]));
        const unsigned long long v = strtoull(eq + 1, nullptr, 10);
        if (key == "batch") in.batch = (int)v;
        else if (key == "contexts") in.contexts = (int)v;
        else if (key == "devices") in.devices = (int)v;
        else if (key == "threads") in.threads = (int)v;
        else if (key == "read_threads") in.read_threads = (int)v;
        else if (key == "host_only") in.host_only = v != 0;
        else if (key == "host_parse") in.host_parse = v != 0;
        else if (key == "ingest_only") in.ingest_only = v != 0;
        else if (key == "ramp") in.ramp = v != 0;
        else if (key == "stage_ahead") in.stage_ahead = v != 0;
        else if (key == "pe") in.pe = v != 0;
        else if (key == "bs") in.bs = v;
        else if (key == "size0") in.size[0] = v;
        else if (key == "size1") in.size[1] = v;
        else if (key == "gz0") in.gz[0] = v != 0;
        else if (key == "gz1") in.gz[1] = v != 0;
        else if (key == "reg0") in.regular[0] = v != 0;
        else if (key == "reg1") in.regular[1] = v != 0;
        else if (key == "hw_threads") in.hw_threads = (unsigned)v;
        else if (key == "nctx") nctx = (long long)v;
        else return 2;
    }
    const cli::CliKnobs k = cli::parse_cli_knobs(env);
    const cli::BatchPlan p = cli::plan_batches(in, k, nctx < 0 ? cli::plan_contexts_asked(in) : nctx);
    puts64("asked", cli::plan_contexts_asked(in));
    put("dev_parse", p.dev_parse);
    puts64("nparse", p.nparse);
    put("seg_plain", p.seg_plain);
    put("early_read", p.early_read);
    put("texts_pinned", p.texts_pinned);
    put("cut_window", p.cut_window);
    put("text_win", p.text_win);
    put("tstride", p.tstride);
    put("prefill_windows", p.prefill_windows);
    put("prefill_chunks", p.prefill_chunks);
    puts64("B", p.B);
    puts64("C", p.C);
    put("ramp", p.ramp);
    put("stream_opt", p.stream_opt);
    put("max_inflight", p.max_inflight);
    puts64("seg_ahead", p.seg_ahead);
    put("seg_window", p.seg_window);
    puts64("seg_ahead_bytes", p.seg_ahead_bytes);
    put("seg_bytes", p.seg_bytes);
    puts64("ring_segs", p.ring_segs);
    put("ramp_n", p.ramp_start.size());
    for (size_t i = 0; i < p.ramp_start.size(); i++) puts64(("rs" + std::to_string(i)).c_str(), p.ramp_start[i]);
    for (long long b = 0; b <= p.C + 4; b++) puts64(("bstart" + std::to_string(b)).c_str(), p.bstart(b));
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "--knobs")) return knobs();
    if (argc >= 2 && !strcmp(argv[1], "--plan")) {   // (several plans: their keys separated by "--", a line each)
        for (int a = 2, e; a <= argc; a = e + 1) {
            for (e = a; e < argc && strcmp(argv[e], "--"); e++) {}
            if (const int rc = plan(a, e, argv)) return rc;
        }
        return 0;
    }
    fprintf(stderr, "usage: cli_emu --knobs | --plan key=value ...\n");
    return 2;
}
