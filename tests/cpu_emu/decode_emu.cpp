// decode_emu.cpp -- drives fastqueeze_amd/csrc/sa_decode_logic.h on the host the
// way a kernel with one wave per block would drive it: the 64-lane model step
// run as a loop over the lanes (LoopOps), every chain decoded in slices that
// stop and resume through the stored DecChain, the placement between the two
// chains, the host pre-pass of arc_decode_host.h in front and the MD5 check
// behind (tests/test_decode_emu.py compares every block with the input that was
// encoded and with sa_decode_block).
//
//   decode_emu blocks <file> [outdir]
//     file: i32 slevel, qlevel, md5, bin_mode; u32 slice; u32 n; 512 bytes ID
//     template; then per block u32 len, u32 long_reads, u32 cap and len bytes.
//     Prints per block "<rc> <status> <md5_ok> <events> <qual launches> <seq
//     launches>" (events: the DEC_EV_* bits seen); with outdir, block i's arrays
//     go to outdir/i.names, .nl, .seq, .sl, .qual.  The encoded block, the chain
//     outputs and the tables live in heap blocks of exactly their sizes, so a
//     sanitizer build sees any access outside them.
//   decode_emu range0
//     the bounded renormalisation from a constructed coder state whose squeeze
//     leaves range 0: prints "<status> <bytes read>".
//   decode_emu plan <slevel> <qlevel> <free bytes> <cap> {<enc> <bases> <side> <nreads>}...
//     plan_decode: "<qual_table> <seq_table> <budget> <max_block> <inflight>
//     <unsupported>", then per block "<bytes> <unsupported>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastqueeze_amd/csrc/arc_decode_host.h"
#include "../../fastqueeze_amd/csrc/sa_decode_logic.h"

using namespace sa;

struct LoopOps {   // the wave as a loop: register arrays of 64, one entry a lane
    static constexpr int N = 64;
    template <class F> void each(F f)
    {
        for (uint32_t l = 0; l < 64; l++) f(l, l);
    }
    uint32_t scan(const uint32_t* in, uint32_t* out)
    {
        uint32_t acc = 0;
        for (int l = 0; l < 64; l++) {
            out[l] = acc;
            acc += in[l];
        }
        return acc;
    }
    uint32_t first(const uint32_t* a, uint32_t v)
    {
        for (uint32_t l = 0; l < 64; l++)
            if (a[l] == v) return l;
        return 64;
    }
    uint32_t get(const uint32_t* a, uint32_t src) { return a[src]; }
    uint32_t ld8(const uint8_t* p) { return *p; }
    uint32_t ld32(const uint32_t* p) { return *p; }
    void st8(uint8_t* p, uint8_t v) { *p = v; }
    void st32(uint32_t* p, uint32_t v) { *p = v; }
    void fill(uint8_t* p, uint32_t n, uint8_t v)
    {
        if (n) memset(p, v, n);
    }
};

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "decode_emu: cannot open %s\n", path);
        exit(2);
    }
    uint8_t buf[1 << 16];
    size_t r;
    while ((r = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + r);
    fclose(f);
    return v;
}

static uint32_t rd32(const std::vector<uint8_t>& v, size_t at)
{
    if (at + 4 > v.size()) {
        fprintf(stderr, "decode_emu: short file\n");
        exit(2);
    }
    return v[at] | v[at + 1] << 8 | v[at + 2] << 16 | (uint32_t)v[at + 3] << 24;
}

static void dump(const std::string& p, const void* d, size_t n)
{
    FILE* o = fopen(p.c_str(), "wb");
    if (!o || (n && fwrite(d, 1, n, o) != n)) {
        fprintf(stderr, "decode_emu: cannot write %s\n", p.c_str());
        exit(2);
    }
    fclose(o);
}

static int run_range0()
{
    // low ends in 0xffffff and low + range carries into the top byte: the squeeze
    // gives range = 0xffffff - (low & 0xffffff) = 0, and no later round changes it
    DecChain c{};
    c.low = 0x00ffffffffffffffull;
    c.code = c.low;
    c.range = 0xffffffffu;
    uint8_t* in = (uint8_t*)calloc(64, 1);
    dec_consume(c, in, 64, 1, 0, 1);   // range = 1
    printf("%u %u\n", c.status, c.pos);
    free(in);
    return 0;
}

static int run_plan(int argc, char** argv)
{
    sa_cfg cfg{};
    cfg.slevel = atoi(argv[2]);
    cfg.qlevel = atoi(argv[3]);
    const uint64_t free_b = strtoull(argv[4], nullptr, 10);
    const uint32_t cap = (uint32_t)strtoul(argv[5], nullptr, 10);
    std::vector<DecBlockSize> bs;
    for (int k = 6; k + 3 < argc; k += 4)
        bs.push_back({strtoull(argv[k], nullptr, 10), strtoull(argv[k + 1], nullptr, 10), strtoull(argv[k + 2], nullptr, 10),
                      (uint32_t)strtoul(argv[k + 3], nullptr, 10), 0});
    std::vector<uint64_t> per(bs.size() + 1);
    std::vector<uint8_t> un(bs.size() + 1);
    const DecPlan p = plan_decode(cfg, (uint32_t)bs.size(), bs.data(), free_b, cap, per.data(), un.data());
    printf("%llu %llu %llu %llu %u %u\n", (unsigned long long)p.qual_table, (unsigned long long)p.seq_table,
           (unsigned long long)p.budget, (unsigned long long)p.max_block, p.inflight, p.unsupported);
    for (size_t i = 0; i < bs.size(); i++) printf("%llu %u\n", (unsigned long long)per[i], un[i]);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "range0")) return run_range0();
    if (argc >= 6 && !strcmp(argv[1], "plan")) return run_plan(argc, argv);
    if (argc < 3 || strcmp(argv[1], "blocks")) {
        fprintf(stderr, "usage: decode_emu blocks <file> [outdir] | range0 | plan ...\n");
        return 2;
    }
    const std::vector<uint8_t> f = slurp(argv[2]);
    sa_cfg cfg{};
    cfg.slevel = (int32_t)rd32(f, 0);
    cfg.qlevel = (int32_t)rd32(f, 4);
    cfg.md5 = (int32_t)rd32(f, 8);
    cfg.bin_mode = (int32_t)rd32(f, 12);
    const uint32_t slice = rd32(f, 16), nblocks = rd32(f, 20);
    if (f.size() < 24 + 512 || !slice) return 2;
    const uint8_t* tmpl = f.data() + 24;
    size_t at = 24 + 512;
    LoopOps w;
    const uint32_t nctx = dec_qual_contexts(cfg.qlevel), smask = dec_seq_mask(cfg.slevel);
    for (uint32_t b = 0; b < nblocks; b++) {
        const uint32_t len = rd32(f, at), long_reads = rd32(f, at + 4), cap = rd32(f, at + 8);
        at += 12;
        if (at + len > f.size()) return 2;
        uint8_t* in = (uint8_t*)malloc(len ? len : 1);
        memcpy(in, f.data() + at, len);
        at += len;
        const uint32_t mr = cap / 4 + 8;
        std::vector<uint8_t> names(cap), seq(cap), qual(cap);
        std::vector<uint16_t> nl(mr);
        std::vector<int32_t> sl(mr);
        sa_decoded o{names.data(), nl.data(), seq.data(), sl.data(), qual.data(), cap, cap, mr, 0, 1};
        sadh::DecPre pre;
        uint32_t status = 0, ev = 0, nq = 0, ns = 0;
        int64_t rc = -1;
        if (!sadh::dec_prepass(in, len, &cfg, tmpl, (int32_t)long_reads, &o, pre)) {
            status = SA_DEC_LAYOUT;
        } else {
            // what a device would hold of a block: the payloads, the lengths, the outputs, the tables
            uint8_t* qin = (uint8_t*)malloc(pre.qual_len ? pre.qual_len : 1);
            uint8_t* sin = (uint8_t*)malloc(pre.seq_len ? pre.seq_len : 1);
            memcpy(qin, pre.qual, pre.qual_len);
            memcpy(sin, pre.seq, pre.seq_len);
            uint8_t* Q = (uint8_t*)malloc(pre.total ? pre.total : 1);
            uint8_t* S = (uint8_t*)calloc(pre.total ? pre.total : 1, 1);
            memset(Q, 0xa5, pre.total);
            uint8_t* models = (uint8_t*)malloc((size_t)nctx * DEC_QM_STRIDE);
            for (uint32_t c = 0; c < nctx; c++)
                for (uint32_t e = 0; e < DEC_QSYM; e++) sm_init_entry(models + (size_t)c * DEC_QM_STRIDE, e);
            DecChain stored{};   // the state in "global memory" between the launches
            while (!stored.done) {
                DecChain c = stored;
                dec_qual_slice(w, c, qin, pre.qual_len, pre.len.data(), pre.n, Q, models, cfg.qlevel, slice, ev);
                stored = c;
                nq++;
            }
            free(models);
            status = stored.status;
            if (!status)
                status = dec_place(Q, S, (uint32_t)pre.tip_off.size(), pre.tip_off.data(), pre.tip_len.data(), pre.side.maxq.data(),
                                   pre.side.exc.data(), pre.side.gaps.data(), pre.side.gaps.size(), pre.side.chs.data(),
                                   pre.side.chs.size());
            if (!status) {
                const size_t tb = 4 * ((size_t)smask + 1);
                uint8_t* tab = (uint8_t*)malloc(tb);
                memset(tab, 3, tb);
                stored = DecChain{};
                while (!stored.done) {
                    DecChain c = stored;
                    dec_seq_slice(w, c, sin, pre.seq_len, pre.len.data(), pre.n, S, tab, smask, slice, ev);
                    stored = c;
                    ns++;
                }
                free(tab);
                status = stored.status;
            }
            if (!status) {
                memcpy(o.qual, Q, pre.total);
                memcpy(o.seq, S, pre.total);
                if (cfg.md5) o.md5_ok = sadh::dec_md5_verify(&o, pre.name_total, pre.total, true, pre.dg_id, pre.dg_q, pre.dg_s);
                rc = (int64_t)pre.n;
            }
            free(qin);
            free(sin);
            free(Q);
            free(S);
        }
        printf("%lld %u %d %u %u %u\n", (long long)rc, status, (int)o.md5_ok, ev, nq, ns);
        if (argc >= 4 && rc >= 0) {
            const std::string p = std::string(argv[3]) + "/" + std::to_string(b);
            dump(p + ".names", o.names, pre.name_total);
            dump(p + ".nl", o.name_lens, 2 * (size_t)pre.n);
            dump(p + ".seq", o.seq, pre.total);
            dump(p + ".sl", o.seq_lens, 4 * (size_t)pre.n);
            dump(p + ".qual", o.qual, pre.total);
        }
        free(in);
    }
    return 0;
}
