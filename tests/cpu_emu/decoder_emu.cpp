// decoder_emu.cpp -- the driver of sa_decode_blocks (fastqueeze_amd/csrc/sa_decoder.h:
// dec_run) on the host, over a backend whose "device" is heap memory and whose
// slice calls are dec_block_qual / dec_block_seq<LoopOps>, a loop over the blocks
// of the group where the device has one wave per block (tests/test_decoder_host.py).
//
//   decoder_emu <mode> <file> <cap> [outdir]
//     mode: run         the backend as described
//           stuck       the slice calls change nothing (a device that makes no progress)
//           stuck_but0  the slice calls advance the group's first block only
//     file: decode_emu's "blocks" file (i32 slevel, qlevel, md5, bin_mode; u32 slice;
//           u32 n; 512 bytes ID template; per block u32 len, u32 long_reads, u32 cap
//           and len bytes); a slevel < 0 stands for a lossy config (-l) at slevel 3
//     cap:  SA_DEC_INFLIGHT (0: none)
//     Prints "<rc> <groups> <inflight> <slice> <qual launches> <seq launches>
//     <unsupported> <backend calls>", then per block "<status> <md5_ok> <nreads>";
//     with outdir, a block without a status leaves outdir/i.names, .nl, .seq, .sl, .qual.
//     The arena and both staging buffers are heap blocks of exactly their sizes,
//     so a sanitizer build sees any access outside them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastqueeze_amd/csrc/sa_decoder.h"

using namespace sa;

struct LoopOps {   // the wave as a loop (decode_emu.cpp)
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

enum Mode { RUN, STUCK, STUCK_BUT0 };

struct EmuBackend {
    Mode mode = RUN;
    uint32_t calls = 0;
    uint8_t *arena = nullptr, *h_up = nullptr, *h_out = nullptr;
    std::vector<DecDesc> desc;
    std::vector<DecChain> qchain, schain;
    std::vector<uint32_t> status;
    LoopOps w;
    uint32_t ev = 0;

    void drop()
    {
        free(arena);
        free(h_up);
        free(h_out);
        arena = h_up = h_out = nullptr;
    }
    ~EmuBackend() { drop(); }
    uint64_t free_bytes()
    {
        calls++;
        return 64ull << 30;
    }
    bool alloc(uint64_t arena_bytes, uint64_t up, uint64_t out, uint32_t nb, uint8_t** hu, uint8_t** ho)
    {
        calls++;
        drop();   // (exact sizes for the sanitizers, so nothing is recycled here)
        arena = (uint8_t*)malloc(arena_bytes ? arena_bytes : 1);
        h_up = (uint8_t*)malloc(up ? up : 1);
        h_out = (uint8_t*)malloc(out ? out : 1);
        memset(arena, 0xa5, arena_bytes);
        memset(h_up, 0, up);
        desc.assign(nb, DecDesc{});
        qchain.assign(nb, DecChain{});
        schain.assign(nb, DecChain{});
        status.assign(nb, 0xffffffffu);
        *hu = h_up;
        *ho = h_out;
        return true;
    }
    bool upload(const DecDesc* d, uint32_t nb, uint64_t up)
    {
        calls++;
        memcpy(arena, h_up, up);
        for (uint32_t b = 0; b < nb; b++) desc[b] = d[b];
        return true;
    }
    bool init(uint32_t nb, uint64_t out_off, uint64_t out, uint64_t qual_table, uint64_t seq_table)
    {
        calls++;
        memset(arena + out_off, 0, out);
        for (uint32_t b = 0; b < nb; b++) {
            for (uint64_t c = 0; c < qual_table / DEC_QM_STRIDE; c++)
                for (uint32_t e = 0; e < DEC_QSYM; e++) sm_init_entry(arena + desc[b].models + c * DEC_QM_STRIDE, e);
            memset(arena + desc[b].tab, 3, seq_table);
            qchain[b] = schain[b] = DecChain{};
            status[b] = 0;
        }
        return true;
    }
    bool moves(uint32_t b) const { return mode == RUN || (mode == STUCK_BUT0 && b == 0); }
    bool qual_slice(uint32_t nb, int32_t qlevel, uint32_t slice)
    {
        calls++;
        for (uint32_t b = 0; b < nb; b++) {
            DecChain c = qchain[b];
            if (c.done || !moves(b)) continue;
            dec_block_qual(w, arena, desc[b], c, qlevel, slice, ev);
            qchain[b] = c;
        }
        return true;
    }
    bool place(uint32_t nb)
    {
        calls++;
        for (uint32_t b = 0; b < nb; b++) status[b] = dec_block_place(arena, desc[b], qchain[b], schain[b]);
        return true;
    }
    bool seq_slice(uint32_t nb, uint32_t mask, uint32_t slice)
    {
        calls++;
        for (uint32_t b = 0; b < nb; b++) {
            DecChain c = schain[b];
            if (c.done || !moves(b)) continue;
            dec_block_seq(w, arena, desc[b], c, mask, slice, ev);
            schain[b] = c;
        }
        return true;
    }
    bool chains(int which, DecChain* c, uint32_t* st, uint32_t nb)
    {
        calls++;
        for (uint32_t b = 0; b < nb; b++) {
            c[b] = which ? schain[b] : qchain[b];
            if (st) st[b] = status[b];
        }
        return true;
    }
    bool download(uint64_t out_off, uint64_t out)
    {
        calls++;
        memcpy(h_out, arena + out_off, out);
        return true;
    }
    bool finish(sa_decode_info&)
    {
        calls++;
        return true;
    }
};

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "decoder_emu: cannot open %s\n", path);
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
        fprintf(stderr, "decoder_emu: short file\n");
        exit(2);
    }
    return v[at] | v[at + 1] << 8 | v[at + 2] << 16 | (uint32_t)v[at + 3] << 24;
}

static void dump(const std::string& p, const void* d, size_t n)
{
    FILE* o = fopen(p.c_str(), "wb");
    if (!o || (n && fwrite(d, 1, n, o) != n)) {
        fprintf(stderr, "decoder_emu: cannot write %s\n", p.c_str());
        exit(2);
    }
    fclose(o);
}

struct Arrays {
    std::vector<uint8_t> names, seq, qual;
    std::vector<uint16_t> nl;
    std::vector<int32_t> sl;
};

int main(int argc, char** argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: decoder_emu run|stuck|stuck_but0 <file> <cap> [outdir]\n");
        return 2;
    }
    EmuBackend be;
    if (!strcmp(argv[1], "stuck")) be.mode = STUCK;
    else if (!strcmp(argv[1], "stuck_but0")) be.mode = STUCK_BUT0;
    else if (strcmp(argv[1], "run")) return 2;
    const std::vector<uint8_t> f = slurp(argv[2]);
    sa_cfg cfg{};
    cfg.slevel = (int32_t)rd32(f, 0);
    if (cfg.slevel < 0) {
        cfg.slevel = 3;
        cfg.lossy = 1.0;
    }
    cfg.qlevel = (int32_t)rd32(f, 4);
    cfg.md5 = (int32_t)rd32(f, 8);
    cfg.bin_mode = (int32_t)rd32(f, 12);
    sadec::DecKnobs kn;
    kn.slice = rd32(f, 16);
    kn.inflight = (uint32_t)strtoul(argv[3], nullptr, 10);
    const uint32_t n = rd32(f, 20);
    if (f.size() < 24 + 512 || !kn.slice) return 2;
    const uint8_t* tmpl = f.data() + 24;
    size_t at = 24 + 512;
    std::vector<uint8_t*> in(n);
    std::vector<uint64_t> len(n);
    std::vector<int32_t> lng(n);
    std::vector<Arrays> arr(n);
    std::vector<sa_decoded> out(n);
    std::vector<uint32_t> status(n, 0xffffffffu);
    for (uint32_t b = 0; b < n; b++) {
        const uint32_t l = rd32(f, at), cap = rd32(f, at + 8);
        lng[b] = (int32_t)rd32(f, at + 4);
        at += 12;
        if (at + l > f.size()) return 2;
        in[b] = (uint8_t*)malloc(l ? l : 1);   // (exactly the block: a read past it is seen)
        memcpy(in[b], f.data() + at, l);
        len[b] = l;
        at += l;
        const uint32_t mr = cap / 4 + 8;
        Arrays& a = arr[b];
        a.names.resize(cap);
        a.seq.resize(cap);
        a.qual.resize(cap);
        a.nl.resize(mr);
        a.sl.resize(mr);
        out[b] = sa_decoded{a.names.data(), a.nl.data(), a.seq.data(), a.sl.data(), a.qual.data(), cap, cap, mr, 0, 1};
    }
    sa_decode_info info{};
    std::string err;
    const int rc = sadec::dec_run(be, in.data(), len.data(), lng.data(), n, &cfg, tmpl, 2, out.data(), status.data(), kn, info, err);
    if (rc < 0) fprintf(stderr, "decoder_emu: %s\n", err.c_str());
    printf("%d %u %u %u %u %u %u %u\n", rc, info.groups, info.inflight, info.slice, info.qual_launches, info.seq_launches,
           info.unsupported, be.calls);
    for (uint32_t b = 0; b < n; b++) {
        printf("%u %d %u\n", status[b], (int)out[b].md5_ok, out[b].nreads);
        if (argc >= 5 && !status[b]) {
            const std::string p = std::string(argv[4]) + "/" + std::to_string(b);
            uint64_t names = 0, total = 0;
            for (uint32_t r = 0; r < out[b].nreads; r++) {
                names += out[b].name_lens[r];
                total += (uint64_t)out[b].seq_lens[r];
            }
            dump(p + ".names", out[b].names, names);
            dump(p + ".nl", out[b].name_lens, 2 * (size_t)out[b].nreads);
            dump(p + ".seq", out[b].seq, total);
            dump(p + ".sl", out[b].seq_lens, 4 * (size_t)out[b].nreads);
            dump(p + ".qual", out[b].qual, total);
        }
        free(in[b]);
    }
    return 0;
}
