// gunzip_emu.cpp -- drives fastqueeze_amd/csrc/sa_gunzip.h on the host: the
// finder, the speculative waves, the chain, the resolve and the CRC one after
// the other (lane 0 of 1), through the same gz_run that sa_gunzip_run is, the
// way sa_gunzip.hip's kernels drive them one wave per chunk
// (tests/test_gunzip.py compares the text with zlib).
//
//   gunzip_emu run <file> <chunk> <ratio> <slab> <out_cap> <outfile> [statefile]
//     Feeds the gzip file in slabs of <slab> compressed bytes (0: the whole
//     file), carrying what a call leaves unconsumed into the next, and appends
//     every call's text to <outfile>.  Prints per call
//       call <rc> <in_bytes> <in_used> <out_bytes> <chunks> <candidates> <confirmed>
//            <false_skipped> <members> <end_wave> <end_why> <late_markers>
//     (late_markers: markers at symbol 32768 or later of a confirmed wave) and
//       final <rc> <text bytes> <file bytes consumed> <end|handover|error|stuck>
//     handover: a call with at least two chunks confirmed less than one chunk,
//     or made no progress at the end of the file; the state goes to <statefile>:
//     u32 in_stream, bit, win_len, crc; u64 len; the 32768 window bytes.
//     The input of a call, its output and every wave's symbol range live in heap
//     blocks of exactly their sizes, so a sanitizer build sees any access
//     outside them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastqueeze_amd/csrc/sa_gunzip.h"

using namespace sa;

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "gunzip_emu: cannot open %s\n", path);
        exit(2);
    }
    uint8_t buf[1 << 16];
    size_t r;
    while ((r = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + r);
    fclose(f);
    return v;
}

struct EmuBackend {
    const uint8_t* in = nullptr;
    uint32_t in_len = 0;
    const sa_gunzip_state* st = nullptr;
    std::vector<uint8_t> win;                   // nw + 1 slots
    std::vector<uint16_t*> sym;                 // one heap block per wave, exactly its range
    uint16_t* ring = nullptr;
    InflTabs tabs;
    uint32_t crc_tab[256];
    uint64_t late_markers = 0;
    EmuBackend()
    {
        ring = static_cast<uint16_t*>(aligned_alloc(16, GZ_RING * 2));
        for (uint32_t i = 0; i < 256; i++) crc_tab[i] = crc32_entry(i);
    }
    ~EmuBackend()
    {
        free_sym();
        free(ring);
    }
    void free_sym()
    {
        for (uint16_t* p : sym) free(p);
        sym.clear();
    }
    bool upload(const uint8_t* i, uint32_t n, const sa_gunzip_state* s)
    {
        in = i;
        in_len = n;
        st = s;
        return true;
    }
    bool find(uint32_t nchunks, uint32_t chunk, uint32_t* cand)
    {
        for (uint32_t k = 1; k < nchunks; k++) {
            const uint64_t to = std::min<uint64_t>((uint64_t)(k + 1) * chunk, in_len) * 8;
            cand[k] = gz_find_first(in, in_len, k * chunk * 8, (uint32_t)to, tabs, 0, 1);
        }
        return true;
    }
    std::vector<GzWaveRes> res;
    bool spec(const GzPlan& p, bool at_header, uint32_t win_len)
    {
        const size_t nw = p.starts.size();
        win.assign((nw + 1) * (size_t)GZ_RING, 0);
        memcpy(win.data(), st->window, GZ_RING);
        res.assign(nw, GzWaveRes{});
        free_sym();
        for (size_t j = 0; j < nw; j++) {
            sym.push_back(static_cast<uint16_t*>(aligned_alloc(16, (size_t)p.cap[j] * 2)));
            gz_wave(in, in_len, p.starts.data(), (uint32_t)nw, (uint32_t)j, j == 0, j == 0 && at_header, win.data(), win_len, ring,
                    tabs, sym[j], p.cap[j], &res[j], 0, 1);
        }
        return true;
    }
    bool chain(const GzPlan& p, uint32_t win_len, uint64_t out_cap, bool first_header, GzChainEnd& e, std::vector<uint32_t>& order,
               std::vector<uint64_t>& woff, std::vector<uint32_t>& wwl, std::vector<GzWaveRes>& r)
    {
        const uint32_t nw = (uint32_t)p.starts.size();
        e = GzChainEnd{};
        uint32_t j = 0, wl = win_len;
        for (;;) {
            GzChainStep s{};
            const uint64_t off = e.text;
            if (!gz_chain_step(res[j], j, nw, p.starts.data(), wl, out_cap, first_header, e, s)) break;
            order.push_back(j);
            woff.push_back(off);
            wwl.push_back(wl);
            gz_window_next(win.data() + (size_t)j * GZ_RING, sym[j], res[j].lb_sym, win.data() + (size_t)s.next_slot * GZ_RING, 0, 1);
            if (s.last) break;
            j = s.next_slot;
            wl = s.next_len;
        }
        r = res;
        return true;
    }
    bool resolve(const GzPlan&, const std::vector<uint32_t>& order, const std::vector<uint64_t>& woff,
                 const std::vector<uint32_t>& wwl, const std::vector<GzWaveRes>& r, uint8_t* out, uint64_t)
    {
        for (size_t k = 0; k < order.size(); k++) {
            const uint32_t j = order[k];
            for (uint32_t i = 0; i < r[j].lb_sym; i++) {
                const uint16_t s = sym[j][i];
                if (s >= 256 && i >= GZ_RING) late_markers++;
                out[woff[k] + i] = gz_resolve_sym(s, win.data() + (size_t)j * GZ_RING, wwl[k], bad);
            }
        }
        return true;
    }
    bool crc(const std::vector<GzAccount::Task>& tasks, const uint8_t* out, std::vector<uint32_t>& crcs)
    {
        for (size_t i = 0; i < tasks.size(); i++) crcs[i] = gz_crc_task(out + tasks[i].off, tasks[i].len, crc_tab);
        return true;
    }
    bool window(uint32_t slot, uint8_t* dst)
    {
        memcpy(dst, win.data() + (size_t)slot * GZ_RING, GZ_RING);
        return true;
    }
    bool bad = false;
    bool finish(sa_gunzip_info&, bool& b)
    {
        b = bad;
        return true;
    }
};

int main(int argc, char** argv)
{
    if (argc < 8 || strcmp(argv[1], "run")) {
        fprintf(stderr, "usage: gunzip_emu run <file> <chunk> <ratio> <slab> <out_cap> <outfile> [statefile]\n");
        return 2;
    }
    const std::vector<uint8_t> file = slurp(argv[2]);
    const uint32_t chunk = (uint32_t)strtoul(argv[3], nullptr, 10), ratio = (uint32_t)strtoul(argv[4], nullptr, 10);
    const size_t slab = strtoull(argv[5], nullptr, 10) ? strtoull(argv[5], nullptr, 10) : file.size() + 1;
    const uint64_t out_cap = strtoull(argv[6], nullptr, 10);
    FILE* fo = fopen(argv[7], "wb");
    if (!fo || !chunk) return 2;
    sa_gunzip_state* st = new sa_gunzip_state();
    std::vector<uint8_t> carry;
    size_t at = 0;
    uint64_t text = 0;
    int rc = 0;
    const char* how = "end";
    for (;;) {
        const size_t take = std::min(slab, file.size() - at);
        const size_t n = carry.size() + take;
        uint8_t* in = new uint8_t[n ? n : 1];
        if (!carry.empty()) memcpy(in, carry.data(), carry.size());
        if (take) memcpy(in + carry.size(), file.data() + at, take);
        at += take;
        const int eof = at == file.size();
        uint8_t* out = new uint8_t[out_cap ? out_cap : 1];
        uint64_t out_bytes = 0, in_used = 0;
        sa_gunzip_info info{};
        std::string err;
        EmuBackend be;
        rc = gz_run(be, in, n, eof, st, out, out_cap, &out_bytes, &in_used, &info, chunk, ratio, err);
        printf("call %d %zu %llu %llu %u %u %u %u %u %u %u %llu\n", rc, n, (unsigned long long)in_used, (unsigned long long)out_bytes,
               info.chunks, info.candidates, info.waves_confirmed, info.false_skipped, info.members_ended, info.end_wave,
               info.end_why, (unsigned long long)be.late_markers);
        if (out_bytes > out_cap || in_used > n) {
            fprintf(stderr, "gunzip_emu: the call reports more than it was given\n");
            return 3;
        }
        fwrite(out, 1, out_bytes, fo);
        text += out_bytes;
        carry.assign(in + in_used, in + n);
        delete[] in;
        delete[] out;
        if (rc) {
            how = "error";
            if (rc < 0) fprintf(stderr, "gunzip_emu: %s\n", err.c_str());
            break;
        }
        if (st->ended || (eof && carry.empty())) break;
        if ((info.chunks >= 2 && in_used < chunk) || (eof && !in_used && !out_bytes)) {
            how = "handover";
            break;
        }
        if (!take && !in_used && !out_bytes) {   // (cannot happen: no progress at the end of the file is a handover)
            how = "stuck";
            break;
        }
    }
    fclose(fo);
    printf("final %d %llu %llu %s\n", rc, (unsigned long long)text, (unsigned long long)(at - carry.size()), how);
    if (argc > 8) {
        FILE* fs = fopen(argv[8], "wb");
        if (!fs) return 2;
        const uint32_t h[4] = {st->in_stream, st->bit, st->win_len, st->crc};
        fwrite(h, 4, 4, fs);
        fwrite(&st->len, 8, 1, fs);
        fwrite(st->window, 1, GZ_RING, fs);
        fclose(fs);
    }
    delete st;
    return 0;
}
