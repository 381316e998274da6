// gunzip_backend.h -- gz_run's backend on the host, for gunzip_emu.cpp and
// gzstream_emu.cpp: the finder, the speculative waves, the chain, the resolve
// and the CRC of fastqueeze_amd/csrc/sa_gunzip.h one after the other (lane 0 of
// 1), the way sa_gunzip.hip's kernels drive them one wave per chunk.  Every
// wave's symbol range is a heap block of exactly its size, so a sanitizer build
// sees any access outside it.
#pragma once
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastqueeze_amd/csrc/sa_gunzip.h"

namespace sa {

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

}  // namespace sa
