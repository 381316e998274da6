// devcut_emu.cpp -- CPU emulation of the device block cut (sa_devcut.h) and of
// the devtext's buffer around it, checked against the host cut.
//
// Stand-alone (g++, links fastqueeze_amd/csrc/fastq_host.cpp):
//   devcut_emu f1 f2|- block_size piece cap max_blocks eof [nocarry]
// The inputs are fed `piece` bytes at a time into one buffer of `cap` bytes per
// input (0: the input's size) that works as sa_devtext does: append at the
// write position, the unread bytes moved to the front when the room behind it
// runs out, one newline count per 4 KiB tile taken with k_dt_count's function.
// After every round of appends dc_cut_blocks -- the function k_dt_cut runs,
// here with the wave's lanes as a loop -- cuts at most max_blocks blocks, and
// every length and the reason it stopped are compared with repeated
// sa_cut_next_se / sa_cut_next_pe on the same bytes with the same avail and
// eof.  eof = 0: the inputs never count as ended (a reader in mid-file).
// Output: "B len1 len2" per block, "E end" per cut call, "end <why> blocks <n>";
// with nocarry also "NOCARRY ..." lines: the first call's answer if the match
// counter were reset at every candidate.  Exit 1 on any difference.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastqueeze_amd/csrc/sa_devcut.h"

using namespace sa;

namespace {

std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

struct EmuText {   // sa_devtext on the host
    uint8_t* buf = nullptr;
    std::vector<uint32_t> tiles;
    uint64_t cap = 0, rd = 0, wr = 0;
    uint64_t moves = 0;
    explicit EmuText(uint64_t c) : cap(c)
    {
        if (posix_memalign((void**)&buf, 16, cap + 32) != 0) std::exit(2);
        std::memset(buf, 0, cap + 32);
        tiles.assign(cap / DC_TILE + 2, 0);
    }
    ~EmuText() { std::free(buf); }
    void count(uint64_t lo, uint64_t hi)   // k_dt_count over the tiles of [lo, hi), the text ending at hi
    {
        if (lo >= hi) return;
        for (uint64_t t = lo / DC_TILE; t < (hi + DC_TILE - 1) / DC_TILE; t++) {
            uint32_t n = 0;
            for (uint32_t th = 0; th < 256; th++) n += dc_tile_thread_count(buf, t, hi, th);
            tiles.at(t) = n;
        }
    }
    uint64_t room() const { return cap - (wr - rd); }
    void append(const uint8_t* p, uint64_t n)
    {
        if (n > room()) std::exit(3);
        if (n > cap - wr) {
            std::memmove(buf, buf + rd, wr - rd);
            wr -= rd;
            rd = 0;
            ++moves;
            count(0, wr);
        }
        std::memcpy(buf + wr, p, n);
        count(wr, wr + n);
        wr += n;
    }
    DcSide side(bool eof) const { return DcSide{buf, tiles.data(), rd, wr, eof ? 1 : 0, 0}; }
};

size_t first_line_len(const std::vector<uint8_t>& t)
{
    const void* nl = std::memchr(t.data(), '\n', t.size());
    return nl ? (size_t)((const uint8_t*)nl - t.data()) + 1 : t.size();
}

// the host cut, block after block, on the same windows
uint32_t ref_cut(const EmuText& a, bool eof1, const EmuText* b, bool eof2, uint64_t bs, const uint8_t* first, uint64_t flen,
                 std::vector<uint64_t>& l1, std::vector<uint64_t>& l2, uint32_t max_blocks, int32_t* end)
{
    uint64_t p1 = a.rd, p2 = b ? b->rd : 0;
    uint32_t nb = 0;
    for (;;) {
        const uint64_t av1 = a.wr - p1, av2 = b ? b->wr - p2 : 0;
        if (b ? (av1 == 0 && av2 == 0 && eof1 && eof2) : (av1 == 0 && eof1)) {
            *end = SA_CUT_DONE;
            return nb;
        }
        if (nb >= max_blocks) {
            *end = SA_CUT_FULL;
            return nb;
        }
        uint64_t e1 = 0, e2 = 0;
        if (!b) {
            const int64_t r = sa_cut_next_se(a.buf + p1, av1, eof1, bs, first, flen);
            if (r < 0) {
                *end = av1 < bs && !eof1 ? SA_CUT_MORE : SA_CUT_NONE;
                return nb;
            }
            e1 = (uint64_t)r;
        } else {
            const uint64_t half = (uint64_t)((uint32_t)bs >> 1);
            if (sa_cut_next_pe(a.buf + p1, av1, eof1, b->buf + p2, av2, eof2, bs, first, flen, &e1, &e2) != 0) {
                *end = (av1 < half && !eof1) || (av2 < half && !eof2) ? SA_CUT_MORE : SA_CUT_NONE;
                return nb;
            }
        }
        l1.push_back(e1);
        l2.push_back(e2);
        p1 += e1;
        p2 += e2;
        ++nb;
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: devcut_emu f1 f2|- block_size piece cap max_blocks eof [nocarry]\n");
        return 2;
    }
    const std::vector<uint8_t> in1 = slurp(argv[1]);
    const bool pe = std::strcmp(argv[2], "-") != 0;
    const std::vector<uint8_t> in2 = pe ? slurp(argv[2]) : std::vector<uint8_t>();
    const uint64_t bs = std::strtoull(argv[3], nullptr, 10);
    uint64_t piece = std::strtoull(argv[4], nullptr, 10);
    const uint64_t cap_arg = std::strtoull(argv[5], nullptr, 10);
    const uint32_t max_blocks = (uint32_t)std::strtoul(argv[6], nullptr, 10);
    const bool eof_at_end = std::atoi(argv[7]) != 0;
    const bool nocarry = argc > 8 && std::strcmp(argv[8], "nocarry") == 0;
    if (!piece) piece = std::max<uint64_t>(1, std::max(in1.size(), in2.size()));
    if (!bs || (pe && bs < 2) || !max_blocks) return 2;

    EmuText t1(cap_arg ? cap_arg : std::max<uint64_t>(in1.size(), 1)), t2(cap_arg ? cap_arg : std::max<uint64_t>(in2.size(), 1));
    const size_t flen = first_line_len(in1);
    std::vector<uint8_t> first(in1.begin(), in1.begin() + (long)flen);
    first.push_back(0);
    if (!flen) return 2;

    const DcLoopLanes ln;
    uint64_t fed1 = 0, fed2 = 0, total = 0;
    std::vector<uint64_t> len1(max_blocks), len2(max_blocks);
    int32_t end = 0;
    bool first_call = true;
    for (;;) {
        uint64_t progress = 0;
        auto feed = [&](EmuText& t, const std::vector<uint8_t>& in, uint64_t& fed) {
            const uint64_t n = std::min<uint64_t>({piece, in.size() - fed, t.room()});
            if (n) t.append(in.data() + fed, n);
            fed += n;
            progress += n;
        };
        feed(t1, in1, fed1);
        if (pe) feed(t2, in2, fed2);
        const bool eof1 = eof_at_end && fed1 == in1.size(), eof2 = eof_at_end && fed2 == in2.size();
        for (;;) {   // cut until the text on hand is used up
            const uint32_t nb = dc_cut_blocks(ln, t1.side(eof1), pe ? t2.side(eof2) : t1.side(eof1), pe, bs, first.data(), flen,
                                              len1.data(), len2.data(), max_blocks, &end);
            std::vector<uint64_t> r1, r2;
            int32_t rend = 0;
            const uint32_t rn = ref_cut(t1, eof1, pe ? &t2 : nullptr, eof2, bs, first.data(), flen, r1, r2, max_blocks, &rend);
            if (nb != rn || end != rend) {
                std::fprintf(stderr, "MISMATCH: %u blocks end %d, the host cut gives %u blocks end %d (after block %llu)\n", nb,
                             end, rn, rend, (unsigned long long)total);
                return 1;
            }
            for (uint32_t i = 0; i < nb; i++)
                if (len1[i] != r1[i] || (pe && len2[i] != r2[i])) {
                    std::fprintf(stderr, "MISMATCH at block %llu: %llu / %llu, the host cut gives %llu / %llu\n",
                                 (unsigned long long)(total + i), (unsigned long long)len1[i], (unsigned long long)len2[i],
                                 (unsigned long long)r1[i], (unsigned long long)r2[i]);
                    return 1;
                }
            if (nocarry && first_call) {
                std::vector<uint64_t> n1(max_blocks), n2(max_blocks);
                int32_t nend = 0;
                const uint32_t nn = dc_cut_blocks(ln, t1.side(eof1), pe ? t2.side(eof2) : t1.side(eof1), pe, bs, first.data(),
                                                  flen, n1.data(), n2.data(), max_blocks, &nend, false);
                for (uint32_t i = 0; i < nn; i++)
                    std::printf("NOCARRY B %llu %llu\n", (unsigned long long)n1[i], (unsigned long long)n2[i]);
                std::printf("NOCARRY E %d\n", nend);
            }
            first_call = false;
            for (uint32_t i = 0; i < nb; i++) {   // sa_devtext_take
                std::printf("B %llu %llu\n", (unsigned long long)len1[i], (unsigned long long)len2[i]);
                t1.rd += len1[i];
                t2.rd += len2[i];
            }
            std::printf("E %d\n", end);
            total += nb;
            progress += nb;
            if (end != SA_CUT_FULL) break;
        }
        if (end == SA_CUT_DONE || end == SA_CUT_NONE || !progress) break;
    }
    std::printf("end %d blocks %llu moves %llu rd %llu %llu\n", end, (unsigned long long)total,
                (unsigned long long)(t1.moves + t2.moves), (unsigned long long)t1.rd, (unsigned long long)t2.rd);
    return 0;
}
