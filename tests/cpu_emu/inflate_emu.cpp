// inflate_emu.cpp -- drives fastqueeze_amd/csrc/sa_inflate.h on the host, one
// member after the other, the way k_inflate_bgzf drives it one wave per member
// (tests/test_inflate.py compares every line with zlib).
//
//   inflate_emu members <file> [outdir]
//     file: u32 n, then per member u32 in_len, u32 isize, u32 crc and in_len
//     bytes.  Prints per member "<status> <crc of the output, serial> <crc from
//     the 64 lane shares>"; with outdir, member i's output goes to outdir/i.
//     Each member's input and output live in heap blocks of exactly their
//     sizes, so a sanitizer build sees any access outside them.
//   inflate_emu scan <file> <max_members> [max_isize]
//     sa_bgzf_scan's walk over the file: "<ret> <consumed> <out_bytes>", then
//     per member "<in_off> <in_len> <out_off> <isize> <crc>".  max_isize: the
//     walk's limit on a member's ISIZE (default: sa_bgzf_scan's, 65536).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fastqueeze_amd/csrc/sa_inflate.h"

using namespace sa;

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "inflate_emu: cannot open %s\n", path);
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
        fprintf(stderr, "inflate_emu: short file\n");
        exit(2);
    }
    return v[at] | v[at + 1] << 8 | v[at + 2] << 16 | (uint32_t)v[at + 3] << 24;
}

int main(int argc, char** argv)
{
    if (argc >= 4 && !strcmp(argv[1], "scan")) {
        const std::vector<uint8_t> f = slurp(argv[2]);
        const uint64_t maxm = strtoull(argv[3], nullptr, 10);
        std::vector<sa_bgzf_member> ms(maxm);
        uint64_t consumed = 0, out_bytes = 0;
        const uint32_t max_isize = argc >= 5 ? (uint32_t)strtoul(argv[4], nullptr, 10) : INFL_MAX_ISIZE;
        const int64_t n = bgzf_scan(f.data(), f.size(), ms.data(), maxm, &consumed, &out_bytes, max_isize);
        printf("%lld %llu %llu\n", (long long)n, (unsigned long long)consumed, (unsigned long long)out_bytes);
        for (int64_t i = 0; i < n; i++)
            printf("%llu %u %llu %u %u\n", (unsigned long long)ms[i].in_off, ms[i].in_len,
                   (unsigned long long)ms[i].out_off, ms[i].isize, ms[i].crc);
        return 0;
    }
    if (argc < 3 || strcmp(argv[1], "members")) {
        fprintf(stderr, "usage: inflate_emu members <file> [outdir] | scan <file> <max_members> [max_isize]\n");
        return 2;
    }
    const std::vector<uint8_t> f = slurp(argv[2]);
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256; i++) tab[i] = crc32_entry(i);
    uint32_t shift[64];
    for (uint32_t k = 0; k < 64; k++) shift[k] = crc32_chunk_shift(63 - k);
    InflTabs* t = new InflTabs;
    const uint32_t n = rd32(f, 0);
    size_t at = 4;
    for (uint32_t m = 0; m < n; m++) {
        const uint32_t in_len = rd32(f, at), isize = rd32(f, at + 4), crc = rd32(f, at + 8);
        at += 12;
        if (at + in_len > f.size() || isize > INFL_MAX_ISIZE) {
            fprintf(stderr, "inflate_emu: bad member %u\n", m);
            return 2;
        }
        uint8_t* in = (uint8_t*)malloc(in_len ? in_len : 1);
        uint8_t* out = (uint8_t*)malloc(isize);   // (an empty member's block has no byte: any store into it is reported)
        memcpy(in, f.data() + at, in_len);
        memset(out, 0xa5, isize);
        at += in_len;
        memset(t, 0xff, sizeof *t);   // (no table state carries over between members)
        uint32_t st, serial = 0, shares = 0;
        if (isize == 0) {   // (k_inflate_bgzf: inflated like any other, into no room)
            st = infl_member(in, in_len, out, 0, *t, 0, 1);
            if (st == 0 && crc) st = SA_INFL_CRC;
        } else {
            st = infl_member(in, in_len, out, isize, *t, 0, 1);
            if (st == 0) {
                uint32_t c = 0xffffffffu;
                for (uint32_t i = 0; i < isize; i++) c = tab[(c ^ out[i]) & 0xffu] ^ (c >> 8);
                serial = ~c;
                uint32_t x = 0;
                for (uint32_t k = 0; k < 64; k++) x ^= crc32_share(out, isize, k, shift[k], tab);
                shares = ~x;
                if (shares != crc) st = SA_INFL_CRC;
            }
        }
        printf("%u %08x %08x\n", st, serial, shares);
        if (argc >= 4 && (st == 0 || st == SA_INFL_CRC) && isize) {
            const std::string p = std::string(argv[3]) + "/" + std::to_string(m);
            FILE* o = fopen(p.c_str(), "wb");
            if (!o || fwrite(out, 1, isize, o) != isize) return 2;
            fclose(o);
        }
        free(in);
        free(out);
    }
    delete t;
    return 0;
}
