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

#include "gunzip_backend.h"

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
