// gzstream_emu.cpp -- drives fastqueeze_amd/csrc/cli_gzstream.h, the gzip input
// of seqarc_amd, without the library or a device: GzStream's threads, queues and
// shutdown paths are the command line's, and its device calls are host code
// (malloc for the page-locked memory, sa_inflate.h's infl_member per BGZF
// member, sa_gunzip.h's gz_run over gunzip_backend.h's EmuBackend in chunks of
// 4,096) (tests/test_gzstream.py compares the text with zlib, in sanitizer
// builds too).
//
//   gzstream_emu <file> <mode> <workers> <slab> <in_flight> <room> <out_cap> <queue_cap> <read_limit> <outfile>
//     mode: host | dev-inflate | dev-gunzip | both (gpu_device / gunzip_device as
//     --gpu-inflate / --gpu-gunzip set them); -v is on.  The sizes are
//     GzStream's slab_bytes, slabs_in_flight, gunzip_room, out_cap and
//     queue_cap.  Reads the text through GzStream::read in odd-sized requests
//     into <outfile>; after <read_limit> requests (0: none) it stops reading and
//     destroys the stream.  Prints "final <ok|error|left> <text bytes>"; exit
//     status 1 after an error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <vector>

#include "../../fastqueeze_amd/csrc/cli_gzstream.h"
#include "gunzip_backend.h"

struct sa_inflater {
    sa::InflTabs tabs;
    uint32_t crc_tab[256];
    std::string err;
};
struct sa_gunzipper {
    std::string err;
};
static const uint32_t kChunk = 4096, kRatio = 8;

static sa_inflater* inflater_create(int)
{
    sa_inflater* f = new sa_inflater();
    for (uint32_t i = 0; i < 256; i++) f->crc_tab[i] = sa::crc32_entry(i);
    return f;
}

// sa_inflate_members: the descriptor checks, then one member after the other
static int inflate_members(sa_inflater* f, const uint8_t* in, uint64_t in_bytes, const sa_bgzf_member* ms, uint32_t n, uint8_t* out,
                           uint64_t out_bytes, uint32_t*)
{
    for (uint32_t i = 0; i < n; i++)
        if (ms[i].in_off > in_bytes || ms[i].in_len > in_bytes - ms[i].in_off || ms[i].out_off > out_bytes ||
            ms[i].isize > out_bytes - ms[i].out_off || ms[i].isize > sa::INFL_MAX_ISIZE) {
            f->err = "sa_inflate_members: member " + std::to_string(i) + " is out of range";
            return -1;
        }
    int failed = 0;
    for (uint32_t i = 0; i < n; i++) {
        const sa_bgzf_member& m = ms[i];
        uint8_t* o = out + m.out_off;
        uint32_t crc = 0;
        // (an empty member is inflated like any other: good only if its stream ends having produced nothing)
        if (sa::infl_member(in + m.in_off, m.in_len, o, m.isize, f->tabs, 0, 1) != 0) {
            failed++;
            continue;
        }
        if (m.isize) {
            uint32_t c = 0xffffffffu;
            for (uint32_t k = 0; k < m.isize; k++) c = f->crc_tab[(c ^ o[k]) & 0xffu] ^ (c >> 8);
            crc = ~c;
        }
        failed += crc != m.crc;
    }
    return failed;
}

static int gunzip_run(sa_gunzipper* g, const uint8_t* in, uint64_t in_bytes, int eof, sa_gunzip_state* st, uint8_t* out,
                      uint64_t out_cap, uint64_t* out_bytes, uint64_t* in_used, sa_gunzip_info* info)
{
    sa::EmuBackend be;
    return sa::gz_run(be, in, in_bytes, eof, st, out, out_cap, out_bytes, in_used, info, kChunk, kRatio, g->err);
}

static const GzDevice kEmuDevice = {
    [](uint64_t n) { return malloc(n ? n : 1); },
    [](void* p) { free(p); },
    inflater_create,
    [](sa_inflater* f) { delete f; },
    [](const sa_inflater* f) { return f->err.c_str(); },
    [](const sa_inflater*) { return 0.0f; },
    inflate_members,
    [](int) { return new sa_gunzipper(); },
    [](sa_gunzipper* g) { delete g; },
    [](const sa_gunzipper*) { return kChunk; },
    [](const sa_gunzipper* g) { return g->err.c_str(); },
    gunzip_run,
};

int main(int argc, char** argv)
{
    if (argc != 11) {
        fprintf(stderr, "usage: gzstream_emu <file> host|dev-inflate|dev-gunzip|both <workers> <slab> <in_flight> <room> <out_cap> "
                        "<queue_cap> <read_limit> <outfile>\n");
        return 2;
    }
    const std::string mode = argv[2];
    const int fd = open(argv[1], O_RDONLY);
    FILE* fo = fopen(argv[10], "wb");
    if (fd < 0 || !fo) return 2;
    const uint64_t read_limit = strtoull(argv[9], nullptr, 10);
    uint64_t text = 0, reads = 0;
    long r = 0;
    {
        GzStream gz(kEmuDevice);
        gz.gpu_device = mode == "dev-inflate" || mode == "both" ? 0 : -1;
        gz.gunzip_device = mode == "dev-gunzip" || mode == "both" ? 0 : -1;
        gz.verbose = true;
        gz.name = argv[1];
        gz.slab_bytes = strtoull(argv[4], nullptr, 10);
        gz.slabs_in_flight = strtoull(argv[5], nullptr, 10);
        gz.gunzip_room = strtoull(argv[6], nullptr, 10);
        gz.out_cap = strtoull(argv[7], nullptr, 10);
        gz.queue_cap = strtoull(argv[8], nullptr, 10);
        gz.start(fd, atoi(argv[3]));
        static const size_t kAsk[] = {7, 4099, 65521, 300007, 1};
        std::vector<uint8_t> buf(300007);
        while (!read_limit || reads < read_limit) {
            r = gz.read(buf.data(), kAsk[reads++ % 5]);
            if (r <= 0) break;
            fwrite(buf.data(), 1, (size_t)r, fo);
            text += (uint64_t)r;
        }
    }   // (the stream's destructor: the reader goes away, the producer's threads end)
    fclose(fo);
    close(fd);
    printf("final %s %llu\n", r < 0 ? "error" : r == 0 ? "ok" : "left", (unsigned long long)text);
    return r < 0 ? 1 : 0;
}
