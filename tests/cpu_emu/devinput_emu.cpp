// devinput_emu.cpp -- drives fastqueeze_amd/csrc/cli_devinput.h, the compressed
// input of seqarc_amd --gpu-text, without the library or a device: DevInput's file
// thread, its pump() and its takeover by the host are the command line's, and its
// library calls are host code: a devtext emulated as a heap block of exactly its
// capacity with a read and a write position and the library's room and
// move-to-the-front rule, sa_gunzip_run_dev as sa_gunzip.h's gz_run over
// gunzip_backend.h's EmuBackend (chunks of 4,096) writing at the write position,
// sa_inflate_members_dev as sa_inflate.h's infl_member per BGZF member.
// tests/test_devinput.py compares the text with zlib, in sanitizer builds too.
//
//   devinput_emu <file> bgzf|gzip <slab> <room> <capacity> <call_bytes> <append_bytes> <queue_cap> <want> <take>
//                <pump_limit> <outfile>
//     The sizes are GzStream's slab_bytes, gunzip_room and queue_cap and DevInput's
//     capacity, call_bytes and append_bytes.  As read_device does, the program pumps
//     the devtext to <want> bytes, then takes up to <take> bytes out of it into
//     <outfile>, until the input is used up; after <pump_limit> pumps (0: none) it
//     stops and destroys the input.  -v is on.  Prints "stats <calls> <members>
//     <host bytes> <moves>" and "final <ok|error|left> <text bytes>"; exit status 1
//     after an error, whose text goes to stderr behind "devinput_emu: ".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <vector>

#include "../../fastqueeze_amd/csrc/cli_devinput.h"
#include "gunzip_backend.h"

struct sa_inflater {
    sa::InflTabs tabs;
    uint32_t crc_tab[256];
    std::string err;
};
struct sa_gunzipper {
    std::string err;
};
struct sa_devtext {
    uint8_t* buf = nullptr;   // exactly cap bytes
    uint64_t cap = 0, rd = 0, wr = 0, moves = 0;
    std::string err;
};
static const uint32_t kChunk = 4096, kRatio = 8;

static sa_inflater* inflater_create(int)
{
    sa_inflater* f = new sa_inflater();
    for (uint32_t i = 0; i < 256; i++) f->crc_tab[i] = sa::crc32_entry(i);
    return f;
}

static uint64_t dt_room(const sa_devtext* dt) { return dt->cap - (dt->wr - dt->rd); }

// the library's dt_make_room: the unread bytes to the front when the room behind wr is too small
static int dt_make_room(sa_devtext* dt, uint64_t n)
{
    const uint64_t have = dt->wr - dt->rd;
    if (n > dt->cap - have) return -3;
    if (n <= dt->cap - dt->wr) return 0;
    memmove(dt->buf, dt->buf + dt->rd, have);
    dt->rd = 0;
    dt->wr = have;
    dt->moves++;
    return 0;
}

static int dt_append(sa_devtext* dt, const uint8_t* bytes, uint64_t n)
{
    if (dt_make_room(dt, n)) {
        dt->err = "sa_devtext_append: more bytes than sa_devtext_room";
        return -3;
    }
    memcpy(dt->buf + dt->wr, bytes, n);
    dt->wr += n;
    return 0;
}

// sa_inflate_members_dev: the members back to back from the write position, which moves only if all are good
static int inflate_members_dev(sa_inflater* f, const uint8_t* in, uint64_t in_bytes, const sa_bgzf_member* ms, uint32_t n,
                               sa_devtext* dt, uint32_t*)
{
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (ms[i].in_off > in_bytes || ms[i].in_len > in_bytes - ms[i].in_off || ms[i].isize > sa::INFL_MAX_ISIZE) {
            f->err = "sa_inflate_members_dev: member " + std::to_string(i) + " is out of range";
            return -2;
        }
        total += ms[i].isize;
    }
    if (dt_make_room(dt, total)) {
        f->err = "sa_inflate_members_dev: the members' text exceeds sa_devtext_room";
        return -3;
    }
    int failed = 0;
    uint64_t o = dt->wr;
    for (uint32_t i = 0; i < n; i++) {
        const sa_bgzf_member& m = ms[i];
        uint8_t dummy = 0;
        uint8_t* out = m.isize ? dt->buf + o : &dummy;
        o += m.isize;
        if (sa::infl_member(in + m.in_off, m.in_len, out, m.isize, f->tabs, 0, 1) != 0) {
            failed++;
            continue;
        }
        uint32_t crc = 0;
        if (m.isize) {
            uint32_t c = 0xffffffffu;
            for (uint32_t k = 0; k < m.isize; k++) c = f->crc_tab[(c ^ out[k]) & 0xffu] ^ (c >> 8);
            crc = ~c;
        }
        failed += crc != m.crc;
    }
    if (failed) return failed;
    dt->wr += total;
    return 0;
}

// sa_gunzip_run_dev: -3 above the room; room made; the text at the write position, which moves on 0 only
static int gunzip_run_dev(sa_gunzipper* g, const uint8_t* in, uint64_t in_bytes, int eof, sa_gunzip_state* st, sa_devtext* dt,
                          uint64_t out_cap, uint64_t* text_bytes, uint64_t* in_used, sa_gunzip_info* info)
{
    *text_bytes = 0;
    if (dt_make_room(dt, out_cap)) {
        g->err = "sa_gunzip_run_dev: out_cap exceeds sa_devtext_room";
        return -3;
    }
    sa::EmuBackend be;
    uint64_t text = 0;
    const int rc = sa::gz_run(be, in, in_bytes, eof, st, dt->buf + dt->wr, out_cap, &text, in_used, info, kChunk, kRatio, g->err);
    if (rc != 0) return rc;
    dt->wr += text;
    *text_bytes = text;
    return 0;
}

static const GzDevice kEmuDevice = {
    [](uint64_t n) { return malloc(n ? n : 1); },
    [](void* p) { free(p); },
    inflater_create,
    [](sa_inflater* f) { delete f; },
    [](const sa_inflater* f) { return f->err.c_str(); },
    [](const sa_inflater*) { return 0.0f; },
    nullptr,   // (sa_inflate_members: DevInput has no host output)
    [](int) { return new sa_gunzipper(); },
    [](sa_gunzipper* g) { delete g; },
    [](const sa_gunzipper*) { return kChunk; },
    [](const sa_gunzipper* g) { return g->err.c_str(); },
    nullptr,   // (sa_gunzip_run)
};

static const DevTextCalls kEmuText = {
    [](int, uint64_t cap) {
        sa_devtext* dt = new sa_devtext();
        dt->buf = static_cast<uint8_t*>(malloc(cap ? cap : 1));
        dt->cap = cap;
        return dt;
    },
    [](sa_devtext* dt) {
        free(dt->buf);
        delete dt;
    },
    [](const sa_devtext* dt) { return dt->wr - dt->rd; },
    dt_room,
    dt_append,
    [](const sa_devtext* dt) { return dt->err.c_str(); },
    [](const sa_devtext*, float* a, float* b) {
        if (a) *a = 0.f;
        if (b) *b = 0.f;
    },
    inflate_members_dev,
    gunzip_run_dev,
};

int main(int argc, char** argv)
{
    if (argc != 13) {
        fprintf(stderr, "usage: devinput_emu <file> bgzf|gzip <slab> <room> <capacity> <call_bytes> <append_bytes> <queue_cap> <want> "
                        "<take> <pump_limit> <outfile>\n");
        return 2;
    }
    auto num = [&](int i) { return strtoull(argv[i], nullptr, 10); };
    const int fd = open(argv[1], O_RDONLY);
    FILE* fo = fopen(argv[12], "wb");
    if (fd < 0 || !fo) return 2;
    const uint64_t want = num(9), take = num(10), pump_limit = num(11);
    uint64_t text = 0, pumps = 0;
    std::string err;
    bool ok = true, left = false;
    {
        DevInput d(kEmuDevice, kEmuText);
        d.gz.verbose = true;
        d.gz.slab_bytes = num(3);
        d.gz.gunzip_room = num(4);
        d.capacity = num(5);
        d.call_bytes = num(6);
        d.append_bytes = num(7);
        d.gz.queue_cap = num(8);
        ok = d.start(fd, argv[1], 0, std::string(argv[2]) == "bgzf" ? DevInput::BGZF : DevInput::GZIP, err);
        while (ok) {
            if (pump_limit && pumps == pump_limit) {
                left = true;
                break;
            }
            pumps++;
            if (!d.pump(want, err)) {
                ok = false;
                break;
            }
            const uint64_t avail = d.dt->wr - d.dt->rd;
            if (!avail && d.eof) break;
            if (avail < want && !d.eof) {
                err = "pump returned short of the window";
                ok = false;
                break;
            }
            const uint64_t k = std::min(avail, take);
            fwrite(d.dt->buf + d.dt->rd, 1, (size_t)k, fo);
            d.dt->rd += k;
            text += k;
        }
        d.close();
        if (d.dt) {
            d.say(0.0, 0, 0, 0.0);
            printf("stats %llu %llu %llu %llu\n", (unsigned long long)d.calls, (unsigned long long)d.members,
                   (unsigned long long)d.host_bytes, (unsigned long long)d.dt->moves);
        }
    }   // (the input's destructor: the file thread and the host's have ended)
    fclose(fo);
    close(fd);
    if (!ok) fprintf(stderr, "devinput_emu: %s\n", err.c_str());
    printf("final %s %llu\n", !ok ? "error" : left ? "left" : "ok", (unsigned long long)text);
    return ok ? 0 : 1;
}
