// cli_gzstream.h -- the gzip input of seqarc_amd -c (host C++; no device header).
//
// The reference inflates with gzread on its reader thread.  Here a producer
// thread per input inflates ahead of the block cut into a bounded queue of
// chunks (GzQueue).  BGZF files (bgzip: gzip members of <= 64 KiB with the 'BC'
// extra field giving each member's size) are inflated in parallel: the producer
// reads a slab of members (BgzfReader), `workers` threads inflate them into
// their places (each member's ISIZE gives its output size) and check their CRCs
// (run_bgzf), or the first device does (--gpu-inflate: run_bgzf_gpu).  Other
// gzip files (one member, or several concatenated) inflate on the producer
// thread (run_plain), or on the first device by speculation (--gpu-gunzip:
// run_plain_gpu, which hands the rest of a file it cannot spread over waves to
// run_host_from).
//
// The two device paths are two loops over the same two parts: a SlabFeed (the
// reader thread publishes page-locked input slabs in file order, the device
// thread works on the oldest and retires it) and an OutPair (the device thread
// fills one of two page-locked output slabs while a copier thread copies the
// other into the queue's chunk).  Their device calls go through GzDevice, so
// that tests/cpu_emu/gzstream_emu.cpp drives all of this without the library.
// What a gunzip loop does after a call is gz_after_call, which --gpu-text's
// gzip input (cli_devinput.h) follows too.
#pragma once
#include <dlfcn.h>
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/resource.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/seqarc_amd.h"
#include "sa_inflate.h"

// byte buffers that resize without zero-filling (filled right after)
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U>&) noexcept {}
    template <class U>
    void construct(U* p) noexcept
    {
        ::new ((void*)p) U;
    }
    template <class U, class... A>
    void construct(U* p, A&&... a)
    {
        ::new ((void*)p) U(std::forward<A>(a)...);
    }
};
using Bytes = std::vector<uint8_t, NoInitAlloc<uint8_t>>;

// BGZF members are whole raw-deflate streams of known output size: the
// system's libdeflate (whole-buffer decompression, PCLMUL CRC-32) inflates them
// at several times zlib 1.2.11's rate.  It is loaded at run time; without it
// the members go through zlib as before.  (Declared here: the image has the
// library but no header; these four entry points are libdeflate's stable API.)
struct LibDeflate {
    void* (*alloc)() = nullptr;
    int (*decompress)(void*, const void*, size_t, void*, size_t, size_t*) = nullptr;
    void (*release)(void*) = nullptr;
    uint32_t (*crc32)(uint32_t, const void*, size_t) = nullptr;
    LibDeflate()
    {
        if (std::getenv("SA_NO_LIBDEFLATE")) return;   // (A/B)
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = reinterpret_cast<void* (*)()>(dlsym(h, "libdeflate_alloc_decompressor"));
        decompress = reinterpret_cast<int (*)(void*, const void*, size_t, void*, size_t, size_t*)>(
            dlsym(h, "libdeflate_deflate_decompress"));
        release = reinterpret_cast<void (*)(void*)>(dlsym(h, "libdeflate_free_decompressor"));
        crc32 = reinterpret_cast<uint32_t (*)(uint32_t, const void*, size_t)>(dlsym(h, "libdeflate_crc32"));
        if (!alloc || !decompress || !release || !crc32) alloc = nullptr;
    }
    bool ok() const { return alloc != nullptr; }
};
inline const LibDeflate& libdeflate()
{
    static const LibDeflate d;
    return d;
}

// Inflate threads run at a lower priority than the encoder threads: those
// sleep on their streams and wake for a few host steps per batch, and with
// every core inflating they woke late (BGZF short leg, r4i: encode busy 14.3 s
// against 7.1 s on plain input).
inline void lower_priority()
{
    (void)setpriority(PRIO_PROCESS, (id_t)syscall(SYS_gettid), 5);
}

// The library calls of the two device paths (seqarc_amd.h has their contracts).
// The command line fills this with the library's functions, a test with host code.
struct GzDevice {
    void* (*host_alloc)(uint64_t);
    void (*host_free)(void*);
    sa_inflater* (*inflater_create)(int);
    void (*inflater_destroy)(sa_inflater*);
    const char* (*inflater_error)(const sa_inflater*);
    float (*inflater_kernel_ms)(const sa_inflater*);
    int (*inflate_members)(sa_inflater*, const uint8_t*, uint64_t, const sa_bgzf_member*, uint32_t, uint8_t*, uint64_t, uint32_t*);
    sa_gunzipper* (*gunzipper_create)(int);
    void (*gunzipper_destroy)(sa_gunzipper*);
    uint32_t (*gunzipper_chunk)(const sa_gunzipper*);
    const char* (*gunzipper_error)(const sa_gunzipper*);
    int (*gunzip_run)(sa_gunzipper*, const uint8_t*, uint64_t, int, sa_gunzip_state*, uint8_t*, uint64_t, uint64_t*, uint64_t*,
                      sa_gunzip_info*);
};

using GzTime = std::chrono::steady_clock::time_point;
inline GzTime gz_now() { return std::chrono::steady_clock::now(); }
inline double gz_ms_since(GzTime t) { return std::chrono::duration<double, std::milli>(gz_now() - t).count(); }

// The bounded queue of inflated chunks between an input's inflate threads and
// the block cut's read().
struct GzQueue {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Bytes> q;
    size_t q_bytes = 0;
    size_t queue_cap = 512u << 20;   // push waits while this many bytes are queued
    bool done = false, failed = false, stop = false;
    Bytes cur;
    size_t cur_at = 0;

    bool push(Bytes&& v)   // false: the reader went away
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || q_bytes < queue_cap; });
        if (stop) return false;
        q_bytes += v.size();
        q.push_back(std::move(v));
        cv.notify_all();
        return true;
    }
    void end(bool ok)   // the producer: nothing more comes
    {
        std::lock_guard<std::mutex> g(mu);
        failed = !ok;
        done = true;
        cv.notify_all();
    }
    void go_away()   // the reader: every push from now on returns false
    {
        std::lock_guard<std::mutex> g(mu);
        stop = true;
        cv.notify_all();
    }
    // up to n bytes into dst; 0 at the end; -1 on a gzip error
    long read(uint8_t* dst, size_t n)
    {
        size_t got = 0;
        while (got < n) {
            if (cur_at == cur.size()) {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !q.empty() || done; });
                if (q.empty()) {
                    if (failed) return -1;
                    break;
                }
                cur = std::move(q.front());
                q.pop_front();
                q_bytes -= cur.size();
                cur_at = 0;
                cv.notify_all();
            }
            const size_t k = std::min(n - got, cur.size() - cur_at);
            memcpy(dst + got, cur.data() + cur_at, k);
            cur_at += k;
            got += k;
        }
        return (long)got;
    }
};

// The input side of a device path.  The reader thread reads the file into
// recycled page-locked slabs and publishes them in file order, up to in_flight
// ahead; the device thread works on the oldest, which stays queued until it is
// retired (the reader counts it in flight).  The device thread ends the path by
// retiring a slab with a flag: bad (a call failed), stopped (the reader of the
// text went away, or the stream is over) or takeover (the gunzip path leaves the
// rest of the file to the host).  Slab: anything with `uint8_t* in`.
template <class Slab>
struct SlabFeed {
    const GzDevice& dev;
    const size_t in_flight;
    std::mutex pm;
    std::condition_variable pcv;
    std::deque<std::unique_ptr<Slab>> jobs;   // in file order
    std::vector<uint8_t*> free_in;
    bool quit = false, bad = false, stopped = false, takeover = false;
    double idle_ms = 0, in_alloc_ms = 0;   // (-v: the device thread waiting for a slab; the reader allocating them)
    std::thread device;

    SlabFeed(const GzDevice& d, size_t n) : dev(d), in_flight(n) {}
    // reader: a buffer of `bytes` once fewer than in_flight slabs are queued -- a recycled one, a new one
    // while fewer than in_flight + 1 exist.  nullptr: the path has ended (or no memory: bad)
    uint8_t* get(size_t bytes)
    {
        std::unique_lock<std::mutex> lk(pm);
        pcv.wait(lk, [&] { return bad || stopped || takeover || jobs.size() < in_flight; });
        if (bad || stopped || takeover) return nullptr;
        if (!free_in.empty()) {
            uint8_t* p = free_in.back();
            free_in.pop_back();
            return p;
        }
        lk.unlock();
        const auto t0 = gz_now();
        uint8_t* p = static_cast<uint8_t*>(dev.host_alloc(bytes));
        in_alloc_ms += gz_ms_since(t0);
        lk.lock();
        if (!p) bad = true;
        return p;
    }
    void put_back(uint8_t* p)   // reader: a buffer of get() that is not published after all
    {
        std::lock_guard<std::mutex> g(pm);
        free_in.push_back(p);
    }
    void publish(std::unique_ptr<Slab> s)   // reader
    {
        {
            std::lock_guard<std::mutex> g(pm);
            jobs.push_back(std::move(s));
        }
        pcv.notify_all();
    }
    // device thread: the oldest slab; nullptr once the reader has finished and none is left
    Slab* next()
    {
        const auto t0 = gz_now();
        std::unique_lock<std::mutex> lk(pm);
        pcv.wait(lk, [&] { return quit || !jobs.empty(); });
        idle_ms += gz_ms_since(t0);   // (waiting for the reader's next slab)
        return jobs.empty() ? nullptr : jobs.front().get();
    }
    // device thread: the oldest slab is done, its buffer is free again
    void retire(bool failed, bool stop, bool leave)
    {
        std::lock_guard<std::mutex> g(pm);
        free_in.push_back(jobs.front()->in);
        jobs.pop_front();
        if (failed) bad = true;
        if (stop) stopped = true;
        if (leave) takeover = true;
        pcv.notify_all();
    }
    void reader_gone()   // device thread, after its last slab: the copier found the text's reader gone
    {
        std::lock_guard<std::mutex> g(pm);
        stopped = true;
        takeover = false;
        pcv.notify_all();
    }
    // reader: after the last slab, until the device thread has retired them all or ended the path
    void wait_drained()
    {
        std::unique_lock<std::mutex> lk(pm);
        pcv.wait(lk, [&] { return bad || stopped || takeover || jobs.empty(); });
    }
    // reader: the end on every way out.  The device thread drains the queue unless it ended the path;
    // every buffer is freed.  false: the path failed
    bool finish()
    {
        {
            std::lock_guard<std::mutex> g(pm);
            quit = true;
        }
        pcv.notify_all();
        device.join();   // (no other thread is left)
        for (auto& j : jobs) dev.host_free(j->in);
        for (uint8_t* p : free_in) dev.host_free(p);
        return !bad;
    }
};

// The output side of a device path: two page-locked output slabs.  While the
// copier thread copies one into the queue's chunk, the next device call fills
// the other.  The device thread owns it: get() / hand() per call, close() last.
struct OutPair {
    struct Out {
        uint8_t* p = nullptr;
        uint64_t cap = 0, bytes = 0;
        bool busy = false;   // handed to the copier
    } outs[2];
    const GzDevice& dev;
    GzQueue& queue;
    const char* const opt;   // "--gpu-inflate" / "--gpu-gunzip", for the message
    std::mutex cm;
    std::condition_variable ccv;
    std::deque<int> handed;   // output slabs to copy, in order
    bool cquit = false, cgone = false;
    int turn = 0;
    // -v: the host copies run on the copier thread beside the device calls
    double copy_ms = 0, push_ms = 0, out_wait_ms = 0, alloc_ms = 0;
    std::thread copier;

    OutPair(const GzDevice& d, GzQueue& q, const char* o) : dev(d), queue(q), opt(o)
    {
        copier = std::thread([this]() {
            lower_priority();
            for (;;) {
                int k;
                {
                    std::unique_lock<std::mutex> lk(cm);
                    ccv.wait(lk, [&] { return cquit || !handed.empty(); });
                    if (handed.empty()) break;
                    k = handed.front();
                }
                bool ok = true;
                if (!cgone) {   // (only this thread writes cgone)
                    auto t0 = gz_now();
                    Bytes chunk(outs[k].bytes);
                    memcpy(chunk.data(), outs[k].p, outs[k].bytes);
                    copy_ms += gz_ms_since(t0);
                    t0 = gz_now();
                    ok = queue.push(std::move(chunk));
                    push_ms += gz_ms_since(t0);   // (the queue is full: the block cut is behind)
                }
                std::lock_guard<std::mutex> g(cm);
                if (!ok) cgone = true;
                handed.pop_front();
                outs[k].busy = false;
                ccv.notify_all();
            }
        });
    }
    // The next slab, once the copier has let go of it, with room for `need` bytes (grown to `grow`
    // otherwise).  nullptr: the reader went away (gone), or no memory (said on stderr)
    Out* get(uint64_t need, uint64_t grow, bool& gone)
    {
        Out& o = outs[turn];
        turn ^= 1;
        {
            const auto t0 = gz_now();
            std::unique_lock<std::mutex> lk(cm);
            ccv.wait(lk, [&] { return !o.busy; });
            out_wait_ms += gz_ms_since(t0);   // (the copier still holds this slab)
            if (cgone) {
                gone = true;
                return nullptr;
            }
        }
        if (need > o.cap) {
            const auto t0 = gz_now();
            if (o.p) dev.host_free(o.p);
            o.cap = grow;
            o.p = static_cast<uint8_t*>(dev.host_alloc(o.cap));
            if (!o.p) {
                fprintf(stderr, "seqarc_amd: %s: cannot allocate %llu bytes of host memory\n", opt, (unsigned long long)o.cap);
                o.cap = 0;
                return nullptr;
            }
            alloc_ms += gz_ms_since(t0);
        }
        return &o;
    }
    void hand(Out& o, uint64_t bytes)   // a filled slab to the copier
    {
        std::lock_guard<std::mutex> g(cm);
        o.bytes = bytes;
        o.busy = true;
        handed.push_back((int)(&o - outs));
        ccv.notify_all();
    }
    bool close()   // true: the reader went away
    {
        {
            std::lock_guard<std::mutex> g(cm);
            cquit = true;
        }
        ccv.notify_all();
        copier.join();   // (it copies what was handed to it first)
        for (Out& o : outs)
            if (o.p) dev.host_free(o.p);
        return cgone;
    }
};

// What a --gpu-gunzip loop does after a call that returned 0 (run_plain_gpu, and
// cli_devinput.h's gzip input).  left: the input bytes the call did not consume;
// last: the slab is the file's last; room: the bytes a slab has in front for a
// carry; text_bytes: the text the call delivered.
//   Over      the stream is over
//   Leave     the device path ends and the host continues from the state: a call
//             of two chunks or more that confirmed less than one, a last slab
//             without any progress, one wave confirmed in a call of four chunks
//             or more (the stream has no block starts to find -- stored or fixed
//             blocks only -- and one wave would go on doing all the work), or
//             more left than the next slab has room for
//   Again     another call on what is left (the last slab's rest runs alone)
//   NextSlab  what is left goes in front of the next slab
enum class GzAfter { Over, Leave, Again, NextSlab };
inline GzAfter gz_after_call(const sa_gunzip_info& info, const sa_gunzip_state& gs, uint64_t in_used, uint64_t text_bytes,
                             uint64_t left, bool last, uint64_t chunk, uint64_t room)
{
    if (gs.ended || (last && left == 0)) return GzAfter::Over;
    const bool low = (info.chunks >= 2 && in_used < chunk) || (last && !in_used && !text_bytes) ||
                     (info.chunks >= 4 && info.waves_confirmed == 1 && info.end_why != SA_GZ_OUTCAP);
    if (low || (!last && left > room)) return GzAfter::Leave;
    if (!last && (info.end_why != SA_GZ_OUTCAP && info.end_why != SA_GZ_BREAKS && info.end_why != SA_GZ_FULL)) return GzAfter::NextSlab;
    if (!last && left < chunk) return GzAfter::NextSlab;
    return GzAfter::Again;
}

struct GzStream : GzQueue {
    int fd = -1;
    int workers = 1;
    bool bgzf = false;
    std::thread prod;

    const GzDevice& dev;
    int gpu_device = -1;      // >= 0 (--gpu-inflate): BGZF members are inflated on this device
    int gunzip_device = -1;   // >= 0 (--gpu-gunzip): gzip that is not BGZF is inflated on this device
    bool verbose = false;
    std::string name;
    // (the command line leaves these alone; a test makes a small file span many slabs with them)
    size_t slab_bytes = 32u << 20;      // compressed bytes read at a time (the BGZF paths and --gpu-gunzip)
    size_t slabs_in_flight = 4;         // ... and how many of them the reader is ahead
    size_t gunzip_room = 8u << 20;      // in front of a --gpu-gunzip slab: the carry
    uint64_t out_cap = 512ull << 20;    // output bytes per device call (a slab of long runs inflates 1000-fold)

    explicit GzStream(const GzDevice& d) : dev(d) {}
    bool start(int f, int w)
    {
        fd = f;
        workers = std::max(1, w);
        uint8_t h[18];
        const ssize_t r = ::pread(fd, h, sizeof h, 0);
        bgzf = r == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[10] == 6 && h[11] == 0 &&
               h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0;
        prod = std::thread([this]() {
            lower_priority();
            if (gpu_device >= 0 && !bgzf && gunzip_device < 0 && verbose)
                fprintf(stderr, "seqarc_amd: --gpu-inflate: %s is gzip but not BGZF, inflating it on the host\n", name.c_str());
            end(bgzf ? (gpu_device >= 0 ? run_bgzf_gpu() : run_bgzf()) : gunzip_device >= 0 ? run_plain_gpu() : run_plain());
        });
        return true;
    }
    ~GzStream()
    {
        go_away();
        if (prod.joinable()) prod.join();
    }
    long readn(uint8_t* dst, size_t n, uint64_t& at)
    {
        size_t got = 0;
        while (got < n) {
            const ssize_t r = ::pread(fd, dst + got, n - got, (off_t)(at + got));
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) return -1;
            if (r == 0) break;
            got += (size_t)r;
        }
        at += got;
        return (long)got;
    }
    // one member or several concatenated (gzread's reading of them)
    // (at0: the file offset of the first member -- run_host_from continues a file there)
    bool run_plain(uint64_t at0 = 0)
    {
        z_stream z{};
        if (inflateInit2(&z, 15 + 16) != Z_OK) return false;
        std::vector<uint8_t> in(4u << 20);
        uint64_t at = at0;
        bool eof = false, member_end = false;
        Bytes out(8u << 20);
        size_t have = 0;
        for (;;) {
            if (z.avail_in == 0 && !eof) {
                const long r = readn(in.data(), in.size(), at);
                if (r < 0) { inflateEnd(&z); return false; }
                if (r == 0) eof = true;
                z.next_in = in.data();
                z.avail_in = (uInt)r;
            }
            if (z.avail_in == 0 && eof) break;
            if (member_end) {   // the next member, if it is one (trailing bytes otherwise end the stream)
                if (z.avail_in < 2 && !eof) {
                    // (rare: a member boundary at the end of a read slab) keep the byte, read more
                    memmove(in.data(), z.next_in, z.avail_in);
                    const long r = readn(in.data() + z.avail_in, in.size() - z.avail_in, at);
                    if (r < 0) { inflateEnd(&z); return false; }
                    if (r == 0) eof = true;
                    z.next_in = in.data();
                    z.avail_in += (uInt)r;
                }
                if (z.avail_in < 2 || z.next_in[0] != 0x1f || z.next_in[1] != 0x8b) break;
                inflateReset(&z);
                member_end = false;
            }
            z.next_out = out.data() + have;
            z.avail_out = (uInt)(out.size() - have);
            const int rc = inflate(&z, Z_NO_FLUSH);
            have = out.size() - z.avail_out;
            if (rc == Z_STREAM_END) member_end = true;
            else if (rc != Z_OK && rc != Z_BUF_ERROR) { inflateEnd(&z); return false; }
            else if (rc == Z_BUF_ERROR && z.avail_in == 0 && eof) { inflateEnd(&z); return false; }   // truncated
            if (have == out.size() || (member_end && have > (6u << 20))) {
                out.resize(have);
                if (!push(std::move(out))) { inflateEnd(&z); return true; }
                out = Bytes();
                out.resize(8u << 20);
                have = 0;
            }
        }
        inflateEnd(&z);
        if (!member_end && at > 0) return false;   // ended inside a member
        out.resize(have);
        if (have && !push(std::move(out))) return true;
        return true;
    }
    // A BGZF file slab by slab, for both BGZF paths: what the last slab's end cut
    // off a member goes in front of the next read, and sa::bgzf_scan walks the
    // whole members.
    struct BgzfReader {
        GzStream& gz;
        std::vector<uint8_t> carry;   // a member cut by the end of the previous slab
        uint64_t at = 0;
        bool eof = false;
        bool more() const { return !eof || !carry.empty(); }
        // buf[0 .. slab_bytes): the next slab and its members.  1: members to inflate, `total` text bytes;
        // 0: the file ended with the slab before; -1: a read error, not BGZF after all (or a member larger
        // than max_isize), no whole member (a truncated member, or trailing bytes that are no member), or
        // less than a member header left at the end of the file
        int next(uint8_t* buf, std::vector<sa_bgzf_member>& ms, uint64_t& total, uint32_t max_isize)
        {
            const size_t c0 = carry.size(), room = gz.slab_bytes - c0;
            if (c0) memcpy(buf, carry.data(), c0);
            carry.clear();
            const long r = eof ? 0 : gz.readn(buf + c0, room, at);
            if (r < 0) return -1;
            if ((size_t)r < room) eof = true;
            const size_t have = c0 + (size_t)r;
            if (eof && have == 0) return 0;
            uint64_t consumed = 0;
            const int64_t n = sa::bgzf_scan(buf, have, nullptr, UINT64_MAX, &consumed, &total, max_isize);   // (counts them)
            if (n <= 0) return -1;
            ms.resize((size_t)n);
            sa::bgzf_scan(buf, have, ms.data(), ms.size(), &consumed, &total, max_isize);
            carry.assign(buf + consumed, buf + have);
            return eof && !carry.empty() && carry.size() < 18 ? -1 : 1;
        }
    };
    // BGZF: slabs of whole members; a pool of `workers` threads inflates the
    // members of up to slabs_in_flight slabs (each member into its place, by its
    // ISIZE; CRC checked), while this thread reads and parses the next slab;
    // finished slabs leave in order.  (Round 3 started the workers per slab
    // and joined them before the next one: every slab waited for its slowest
    // member and the threads' start-up; the outputs were zero-filled first.)
    bool run_bgzf()
    {
        struct Slab {
            std::vector<uint8_t> in;
            std::vector<sa_bgzf_member> ms;
            Bytes out;
            size_t next = 0, done = 0;
            bool bad = false;
        };
        std::mutex pm;
        std::condition_variable pcv;
        std::deque<std::unique_ptr<Slab>> jobs;   // in file order
        bool quit = false;
        auto work = [&]() {
            lower_priority();
            const LibDeflate& ld = libdeflate();
            void* dd = ld.ok() ? ld.alloc() : nullptr;
            z_stream z{};
            const bool ok = dd ? true : inflateInit2(&z, -15) == Z_OK;
            std::unique_lock<std::mutex> lk(pm);
            for (;;) {
                Slab* s = nullptr;
                pcv.wait(lk, [&] {
                    if (quit) return true;
                    for (auto& j : jobs)
                        if (j->next < j->ms.size()) return true;
                    return false;
                });
                if (quit) break;
                for (auto& j : jobs)
                    if (j->next < j->ms.size()) { s = j.get(); break; }
                const size_t i = s->next++;
                lk.unlock();
                const sa_bgzf_member& m = s->ms[i];
                const uint8_t* src = s->in.data() + m.in_off;
                uint8_t* dst = s->out.data() + m.out_off;
                bool bad = !ok;
                // An empty member (the BGZF end-of-file marker) is inflated like any other, into a
                // one-byte dummy (its place in the slab's output may be no memory at all, and zlib
                // refuses a null next_out): it is good only if its stream ends having produced no byte.
                // A member with data behind a zeroed trailer produces one, or runs out of room.
                uint8_t dummy = 0;
                if (ok && m.isize == 0 && dd) {
                    size_t got = 1;
                    bad = ld.decompress(dd, src, m.in_len, &dummy, 1, &got) != 0 || got != 0 || m.crc != 0;
                } else if (ok && m.isize == 0) {
                    inflateReset(&z);
                    z.next_in = const_cast<uint8_t*>(src);
                    z.avail_in = (uInt)m.in_len;
                    z.next_out = &dummy;
                    z.avail_out = 1;
                    bad = inflate(&z, Z_FINISH) != Z_STREAM_END || z.avail_out != 1 || m.crc != 0;
                } else if (dd) {
                    size_t got = 0;
                    const int rc = ld.decompress(dd, src, m.in_len, dst, m.isize, &got);
                    bad = rc != 0 || got != m.isize || ld.crc32(0, dst, m.isize) != m.crc;
                } else if (ok) {
                    inflateReset(&z);
                    z.next_in = const_cast<uint8_t*>(src);
                    z.avail_in = (uInt)m.in_len;
                    z.next_out = dst;
                    z.avail_out = (uInt)m.isize;
                    const int rc = inflate(&z, Z_FINISH);
                    bad = rc != Z_STREAM_END || z.avail_out != 0 || crc32(0L, dst, (uInt)m.isize) != m.crc;
                }
                lk.lock();
                s->bad |= bad;
                if (++s->done == s->ms.size()) pcv.notify_all();
            }
            if (dd) ld.release(dd);
            else if (ok) inflateEnd(&z);
        };
        std::vector<std::thread> pool;
        for (int k = 0; k < workers; k++) pool.emplace_back(work);
        auto finish = [&](bool rc) {
            {
                std::lock_guard<std::mutex> g(pm);
                quit = true;
            }
            pcv.notify_all();
            for (auto& t : pool) t.join();
            return rc;
        };
        // the oldest slab, once inflated, to the reader (false: failed or the reader went away)
        auto retire = [&](bool& stopped) -> bool {
            std::unique_ptr<Slab> s;
            {
                std::unique_lock<std::mutex> lk(pm);
                pcv.wait(lk, [&] { return jobs.front()->done == jobs.front()->ms.size(); });
                s = std::move(jobs.front());
                jobs.pop_front();
            }
            if (s->bad) return false;
            if (!s->out.empty() && !push(std::move(s->out))) stopped = true;
            return true;
        };
        BgzfReader rd{*this};
        bool stopped = false;
        while (rd.more()) {
            std::unique_ptr<Slab> s(new Slab());
            s->in.resize(slab_bytes);
            uint64_t total = 0;
            // (no limit on a member's ISIZE here: zlib and libdeflate take what the format allows)
            const int got = rd.next(s->in.data(), s->ms, total, UINT32_MAX);
            if (got < 0) return finish(false);
            if (got == 0) break;
            s->out.resize(total);   // (default-initialised: no zero fill)
            size_t n;
            {
                std::lock_guard<std::mutex> g(pm);
                jobs.push_back(std::move(s));
                n = jobs.size();
            }
            pcv.notify_all();
            if (n >= slabs_in_flight && !retire(stopped)) return finish(false);
            if (stopped) return finish(true);
        }
        for (;;) {
            {
                std::lock_guard<std::mutex> g(pm);
                if (jobs.empty()) break;
            }
            if (!retire(stopped)) return finish(false);
            if (stopped) return finish(true);
        }
        return finish(true);
    }
    // BGZF with --gpu-inflate: the same slabs, carry and in-order retirement, but
    // a slab's members are inflated on the device by sa_inflate_members (one
    // sa_inflater per input, driven by one thread in place of the `workers`
    // pool) while this thread reads and scans the next slabs.  Within the device
    // thread H2D, kernel and D2H of a call still run one after the other.
    bool run_bgzf_gpu()
    {
        struct Slab {
            uint8_t* in = nullptr;   // host_alloc, slab_bytes
            std::vector<sa_bgzf_member> ms;
        };
        const auto t_begin = gz_now();
        sa_inflater* infl = dev.inflater_create(gpu_device);
        const double create_ms = gz_ms_since(t_begin);
        if (!infl) {
            fprintf(stderr, "seqarc_amd: --gpu-inflate: no usable gfx950 device %d\n", gpu_device);
            return false;
        }
        SlabFeed<Slab> feed(dev, slabs_in_flight);
        OutPair out(dev, *this, "--gpu-inflate");
        // -v: where the input's time went (the device calls run one after the other on the device thread)
        double kernel_ms = 0, call_ms = 0;
        uint64_t n_slabs = 0, n_members = 0, text_bytes = 0;
        feed.device = std::thread([&]() {
            lower_priority();
            std::vector<sa_bgzf_member> grp;
            while (Slab* s = feed.next()) {
                bool fail = false, gone = false;
                for (size_t a = 0; a < s->ms.size() && !fail && !gone;) {
                    size_t b = a;
                    uint64_t total = 0;
                    while (b < s->ms.size() && (b == a || total + s->ms[b].isize <= out_cap)) total += s->ms[b++].isize;
                    const uint64_t in0 = s->ms[a].in_off, in1 = s->ms[b - 1].in_off + s->ms[b - 1].in_len;
                    grp.assign(s->ms.begin() + (std::ptrdiff_t)a, s->ms.begin() + (std::ptrdiff_t)b);
                    const uint64_t out0 = grp[0].out_off;
                    for (sa_bgzf_member& m : grp) {
                        m.in_off -= in0;
                        m.out_off -= out0;
                    }
                    OutPair::Out* o = out.get(total, total + total / 8, gone);
                    if (!o) {
                        fail = !gone;
                        break;
                    }
                    const auto t0 = gz_now();
                    const int rc = dev.inflate_members(infl, s->in + in0, in1 - in0, grp.data(), (uint32_t)grp.size(), o->p, total,
                                                       nullptr);
                    if (rc < 0) fprintf(stderr, "seqarc_amd: --gpu-inflate: %s\n", dev.inflater_error(infl));
                    if (rc != 0) {   // (> 0: members that do not inflate or whose CRC differs -- the host path's error)
                        fail = true;
                        break;
                    }
                    call_ms += gz_ms_since(t0);
                    kernel_ms += dev.inflater_kernel_ms(infl);
                    n_members += grp.size();
                    text_bytes += total;
                    if (total) out.hand(*o, total);
                    a = b;
                }
                n_slabs++;
                feed.retire(fail, gone, false);
                if (fail || gone) break;
            }
            if (out.close()) feed.reader_gone();
        });
        auto finish = [&](bool rc) {
            rc = feed.finish() && rc;
            if (verbose)
                fprintf(stderr,
                        "seqarc_amd: --gpu-inflate: %s: %llu slab(s), %llu member(s), %llu text bytes on device %d in %.1f ms: "
                        "inflater create %.1f ms, slab alloc %.1f + %.1f ms, sa_inflate_members %.1f ms (inflate kernel %.1f ms), "
                        "host copy %.1f ms beside them (the device thread waited %.1f ms for it), queue wait %.1f ms, waiting for slabs "
                        "%.1f ms\n",
                        name.c_str(), (unsigned long long)n_slabs, (unsigned long long)n_members,
                        (unsigned long long)text_bytes, gpu_device, gz_ms_since(t_begin), create_ms, feed.in_alloc_ms, out.alloc_ms,
                        call_ms, kernel_ms, out.copy_ms, out.out_wait_ms, out.push_ms, feed.idle_ms);
            dev.inflater_destroy(infl);
            return rc;
        };
        BgzfReader rd{*this};
        while (rd.more()) {
            std::unique_ptr<Slab> s(new Slab());
            s->in = feed.get(slab_bytes);
            if (!s->in) return finish(true);   // (false all the same if the path failed)
            uint64_t total = 0;
            // (a member of more than 65,536 text bytes is an error here: the kernel's window holds no more)
            const int got = rd.next(s->in, s->ms, total, sa::INFL_MAX_ISIZE);
            if (got <= 0) {
                feed.put_back(s->in);
                return finish(got == 0);
            }
            feed.publish(std::move(s));
        }
        feed.wait_drained();
        return finish(true);
    }
    // The rest of a gzip file on the host, from where sa_gunzip_run left it: inside
    // a deflate stream a raw inflate with the state's window as its dictionary,
    // primed with the bits left of the current byte, the member's running CRC-32
    // and length carried on and compared with the trailer here; the members after
    // it through run_plain.
    bool run_host_from(const sa_gunzip_state& gs, uint64_t at)
    {
        if (gs.ended) return true;
        if (gs.in_stream) {
            z_stream z{};
            if (inflateInit2(&z, -15) != Z_OK) return false;
            auto fail = [&]() {
                inflateEnd(&z);
                return false;
            };
            if (gs.win_len && inflateSetDictionary(&z, gs.window + (32768 - gs.win_len), gs.win_len) != Z_OK) return fail();
            std::vector<uint8_t> in(4u << 20);
            Bytes out(8u << 20);
            size_t have = 0;
            uint32_t crc = gs.crc;
            uint64_t len = gs.len;
            bool eof = false, first = true, end = false;
            while (!end) {
                if (z.avail_in == 0) {
                    const long r = eof ? 0 : readn(in.data(), in.size(), at);
                    if (r <= 0) return fail();   // a read error, or the file ends inside the member
                    z.next_in = in.data();
                    z.avail_in = (uInt)r;
                    if (first && gs.bit) {
                        if (inflatePrime(&z, 8 - (int)gs.bit, in[0] >> gs.bit) != Z_OK) return fail();
                        z.next_in++;
                        z.avail_in--;
                    }
                    first = false;
                }
                z.next_out = out.data() + have;
                z.avail_out = (uInt)(out.size() - have);
                const int rc = inflate(&z, Z_NO_FLUSH);
                const size_t now_have = out.size() - z.avail_out;
                crc = (uint32_t)crc32(crc, out.data() + have, (uInt)(now_have - have));
                len += now_have - have;
                have = now_have;
                if (rc == Z_STREAM_END) end = true;
                else if (rc != Z_OK && rc != Z_BUF_ERROR) return fail();
                if (have == out.size() || end) {
                    out.resize(have);
                    if (have && !push(std::move(out))) {
                        inflateEnd(&z);
                        return true;
                    }
                    out = Bytes();
                    out.resize(8u << 20);
                    have = 0;
                }
            }
            // the trailer: what inflate left of the slab, then the file
            uint8_t t[8];
            size_t k = std::min<size_t>(8, z.avail_in);
            memcpy(t, z.next_in, k);
            at -= z.avail_in - k;   // (readn moved `at` past the slab)
            inflateEnd(&z);
            if (k < 8 && readn(t + k, 8 - k, at) != (long)(8 - k)) return false;
            const uint32_t tcrc = t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24;
            const uint32_t tlen = t[4] | t[5] << 8 | t[6] << 16 | (uint32_t)t[7] << 24;
            if (tcrc != crc || tlen != (uint32_t)len) return false;
        }
        // the next member, if it is one (trailing bytes otherwise end the stream)
        uint8_t m[2];
        uint64_t peek = at;
        if (readn(m, 2, peek) != 2 || m[0] != 0x1f || m[1] != 0x8b) return true;
        return run_plain(at);
    }
    // Gzip that is not BGZF with --gpu-gunzip: run_bgzf_gpu's shape around
    // sa_gunzip_run.  This thread reads the file into slabs, each with room in
    // front; the device thread puts what the last call left unconsumed (the
    // unconfirmed tail of its slab) into that room and inflates carry + slab.  A
    // call of two chunks or more that confirms less than one chunk of compressed
    // bytes (stored-only files, runs of enormous ratio, many tiny members: one
    // wave does all the work), or leaves more than the room holds, ends the
    // device path: the host continues from the state (run_host_from).
    bool run_plain_gpu()
    {
        struct Slab {
            uint8_t* in = nullptr;   // host_alloc, gunzip_room + slab_bytes
            size_t have = 0;
            uint64_t file_at = 0;
            bool last = false;
        };
        const auto t_begin = gz_now();
        sa_gunzipper* gz = dev.gunzipper_create(gunzip_device);
        const double create_ms = gz_ms_since(t_begin);
        if (!gz) {
            fprintf(stderr, "seqarc_amd: --gpu-gunzip: no usable gfx950 device %d\n", gunzip_device);
            return false;
        }
        const uint64_t chunk = dev.gunzipper_chunk(gz);
        SlabFeed<Slab> feed(dev, slabs_in_flight);
        OutPair out(dev, *this, "--gpu-gunzip");
        std::unique_ptr<sa_gunzip_state> gs(new sa_gunzip_state());
        uint64_t host_at = 0;   // takeover: the file offset the host continues at
        double kernel_ms[5] = {}, call_ms = 0;
        uint64_t n_calls = 0, n_chunks = 0, n_cand = 0, n_conf = 0, n_false = 0, n_members = 0, text_bytes = 0;
        feed.device = std::thread([&]() {
            lower_priority();
            std::vector<uint8_t> carry;   // what the last call left of its input
            bool fail = false, gone = false, leave = false, over = false;
            while (!fail && !gone && !leave && !over) {
                Slab* s = feed.next();
                if (!s) break;
                // carry + slab, contiguous; then again with what is left, until a call needs the next slab
                uint8_t* in = s->in + gunzip_room - carry.size();
                size_t n = carry.size() + s->have;
                uint64_t in_at = s->file_at - carry.size();   // the file offset of in[0]
                if (!carry.empty()) memcpy(in, carry.data(), carry.size());
                carry.clear();
                for (;;) {
                    const uint64_t want = std::min<uint64_t>(out_cap, 6ull * n + (64u << 20));
                    OutPair::Out* o = out.get(want, want, gone);
                    if (!o) {
                        fail = !gone;
                        break;
                    }
                    const auto t0 = gz_now();
                    uint64_t out_bytes = 0, in_used = 0;
                    sa_gunzip_info info{};
                    const int rc = dev.gunzip_run(gz, in, n, s->last ? 1 : 0, gs.get(), o->p, o->cap, &out_bytes, &in_used, &info);
                    if (rc < 0) fprintf(stderr, "seqarc_amd: --gpu-gunzip: %s\n", dev.gunzipper_error(gz));
                    if (rc > 0)
                        fprintf(stderr, "seqarc_amd: --gpu-gunzip: %s: the gzip stream is corrupt (status %d near byte %llu)\n",
                                name.c_str(), rc, (unsigned long long)(in_at + in_used));
                    if (rc != 0) {   // (> 0: the host path's error)
                        fail = true;
                        break;
                    }
                    call_ms += gz_ms_since(t0);
                    const float k[5] = {info.find_ms, info.spec_ms, info.chain_ms, info.resolve_ms, info.crc_ms};
                    for (int i = 0; i < 5; i++) kernel_ms[i] += k[i];
                    n_calls++;
                    n_chunks += info.chunks;
                    n_cand += info.candidates;
                    n_conf += info.waves_confirmed;
                    n_false += info.false_skipped;
                    n_members += info.members_ended;
                    text_bytes += out_bytes;
                    if (out_bytes) out.hand(*o, out_bytes);
                    in += in_used;
                    n -= in_used;
                    in_at += in_used;
                    const GzAfter next = gz_after_call(info, *gs, in_used, out_bytes, n, s->last, chunk, gunzip_room);
                    if (next == GzAfter::Over) {
                        over = true;
                        break;
                    }
                    if (next == GzAfter::Leave) {
                        leave = true;
                        host_at = in_at;
                        if (verbose)
                            fprintf(stderr,
                                    "seqarc_amd: --gpu-gunzip: %s: a call of %u chunk(s) confirmed %llu compressed bytes (wave %u "
                                    "ended it: %u); the host takes over at byte %llu\n",
                                    name.c_str(), info.chunks, (unsigned long long)in_used, info.end_wave, info.end_why,
                                    (unsigned long long)host_at);
                        break;
                    }
                    if (next == GzAfter::NextSlab) break;   // the next slab goes behind what is left
                }
                if (!fail && !gone && !leave && !over) carry.assign(in, in + n);
                feed.retire(fail, gone || over, leave);
            }
            if (out.close()) feed.reader_gone();
        });
        auto finish = [&](bool rc) {
            rc = feed.finish() && rc;
            if (verbose)
                fprintf(stderr,
                        "seqarc_amd: --gpu-gunzip: %s: %llu call(s), %llu chunk(s), %llu candidate(s), %llu wave(s) confirmed, %llu false "
                        "candidate(s) skipped, %llu member(s), %llu text bytes on device %d in %.1f ms: gunzipper create %.1f ms, slab "
                        "alloc %.1f + %.1f ms, sa_gunzip_run %.1f ms (gunzip kernels: find %.1f, spec %.1f, chain %.1f, resolve %.1f, "
                        "crc %.1f ms), host copy %.1f ms beside them (the device thread waited %.1f ms for it), queue wait %.1f ms, "
                        "waiting for slabs %.1f ms%s\n",
                        name.c_str(), (unsigned long long)n_calls, (unsigned long long)n_chunks, (unsigned long long)n_cand,
                        (unsigned long long)n_conf, (unsigned long long)n_false, (unsigned long long)n_members,
                        (unsigned long long)text_bytes, gunzip_device, gz_ms_since(t_begin), create_ms, feed.in_alloc_ms, out.alloc_ms,
                        call_ms, kernel_ms[0], kernel_ms[1], kernel_ms[2], kernel_ms[3], kernel_ms[4], out.copy_ms, out.out_wait_ms,
                        out.push_ms, feed.idle_ms, feed.takeover ? "; the host inflated the rest" : "");
            dev.gunzipper_destroy(gz);
            if (rc && feed.takeover) rc = run_host_from(*gs, host_at);
            return rc;
        };
        uint64_t at = 0;
        bool eof = false;
        while (!eof) {
            std::unique_ptr<Slab> s(new Slab());
            s->in = feed.get(gunzip_room + slab_bytes);
            if (!s->in) return finish(true);   // (false all the same if the path failed)
            s->file_at = at;
            const long r = readn(s->in + gunzip_room, slab_bytes, at);
            if (r < 0) {
                feed.put_back(s->in);
                return finish(false);
            }
            if ((size_t)r < slab_bytes) eof = true;
            s->have = (size_t)r;
            s->last = eof;
            feed.publish(std::move(s));
        }
        feed.wait_drained();
        return finish(true);
    }
};
