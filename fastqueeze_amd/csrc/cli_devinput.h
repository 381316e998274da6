// cli_devinput.h -- a compressed input of seqarc_amd -c --gpu-text (host C++; no
// device header): the file inflated into a devtext (sa_devtext), where the
// block cut finds it.  The compressed side is cli_gzstream.h's: a file thread
// reads slabs and publishes them through a SlabFeed.  There is no output side:
// the reader thread of the pipeline (read_device) calls pump(), which takes the
// oldest slab and inflates it into the devtext -- one thread drives the devtext.
//
//   BGZF   slabs of whole members (GzStream::BgzfReader: the carry, the member
//          walk, its three errors); pump() calls sa_inflate_members_dev with as
//          many of a slab's members as the devtext has room for.
//   gzip   (with --gpu-gunzip) slabs with room in front, as run_plain_gpu's reader
//          makes them; pump() puts what the last call left unconsumed into that
//          room and calls sa_gunzip_run_dev on carry + slab with the devtext's
//          room as out_cap, and again on what a call left, by run_plain_gpu's
//          rule (gz_after_call).  Where that rule leaves the device path, the
//          host continues from the state (GzStream::run_host_from on a thread of
//          its own, into the stream's queue) and pump() appends what it reads
//          from the queue to the same devtext (sa_devtext_append).
//
// The library calls go through GzDevice and DevTextCalls, so that
// tests/cpu_emu/devinput_emu.cpp drives all of this without the library.
#pragma once
#include "cli_gzstream.h"

// The devtext side of the library (seqarc_amd.h has the contracts).
struct DevTextCalls {
    sa_devtext* (*devtext_create)(int, uint64_t);
    void (*devtext_destroy)(sa_devtext*);
    uint64_t (*devtext_avail)(const sa_devtext*);
    uint64_t (*devtext_room)(const sa_devtext*);
    int (*devtext_append)(sa_devtext*, const uint8_t*, uint64_t);
    const char* (*devtext_error)(const sa_devtext*);
    void (*devtext_kernel_ms)(const sa_devtext*, float*, float*);
    int (*inflate_members_dev)(sa_inflater*, const uint8_t*, uint64_t, const sa_bgzf_member*, uint32_t, sa_devtext*, uint32_t*);
    int (*gunzip_run_dev)(sa_gunzipper*, const uint8_t*, uint64_t, int, sa_gunzip_state*, sa_devtext*, uint64_t, uint64_t*, uint64_t*,
                          sa_gunzip_info*);
};

struct DevInput {
    enum Kind { BGZF, GZIP };
    struct Slab {
        uint8_t* in = nullptr;   // host_alloc: slab_bytes (BGZF), gunzip_room + slab_bytes (gzip)
        std::vector<sa_bgzf_member> ms;   // BGZF
        size_t have = 0;                  // gzip: bytes read behind the room
        uint64_t file_at = 0;             // ... and their file offset
        bool last = false;                // ... the file ends with them
    };
    const GzDevice& dev;
    const DevTextCalls& dc;
    // (the command line leaves these alone; a test makes a small file span many slabs and calls with them)
    uint64_t capacity = 1ull << 30;      // the devtext's bytes (per mate)
    uint64_t call_bytes = 256ull << 20;  // text bytes of one device call at most
    uint64_t append_bytes = 8ull << 20;  // takeover: text bytes read from the host's queue per append at most
    // never started: the file as BgzfReader, run_host_from and readn see it (fd, slab_bytes, gunzip_room), and
    // after a takeover the queue the host fills
    GzStream gz;
    SlabFeed<Slab> feed;
    Kind kind = BGZF;
    int device = 0;
    sa_inflater* infl = nullptr;
    sa_gunzipper* gunz = nullptr;
    sa_devtext* dt = nullptr;
    std::string name;
    bool file_bad = false;   // (under feed.pm) the file thread ended on an error
    // ---- the reader thread's ----
    Slab* cur = nullptr;     // the slab being inflated ...
    size_t at = 0;           // BGZF: ... and its next member
    bool eof = false, started = false, closed = false;
    std::vector<sa_bgzf_member> grp;
    uint64_t members = 0, text_bytes = 0, calls = 0;   // (-v)
    double kernel_ms = 0, count_ms = 0, call_ms = 0;
    // gzip
    std::unique_ptr<sa_gunzip_state> gs;
    std::vector<uint8_t> carry;   // what the last call left of its input
    uint8_t* in = nullptr;        // the rest of carry + slab
    size_t n = 0;
    uint64_t in_at = 0;           // the file offset of in[0]
    uint64_t chunk = 0;
    bool host_on = false;         // the host took over: pump() drains its queue
    uint64_t host_at = 0, host_bytes = 0;
    Bytes host_buf;
    double gz_kernel_ms[5] = {}, create_ms = 0, host_ms = 0;
    uint64_t n_chunks = 0, n_cand = 0, n_conf = 0, n_false = 0;

    DevInput(const GzDevice& d, const DevTextCalls& c) : dev(d), dc(c), gz(d), feed(d, 4) {}

    bool start(int fd, const char* path, int device_, Kind k, std::string& err)
    {
        name = path;
        kind = k;
        device = device_;
        gz.fd = fd;
        gz.name = path;
        const auto t0 = gz_now();
        if (kind == BGZF) infl = dev.inflater_create(device);
        else gunz = dev.gunzipper_create(device);
        create_ms = gz_ms_since(t0);
        dt = infl || gunz ? dc.devtext_create(device, capacity) : nullptr;
        if (!dt) {
            err = "--gpu-text: no usable gfx950 device " + std::to_string(device) + ", or no device memory for the text";
            return false;
        }
        if (kind == GZIP) {
            gs.reset(new sa_gunzip_state());
            chunk = dev.gunzipper_chunk(gunz);
        }
        feed.device = std::thread([this]() {   // (SlabFeed joins it in finish(); here it is the file's reader)
            lower_priority();
            const bool ok = kind == BGZF ? read_bgzf() : read_gzip();
            {   // the end: the slabs still queued are taken, then next() gives nullptr
                std::lock_guard<std::mutex> g(feed.pm);
                file_bad = !ok || feed.bad;
                feed.quit = true;
            }
            feed.pcv.notify_all();
        });
        started = true;
        return true;
    }
    // ---- the file thread ----
    bool read_bgzf()
    {
        GzStream::BgzfReader rd{gz};
        while (rd.more()) {
            std::unique_ptr<Slab> s(new Slab());
            s->in = feed.get(gz.slab_bytes);
            if (!s->in) break;   // (the pipeline's reader stopped, or no memory: feed.bad)
            uint64_t total = 0;
            // (a member of more than 65,536 text bytes is an error: the kernel's window holds no more)
            const int got = rd.next(s->in, s->ms, total, sa::INFL_MAX_ISIZE);
            if (got <= 0) {
                feed.put_back(s->in);
                return got == 0;
            }
            feed.publish(std::move(s));
        }
        return true;
    }
    bool read_gzip()   // run_plain_gpu's reader: slabs with room in front for the carry
    {
        uint64_t file_at = 0;
        for (bool end = false; !end;) {
            std::unique_ptr<Slab> s(new Slab());
            s->in = feed.get(gz.gunzip_room + gz.slab_bytes);
            if (!s->in) break;   // (the pipeline's reader stopped, the stream is over, the host took over, or no memory)
            s->file_at = file_at;
            const long r = gz.readn(s->in + gz.gunzip_room, gz.slab_bytes, file_at);
            if (r < 0) {
                feed.put_back(s->in);
                return false;
            }
            if ((size_t)r < gz.slab_bytes) end = true;
            s->have = (size_t)r;
            s->last = end;
            feed.publish(std::move(s));
        }
        return true;
    }
    // ---- the pipeline's reader thread ----
    void count_time()
    {
        float cms = 0;
        dc.devtext_kernel_ms(dt, &cms, nullptr);
        count_ms += cms;
    }
    // inflates into the devtext until it holds `want` bytes or the input is used up; false: err
    bool pump(uint64_t want, std::string& err) { return kind == BGZF ? pump_bgzf(want, err) : pump_gzip(want, err); }
    bool pump_bgzf(uint64_t want, std::string& err)
    {
        while (!eof && dc.devtext_avail(dt) < want) {
            if (!cur) {
                cur = feed.next();
                at = 0;
                if (!cur) {
                    std::lock_guard<std::mutex> g(feed.pm);
                    if (file_bad) {
                        err = "read error on " + name + " (not BGZF throughout, a member cut short, or bytes after the last member)";
                        return false;
                    }
                    eof = true;
                    break;
                }
            }
            // members [at, b): what the devtext has room for, at most call_bytes text bytes
            const uint64_t room = std::min<uint64_t>(dc.devtext_room(dt), call_bytes);
            size_t b = at;
            uint64_t total = 0;
            while (b < cur->ms.size() && total + cur->ms[b].isize <= room) total += cur->ms[b++].isize;
            if (b == at) {   // (want is far below the capacity: a devtext short of it has room for a member)
                err = "--gpu-text: the device text of " + name + " has no room for a member";
                return false;
            }
            const uint64_t in0 = cur->ms[at].in_off, in1 = cur->ms[b - 1].in_off + cur->ms[b - 1].in_len;
            grp.assign(cur->ms.begin() + (std::ptrdiff_t)at, cur->ms.begin() + (std::ptrdiff_t)b);
            for (sa_bgzf_member& m : grp) m.in_off -= in0;
            const auto t0 = gz_now();
            const int rc = dc.inflate_members_dev(infl, cur->in + in0, in1 - in0, grp.data(), (uint32_t)grp.size(), dt, nullptr);
            if (rc != 0) {   // (> 0: members that do not inflate or whose CRC differs -- the host path's error)
                err = rc < 0 ? std::string("--gpu-text: ") + dev.inflater_error(infl) : "read error on " + name + " (a BGZF member does not inflate, or its CRC differs)";
                return false;
            }
            call_ms += gz_ms_since(t0);
            kernel_ms += dev.inflater_kernel_ms(infl);
            count_time();
            members += grp.size();
            text_bytes += total;
            calls++;
            at = b;
            if (at == cur->ms.size()) {
                feed.retire(false, false, false);
                cur = nullptr;
            }
        }
        return true;
    }
    bool pump_gzip(uint64_t want, std::string& err)
    {
        while (!eof && dc.devtext_avail(dt) < want) {
            if (host_on) {   // the host inflates the rest into the queue: its text reaches the same devtext
                const uint64_t ask = std::min<uint64_t>(dc.devtext_room(dt), append_bytes);
                if (!ask) {   // (want is far below the capacity)
                    err = "--gpu-text: the device text of " + name + " has no room";
                    return false;
                }
                if (host_buf.size() < ask) host_buf.resize(ask);
                const auto t0 = gz_now();
                const long r = gz.read(host_buf.data(), ask);
                if (r < 0) {
                    err = "read error on " + name + " (the gzip stream does not inflate, is cut short, or its CRC or length differs)";
                    return false;
                }
                if (r == 0) {
                    eof = true;
                    break;
                }
                if (dc.devtext_append(dt, host_buf.data(), (uint64_t)r) != 0) {
                    err = std::string("--gpu-text: ") + dc.devtext_error(dt);
                    return false;
                }
                host_ms += gz_ms_since(t0);
                count_time();
                host_bytes += (uint64_t)r;
                text_bytes += (uint64_t)r;
                continue;
            }
            if (!cur) {
                cur = feed.next();
                if (!cur) {   // (the last slab's call ends the stream or fails: the file thread gave up before it)
                    err = "read error on " + name;
                    return false;
                }
                // carry + slab, contiguous; then again with what is left, until a call needs the next slab
                in = cur->in + gz.gunzip_room - carry.size();
                n = carry.size() + cur->have;
                in_at = cur->file_at - carry.size();
                if (!carry.empty()) memcpy(in, carry.data(), carry.size());
                carry.clear();
            }
            const auto t0 = gz_now();
            uint64_t text = 0, in_used = 0;
            sa_gunzip_info info{};
            const int rc = dc.gunzip_run_dev(gunz, in, n, cur->last ? 1 : 0, gs.get(), dt,
                                             std::min<uint64_t>(dc.devtext_room(dt), call_bytes), &text, &in_used, &info);
            if (rc != 0) {   // (> 0: the host path's error)
                err = rc < 0 ? std::string("--gpu-text: ") + dev.gunzipper_error(gunz)
                             : "read error on " + name + " (the gzip stream is corrupt: status " + std::to_string(rc) + " near byte " +
                                   std::to_string(in_at + in_used) + ")";
                return false;
            }
            call_ms += gz_ms_since(t0);
            const float k[5] = {info.find_ms, info.spec_ms, info.chain_ms, info.resolve_ms, info.crc_ms};
            for (int i = 0; i < 5; i++) gz_kernel_ms[i] += k[i];
            if (text) count_time();   // (a call without text counts nothing)
            calls++;
            n_chunks += info.chunks;
            n_cand += info.candidates;
            n_conf += info.waves_confirmed;
            n_false += info.false_skipped;
            members += info.members_ended;
            text_bytes += text;
            in += in_used;
            n -= in_used;
            in_at += in_used;
            switch (gz_after_call(info, *gs, in_used, text, n, cur->last, chunk, gz.gunzip_room)) {
            case GzAfter::Over:
                eof = true;
                feed.retire(false, true, false);
                cur = nullptr;
                break;
            case GzAfter::Leave:
                host_at = in_at;
                if (gz.verbose)
                    fprintf(stderr,
                            "seqarc_amd: --gpu-text: %s: a call of %u chunk(s) confirmed %llu compressed bytes (wave %u ended it: "
                            "%u); the host takes over at byte %llu\n",
                            name.c_str(), info.chunks, (unsigned long long)in_used, info.end_wave, info.end_why,
                            (unsigned long long)host_at);
                feed.retire(false, false, true);
                cur = nullptr;
                host_on = true;
                gz.prod = std::thread([this]() {   // (~GzStream, or close(), joins it)
                    lower_priority();
                    gz.end(gz.run_host_from(*gs, host_at));
                });
                break;
            case GzAfter::NextSlab:
                carry.assign(in, in + n);
                feed.retire(false, false, false);
                cur = nullptr;
                break;
            case GzAfter::Again:
                break;
            }
        }
        return true;
    }
    // -v: where the input's time went (cut_ms .. room_wait: the block cut's, from read_device)
    void say(double cut_ms, long long blocks, unsigned long long cuts, double room_wait) const
    {
        if (kind == BGZF) {
            fprintf(stderr,
                    "seqarc_amd: --gpu-text: %s: %llu member(s), %llu text bytes in %llu call(s) on device %d: "
                    "sa_inflate_members_dev %.3f s (inflate kernel %.3f s, newline count %.1f ms); cut %.1f ms over "
                    "%lld blocks in %llu call(s); waited %.3f s for room\n",
                    name.c_str(), (unsigned long long)members, (unsigned long long)text_bytes, (unsigned long long)calls, device,
                    call_ms / 1e3, kernel_ms / 1e3, count_ms, cut_ms, blocks, cuts, room_wait);
            return;
        }
        fprintf(stderr,
                "seqarc_amd: --gpu-text: %s: gzip: %llu call(s), %llu chunk(s), %llu candidate(s), %llu wave(s) confirmed, %llu false "
                "candidate(s) skipped, %llu member(s), %llu text bytes on device %d: gunzipper create %.1f ms, sa_gunzip_run_dev "
                "%.3f s (gunzip kernels: find %.1f, spec %.1f, chain %.1f, resolve %.1f, crc %.1f ms; newline count %.1f ms), "
                "waiting for slabs %.1f ms; cut %.1f ms over %lld blocks in %llu call(s); waited %.3f s for room",
                name.c_str(), (unsigned long long)calls, (unsigned long long)n_chunks, (unsigned long long)n_cand,
                (unsigned long long)n_conf, (unsigned long long)n_false, (unsigned long long)members, (unsigned long long)text_bytes,
                device, create_ms, call_ms / 1e3, gz_kernel_ms[0], gz_kernel_ms[1], gz_kernel_ms[2], gz_kernel_ms[3], gz_kernel_ms[4],
                count_ms, feed.idle_ms, cut_ms, blocks, cuts, room_wait);
        if (host_on)
            fprintf(stderr, "; the host inflated the rest from byte %llu: %llu text bytes appended in %.3f s", (unsigned long long)host_at,
                    (unsigned long long)host_bytes, host_ms / 1e3);
        fprintf(stderr, "\n");
    }
    // the reader thread, on every way out: the file thread and the host's ended and joined, the slabs freed
    void close()
    {
        if (!started || closed) return;
        closed = true;
        if (cur) feed.retire(false, true, false);
        else feed.reader_gone();
        cur = nullptr;
        feed.finish();
        gz.go_away();
        if (gz.prod.joinable()) gz.prod.join();
    }
    ~DevInput()
    {
        close();
        if (infl) dev.inflater_destroy(infl);
        if (gunz) dev.gunzipper_destroy(gunz);
        if (dt) dc.devtext_destroy(dt);
    }
};
