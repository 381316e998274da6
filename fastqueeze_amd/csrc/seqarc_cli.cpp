// seqarc_amd -- the SeqArc command line over libseqarc_amd (host C++).
//
//   seqarc_amd -i ref.fa                                                   -> ref.fa.hash, ref.fa.md5
//   seqarc_amd -c [options] [ref.fa] -1 A.fq[.gz] [-2 B.fq[.gz]] (-o OUT | OUT)  -> OUT.arc
//   seqarc_amd -d [options] [ref.fa] ARCHIVE.arc [PREFIX] [-o PREFIX]
//
//   ref.fa     the HASH index path (SeqArcContext::doBuildIndex@0x419db0 /
//              HashAlignment::buildRefIndex@0x410190 for -i; with -c the blocks
//              take EncapFqzComp::doAlignEncode@0x42d4c0, aligned on the GPU;
//              the index is read from ref.fa.hash, or built on the GPU if absent)
//   -I N       max insert size of PE alignment (param+0x28), --maxmis M (param+0x1b60, 7)
//   -t N       host threads that parse (-c) or decode (-d) blocks
//   -l R       R-Block lossy qualities (rblock@0x426c10)      -n  no per-block MD5
//   -f         overwrite existing outputs ("%s has exist!" otherwise, .rodata +0x877)
//   -p         outputs in the directory of the input (README.md "-p")
//   -P 1|2|3   decode to stdout: SE or PE1 reads / PE2 reads / each pair in order
//              (DecodePipeOutJob@0x42f930)
//   --slevel K --qlevel Q   the reference's developer options (./seqarc.config)
//   --devices N   GPUs (default 1), --contexts K   encoder contexts per GPU
//   --batch B     blocks per encode, --block-size MiB (default 50)
//   --share-device   all contexts on one GPU (tests of the multi-GPU gather)
//   --host-only      read, cut and parse only (no device; measures the host pipeline)
//   --host-parse     parse the blocks on host threads (default: on the device, sa_stage_text)
//   --read-threads N plain-file reader threads (default 16; 0: the per-block window reader)
//   --writers N      archive writer threads (default 8: page maps at the blocks' offsets; 1: write(2))
//   --ingest-only    the reader and block cut alone, batches dealt to devices x contexts
//                    consumers (no device); --ingest-crc: the consumers CRC the texts
//   --gpu-inflate    BGZF inputs are inflated on the first device (sa_inflate_members)
//   --gpu-text       BGZF inputs are inflated into device memory and stay there: the block
//                    cut runs on the device and the blocks reach the parse device to device
//                    (sa_devtext; one device, device parse; off by default)
//                    instead of on host threads; other gzip files keep the host path
//   --gpu-gunzip     gzip inputs that are not BGZF (gzip, pigz, concatenated members) are
//                    inflated on the first device by speculation (sa_gunzip_run); with
//                    --gpu-text their text stays on the device too (sa_gunzip_run_dev)
//   --gpu-decode     -d: the blocks of a no-reference, lossless archive are decoded on the
//                    device, windows of blocks a call (sa_decode_blocks; --device N; off by
//                    default); a block the device does not take is decoded on the host
//
// Compression mirrors SeqArc-1.6 main@0x41fd40 -> SeqArcContext::doReadAndEncode
// @0x41a4e0 as a stream: one reader thread cuts 50 MiB blocks as the input
// arrives (doReadJob@0x432a80 / doReadPEJob@0x432d10, plain or gzip), -t parser
// threads turn them into the SoA blocks (getBlockRead[PE]), the first block
// decides the ID template (IDProcess::analysisIDBinType@0x4310a0), encoder
// threads -- K contexts per GPU sharing one front scratch, batches dealt round
// robin -- encode batches of blocks, and this thread writes them in input order
// (the reference's -t 1 order; the copies on --writers threads) after a 16-byte header, then the trailer
// (SeqArcFile::writeFileInfo@0x4171b0).  The blocks in flight are bounded
// (ReadBufPool@0x4341e0 plays that role in the reference).
#include <dlfcn.h>
#include <emmintrin.h>
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/seqarc_amd.h"
#include "cli_devinput.h"
#include "cli_gzstream.h"
#include "cli_knobs.h"
#include "cli_plan.h"

namespace {

int usage()
{
    fprintf(stderr,
            "usage: seqarc_amd -c [-t N] [-l R] [-n] [-f] [-p] -1 A.fq[.gz] [-2 B.fq[.gz]] (-o OUT | OUT)\n"
            "                  [--slevel K] [--qlevel Q] [--devices N] [--contexts K] [--batch BLOCKS]\n"
            "                  [--block-size MiB] [--device D] [--share-device] [--ramp] [--release]\n"
            "                  [--stage-ahead] [--writers N] [--read-threads N] [--gpu-inflate] [--gpu-text]\n"
            "                  [--gpu-gunzip]\n"
            "       seqarc_amd -d [-t N] [-f] [-p] [-P 1|2|3] [--gpu-decode] [--device D] [ref.fa] ARCHIVE.arc [PREFIX]\n"
            "                  [-o PREFIX]\n"
            "       seqarc_amd -i ref.fa            (HASH index: ref.fa.hash + ref.fa.md5)\n"
            "       (-s with -i / -c / -d and ref.fa: the index image in /dev/shm/<ref file name>)\n"
            "       (-c / -d with ref.fa: the reference path; -I N insert size, --maxmis M)\n"
            "       (--gpu-inflate: BGZF inputs of -c are inflated on the first device, not on host threads)\n"
            "       (--gpu-text: BGZF inputs of -c are inflated, cut into blocks and parsed on the device, the text\n"
            "        never on the host; not with --ingest-only, --host-only, --host-parse, --stage-ahead)\n"
            "       (--gpu-gunzip: gzip inputs of -c that are not BGZF are inflated on the first device; with\n"
            "        --gpu-text their text stays on the device as well)\n"
            "       (--gpu-decode: -d decodes the blocks of a no-reference, lossless archive on the device)\n");
    return 2;
}

bool slurp(const std::string& path, std::vector<uint8_t>& out)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n >= 0 && fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

bool spill(const std::string& path, const uint8_t* p, size_t n)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

bool is_fasta_name(const std::string& s)
{
    for (const char* e : {".fa", ".fasta", ".fna"}) {
        const size_t l = strlen(e);
        if (s.size() > l && s.compare(s.size() - l, l, e) == 0) return true;
    }
    return false;
}

// The genome the index packs (k_hash_pack, buildRefIndex@0x410190: every
// line not starting with '>', up to strlen - 1 characters), 16 bases a word,
// 2 bits a base (code & 3: N reads as A), the last word left-aligned
bool pack_fasta(const std::vector<uint8_t>& fa, std::vector<uint32_t>& words, uint64_t& bases)
{
    words.clear();
    bases = 0;
    uint32_t w = 0;
    bool header = false;
    for (size_t at = 0; at < fa.size();) {
        const uint8_t* p = fa.data() + at;
        const uint8_t* e = (const uint8_t*)memchr(p, '\n', fa.size() - at);
        const size_t len = e ? (size_t)(e - p) + 1 : fa.size() - at;
        at += len;
        if (p[0] == '>') { header = true; continue; }
        const uint8_t* z = (const uint8_t*)memchr(p, 0, len);
        const size_t sl = z ? (size_t)(z - p) : len;
        if (sl <= 1) continue;
        if (!header) return false;
        for (size_t i = 0; i + 1 < sl; i++) {
            uint32_t c;
            switch (p[i] | 0x20) {
            case 'c': c = 1; break;
            case 'g': c = 2; break;
            case 't': c = 3; break;
            case 'm': c = 1; break;   // IUPAC codes 5..14, & 3
            case 'r': c = 2; break;
            case 'y': c = 3; break;
            case 'k': c = 0; break;
            case 's': c = 1; break;
            case 'w': c = 2; break;
            case 'h': c = 3; break;
            case 'b': c = 0; break;
            case 'v': c = 1; break;
            case 'd': c = 2; break;
            default: c = 0;   // A, N and anything else
            }
            w = (w << 2) | c;
            if (++bases % 16 == 0) { words.push_back(w); w = 0; }
        }
    }
    if (bases % 16) words.push_back(w << (2 * (16 - bases % 16)));
    if (words.empty()) words.push_back(0);
    return header;
}

std::string dir_of(const std::string& p)
{
    const size_t s = p.rfind('/');
    return s == std::string::npos ? std::string() : p.substr(0, s + 1);
}


// isFileExist@0x40cc50 + getFileSize@0x40cc10: an existing non-empty output
// stops the run unless -f (SeqArcParam::parseOptFromMem@0x407210)
bool may_write(const std::string& path, bool force)
{
    struct stat sb;
    if (!force && stat(path.c_str(), &sb) == 0 && sb.st_size > 0) {
        fprintf(stderr, "seqarc_amd: %s has exist!\n", path.c_str());
        return false;
    }
    return true;
}

// An uninitialised growable array (std::vector would zero-fill the tens of MB
// of every block's buffers, which costs more than parsing them).  `pinned`
// (set while empty): page-locked storage (sa_host_alloc), so that staging the
// text to the device is a DMA.
template <class T>
struct Buf {
    T* d = nullptr;
    size_t n = 0, cap = 0;
    bool pinned = false;
    bool external = false;   // d belongs to an arena (TextPool): never freed here
    bool huge = false;       // (set while empty) 2 MiB-aligned with the huge-page hint (OutPool)
    // how d was allocated (its allocator frees it, whatever the flags above ask
    // of the next allocation)
    enum Kind : uint8_t { K_NEW, K_ALIGNED, K_PINNED } kind = K_NEW;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept { take(o); }
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) {
            release();
            take(o);
        }
        return *this;
    }
    ~Buf() { release(); }
    void take(Buf& o)
    {
        d = o.d;
        n = o.n;
        cap = o.cap;
        pinned = o.pinned;
        external = o.external;
        huge = o.huge;
        kind = o.kind;
        o.d = nullptr;
        o.n = o.cap = 0;
        o.external = false;
    }
    void reserve(size_t c)
    {
        if (c <= cap) return;
        T* nd = pinned ? static_cast<T*>(sa_host_alloc(c * sizeof(T))) : nullptr;
        Kind nk = K_PINNED;
        if (!nd && huge) {
            void* q = nullptr;
            if (posix_memalign(&q, 2u << 20, c * sizeof(T)) == 0) {
                (void)madvise(q, c * sizeof(T), MADV_HUGEPAGE);
                nd = static_cast<T*>(q);
                nk = K_ALIGNED;
            }
        }
        if (!nd) {   // (pageable when page-locked memory runs out: staging is then a slower copy)
            nd = new T[c];
            nk = K_NEW;
        }
        if (n) memcpy(nd, d, n * sizeof(T));
        free_(d);   // (with the old buffer's own allocator)
        d = nd;
        kind = nk;
        cap = c;
        external = false;
        pinned = nk == K_PINNED;
    }
    void resize(size_t c)
    {
        reserve(c);
        n = c;
    }
    void free_(T* p)
    {
        if (!p || external) return;
        if (kind == K_PINNED) sa_host_free(p);
        else if (kind == K_ALIGNED) free(p);
        else delete[] p;
    }
    void release()
    {
        free_(d);
        d = nullptr;
        n = cap = 0;
        external = false;
    }
    T& operator[](size_t i) { return d[i]; }
    const T& operator[](size_t i) const { return d[i]; }
    T* data() { return d; }
    const T* data() const { return d; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
};

// ---- gzip input -------------------------------------------------------------
// GzStream (cli_gzstream.h) inflates a gzip input ahead of the block cut on
// threads of its own; its two device paths call the library through this table.
const GzDevice kGzDevice = {sa_host_alloc,      sa_host_free,          sa_inflater_create, sa_inflater_destroy,
                            sa_inflater_error,  sa_inflater_kernel_ms, sa_inflate_members, sa_gunzipper_create,
                            sa_gunzipper_destroy, sa_gunzipper_chunk,  sa_gunzipper_error, sa_gunzip_run};

// ---- input ---------------------------------------------------------------
// getFileType@0x40d9f0 (gzip magic); plain files are read with read(2) /
// parallel pread slices, gzip through a GzStream (inflated ahead, BGZF in
// parallel).
int g_gz_workers = 8;   // inflate threads per BGZF input (-t / 2 for PE)
int g_gpu_inflate_dev = -1;   // --gpu-inflate: the device that inflates BGZF inputs
int g_gpu_gunzip_dev = -1;    // --gpu-gunzip: the device that inflates gzip inputs that are not BGZF
bool g_gz_verbose = false;

struct Input {
    int fd = -1;
    std::unique_ptr<GzStream> gz;
    bool is_gz = false, eof = false, seekable = true;
    uint64_t off = 0;   // file offset of the next byte (plain files)
    // raw: a gzip input is not inflated here (--gpu-text: a DevInput reads the file)
    bool open(const char* path, bool raw = false)
    {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        unsigned char m[2] = {0, 0};
        is_gz = ::pread(fd, m, 2, 0) == 2 && m[0] == 0x1f && m[1] == 0x8b;
        if (is_gz && !raw) {
            gz.reset(new GzStream(kGzDevice));
            gz->gpu_device = g_gpu_inflate_dev;
            gz->gunzip_device = g_gpu_gunzip_dev;
            gz->verbose = g_gz_verbose;
            gz->name = path;
            gz->start(fd, g_gz_workers);
        }
        return true;
    }
    // A plain file is read in slices by several threads at once (pread): one
    // thread copies ~4 GB/s out of the page cache, below the device's rate.
    long pread_all(uint8_t* dst, size_t n, uint64_t at)
    {
        size_t got = 0;
        while (got < n) {
            const ssize_t r = ::pread(fd, dst + got, n - got, (off_t)(at + got));
            if (r < 0 && errno == EINTR) continue;
            if (r < 0) return -1;
            if (r == 0) break;
            got += (size_t)r;
        }
        return (long)got;
    }
    // appends up to n bytes to b; false on a read error
    bool fill(Buf<uint8_t>& b, size_t n)
    {
        size_t have = b.size();
        b.resize(have + n);
        const size_t kSlice = 8u << 20;
        if (!is_gz && seekable && !eof && n >= 2 * kSlice) {
            // (four slices: the box's CPU share is a cgroup quota -- more copy
            // threads throttle the whole process, encoder threads included)
            const size_t ns = std::min<size_t>(4, n / kSlice), part = (n + ns - 1) / ns;
            std::vector<std::future<long>> fs;
            for (size_t i = 1; i < ns; i++) {
                const size_t s0 = i * part, len = std::min(n, s0 + part) - s0;
                fs.push_back(std::async(std::launch::async,
                                        [this, &b, have, s0, len]() { return pread_all(b.data() + have + s0, len, off + s0); }));
            }
            const long r0 = pread_all(b.data() + have, std::min(n, part), off);
            std::vector<long> rs{r0};
            for (auto& f : fs) rs.push_back(f.get());
            if (r0 >= 0 || errno != ESPIPE) {
                size_t got = 0;
                for (size_t i = 0; i < rs.size(); i++) {
                    if (rs[i] < 0) { b.resize(have); return false; }
                    const size_t want = std::min(n, i * part + part) - i * part;
                    got += (size_t)rs[i];
                    if ((size_t)rs[i] < want) {   // end of file inside slice i
                        eof = true;
                        break;
                    }
                }
                off += got;
                b.resize(have + got);
                return true;
            }
            seekable = false;   // a pipe: sequential reads below
        }
        size_t got = 0;
        while (got < n && !eof) {
            long r;
            if (is_gz) {
                r = gz->read(b.data() + have + got, n - got);
            } else {
                r = (long)::read(fd, b.data() + have + got, n - got);
                if (r < 0 && errno == EINTR) continue;
                if (r > 0) off += (uint64_t)r;
            }
            if (r < 0) { b.resize(have + got); return false; }
            if (r == 0) eof = true;
            got += (size_t)r;
        }
        b.resize(have + got);
        return true;
    }
    ~Input()
    {
        gz.reset();
        if (fd >= 0) ::close(fd);
    }
};

// the file starts with a BGZF member header (GzStream::start's test)
bool is_bgzf_file(const char* path)
{
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return false;
    uint8_t h[18];
    const ssize_t r = ::pread(fd, h, sizeof h, 0);
    ::close(fd);
    return r == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[10] == 6 && h[11] == 0 && h[12] == 'B' &&
           h[13] == 'C' && h[14] == 2 && h[15] == 0;
}

// the file starts with a gzip member header
bool is_gzip_file(const char* path)
{
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return false;
    uint8_t m[2] = {0, 0};
    const ssize_t r = ::pread(fd, m, 2, 0);
    ::close(fd);
    return r == 2 && m[0] == 0x1f && m[1] == 0x8b;
}

// --gpu-text: a compressed input inflated into a devtext (DevInput, cli_devinput.h);
// its devtext calls go through this table.
const DevTextCalls kDevTextCalls = {sa_devtext_create, sa_devtext_destroy,   sa_devtext_avail,       sa_devtext_room, sa_devtext_append,
                                    sa_devtext_error,  sa_devtext_kernel_ms, sa_inflate_members_dev, sa_gunzip_run_dev};

// Newlines in t[0, len): 64 bytes a step (compare, movemask, popcount).
uint64_t count_newlines(const uint8_t* t, uint64_t len)
{
    uint64_t n = 0, i = 0;
    const __m128i nl = _mm_set1_epi8('\n');
    for (; i + 64 <= len; i += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i*)(t + i));
        const __m128i b = _mm_loadu_si128((const __m128i*)(t + i + 16));
        const __m128i c = _mm_loadu_si128((const __m128i*)(t + i + 32));
        const __m128i d = _mm_loadu_si128((const __m128i*)(t + i + 48));
        const uint64_t m = (uint64_t)(uint16_t)_mm_movemask_epi8(_mm_cmpeq_epi8(a, nl)) |
                           (uint64_t)(uint16_t)_mm_movemask_epi8(_mm_cmpeq_epi8(b, nl)) << 16 |
                           (uint64_t)(uint16_t)_mm_movemask_epi8(_mm_cmpeq_epi8(c, nl)) << 32 |
                           (uint64_t)(uint16_t)_mm_movemask_epi8(_mm_cmpeq_epi8(d, nl)) << 48;
        n += (uint64_t)__builtin_popcountll(m);
    }
    for (; i < len; i++) n += t[i] == '\n';
    return n;
}

// ---- plain files: read ahead in segments (round 5) -------------------------
// The input files are read in segments of S bytes plus an overlap of W bytes
// (one block window: bs / 2 + 64 KiB for PE, bs + 64 KiB for SE), so that every
// window that starts inside a segment lies inside it, into a ring of R
// page-locked buffers per file.  A pool of fill threads copies 4 MiB slices out
// of the page cache (pread: one thread copies ~7 GB/s, eight ~58 GB/s on the
// GPU box, profiles/round5_r5a_ingest_probe.txt) and counts the newlines of
// every 256 KiB chunk of the slice while it is in cache.  The cut then reads a
// window's newline count off the chunk counts (cultPEbuf@0x432180 counts both
// windows' newlines: sa_cut_next_pe_nl) and walks back from the window's end as
// before, and a block is a view into its segment -- no per-block window, no
// carry copy.  A segment's slot is refilled once the cut has moved past it and
// every block in it was staged (its text copied to the device) or parsed.
struct SegReader {
    static constexpr uint64_t kSlice = cli::kSegSlice, kChunk = 256ull << 10;
    struct Seg {
        uint8_t* p = nullptr;
        uint64_t cap = 0;           // bytes of p
        int64_t idx = -1;           // segment number held (-1: none yet)
        uint64_t base = 0, len = 0;
        uint32_t nslices = 0, next_slice = 0, done = 0;
        int refs = 0;               // blocks (and the cut) still reading it
        bool ready = false;         // p is allocated for this segment
        bool filled = false;
    };
    struct File {
        int fd = -1;
        uint64_t size = 0;
        int64_t nseg = 0;
        int64_t next_start = 0;     // next segment number to start filling
        int64_t low = 0;            // the cut's segment (the lower ones are free once their refs are 0)
        std::vector<uint32_t> nl;   // newlines per kChunk of the file (the segments' primary parts)
        std::vector<Seg> ring;
    };
    File f[2];
    int nf = 1;
    uint64_t S = 0, W = 0;
    bool pinned = false, failed = false, stop = false;
    int free_threads = 8;   // threads that release the segments (CliKnobs::free_threads)
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::thread> workers;
    std::atomic<uint64_t> alloc_bytes{0};
    double fill_s = 0;   // fill threads' busy time (under mu)

    // fds: open plain regular files; the cut's window, a segment's bytes and the
    // segments per file are the plan's (cli_plan.h: seg_window, seg_bytes, ring_segs)
    bool start(const int* fds, const uint64_t* sizes, int n, const cli::BatchPlan& plan, int threads, bool pin,
               int free_thr)
    {
        nf = n;
        W = plan.seg_window;
        S = plan.seg_bytes;
        pinned = pin;
        free_threads = free_thr;
        const int R = plan.ring_segs;
        for (int i = 0; i < n; i++) {
            File& F = f[i];
            F.fd = fds[i];
            F.size = sizes[i];
            F.nseg = (int64_t)((F.size + S - 1) / S);
            F.nl.assign((size_t)(F.size / kChunk + 1), 0);
            F.ring.resize((size_t)std::max<int64_t>(1, std::min<int64_t>(R, F.nseg)));
        }
        for (int t = 0; t < std::max(1, threads); t++) workers.emplace_back([this]() { work(); });
        return true;
    }
    ~SegReader() { free_all(); }
    // the fill threads stopped, the segments' page-locked memory released (once
    // every block was staged: off the exit, where unpinning ~10 GB took ~0.5 s)
    void free_all()
    {
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
            cv.notify_all();
        }
        for (auto& t : workers) t.join();
        workers.clear();
        // (on up to free_threads threads, CliKnobs::free_threads)
        std::vector<Seg*> all;
        for (int i = 0; i < nf; i++)
            for (Seg& s : f[i].ring) all.push_back(&s);
        const size_t nt = std::min<size_t>(all.size(), (size_t)free_threads);
        std::vector<std::thread> th;
        for (size_t t = 1; t < nt; t++)
            th.emplace_back([&, t]() {
                for (size_t k = t; k < all.size(); k += nt) free_buf(*all[k]);
            });
        for (size_t k = 0; k < all.size(); k += std::max<size_t>(nt, 1)) free_buf(*all[k]);
        for (auto& t : th) t.join();
    }
    void free_buf(Seg& s)
    {
        if (!s.p) return;
        if (pinned) sa_host_free(s.p);
        else free(s.p);
        s.p = nullptr;
        s.cap = 0;
    }
    // under mu: a slice to fill (file, segment slot, slice), starting a segment when its slot is free
    bool pick(int& fi, Seg*& sg, uint32_t& sl, bool& must_alloc)
    {
        int best = -1;
        uint64_t best_off = ~0ull;
        for (int i = 0; i < nf; i++) {
            File& F = f[i];
            // the lowest segment with slices left, else the next one to start
            Seg* cand = nullptr;
            for (int64_t k = std::max<int64_t>(0, F.next_start - (int64_t)F.ring.size()); k < F.next_start; k++) {
                Seg& s = F.ring[(size_t)(k % (int64_t)F.ring.size())];
                if (s.idx == k && s.ready && s.next_slice < s.nslices) {
                    cand = &s;
                    break;
                }
            }
            uint64_t off;
            if (cand) {
                off = cand->base + (uint64_t)cand->next_slice * kSlice;
            } else {
                if (F.next_start >= F.nseg) continue;
                Seg& s = F.ring[(size_t)(F.next_start % (int64_t)F.ring.size())];
                const bool free_slot = s.idx < 0 || (s.refs == 0 && s.idx < F.low && s.filled);
                if (!free_slot) continue;
                off = (uint64_t)F.next_start * S;
            }
            if (off < best_off) {
                best_off = off;
                best = i;
                sg = cand;
            }
        }
        if (best < 0) return false;
        fi = best;
        File& F = f[best];
        must_alloc = false;
        if (!sg) {   // start segment next_start in its slot
            Seg& s = F.ring[(size_t)(F.next_start % (int64_t)F.ring.size())];
            s.idx = F.next_start++;
            s.base = (uint64_t)s.idx * S;
            s.len = std::min<uint64_t>(S + W, F.size - s.base);
            s.nslices = (uint32_t)((s.len + kSlice - 1) / kSlice);
            s.next_slice = s.done = 0;
            s.filled = false;
            s.ready = s.cap >= s.len;
            must_alloc = !s.ready;
            sg = &s;
        }
        sl = sg->next_slice++;
        return true;
    }
    void work()
    {
        for (;;) {
            int fi = 0;
            Seg* sg = nullptr;
            uint32_t sl = 0;
            bool must_alloc = false;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || failed || pick(fi, sg, sl, must_alloc); });
                if (stop || failed) return;
            }
            const auto t0 = std::chrono::steady_clock::now();
            if (must_alloc) {   // (one worker per segment; the others wait for `ready`)
                free_buf(*sg);
                const uint64_t want = std::max<uint64_t>(sg->len, std::min<uint64_t>(S + W, f[fi].size));
                void* p = pinned ? sa_host_alloc(want) : nullptr;
                if (!p) {   // (no device: pageable, on huge pages where the kernel has them)
                    if (posix_memalign(&p, 2u << 20, want) != 0) p = nullptr;
                    else (void)madvise(p, want, MADV_HUGEPAGE);
                }
                std::lock_guard<std::mutex> g(mu);
                if (!p) {
                    failed = true;
                    cv.notify_all();
                    return;
                }
                alloc_bytes += want;
                sg->p = static_cast<uint8_t*>(p);
                sg->cap = want;
                sg->ready = true;
                cv.notify_all();
            }
            const uint64_t a = (uint64_t)sl * kSlice, n = std::min<uint64_t>(kSlice, sg->len - a);
            uint64_t got = 0;
            while (got < n) {
                const ssize_t r = ::pread(f[fi].fd, sg->p + a + got, n - got, (off_t)(sg->base + a + got));
                if (r < 0 && errno == EINTR) continue;
                if (r <= 0) break;
                got += (uint64_t)r;
            }
            // newlines of the slice's whole chunks in the segment's primary part
            const uint64_t fa = sg->base + a, fe = std::min(sg->base + a + got, std::min(sg->base + S, f[fi].size));
            for (uint64_t c = fa / kChunk; (c + 1) * kChunk <= fe && c * kChunk >= fa; c++)
                f[fi].nl[(size_t)c] = (uint32_t)count_newlines(sg->p + (c * kChunk - sg->base), kChunk);
            std::lock_guard<std::mutex> g(mu);
            fill_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (got < n) {
                failed = true;   // (the file shrank under us)
            } else if (++sg->done == sg->nslices) {
                sg->filled = true;
            }
            cv.notify_all();
        }
    }
    // the cut's window at file offset off: waits for its segment, takes a
    // reference for the block (release(fi, seg)), returns the bytes available
    // from off within the segment; nullptr on a read failure
    const uint8_t* window(int fi, uint64_t off, uint64_t& avail, int64_t& seg)
    {
        File& F = f[fi];
        const int64_t k = std::min<int64_t>((int64_t)(off / S), std::max<int64_t>(F.nseg - 1, 0));
        std::unique_lock<std::mutex> lk(mu);
        F.low = k;
        cv.notify_all();
        Seg& s = F.ring[(size_t)(k % (int64_t)F.ring.size())];
        cv.wait(lk, [&] { return failed || (s.idx == k && s.filled); });
        if (failed) return nullptr;
        s.refs++;
        seg = k;
        avail = s.base + s.len - off;
        return s.p + (off - s.base);
    }
    void release(int fi, int64_t seg)
    {
        if (seg < 0) return;
        std::lock_guard<std::mutex> g(mu);
        Seg& s = f[fi].ring[(size_t)(seg % (int64_t)f[fi].ring.size())];
        if (s.idx == seg && s.refs > 0) s.refs--;
        cv.notify_all();
    }
    // the cut has passed every segment (the end of the input)
    void finish()
    {
        std::lock_guard<std::mutex> g(mu);
        for (int i = 0; i < nf; i++) f[i].low = f[i].nseg;
        cv.notify_all();
    }
    // newlines in [off, off + len) of file fi, inside the segment that holds off
    // (filled): whole chunks of its primary part from the chunk counts, the rest counted
    uint64_t newlines(int fi, uint64_t off, uint64_t len, const uint8_t* at_off)
    {
        const uint64_t seg_base = off / S * S, prim_end = seg_base + S, e = off + len;
        const uint64_t e1 = std::min(e, prim_end);
        uint64_t n = 0;
        const uint64_t ca = (off + kChunk - 1) / kChunk, cb = e1 / kChunk;
        if (ca >= cb) {
            n += count_newlines(at_off, e1 - off);
        } else {
            n += count_newlines(at_off, ca * kChunk - off);
            for (uint64_t c = ca; c < cb; c++) n += f[fi].nl[(size_t)c];
            n += count_newlines(at_off + (cb * kChunk - off), e1 - cb * kChunk);
        }
        if (e > prim_end) n += count_newlines(at_off + (prim_end - off), e - prim_end);
        return n;
    }
};

struct Parsed {
    // (not page-locked: hipHostRegister from the parser threads serialised in
    // the driver -- 129 s of parser time for 14 GB, r2p; pageable staging from
    // five contexts reaches ~19 GB/s, scripts/probe_h2d.py)
    Buf<uint8_t> names, seq, qual;
    Buf<uint16_t> nl;
    Buf<int32_t> sl;
    uint32_t nreads = 0;
    uint64_t text1 = 0, text2 = 0;
    sa_block view() const { return sa_block{names.data(), nl.data(), seq.data(), sl.data(), qual.data(), nreads}; }
};

// Parsed blocks are recycled: a later block reuses their buffers instead of
// faulting in fresh pages (~150 MB per block).
struct ParsedPool {
    std::mutex mu;
    std::vector<std::unique_ptr<Parsed>> free;
    std::unique_ptr<Parsed> get()
    {
        std::lock_guard<std::mutex> g(mu);
        if (free.empty()) return std::unique_ptr<Parsed>(new Parsed());
        std::unique_ptr<Parsed> p = std::move(free.back());
        free.pop_back();
        return p;
    }
    void put(std::unique_ptr<Parsed> p)
    {
        if (!p) return;
        std::lock_guard<std::mutex> g(mu);
        free.push_back(std::move(p));
    }
};

// Text windows are recycled too: a fresh 25-50 MiB allocation per block is
// mapped anew and faults in every page on the first read into it.
//
// Device parse: the windows are page-locked, carved from arena chunks of
// kChunk windows each -- one sa_host_alloc per chunk, not per window (the
// runtime serialises host allocations against the encoder threads' calls).
struct TextPool {
    static constexpr size_t kChunk = cli::kTextChunk;
    std::mutex mu;
    std::vector<Buf<uint8_t>> free;
    std::vector<void*> chunks;
    bool pinned = false;   // new windows in page-locked memory (device parse)
    size_t win = 0;        // window bytes of the arena (set before the first get)
    // (-v) chunks pinned on demand by the reader, and when the last one was
    std::atomic<uint32_t> on_demand{0};
    std::atomic<double> last_on_demand{0.0};
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~TextPool()
    {
        free.clear();
        for (void* c : chunks) sa_host_free(c);
    }
    void add_locked(uint8_t* c)
    {
        chunks.push_back(c);
        for (size_t k = 0; k < kChunk; k++) {
            Buf<uint8_t> b;
            b.pinned = true;
            b.external = true;
            b.d = c + k * win;
            b.cap = win;
            free.push_back(std::move(b));
        }
    }
    // one more chunk of windows, pinned outside the lock (the prefill thread:
    // pinning runs beside the contexts' creation and the reader's first reads)
    bool grow()
    {
        if (!pinned || !win) return false;
        uint8_t* c = static_cast<uint8_t*>(sa_host_alloc(kChunk * win));
        if (!c) return false;
        std::lock_guard<std::mutex> g(mu);
        add_locked(c);
        return true;
    }
    Buf<uint8_t> get()
    {
        std::lock_guard<std::mutex> g(mu);
        if (free.empty() && pinned && win)
            if (uint8_t* c = static_cast<uint8_t*>(sa_host_alloc(kChunk * win))) {
                add_locked(c);
                on_demand++;
                last_on_demand = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            }
        if (free.empty()) {
            Buf<uint8_t> b;
            b.pinned = pinned;
            return b;
        }
        Buf<uint8_t> b = std::move(free.back());
        free.pop_back();
        b.n = 0;
        return b;
    }
    void put(Buf<uint8_t>& b)
    {
        if (!b.cap) return;
        std::lock_guard<std::mutex> g(mu);
        free.push_back(std::move(b));
        b.n = b.cap = 0;
    }
};

// The encoded blocks' host buffers, recycled (round 5): a fresh buffer per
// block is a fresh mapping that the runtime's device-to-host copy faults in
// (and may page-lock) and that is unmapped again once the block is written,
// every batch.  The pool keeps them for the next batch's blocks; the virtual
// size is the output bound (~2x the block's symbols), only the written bytes
// are ever touched.  on = false (CliKnobs::out_pool): a fresh buffer per block (A/B).
struct OutPool {
    std::mutex mu;
    std::vector<Buf<uint8_t>> free;
    const bool on;
    explicit OutPool(bool pool) : on(pool) {}
    void take(Buf<uint8_t>& b, size_t n)
    {
        if (on && !b.cap) {
            std::lock_guard<std::mutex> g(mu);
            if (!free.empty()) {
                b = std::move(free.back());
                free.pop_back();
            }
        }
        if (on && !b.cap) b.huge = true;   // (huge pages: the copies' page-locking is undone 2x faster at the exit, pin_probe)
        if (on && b.cap < n) b.reserve(n + n / 8);   // (slack: the next block's bound may be a little larger)
        b.resize(n);
    }
    void give(Buf<uint8_t>& b)
    {
        if (!on || !b.cap) return;
        std::lock_guard<std::mutex> g(mu);
        free.push_back(std::move(b));
    }
};

struct Job {                     // one block between the reader and the writer
    Buf<uint8_t> t1, t2;          // its FASTQ text (recycled once parsed / staged; a view into a SegReader segment)
    SegReader* segr = nullptr;    // (views: the segments' references, released with the text)
    int64_t seg[2] = {-1, -1};
    uint64_t text1 = 0, text2 = 0;   // its text bytes in input 1 / 2
    uint32_t nreads = 0, len_long = 0;
    std::unique_ptr<Parsed> p;     // host parse (--host-parse; block 0 for the ID template)
    Buf<uint8_t> out;             // the encoded block
    int state = 0;                // 0 read, 1 parsed, 2 encoded
    uint32_t crc = 0;             // --ingest-only: CRC-32 of t1 then t2 (the writer folds them in order)
    sa_devblock* dblk = nullptr;  // --gpu-text: the block's text on the device (t1 / t2: block 0 only, for the ID template)
    Job() = default;
    Job(const Job&) = delete;
    Job& operator=(const Job&) = delete;
    ~Job() { if (dblk) sa_devblock_release(dblk); }
};

// The archive file, written by several threads (round 5).  A block's place
// is known once the blocks before it are (the writer hands them over in input
// order with their offsets); a pool of threads copies each block into a map
// of its page range, and a fallocate thread allocates the file's pages ahead
// of the copies.  One stream of fwrite ran at 1.2 GB/s into tmpfs and the last
// batch's ~450 MB held the run's end 0.39 s after its encode (r5j); the maps
// on 8 threads over allocated pages take 2 GB at ~10 GB/s (2 GB without the
// allocation ahead: 4 GB/s; with MAP_POPULATE: 1 GB/s).  Not a regular file
// (a pipe, a device): one thread, write(2) in order.
class ArcWriter {
public:
    using Done = std::function<void(std::unique_ptr<Job>)>;
    bool open(const std::string& path, int threads, Done done)
    {
        done_ = std::move(done);
        fd_ = ::open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
        if (fd_ < 0) return false;
        struct stat st;
        mapped_ = fstat(fd_, &st) == 0 && S_ISREG(st.st_mode) && threads > 1;
        const int n = mapped_ ? threads : 1;
        for (int i = 0; i < n; i++) pool_.emplace_back([this] { work(); });
        if (mapped_) fa_ = std::thread([this] { allocate(); });
        return true;
    }
    // block j (its encoded bytes j->out) at byte off; the blocks come in order
    void put(std::unique_ptr<Job> j, uint64_t off)
    {
        const uint64_t end = off + j->out.size();
        std::lock_guard<std::mutex> g(mu_);
        if (mapped_ && end > size_) {   // (grown a GiB at a time; cut to the archive's size in finish)
            const uint64_t s = std::max<uint64_t>(end, size_ + (1ull << 30));
            if (ftruncate(fd_, (off_t)s) == 0) size_ = s;   // (else the copies past size_ use pwrite: no map past EOF)
            else bad_ = true;
        }
        end_ = end;
        q_.emplace_back(std::move(j), off);
        cv_.notify_all();
    }
    bool bad() const { return bad_.load(); }
    // every block written; the archive cut to tail_off, the trailer written there, the header at 0
    bool finish(const uint8_t* tail, size_t tn, uint64_t tail_off, const uint8_t* hdr, size_t hn)
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
            cv_.notify_all();
        }
        for (auto& t : pool_) t.join();
        if (fa_.joinable()) fa_.join();
        pool_.clear();
        if (fd_ < 0) return false;
        bool ok = !bad_;
        if (mapped_ && ftruncate(fd_, (off_t)tail_off) != 0) ok = false;
        if (tail && !put_at(tail, tn, tail_off)) ok = false;
        if (hdr && pwrite(fd_, hdr, hn, 0) != (ssize_t)hn) ok = false;   // (a pipe: ESPIPE, as fseek was)
        if (::close(fd_) != 0) ok = false;
        fd_ = -1;
        return ok && hdr;
    }
    // the reserved header bytes at 0 (before the first block)
    bool lead(const uint8_t* p, size_t n) { return put_at(p, n, 0); }
    ~ArcWriter()
    {
        if (fd_ >= 0) finish(nullptr, 0, 0, nullptr, 0);
    }

private:
    static constexpr uint64_t kAhead = 768ull << 20, kStep = 64ull << 20;
    bool put_at(const uint8_t* p, size_t n, uint64_t off)
    {
        if (!mapped_) {   // (in order: lead, the blocks, then the trailer)
            while (n) {
                const ssize_t w = ::write(fd_, p, n);
                if (w <= 0) return false;
                p += w;
                n -= (size_t)w;
            }
            return true;
        }
        while (n) {
            const ssize_t w = pwrite(fd_, p, n, (off_t)off);
            if (w <= 0) return false;
            p += w;
            n -= (size_t)w;
            off += (uint64_t)w;
        }
        return true;
    }
    // A block is copied into a map of its pages only where fallocate has
    // allocated them (alloc_upto_ <= size_): a store to a page the file system
    // cannot back (disk full, quota) raises SIGBUS and would kill the process
    // with a partial archive; everywhere else pwrite, whose errors are reported.
    bool copy(const uint8_t* p, size_t n, uint64_t off)
    {
        if (!n) return true;
        if (!mapped_ || off + n > alloc_upto_.load()) return put_at(p, n, off);
        static const uint64_t pg = (uint64_t)sysconf(_SC_PAGESIZE);
        const uint64_t a = off & ~(pg - 1), len = off + n - a;
        void* m = mmap(nullptr, len, PROT_WRITE, MAP_SHARED, fd_, (off_t)a);
        if (m == MAP_FAILED) return put_at(p, n, off);
        memcpy(static_cast<uint8_t*>(m) + (off - a), p, n);
        munmap(m, len);
        return true;
    }
    void work()
    {
        for (;;) {
            std::unique_ptr<Job> j;
            uint64_t off = 0;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                j = std::move(q_.front().first);
                off = q_.front().second;
                q_.pop_front();
                cv_.notify_all();   // (the allocation ahead follows the queue's head)
            }
            if (!copy(j->out.data(), j->out.size(), off)) bad_ = true;
            done_(std::move(j));
        }
    }
    void allocate()   // the file's pages, kAhead beyond the last block handed over
    {
        uint64_t at = 0;
        for (;;) {
            uint64_t to;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || std::min(end_ + kAhead, size_) > at; });
                if (stop_) return;
                to = std::min(std::min(end_ + kAhead, size_), at + kStep);
            }
            // (a failure -- no space, a quota, unsupported -- ends the allocation:
            // the copies past alloc_upto_ then write with pwrite and report errors)
            if (fallocate(fd_, FALLOC_FL_KEEP_SIZE, (off_t)at, (off_t)(to - at)) != 0) return;
            at = to;
            alloc_upto_ = at;
        }
    }
    int fd_ = -1;
    bool mapped_ = false;
    Done done_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::pair<std::unique_ptr<Job>, uint64_t>> q_;
    uint64_t size_ = 0, end_ = 0;
    std::atomic<uint64_t> alloc_upto_{0};   // bytes of the file fallocate has allocated (from 0)
    bool stop_ = false;
    std::atomic<bool> bad_{false};
    std::vector<std::thread> pool_;
    std::thread fa_;
};

// getFirstLine@0x431eb0: the '+' line of the first record carries no ID
int bare_plus(const uint8_t* t, size_t n)
{
    size_t nl[3] = {0, 0, 0};
    int k = 0;
    for (size_t i = 0; i < n && k < 3; i++)
        if (t[i] == '\n') nl[k++] = i + 1;
    if (k < 3) return 1;
    return nl[2] - nl[1] > 2 ? 0 : 1;
}

// a block's text back to the reader: its windows recycled, its segment references dropped
void give_back(Job& j, TextPool& texts)
{
    texts.put(j.t1);
    texts.put(j.t2);
    if (j.segr) {
        j.segr->release(0, j.seg[0]);
        j.segr->release(1, j.seg[1]);
    }
    j.seg[0] = j.seg[1] = -1;
}

bool parse_job(Job& j, bool pe, ParsedPool& pool, TextPool& texts, bool keep_text)
{
    const uint64_t cap = j.t1.size() + j.t2.size() + 16;
    j.p = pool.get();
    Parsed& p = *j.p;
    p.names.resize(cap);
    p.seq.resize(cap);
    p.qual.resize(cap);
    p.nl.resize(cap / 4 + 8);
    p.sl.resize(cap / 4 + 8);
    const int64_t n = pe ? sa_parse_pe(j.t1.data(), j.t1.size(), j.t2.data(), j.t2.size(), p.names.data(), p.nl.data(),
                                       p.seq.data(), p.sl.data(), p.qual.data())
                         : sa_parse_se(j.t1.data(), j.t1.size(), p.names.data(), p.nl.data(), p.seq.data(),
                                       p.sl.data(), p.qual.data());
    if (n < 0) return false;
    p.nreads = (uint32_t)n;
    p.text1 = j.t1.size();
    p.text2 = j.t2.size();
    uint64_t nb = 0, sb = 0;
    for (uint32_t r = 0; r < p.nreads; r++) {
        nb += p.nl[r];
        sb += (uint64_t)p.sl[r];
    }
    p.names.n = nb;
    p.seq.n = sb;
    p.qual.n = sb;
    p.nl.n = p.nreads;
    p.sl.n = p.nreads;
    j.nreads = p.nreads;
    for (uint32_t r = 0; r < p.nreads; r++) j.len_long |= p.sl[r] > 0xffff;
    if (!keep_text) give_back(j, texts);
    return true;
}

struct Options : cli::PlanOpts {   // (PlanOpts, cli_plan.h: the options the batch plan reads)
    const char *f1 = nullptr, *f2 = nullptr, *out = nullptr, *arc = nullptr, *ref = nullptr;
    bool compress = false, decompress = false, index = false, force = false, in_dir = false, share_device = false,
         verbose = false, release = false, shm = false, maxmis_set = false, ingest_crc = false, gpu_inflate = false, gpu_gunzip = false,
         gpu_decode = false,   // --gpu-decode: -d hands windows of blocks to sa_decode_blocks
         gpu_text = false;   // --gpu-text: BGZF inputs inflated, cut and parsed on the device (DevInput, read_device)
    int writers = 8;        // --writers: the archive writer's copy threads (ArcWriter; 1: write(2) in order)
    int pipe = 0, device = 0, block_mib = 50, maxmis = 7;
    int insert = 0;
    sa_cfg cfg{3, 2, 1, 0, 0.0};
};

bool shm_publish(const char* ref, const uint8_t* p, size_t n, const uint8_t* md5, bool verbose);

// ---- SeqArc -i ref.fa: the HASH index (HashAlignment::buildRefIndex@0x410190,
//      HashRefIndex32::writeIndexFile@0x41ed00 -> "<ref>.hash"; MD5File@0x405950 of
//      the FASTA -> "<ref>.md5", 16 bytes) ----
int build_index(const Options& o)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> fa;
    if (!slurp(o.ref, fa) || fa.empty()) {
        fprintf(stderr, "Error:The file %s may be not exist or empty!\n", o.ref);
        return 1;
    }
    sa_ctx* c = sa_create(o.device);
    if (!c) {
        fprintf(stderr, "seqarc_amd: no usable gfx950 device %d\n", o.device);
        return 1;
    }
    const auto t1 = std::chrono::steady_clock::now();
    sa_hash_index* ix = sa_hash_build(c, (const char*)fa.data(), fa.size(), 14, 2, 1u << 16);
    if (!ix) {
        fprintf(stderr, "seqarc_amd: index build failed: %s\n", sa_last_error(c));
        sa_destroy(c);
        return 1;
    }
    const auto t2 = std::chrono::steady_clock::now();
    std::vector<uint8_t> file(sa_hash_file_bytes(ix));
    int rc = sa_hash_serialize(c, ix, file.data(), file.size());
    uint8_t md[16];
    sa_md5(fa.data(), fa.size(), md);
    if (rc || !spill(std::string(o.ref) + ".hash", file.data(), file.size()) ||
        !spill(std::string(o.ref) + ".md5", md, 16)) {
        fprintf(stderr, "seqarc_amd: cannot write the index files of %s\n", o.ref);
        rc = 1;
    }
    if (rc == 0 && o.shm && !shm_publish(o.ref, file.data(), file.size(), md, o.verbose)) rc = 1;
    const double s_load = std::chrono::duration<double>(t1 - t0).count(),
                 s_build = std::chrono::duration<double>(t2 - t1).count(),
                 s_all = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "seqarc_amd: index of %u bases (%s.hash, %zu bytes): read %.3f s, build %.3f s, total %.3f s\n",
            sa_hash_genome_length(ix), o.ref, file.size(), s_load, s_build, s_all);
    sa_hash_destroy(ix);
    sa_destroy(c);
    return rc;
}

// The reference of -c / -d: its index file (or the FASTA to build it from) and
// the MD5 the archive records (getMd5@0x416810 reads "<ref>.md5")
struct RefFiles {
    std::vector<uint8_t> hash, fasta;
    // the index image: hash's bytes, or (-s) a /dev/shm object mapped read-only
    const uint8_t* hp = nullptr;
    size_t hn = 0;
    void* map = nullptr;
    size_t map_len = 0;
    uint8_t md5[16] = {0};
    bool have_hash() const { return hn > 16; }
    void drop_hash()
    {
        hash.clear();
        hash.shrink_to_fit();
        if (map) munmap(map, map_len);
        map = nullptr;
        hp = nullptr;
        hn = 0;
    }
    ~RefFiles() { drop_hash(); }
};

// the bytes an index image's header announces (HashRefIndex32::loadRefIndexShm@0x41ef80:
// K, bases, words, positions; words, num[4^K], ind[4^K], positions), 0 if no header
uint64_t hash_image_bytes(const uint8_t* p, size_t n)
{
    if (n < 16) return 0;
    uint32_t h[4];
    memcpy(h, p, 16);
    if (h[0] < 1 || h[0] > 16) return 0;
    return 16 + 4ull * (h[2] + 2 * (1ull << (2 * h[0])) + h[3]);
}

// -s: the index image in POSIX shared memory under the reference's file name
// (IHashRefIndex::createShm@0x41f280: shm_open of the basename, an existing
// object of the announced size is kept, one of another size replaced;
// HashRefIndex32::createRefIndexShm@0x41f520 copies the image in after the
// file was read).  Later runs map it instead of reading <ref>.hash.
std::string shm_name(const char* ref)
{
    const std::string r(ref);
    return r.substr(r.rfind('/') + 1);
}

// The object is bound to its reference by a sidecar object "<name>.sa_ref":
// the FASTA's MD5 (the archive's encap 8) and the image size.  The reference
// keys the object by the file's basename alone, so two references of the same
// name would otherwise share one image (and -c would align against the wrong
// genome while recording the right MD5).
struct ShmTag {
    char magic[8];
    uint8_t md5[16];
    uint64_t bytes;
};
constexpr char kShmTagMagic[8] = {'S', 'A', 'R', 'E', 'F', '0', '0', '1'};

std::string shm_tag_name(const char* ref) { return shm_name(ref) + ".sa_ref"; }

// 1: the tag names this reference and size, 0: no tag, -1: another reference or size
int shm_tag_check(const char* ref, const uint8_t* md5, uint64_t bytes)
{
    const int fd = shm_open(shm_tag_name(ref).c_str(), O_RDONLY, 0);
    if (fd < 0) return 0;
    ShmTag t{};
    const bool got = ::pread(fd, &t, sizeof t, 0) == (ssize_t)sizeof t;
    close(fd);
    return got && !memcmp(t.magic, kShmTagMagic, 8) && !memcmp(t.md5, md5, 16) && t.bytes == bytes ? 1 : -1;
}

bool shm_tag_write(const char* ref, const uint8_t* md5, uint64_t bytes)
{
    const std::string nm = shm_tag_name(ref);
    shm_unlink(nm.c_str());
    const int fd = shm_open(nm.c_str(), O_CREAT | O_EXCL | O_RDWR, 0644);
    if (fd < 0) return false;
    ShmTag t{};
    memcpy(t.magic, kShmTagMagic, 8);
    memcpy(t.md5, md5, 16);
    t.bytes = bytes;
    const bool ok = ::pwrite(fd, &t, sizeof t, 0) == (ssize_t)sizeof t;
    close(fd);
    return ok;
}

// <ref>.hash on disk: 1 its header and size equal the image's, 0 no file, -1 they differ
int hash_file_matches(const char* ref, const uint8_t* p, size_t n)
{
    const std::string f = std::string(ref) + ".hash";
    const int fd = ::open(f.c_str(), O_RDONLY);
    if (fd < 0) return 0;
    struct stat sb;
    uint8_t h[16];
    const bool same = fstat(fd, &sb) == 0 && (uint64_t)sb.st_size == n && n >= 16 &&
                      ::pread(fd, h, 16, 0) == 16 && !memcmp(h, p, 16);
    close(fd);
    return same ? 1 : -1;
}

bool shm_publish(const char* ref, const uint8_t* p, size_t n, const uint8_t* md5, bool verbose)
{
    const std::string nm = shm_name(ref);
    int fd = shm_open(nm.c_str(), O_RDWR, 0);
    if (fd >= 0) {
        struct stat sb;
        const bool same = fstat(fd, &sb) == 0 && (uint64_t)sb.st_size == n;
        close(fd);
        // kept only when it is this reference's image (an object of the same
        // size but another reference, or an untagged one, is replaced)
        if (same && shm_tag_check(ref, md5, n) == 1) {
            fprintf(stderr, "createHashShm %s has existed.\n", nm.c_str());
            return true;
        }
        shm_unlink(nm.c_str());
    }
    fd = shm_open(nm.c_str(), O_CREAT | O_EXCL | O_RDWR, 0644);
    if (fd < 0) {
        fprintf(stderr, "shm_open fail.\n");
        return false;
    }
    bool ok = ftruncate(fd, (off_t)n) == 0;
    if (!ok) fprintf(stderr, "ftruncate fail.\n");
    void* m = ok ? mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
    close(fd);
    if (ok && m == MAP_FAILED) {
        fprintf(stderr, "mmap fail.\n");
        ok = false;
    }
    if (!ok) {
        shm_unlink(nm.c_str());
        return false;
    }
    memcpy(m, p, n);
    munmap(m, n);
    if (!shm_tag_write(ref, md5, n)) {
        fprintf(stderr, "shm_open fail.\n");
        shm_unlink(nm.c_str());
        return false;
    }
    if (verbose) fprintf(stderr, "seqarc_amd: index image in /dev/shm/%s (%zu bytes)\n", nm.c_str(), n);
    return true;
}

// 1: mapped, 0: no such object, or the object of another reference while
// <ref>.hash exists (the caller reads the file and republishes), -1: an object
// that is not an index image, or one that cannot be shown to be this
// reference's (md5: the FASTA's, from <ref>.md5 or the FASTA itself)
int shm_map(const char* ref, const uint8_t* md5, RefFiles& rf)
{
    const std::string nm = shm_name(ref);
    const int fd = shm_open(nm.c_str(), O_RDONLY, 0);
    if (fd < 0) return 0;
    struct stat sb;
    void* m = MAP_FAILED;
    size_t n = 0;
    if (fstat(fd, &sb) == 0 && sb.st_size >= 16) {
        n = (size_t)sb.st_size;
        m = mmap(nullptr, n, PROT_READ, MAP_SHARED, fd, 0);
    }
    close(fd);
    if (m == MAP_FAILED || hash_image_bytes((const uint8_t*)m, n) != n) {
        if (m != MAP_FAILED) munmap(m, n);
        fprintf(stderr, "/dev/shm/ %s is wrong file, please delete\n", nm.c_str());
        return -1;
    }
    // bound to this reference: its tag, else (an object without one, e.g. made
    // by SeqArc itself) <ref>.hash's header and size
    const int tag = shm_tag_check(ref, md5, n);
    const int file = tag == 1 ? 1 : hash_file_matches(ref, (const uint8_t*)m, n);
    if (tag < 0 || file < 0 || (tag == 0 && file == 0)) {
        munmap(m, n);
        if (file != 0) return 0;   // (stale or another reference's image: <ref>.hash is read and republished)
        fprintf(stderr, "/dev/shm/ %s is not the index of %s (another reference of the same name?), please delete\n",
                nm.c_str(), ref);
        return -1;
    }
    rf.map = m;
    rf.map_len = n;
    rf.hp = (const uint8_t*)m;
    rf.hn = n;
    return 1;
}

bool load_ref(const char* ref, bool need_fasta, RefFiles& rf, bool use_shm = false, bool verbose = false)
{
    const std::string r(ref);
    auto read_fasta = [&]() {
        if (!rf.fasta.empty()) return true;
        if (!slurp(r, rf.fasta) || rf.fasta.empty()) {
            fprintf(stderr, "Error:The file %s may be not exist or empty!\n", ref);
            return false;
        }
        return true;
    };
    // the reference's MD5 first: the shared-memory image must be this reference's
    std::vector<uint8_t> m;
    const bool have_md5 = slurp(r + ".md5", m) && m.size() == 16;
    if ((!have_md5 || need_fasta) && !read_fasta()) return false;
    if (have_md5) memcpy(rf.md5, m.data(), 16);
    else sa_md5(rf.fasta.data(), rf.fasta.size(), rf.md5);
    bool have_hash = false;
    if (use_shm) {   // (HashAlignment::loadRefIndex: loadRefIndexShm, else loadRefIndexFile)
        const int sm = shm_map(ref, rf.md5, rf);
        if (sm < 0) return false;
        have_hash = sm == 1;
        if (have_hash && verbose) fprintf(stderr, "seqarc_amd: index image from /dev/shm/%s\n", shm_name(ref).c_str());
    }
    if (!have_hash) {
        have_hash = slurp(r + ".hash", rf.hash) && rf.hash.size() > 16;
        if (!have_hash) rf.hash.clear();
        if (have_hash) {
            rf.hp = rf.hash.data();
            rf.hn = rf.hash.size();
            if (use_shm && hash_image_bytes(rf.hp, rf.hn) == rf.hn) (void)shm_publish(ref, rf.hp, rf.hn, rf.md5, verbose);
        }
    }
    return have_hash || read_fasta();
}

// ---- compression: the streaming pipeline ------------------------------------
bool g_fast_exit = false;   // compress() left the device buffers to the process exit

double mono_s()   // CLOCK_MONOTONIC (the clock of Python's time.monotonic: bench.py splits its wall clock)
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
double g_main_s = 0.0;

// the -v stamps bench.py reads (process start -> main and exit -> reaped are the
// caller's to see), then, after a compression that left its device buffers to
// the exit, the exit itself: no runtime teardown, and none of compress()'s
// destructors either (freeing the reader's ~24 GB of page-locked windows took
// 1.35 s after the archive was closed, round 3 g4f)
[[noreturn]] void fast_exit(int rc, bool verbose)
{
    if (verbose) fprintf(stderr, "seqarc_amd: monotonic clock: main %.6f, exit %.6f\n", g_main_s, mono_s());
    fflush(stdout);
    fflush(stderr);
    std::_Exit(rc);
}

// The -v clocks, in seconds from the start of compress().  add / set_min /
// set_max are the pipeline's only compare-exchange loops.
struct Stamps {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double now() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    static void add(std::atomic<double>& a, double d) { for (double c = a.load(); !a.compare_exchange_weak(c, c + d);) {} }
    static void set_min(std::atomic<double>& a, double v) { for (double c = a.load(); v < c && !a.compare_exchange_weak(c, v);) {} }
    static void set_max(std::atomic<double>& a, double v) { for (double c = a.load(); v > c && !a.compare_exchange_weak(c, v);) {} }
    // the main thread's: contexts ready, encoders started, blocks written, threads joined, archive closed
    double ctx = 0, enc_start = 0, written = 0, joined = 0, closed = 0;
    double fill_busy = 0, cut_busy = 0;   // the reader thread's
    // when the stages first / last did something, and their busy time (any thread)
    std::atomic<double> read_done{0}, first_enc{1e30}, last_enc{0}, enc_busy{0}, parse_busy{0}, stage_busy{0},
        seg_freed{0};
};

// What the run holds on the devices.  Released by release() or the destructor;
// leave_to_exit() leaves it all to the process exit (fast_exit).
struct DeviceSet {
    std::vector<sa_ctx*> ctxs;        // K per device; every device's contexts share one front scratch
    std::vector<int> ctx_dev;         // (the device of each context)
    std::vector<sa_ctx*> stagers;     // --stage-ahead: a staging context per context ...
    std::vector<sa_input*> sinputs;   // ... and two device inputs
    // reference path: the index on every device in use, one align_info chain
    // through all batches in input order (the reference's -t 1 thread)
    std::vector<sa_hash_index*> indexes;
    std::vector<sa_align_cfg> acfg;   // (per context)
    sa_align_chain* chain = nullptr;
    bool left = false;   // (a member of the one Pipeline: never copied)
    ~DeviceSet() { if (!left) release(); }
    void leave_to_exit() { left = true; }
    void release()
    {
        for (sa_hash_index* ix : indexes) sa_hash_destroy(ix);
        indexes.clear();
        if (chain) sa_align_chain_destroy(chain);
        chain = nullptr;
        for (sa_input* I : sinputs) sa_input_destroy(I);   // (a null input or context: a creation that failed)
        sinputs.clear();
        for (sa_ctx* s : stagers)
            if (s) sa_destroy(s);
        stagers.clear();
        for (sa_ctx*& c : ctxs) {   // (the count stays: report())
            if (c) sa_destroy(c);
            c = nullptr;
        }
    }
};

struct Joiner {
    std::thread t;
    ~Joiner() { if (t.joinable()) t.join(); }
};

// One compression run: compress() below is the list of its stages.  The
// threads are the reader (cuts blocks), the parsers (host parse; block 0's ID
// template), one encoder per context (and its helper with a feed that stages
// ahead), the segment ring's releaser and the writer (the calling thread).
struct Pipeline {
    // how a batch's blocks become device input, and what the helper thread does meanwhile
    enum Feed {
        WHOLE,    // sa_stage_text of the whole batch into the context's own input, in the
                  // context's cycle (also --host-parse, --host-only and --ingest-only: no helper)
        AHEAD,    // --stage-ahead: the helper stages the next batch into the alternate sa_input
                  // with the context's staging context
        STREAM    // SA_CLI_STREAM=1: sa_text_upload per block as it is cut, the helper uploads
                  // the next batch into the alternate text arena; sa_text_parse in the cycle
    };
    struct Turn {   // a batch in an encoder's hands
        int64_t k = -1;
        std::vector<Job*> js;
        double asked = 0, ready = 0;   // (-v) when the encoder asked for it, when it had it
    };

    // ---- set by the main thread before the threads that read it start ----
    const Options& o;
    const cli::CliKnobs& kn;
    const bool pe;
    Stamps st;
    Input in1, in2;
    // --gpu-text applies: the inputs are BGZF (or, with --gpu-gunzip, gzip) and their text lives in these (read_device)
    bool dev_text = false;
    std::unique_ptr<DevInput> dv1, dv2;
    std::string path;
    cli::PlanIn pin;
    cli::BatchPlan plan;
    Feed feed = WHOLE;
    std::string ctx_err;
    RefFiles rf;
    // ---- pools, each with a lock of its own (declared before the jobs: outlive them) ----
    ParsedPool pool;
    OutPool outpool;
    TextPool texts;
    Joiner prefill;   // pins the windows the reader will hold, beside the reader
    // ---- guarded by mu (cv signals every change) ----
    std::mutex mu;
    std::condition_variable cv;
    std::map<int64_t, std::unique_ptr<Job>> jobs;   // (a Job's text and output belong to the thread whose turn its state says it is)
    std::deque<int64_t> to_parse;
    int64_t nread = 0, nblocks = -1, written = 0, next_batch = 0, staged = 0;
    bool failed = false, tmpl_ready = false, seg_stop = false;
    std::string err;
    uint64_t total_in = 0;
    sa_cfg cfg;   // (bin_mode: written with tmpl_ready, read by the encoders after it)
    // ---- owned by one thread until the joins ----
    uint8_t tmpl[512] = {0};   // the parser of block 0
    int plus_bare = 1;         // the reader
    // ---- the writer's (the main thread) ----
    std::vector<sa_arc_block> info;
    uint64_t total = 0;   // the blocks' bytes
    uint32_t text_crc = 0;
    uint8_t hdr[16] = {0};
    int64_t tl = -1;   // the trailer's bytes
    int rc = 0;
    std::unique_ptr<SegReader> segr;
    std::thread seg_free, reader;
    std::vector<std::thread> parsers, encoders;
    ArcWriter aw;
    DeviceSet dev;

    Pipeline(const Options& opt, const cli::CliKnobs& k)
        : o(opt), kn(k), pe(opt.f2 && *opt.f2), outpool(k.out_pool), cfg(opt.cfg) {}

    void fail(const std::string& m)
    {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!failed) err = m;
            failed = true;
            cv.notify_all();
        }
        // contexts waiting on the alignment chain for a batch that will never
        // reach it return instead of waiting forever
        if (dev.chain) sa_align_chain_fail(dev.chain);
    }

    // ---- stage: the inputs opened, the output checked, the plan made ----
    bool open_inputs()
    {
        // inflate threads per BGZF input: the -t share (the device parse leaves the host threads free)
        g_gz_workers = std::max(2, (o.threads > 0 ? o.threads : 16) / (pe ? 2 : 1));
        g_gpu_inflate_dev = o.gpu_inflate ? o.device : -1;
        g_gpu_gunzip_dev = o.gpu_gunzip ? o.device : -1;
        g_gz_verbose = o.verbose;
        struct stat sb;
        for (const char* f : {o.f1, pe ? o.f2 : nullptr}) {
            if (f && (stat(f, &sb) != 0 || sb.st_size == 0)) {   // doCheckSetEncodeOpt@0x407fa0
                fprintf(stderr, "Error:The Src file %s may be not exist or empty!\n", f);
                return false;
            }
        }
        // --gpu-text takes BGZF inputs, and with --gpu-gunzip other gzip inputs, in any mix, on one device;
        // anything else runs as it would without the switch
        if (o.gpu_text) {
            auto takes = [&](const char* f) { return is_bgzf_file(f) || (o.gpu_gunzip && is_gzip_file(f)); };
            const bool all = takes(o.f1) && (!pe || takes(o.f2));
            dev_text = all && o.devices == 1;
            if (!dev_text && o.verbose)
                fprintf(stderr, "seqarc_amd: --gpu-text does not apply (%s): running without it\n",
                        all           ? "more than one device"
                        : o.gpu_gunzip ? "an input is neither BGZF nor gzip"
                                       : "an input is not BGZF");
        }
        if (!in1.open(o.f1, dev_text) || (pe && !in2.open(o.f2, dev_text))) {
            fprintf(stderr, "seqarc_amd: cannot open the input\n");
            return false;
        }
        std::string outp = o.out;
        if (o.in_dir && outp.find('/') == std::string::npos) outp = dir_of(o.f1) + outp;
        path = outp + ".arc";
        if (!may_write(path, o.force)) return false;
        static_cast<cli::PlanOpts&>(pin) = o;
        pin.gpu_text = dev_text;
        pin.pe = pe;
        pin.bs = (uint64_t)o.block_mib << 20;   // BlockSize(M), default 50 (param+0x1b78)
        pin.hw_threads = std::thread::hardware_concurrency();
        for (int i = 0; i < (pe ? 2 : 1); i++) {
            const Input& in = i ? in2 : in1;
            pin.gz[i] = in.is_gz;
            pin.regular[i] = fstat(in.fd, &sb) == 0 && S_ISREG(sb.st_mode);
            if (pin.regular[i]) pin.size[i] = (uint64_t)sb.st_size;
        }
        // (the contexts the options ask for: they do not exist yet)
        plan = cli::plan_batches(pin, kn, cli::plan_contexts_asked(pin));
        texts.pinned = plan.texts_pinned;
        texts.win = (size_t)plan.text_win;
        return true;
    }

    // ---- stage: the contexts (before the reader starts, or with early_read
    // beside its first batch), the prefill thread, the reference index and the
    // chain; false with ctx_err ----
    bool create_contexts()
    {
        // --ingest-only: the reader and the block cut alone, feeding devices x
        // contexts consumers that take batches as the device parse would (no device)
        if (o.host_only || o.ingest_only) dev.ctxs.assign((size_t)o.contexts * (o.ingest_only ? o.devices : 1), nullptr);
        for (int d = 0; d < o.devices && !o.host_only && !o.ingest_only; d++) {
            sa_ctx* first = nullptr;
            for (int k = 0; k < o.contexts; k++) {
                const int dv = o.device + (o.share_device ? 0 : d);
                sa_ctx* c = first ? sa_create_shared(dv, first) : sa_create(dv);
                if (!c) break;
                if (!first) first = c;
                dev.ctxs.push_back(c);
                dev.ctx_dev.push_back(dv);
            }
            if (!first) break;
        }
        // (started once the contexts exist: pinning beside their creation held
        // it up, 0.25 -> 0.83 s, round 3 g4j)
        if (plan.prefill_chunks && !dev.ctxs.empty() && dev.ctxs[0])
            prefill.t = std::thread([this, n = plan.prefill_chunks]() {
                for (size_t i = 0; i < n; i++)
                    if (!texts.grow()) break;
            });
        if (o.verbose)
            for (sa_ctx* c : dev.ctxs)
                if (c) sa_set_timing(c, 1);
        if (dev.ctxs.empty()) {
            ctx_err = "no usable gfx950 device " + std::to_string(o.device);
            return false;
        }
        if (o.ref && !o.host_only && !o.ingest_only && !load_index()) return false;
        const int64_t asked = cli::plan_contexts_asked(pin);
        if ((int64_t)dev.ctxs.size() != asked)
            fprintf(stderr, "seqarc_amd: warning: %zu of %lld encoder contexts created\n", dev.ctxs.size(),
                    (long long)asked);
        // Contexts created before the reader started: the plan again, for the
        // count created.  (early_read: B, the ring and the in-flight bound were
        // sized for the count asked for and the reader runs by them already;
        // fewer contexts only cost pace, hence the warning alone.)
        if (!plan.early_read) plan = cli::plan_batches(pin, kn, (int64_t)dev.ctxs.size());
        if (plan.ramp)
            for (sa_ctx* c : dev.ctxs)
                if (c) sa_set_reserve(c, (uint32_t)plan.B);
        st.ctx = st.now();
        return true;
    }

    bool load_index()
    {
        if (!load_ref(o.ref, false, rf, o.shm, o.verbose)) {
            ctx_err = std::string("cannot load the reference ") + o.ref;
            return false;
        }
        const double ti = st.now();
        sa_ctx* owner = nullptr;
        sa_hash_index* ix = nullptr;
        dev.acfg.resize(dev.ctxs.size());
        for (size_t k = 0; k < dev.ctxs.size(); k++) {
            if (k % (size_t)o.contexts == 0 && !(o.share_device && ix)) {   // the first context of a device
                owner = dev.ctxs[k];
                ix = rf.have_hash() ? sa_hash_load(owner, rf.hp, rf.hn)
                                    : sa_hash_build(owner, (const char*)rf.fasta.data(), rf.fasta.size(), 14, 2, 1u << 16);
                if (!ix) {
                    ctx_err = std::string("reference index: ") + sa_last_error(owner);
                    return false;
                }
                dev.indexes.push_back(ix);
            }
            dev.acfg[k] = sa_align_cfg{ix, pe ? 1 : 0, o.maxmis, 1, (uint32_t)o.insert};
        }
        dev.chain = sa_align_chain_create(0, 0);   // a fresh encode thread's AlignParam (nmis 0)
        if (o.verbose)
            fprintf(stderr, "seqarc_amd: reference %s: index %s in %.3f s\n", o.ref, rf.have_hash() ? "loaded" : "built",
                    st.now() - ti);
        return true;
    }

    // ---- stage: the reader (cuts blocks as the input arrives) ----
    void start_reader()
    {
        if (plan.seg_plain) {
            segr.reset(new SegReader());
            const int fds[2] = {in1.fd, in2.fd};
            // (page-locked for the device parse; --ingest-only too)
            segr->start(fds, pin.size, pe ? 2 : 1, plan, o.read_threads, plan.dev_parse, kn.free_threads);
        }
        // the segments are released as soon as every block is staged (device parse)
        if (segr && plan.dev_parse && kn.ring_free)
            seg_free = std::thread([this]() {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return failed || seg_stop || (nblocks >= 0 && staged >= nblocks); });
                    if (failed || seg_stop) return;
                }
                segr->free_all();
                st.seg_freed = st.now();
            });
        reader = std::thread([this]() {
            if (dev_text) read_device();
            else if (segr) read_segments();
            else read_windows();
        });
    }

    // the reader waits for room: blocks in flight, and (device parse) at most
    // two batches of page-locked text ahead of the staging; false once the run failed
    bool wait_for_room()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] {
            return failed || ((size_t)(nread - written) < plan.max_inflight && (!plan.dev_parse || nread - staged < 2 * plan.B));
        });
        return !failed;
    }

    // block 0: the first line (the cut checks every block's start against it)
    // and whether the '+' lines are bare
    void capture_first(std::vector<uint8_t>& first, const uint8_t* p1, size_t n1, const uint8_t* p2, size_t n2)
    {
        const void* nl = memchr(p1, '\n', n1);
        first.assign(p1, nl ? (const uint8_t*)nl + 1 : p1 + n1);
        plus_bare = pe ? bare_plus(p2, n2) : bare_plus(p1, n1);
    }

    // the next block's end in each input; nl: the windows' newline counts when
    // the source has them (the segment reader).  false: fail() was called
    bool cut(const uint8_t* p1, uint64_t n1, bool eof1, const uint8_t* p2, uint64_t n2, bool eof2,
             const std::vector<uint8_t>& first, const uint64_t* nl, uint64_t& e1, uint64_t& e2)
    {
        const uint64_t bs = pin.bs;
        e1 = e2 = 0;
        if (pe) {
            const int r = nl ? sa_cut_next_pe_nl(p1, n1, eof1, nl[0], p2, n2, eof2, nl[1], bs, first.data(), first.size(), &e1, &e2)
                             : sa_cut_next_pe(p1, n1, eof1, p2, n2, eof2, bs, first.data(), first.size(), &e1, &e2);
            if (r != 0) return fail("PE block cut failed (mates out of step)"), false;
        } else {
            const int64_t e = sa_cut_next_se(p1, n1, eof1, bs, first.data(), first.size());
            if (e < 0) return fail("block cut failed"), false;
            e1 = (uint64_t)e;
        }
        return true;
    }

    // block i (e1 / e2 text bytes) to the parsers or the encoders; last: the input ends with it
    void publish(int64_t i, std::unique_ptr<Job> j, uint64_t e1, uint64_t e2, bool last)
    {
        if (last) {
            st.read_done = st.now();
            if (segr) segr->finish();
        }
        j->text1 = e1;
        j->text2 = e2;
        if (plan.dev_parse && i > 0) j->state = 1;   // (parsed on the device when staged)
        {
            std::lock_guard<std::mutex> g(mu);
            total_in += e1 + e2;
            jobs[i] = std::move(j);
            if (!plan.dev_parse || i == 0) to_parse.push_back(i);
            nread = i + 1;
            if (last) nblocks = nread;
        }
        cv.notify_all();
    }

    void end_input(int64_t i)   // the input ended on a block boundary: i blocks
    {
        if (segr) segr->finish();
        std::lock_guard<std::mutex> g(mu);
        nblocks = i;
        cv.notify_all();
    }

    void read_segments()   // plain regular files: blocks are views into the segments
    {
        const uint64_t want = plan.cut_window;
        std::vector<uint8_t> first;
        uint64_t o1 = 0, o2 = 0;
        for (int64_t i = 0;; i++) {
            if (!wait_for_room()) return;
            if (o1 >= pin.size[0] && (!pe || o2 >= pin.size[1])) return end_input(i);
            const double tf0 = st.now();
            uint64_t av1 = 0, av2 = 0;
            int64_t s1 = -1, s2 = -1;
            const uint8_t* w1 = segr->window(0, o1, av1, s1);
            const uint8_t* w2 = pe ? segr->window(1, o2, av2, s2) : nullptr;
            if (!w1 || (pe && !w2)) return fail("read error on the input");
            const bool eof1 = o1 + av1 >= pin.size[0], eof2 = pe && o2 + av2 >= pin.size[1];
            if (i == 0) capture_first(first, w1, (size_t)std::min(av1, want), w2, (size_t)std::min(av2, want));
            const double tc0 = st.now();
            st.fill_busy += tc0 - tf0;   // (waiting for the fill threads)
            uint64_t e1 = 0, e2 = 0, nl[2] = {0, 0};
            if (pe) {
                nl[0] = segr->newlines(0, o1, std::min(av1, want), w1);
                nl[1] = segr->newlines(1, o2, std::min(av2, want), w2);
            }
            if (!cut(w1, av1, eof1, w2, av2, eof2, first, nl, e1, e2)) return;
            st.cut_busy += st.now() - tc0;
            if (e1 + e2 == 0) return fail("block cut made no progress");
            std::unique_ptr<Job> j(new Job());
            auto view = [](Buf<uint8_t>& b, const uint8_t* p, uint64_t n) {
                b.d = const_cast<uint8_t*>(p);
                b.n = n;
                b.cap = 0;   // (not a window: TextPool::put leaves it)
                b.external = true;
            };
            view(j->t1, w1, e1);
            if (pe) view(j->t2, w2, e2);
            j->segr = segr.get();
            j->seg[0] = s1;
            j->seg[1] = s2;
            o1 += e1;
            o2 += e2;
            const bool last = o1 >= pin.size[0] && (!pe || o2 >= pin.size[1]);
            publish(i, std::move(j), e1, e2, last);
            if (last) return;
        }
    }

    void read_windows()   // gzip inputs, pipes, --read-threads 0: per-block windows, the rest carried over
    {
        Buf<uint8_t> b1 = texts.get(), b2 = texts.get();
        std::vector<uint8_t> first;
        const uint64_t want = plan.cut_window;
        for (int64_t i = 0;; i++) {
            if (!wait_for_room()) return;
            b1.reserve(want);
            if (pe) b2.reserve(want);
            const double tf0 = st.now();
            {   // the two mate files are read concurrently
                std::future<bool> r2;
                if (pe && b2.size() < want && !in2.eof)
                    r2 = std::async(std::launch::async, [&]() { return in2.fill(b2, want - b2.size()); });
                const bool ok1 = b1.size() >= want || in1.eof || in1.fill(b1, want - b1.size());
                const bool ok2 = !r2.valid() || r2.get();
                if (!ok1) return fail("read error on input 1");
                if (!ok2) return fail("read error on input 2");
            }
            if (b1.empty() && (!pe || b2.empty())) return end_input(i);
            if (i == 0) capture_first(first, b1.data(), b1.size(), b2.data(), b2.size());
            const double tc0 = st.now();
            st.fill_busy += tc0 - tf0;
            uint64_t e1 = 0, e2 = 0;
            if (!cut(b1.data(), b1.size(), in1.eof, b2.data(), b2.size(), in2.eof, first, nullptr, e1, e2)) return;
            st.cut_busy += st.now() - tc0;
            std::unique_ptr<Job> j(new Job());
            auto hand_over = [&](Buf<uint8_t>& b, Buf<uint8_t>& to, uint64_t e) {
                Buf<uint8_t> carry = texts.get();   // the bytes after the cut start the next window
                carry.reserve(want);
                memcpy(carry.data(), b.data() + e, b.size() - e);
                carry.n = b.size() - e;
                b.n = e;
                to = std::move(b);
                b = std::move(carry);
            };
            hand_over(b1, j->t1, e1);
            if (pe) hand_over(b2, j->t2, e2);
            const bool last = b1.empty() && b2.empty() && in1.eof && (!pe || in2.eof);
            publish(i, std::move(j), e1, e2, last);
            if (last) return;
        }
    }

    // --gpu-text: compressed inputs whose text stays on the device.  Each mate's
    // devtext is pumped to a cut window (DevInput::pump: sa_inflate_members_dev
    // for BGZF, sa_gunzip_run_dev for other gzip),
    // sa_devtext_cut cuts every block the text holds, and each block leaves as a
    // devblock in its Job -- the encoders upload it device to device (upload).
    // Block 0 is also fetched to the host: the parser needs it for the ID template.
    void read_device()
    {
        constexpr uint64_t kCut = 64;   // blocks per cut call at most
        const uint64_t want = plan.cut_window;
        std::vector<uint8_t> first;
        std::vector<uint64_t> l1(kCut), l2(kCut);
        double room_wait = 0, cut_ms = 0;
        uint64_t cuts = 0;
        std::string e;
        auto done = [&]() {   // every way out: the file threads joined; -v: where the inputs' time went
            for (DevInput* d : {dv1.get(), dv2.get()}) {
                if (!d) continue;
                d->close();
                if (o.verbose) d->say(cut_ms, (long long)nread_local, (unsigned long long)cuts, room_wait);
            }
        };
        dv1.reset(new DevInput(kGzDevice, kDevTextCalls));
        if (pe) dv2.reset(new DevInput(kGzDevice, kDevTextCalls));
        for (DevInput* d : {dv1.get(), dv2.get()})
            if (d) d->gz.verbose = o.verbose;
        auto kind = [](const char* f) { return is_bgzf_file(f) ? DevInput::BGZF : DevInput::GZIP; };
        if (!dv1->start(in1.fd, o.f1, o.device, kind(o.f1), e) || (pe && !dv2->start(in2.fd, o.f2, o.device, kind(o.f2), e)))
            return done(), fail(e);
        for (int64_t i = 0;;) {
            const double tf0 = st.now();
            const uint64_t had = sa_devtext_avail(dv1->dt) + (pe ? sa_devtext_avail(dv2->dt) : 0);
            if (!dv1->pump(want, e) || (pe && !dv2->pump(want, e))) return done(), fail(e);
            const uint64_t a1 = sa_devtext_avail(dv1->dt), a2 = pe ? sa_devtext_avail(dv2->dt) : 0;
            if (i == 0) {   // the first line and the bare-'+' test, on peeked bytes
                if (a1 == 0 && a2 == 0) return done(), end_input(0);
                std::vector<uint8_t> h1, h2;
                auto peek = [&](DevInput& d, uint64_t a, std::vector<uint8_t>& h) {   // the first three lines at least
                    for (uint64_t n = std::min<uint64_t>(a, 1u << 20);; n = std::min(a, want)) {
                        h.resize((size_t)n);
                        if (sa_devtext_peek(d.dt, 0, h.data(), n) != 0) return false;
                        if (n >= std::min(a, want) || std::count(h.begin(), h.end(), (uint8_t)'\n') >= 3) return true;
                    }
                };
                if (!peek(*dv1, a1, h1) || (pe && !peek(*dv2, a2, h2)))
                    return done(), fail(std::string("--gpu-text: ") + sa_devtext_error(dv1->dt));
                capture_first(first, h1.data(), h1.size(), h2.data(), h2.size());
            }
            const double tc0 = st.now();
            st.fill_busy += tc0 - tf0;
            int32_t end = 0;
            const int64_t n = sa_devtext_cut(dv1->dt, dv1->eof, pe ? dv2->dt : nullptr, pe && dv2->eof, pin.bs, first.data(),
                                             first.size(), l1.data(), l2.data(), kCut, &end);
            if (n < 0) return done(), fail(std::string("--gpu-text: ") + sa_devtext_error(dv1->dt));
            float cms = 0;
            sa_devtext_kernel_ms(dv1->dt, nullptr, &cms);
            cut_ms += cms;
            cuts++;
            st.cut_busy += st.now() - tc0;
            for (int64_t b = 0; b < n; b++, i++) {
                const double tw = st.now();
                if (!wait_for_room()) return done();
                room_wait += st.now() - tw;
                std::unique_ptr<Job> j(new Job());
                j->dblk = sa_devtext_take(dv1->dt, l1[(size_t)b], pe ? dv2->dt : nullptr, pe ? l2[(size_t)b] : 0);
                if (!j->dblk) return done(), fail(std::string("--gpu-text: ") + sa_devtext_error(dv1->dt));
                if (i == 0) {
                    j->t1.resize((size_t)l1[0]);
                    if (pe) j->t2.resize((size_t)l2[0]);
                    if (sa_devblock_fetch(j->dblk, j->t1.data(), pe ? j->t2.data() : nullptr) != 0)
                        return done(), fail("--gpu-text: cannot fetch block 0");
                }
                const bool last = b == n - 1 && end == SA_CUT_DONE;
                nread_local = i + 1;
                if (last) done();
                publish(i, std::move(j), l1[(size_t)b], pe ? l2[(size_t)b] : 0, last);
                if (last) return;
            }
            if (end == SA_CUT_DONE) return done(), end_input(i);
            if (end == SA_CUT_NONE) return done(), fail(pe ? "PE block cut failed (mates out of step)" : "block cut failed");
            if (end == SA_CUT_MORE && n == 0 && sa_devtext_avail(dv1->dt) + (pe ? sa_devtext_avail(dv2->dt) : 0) == had)
                return done(), fail("--gpu-text: the block cut asks for more text than the device text holds");
        }
    }
    int64_t nread_local = 0;   // (read_device's own count of its blocks, for its -v line)

    // ---- stage: the parsers (host parse; with the device parse block 0 only,
    // for the ID template) ----
    void start_parsers() { for (int t = 0; t < plan.nparse; t++) parsers.emplace_back([this]() { parse_loop(); }); }

    void parse_loop()
    {
        for (;;) {
            int64_t i;
            Job* j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return failed || !to_parse.empty() || nblocks >= 0; });
                if (failed || (to_parse.empty() && nblocks >= 0)) return;
                i = to_parse.front();
                to_parse.pop_front();
                j = jobs[i].get();
            }
            const double tp = st.now();
            if (!parse_job(*j, pe, pool, texts, plan.dev_parse)) return fail("parse failed");
            Stamps::add(st.parse_busy, st.now() - tp);
            if (i == 0) {   // the ID template of the first block
                const sa_block fb = j->p->view();
                if (sa_analyze_ids(&fb, pe ? 0 : 1, tmpl) != 0) return fail("ID analysis failed");
            }
            if (plan.dev_parse) pool.put(std::move(j->p));   // (only the template needed it)
            {
                std::lock_guard<std::mutex> g(mu);
                j->state = 1;
                if (i == 0) {
                    cfg.bin_mode = tmpl[0];
                    tmpl_ready = true;
                }
            }
            cv.notify_all();
        }
    }

    // ---- stage: the encoders, one host thread per context, batches in order ----
    // By default the stage is part of the context's cycle (WHOLE).  --stage-ahead
    // measured slower (4.7-5.0 against 6.6-6.7 GB/s on 42.8 GB, round 3 g4d: the
    // staging contexts' streams outnumber the hardware queues, and the tails
    // slowed under the concurrent parse); SA_CLI_STREAM: cli_knobs.h.
    void start_encoders()
    {
        const bool have = !dev.ctxs.empty() && dev.ctxs[0];
        if (plan.dev_parse && !o.ingest_only && o.stage_ahead && have) feed = AHEAD;
        else if (plan.stream_opt && have) feed = STREAM;
        for (size_t i = 0; feed == AHEAD && i < dev.ctxs.size(); i++) {
            sa_ctx* s = sa_create(dev.ctx_dev[i]);
            sa_input* a = sa_input_empty(dev.ctx_dev[i]);
            sa_input* b = sa_input_empty(dev.ctx_dev[i]);
            dev.stagers.push_back(s);
            dev.sinputs.push_back(a);
            dev.sinputs.push_back(b);
            if (!s || !a || !b) {   // (the reader and the parsers run: through fail() and the joins)
                fail("cannot create the staging contexts");
                break;
            }
            if (plan.ramp) sa_set_reserve(s, (uint32_t)plan.B);
        }
        st.enc_start = st.now();
        // (after a failure every encoder returns from its first claim, before it looks at its staging context)
        for (size_t ci = 0; ci < dev.ctxs.size(); ci++) encoders.emplace_back([this, ci]() { encode_loop(ci); });
    }

    // (under mu) the end of batch k: its blocks are [bstart(k), batch_end(k))
    int64_t batch_end(int64_t k) { return nblocks >= 0 ? std::min(nblocks, plan.bstart(k + 1)) : plan.bstart(k + 1); }

    bool batch_ready(int64_t k)   // under mu
    {
        if (!tmpl_ready || (nblocks < 0 && nread < batch_end(k))) return false;
        for (int64_t i = plan.bstart(k); i < batch_end(k); i++)
            if (jobs.count(i) == 0 || jobs[i]->state < 1) return false;
        return true;
    }

    // takes batch k (in order) once the reader has cut it: false when the input
    // is exhausted or the run failed
    bool claim(int64_t& k, std::vector<Job*>& js)
    {
        std::unique_lock<std::mutex> lk(mu);
        if (failed) return false;
        k = next_batch++;
        cv.wait(lk, [&] { return failed || (nblocks >= 0 && plan.bstart(k) >= nblocks) || batch_ready(k); });
        if (failed || (nblocks >= 0 && plan.bstart(k) >= nblocks)) return false;
        js.clear();
        for (int64_t i = plan.bstart(k); i < batch_end(k); i++) js.push_back(jobs[i].get());
        return true;
    }

    // STREAM: batch k once its first block is cut (and the ID template known):
    // false when the input ended before it or the run failed
    bool claim_first(int64_t& k)
    {
        std::unique_lock<std::mutex> lk(mu);
        if (failed) return false;
        k = next_batch++;
        cv.wait(lk, [&] {
            return failed || (nblocks >= 0 && plan.bstart(k) >= nblocks) || (tmpl_ready && nread > plan.bstart(k));
        });
        return !(failed || (nblocks >= 0 && plan.bstart(k) >= nblocks));
    }

    sa_text_block text_of(const Job& j) const   // a block's text (its second input only with pe)
    {
        return sa_text_block{j.t1.data(), j.t1.size(), pe ? j.t2.data() : nullptr, pe ? j.t2.size() : 0};
    }

    // the batch's texts are on the device: they go back to the reader, the jobs
    // take what the parse found; by_bound: their output buffers sized by the bound
    void staged_batch(const std::vector<Job*>& js, const std::vector<sa_text_info>& ti, bool give, bool by_bound)
    {
        for (size_t i = 0; i < js.size(); i++) {
            if (give) give_back(*js[i], texts);   // (the device holds the text now)
            js[i]->nreads = ti[i].nreads;
            js[i]->len_long = ti[i].len_long;
            if (by_bound) outpool.take(js[i]->out, ti[i].out_bound);
        }
    }

    // the batch's texts staged (H2D + device parse) since t0 -- WHOLE: into
    // context c's own input (I null; the output buffers by the bound only with
    // SA_CLI_OUT_EXACT=0, else by the encoded sizes after the run); AHEAD: into
    // input I with the staging context c -- and handed back to the reader
    bool stage(sa_ctx* c, sa_input* I, std::vector<Job*>& js, double t0, bool by_bound)
    {
        std::vector<sa_text_block> tin;
        for (Job* j : js) tin.push_back(text_of(*j));
        std::vector<sa_text_info> ti(js.size());
        if ((I ? sa_stage_text_input(c, I, tin.data(), (int)tin.size(), ti.data())
               : sa_stage_text(c, tin.data(), (int)tin.size(), ti.data())) != 0)
            return fail(std::string("staging failed: ") + sa_last_error(c)), false;
        Stamps::add(st.stage_busy, st.now() - t0);
        {
            std::lock_guard<std::mutex> g(mu);
            staged += (int64_t)js.size();
        }
        staged_batch(js, ti, true, by_bound);
        cv.notify_all();   // (text windows are free for the reader)
        return true;
    }

    // STREAM: the blocks of batch k to the device (text arena `slot` of ctx's
    // input), each as soon as the reader has cut it; its text goes back to the reader
    bool upload(sa_ctx* ctx, int slot, int64_t k, std::vector<Job*>& js)
    {
        js.clear();
        const int64_t b0 = plan.bstart(k), b1 = plan.bstart(k + 1);
        for (int64_t i = b0; i < b1; i++) {
            Job* j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return failed || (nblocks >= 0 && i >= nblocks) || (jobs.count(i) && jobs[i]->state >= 1); });
                if (failed) return false;
                if (nblocks >= 0 && i >= nblocks) break;
                j = jobs[i].get();
            }
            const sa_text_block tb = text_of(*j);
            const double t0 = st.now();
            if (j->dblk) {   // --gpu-text: the text is on the device already
                if (sa_text_upload_dev(ctx, nullptr, slot, (int)(i - b0), (int)(b1 - b0), j->dblk, plan.tstride) != 0)
                    return fail(std::string("staging failed: ") + sa_upload_error(ctx)), false;
                sa_devblock_release(j->dblk);
                j->dblk = nullptr;
                j->t1.release();   // (block 0's host copy: the parser is done with it)
                j->t2.release();
            } else if (sa_text_upload(ctx, nullptr, slot, (int)(i - b0), (int)(b1 - b0), &tb, plan.tstride) != 0)
                return fail(std::string("staging failed: ") + sa_last_error(ctx)), false;
            give_back(*j, texts);   // (the device holds the text now)
            {
                std::lock_guard<std::mutex> g(mu);
                staged++;
                Stamps::add(st.stage_busy, st.now() - t0);
            }
            cv.notify_all();
            js.push_back(j);
        }
        return true;
    }

    // STREAM: the uploaded batch parsed on the device, the output buffers by the bound
    bool parse_streamed(sa_ctx* ctx, int slot, Turn& t)
    {
        static const char kPe = 0;   // (a non-NULL text2 marks a PE block for sa_text_parse)
        std::vector<sa_text_block> lens(t.js.size());
        std::vector<sa_text_info> ti(t.js.size());
        for (size_t i = 0; i < t.js.size(); i++)
            lens[i] = sa_text_block{nullptr, t.js[i]->text1, pe ? reinterpret_cast<const uint8_t*>(&kPe) : nullptr,
                                    pe ? t.js[i]->text2 : 0};
        if (sa_text_parse(ctx, nullptr, slot, lens.data(), (int)t.js.size(), plan.tstride, ti.data()) != 0)
            return fail(std::string("staging failed: ") + sa_last_error(ctx)), false;
        staged_batch(t.js, ti, false, true);
        return true;
    }

    // the feed: the encoder's (or its helper's) next batch, as far towards the
    // device as the feed takes it outside the cycle.  1: t holds a batch, 0: no
    // more batches, -1: failed (fail() was called)
    int take(size_t ci, int slot, Turn& t)
    {
        t.asked = st.now();
        if (feed == STREAM) {
            if (!claim_first(t.k)) return 0;
            const bool ok = upload(dev.ctxs[ci], slot, t.k, t.js);
            t.ready = st.now();
            return ok ? 1 : -1;
        }
        if (!claim(t.k, t.js)) return 0;
        t.ready = st.now();
        if (feed == AHEAD && !stage(dev.stagers[ci], dev.sinputs[2 * ci + (size_t)slot], t.js, t.ready, true)) return -1;
        return 1;
    }

    int run(size_t ci, int slot, const sa_cfg& c, int64_t k)   // (the batch's place in the chain: k)
    {
        sa_ctx* ctx = dev.ctxs[ci];
        if (feed == AHEAD) {
            sa_input* I = dev.sinputs[2 * ci + (size_t)slot];
            return dev.chain ? sa_run_input_aligned(ctx, I, &c, &dev.acfg[ci], dev.chain, (uint64_t)k) : sa_run_input(ctx, I, &c);
        }
        return dev.chain ? sa_run_aligned(ctx, &c, &dev.acfg[ci], dev.chain, (uint64_t)k) : sa_run(ctx, &c);
    }

    static void point_outs(const std::vector<Job*>& js, std::vector<sa_out>& outs)
    {
        for (size_t i = 0; i < js.size(); i++) outs[i] = sa_out{js[i]->out.data(), js[i]->out.size(), 0};
    }

    // a batch with no device parse behind it: --ingest-only (the batch is taken,
    // its windows recycled), --host-only, --host-parse.  false: fail() was called
    bool host_batch(size_t ci, const sa_cfg& c, Turn& t, std::vector<sa_out>& outs)
    {
        sa_ctx* ctx = dev.ctxs[ci];
        std::vector<Job*>& js = t.js;
        if (plan.dev_parse) {
            for (size_t i = 0; i < js.size(); i++) {
                if (o.ingest_crc) {   // (a check of the delivered bytes, for the tests: CPU work no device path does)
                    uint32_t x = (uint32_t)crc32(0L, js[i]->t1.data(), (uInt)js[i]->t1.size());
                    if (pe) x = (uint32_t)crc32(x, js[i]->t2.data(), (uInt)js[i]->t2.size());
                    js[i]->crc = x;
                }
                give_back(*js[i], texts);
            }
            {
                std::lock_guard<std::mutex> g(mu);
                staged += (int64_t)js.size();
            }
            cv.notify_all();
            return true;
        }
        std::vector<sa_block> in(js.size());
        for (size_t i = 0; i < js.size(); i++) {
            in[i] = js[i]->p->view();
            outpool.take(js[i]->out, sa_output_bound(&in[i]));   // (uninitialised: only the real bytes are touched)
        }
        point_outs(js, outs);
        if (!ctx) {   // --host-only (SA_CLI_TEST_OUT=n: n bytes of filler a block)
            for (sa_out& x : outs) {
                x.size = std::min<uint64_t>(kn.test_out, x.cap);
                if (x.size) memset(x.data, 0x5a, x.size);
            }
        } else if (dev.chain) {
            if (sa_stage(ctx, in.data(), (int)in.size()) != 0 || run(ci, 0, c, t.k) != 0 ||
                sa_fetch(ctx, outs.data(), (int)outs.size()) != 0)
                return fail(std::string("encode failed: ") + sa_last_error(ctx)), false;
        } else if (sa_encode_blocks(ctx, in.data(), (int)in.size(), &c, outs.data()) != 0)
            return fail(std::string("encode failed: ") + sa_last_error(ctx)), false;
        return true;
    }

    // (-v) per batch: when it became ready, what each step took, device phases;
    // each feed has its own wording.  tp / tr / tf: the parse, run and fetch began
    void batch_line(sa_ctx* ctx, const Turn& t, double tp, double tr, double tf)
    {
        const char* pn[16];
        float pm[16];
        const int np = sa_phase_times(ctx, pn, pm, 16);
        std::string ph;
        for (int x = 0; x < np; x++) {
            char pb[48];
            snprintf(pb, sizeof pb, " %s %.0f", pn[x], pm[x]);
            ph += pb;
        }
        char steps[200];
        const double fetch = st.now() - tf;
        if (feed == AHEAD) {
            snprintf(steps, sizeof steps, "ready %.3f s, staged ahead, run from %.3f s for %.3f s, fetch %.3f s", t.ready, tr,
                     tf - tr, fetch);
        } else if (feed == STREAM) {
            snprintf(steps, sizeof steps, "uploaded %.3f s, parse %.3f s, run %.3f s, fetch %.3f s", t.ready, tr - tp, tf - tr,
                     fetch);
        } else {
            uint32_t grows = 0;
            double alloc_ms = 0;
            sa_alloc_stats(&grows, &alloc_ms);
            snprintf(steps, sizeof steps, "ready %.3f s, stage %.3f s, run %.3f s, fetch %.3f s; grows %u, alloc %.0f ms", t.ready,
                     tr - t.ready, tf - tr, fetch, grows, alloc_ms);
        }
        fprintf(stderr, "seqarc_amd: batch %lld (%zu blocks) context %p: asked %.3f s, %s; device ms:%s\n", (long long)t.k,
                t.js.size(), (void*)ctx, t.asked, steps, ph.c_str());
    }

    // one context's encoder: take (the feed), run, size and fetch, the -v line,
    // account, publish.  With a feed that works ahead, a helper thread takes
    // the next batch into the alternate input / arena (slot ^ 1) meanwhile.
    void encode_loop(size_t ci)
    {
        sa_ctx* ctx = dev.ctxs[ci];
        const bool device = ctx && plan.dev_parse;
        const bool helper = feed == AHEAD || (feed == STREAM && kn.prefetch);   // (SA_CLI_PREFETCH=0: after the batch, A/B)
        Turn cur;
        if (take(ci, 0, cur) <= 0) return;
        for (int slot = 0;; slot ^= 1) {
            const double tp = st.now();
            if (feed == STREAM && !parse_streamed(ctx, slot, cur)) return;
            Turn nxt;
            std::future<int> ahead;   // (declared after nxt: waited for before nxt goes)
            if (helper) ahead = std::async(std::launch::async, [&, s2 = slot ^ 1]() { return take(ci, s2, nxt); });
            Stamps::set_min(st.first_enc, cur.ready);
            std::vector<sa_out> outs(cur.js.size());
            const sa_cfg c = cfg;
            double busy_from = cur.ready;   // the feed's own start of its busy interval: ready, run or parse
            if (!device) {
                if (!host_batch(ci, c, cur, outs)) return;
            } else {
                if (feed == WHOLE && !stage(ctx, nullptr, cur.js, cur.ready, !kn.out_exact)) return;
                point_outs(cur.js, outs);
                const double tr = st.now();
                if (run(ci, slot, c, cur.k) != 0) return fail(std::string("encode failed: ") + sa_last_error(ctx));
                if (feed == WHOLE && kn.out_exact) {   // the output buffers sized by the encoded blocks
                    std::vector<uint64_t> fs(cur.js.size());
                    if (sa_fetch_sizes(ctx, fs.data(), (int)fs.size()) != 0)
                        return fail(std::string("fetch failed: ") + sa_last_error(ctx));
                    for (size_t i = 0; i < fs.size(); i++) outpool.take(cur.js[i]->out, fs[i]);
                    point_outs(cur.js, outs);
                }
                const double tf = st.now();
                if (sa_fetch(ctx, outs.data(), (int)outs.size()) != 0)
                    return fail(std::string("fetch failed: ") + sa_last_error(ctx));
                if (o.verbose) batch_line(ctx, cur, tp, tr, tf);
                if (feed != WHOLE) busy_from = feed == AHEAD ? tr : tp;
            }
            const double t1 = st.now();
            Stamps::add(st.enc_busy, t1 - busy_from);
            Stamps::set_max(st.last_enc, t1);
            {
                std::lock_guard<std::mutex> g(mu);
                for (size_t i = 0; i < cur.js.size(); i++) {
                    cur.js[i]->out.n = outs[i].size;
                    cur.js[i]->state = 2;
                }
            }
            cv.notify_all();
            const int r = helper ? ahead.get() : take(ci, slot ^ 1, nxt);
            if (r <= 0) return;   // (no more batches, or the feed failed: fail() was called)
            cur = std::move(nxt);
        }
    }

    // ---- stage: the writer (this thread): blocks in input order, each handed to
    // the archive writer's threads at its offset (ArcWriter); `written` counts
    // the blocks whose copy is done (the reader's bound on blocks in flight) ----
    void write_blocks()
    {
        const bool opened = aw.open(path, std::max(1, std::min(8, o.writers)), [this](std::unique_ptr<Job> j) {
            if (j->p) pool.put(std::move(j->p));
            outpool.give(j->out);
            j.reset();
            {
                std::lock_guard<std::mutex> g(mu);
                written++;
            }
            cv.notify_all();
        });
        if (!opened || !aw.lead(hdr, 16))   // patched at the end (createOutFile@0x417480 / writeFileInfo@0x4171b0)
            fail("cannot write " + path);
        for (int64_t i = 0;; i++) {
            std::unique_ptr<Job> j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] {
                    return failed || (nblocks >= 0 && i >= nblocks) || (jobs.count(i) && jobs[i]->state == 2);
                });
                if (failed || (nblocks >= 0 && i >= nblocks)) break;
                j = std::move(jobs[i]);
                jobs.erase(i);
            }
            if (aw.bad()) {   // writeData@0x40e070: exit(1)
                fail("write error on " + path);
                break;
            }
            info.push_back(sa_arc_block{(uint32_t)j->out.size(), j->len_long, j->text1, j->text2});
            text_crc = (uint32_t)crc32_combine(text_crc, j->crc, (z_off_t)(j->text1 + j->text2));
            const uint64_t off = 16 + total;
            total += j->out.size();
            aw.put(std::move(j), off);
        }
        st.written = st.now();
    }

    // ---- stage: every thread joined (after a failure too: fail() wakes them all) ----
    void join()
    {
        reader.join();
        for (auto& t : parsers) t.join();
        for (auto& t : encoders) t.join();
        if (seg_free.joinable()) {
            {
                std::lock_guard<std::mutex> g(mu);
                seg_stop = true;   // (wakes it when the run ended early)
                cv.notify_all();
            }
            seg_free.join();
        }
        st.joined = st.now();
    }

    // ---- stage: the trailer and the header, the archive closed -- before the
    // contexts' device buffers are released (~1.4 s for five contexts' ~200 GB).
    // false: the run failed (its message printed, the buffers released) ----
    bool finish_archive()
    {
        if (failed) {
            aw.finish(nullptr, 0, 0, nullptr, 0);
            dev.release();
            fprintf(stderr, "seqarc_amd: %s\n", err.c_str());
            return false;
        }
        sa_arc_info ai{o.f1, pe ? o.f2 : nullptr, pe ? 1 : 0, in1.is_gz ? 1 : 0, plus_bare, cfg.md5,
                       cfg.lossy > 0.0 ? 1 : 0, tmpl, o.ref ? rf.md5 : nullptr, (uint32_t)o.insert};
        std::vector<uint8_t> tr(4096 + 40 * info.size());
        tl = sa_arc_trailer2(&ai, o.maxmis, info.data(), (uint32_t)info.size(), tr.data(), tr.size());
        if (tl < 0) {
            fprintf(stderr, "seqarc_amd: trailer failed\n");
            rc = 1;
        } else {
            sa_arc_header(total, hdr);
        }
        if (!aw.finish(tl < 0 ? nullptr : tr.data(), tl < 0 ? 0 : (size_t)tl, 16 + total, tl < 0 ? nullptr : hdr, 16)) {
            if (tl >= 0) fprintf(stderr, "seqarc_amd: write error on %s\n", path.c_str());
            rc = 1;
        }
        st.closed = st.now();
        return true;
    }

    // ---- stage: the contexts' device buffers (~200 GB for five contexts) are
    // left to the process exit unless --release: the command line exits right
    // after this (compress, g_fast_exit), and the driver reclaims them without
    // the ~1.4 s of hipFree calls (round 3 g3n) ----
    void release_or_leave()
    {
        if (kn.exit_probe) {   // (diagnostics: what the exit would tear down, timed here instead)
            size_t nb = 0, cap = 0;
            const double p0 = st.now();
            {
                std::lock_guard<std::mutex> g(outpool.mu);
                nb = outpool.free.size();
                for (auto& b : outpool.free) cap += b.cap;
                outpool.free.clear();
            }
            const double p1 = st.now();
            dev.release();
            const double p2 = st.now();
            fprintf(stderr, "seqarc_amd: exit probe: output pool %zu buffers, %.3f GB reserved, freed in %.3f s; contexts "
                            "released in %.3f s\n", nb, (double)cap / 1e9, p1 - p0, p2 - p1);
        }
        if (o.release) dev.release();
        else dev.leave_to_exit();
        g_fast_exit = !o.release;
    }

    // ---- stage: the -v lines and the summary ----
    void report()
    {
        const double secs = st.now();
        if (o.verbose)
            fprintf(stderr, "seqarc_amd: blocks written %.3f s, segment ring freed %.3f s, encoders done %.3f s, archive closed %.3f s, contexts %s %.3f s\n",
                    st.written, st.seg_freed.load(), st.joined, st.closed, o.release ? "released" : "left to the exit", secs);
        if (tl < 0) return;
        if (o.verbose)
            fprintf(stderr,
                    "seqarc_amd: contexts ready %.3f s, encoders started %.3f s, input read %.3f s, first encode %.3f s, last encode "
                    "done %.3f s; encode busy %.3f s over %zu contexts, parse busy %.3f s over %d threads; "
                    "reader: fill %.3f s, cut %.3f s; stage %.3f s (%s parse)\n",
                    st.ctx, st.enc_start, st.read_done.load(), st.first_enc.load(), st.last_enc.load(), st.enc_busy.load(),
                    dev.ctxs.size(), st.parse_busy.load(), plan.nparse, st.fill_busy, st.cut_busy, st.stage_busy.load(),
                    plan.dev_parse ? "device" : "host");
        if (o.verbose && texts.pinned) {
            size_t nch;
            {
                std::lock_guard<std::mutex> g(texts.mu);
                nch = texts.chunks.size();
            }
            fprintf(stderr, "seqarc_amd: text windows: %zu chunks of %zu pinned (%zu ahead, %u on demand, the last at "
                            "%.3f s)\n", nch, TextPool::kChunk, plan.prefill_chunks, texts.on_demand.load(),
                    texts.last_on_demand.load());
        }
        if (o.ingest_only) fprintf(stderr, "seqarc_amd: ingest text crc32 %08x\n", text_crc);
        fprintf(stderr, "seqarc_amd: %zu block(s), %llu -> %llu bytes (%.2fx), %.3f s, %.1f MB/s\n", info.size(),
                (unsigned long long)total_in, (unsigned long long)(16 + total + tl),
                (double)total_in / (double)(16 + total + tl), secs, (double)total_in / secs / 1e6);
    }
};

// -c: the pipeline's stages in order
int compress(const Options& o, const cli::CliKnobs& kn)
{
    Pipeline p(o, kn);
    if (!p.open_inputs()) return 1;
    if (!p.plan.early_read && !p.create_contexts()) {
        fprintf(stderr, "seqarc_amd: %s\n", p.ctx_err.c_str());
        return 1;
    }
    p.start_reader();
    p.start_parsers();
    // early_read: the contexts now, beside the reader's first batch
    if (p.plan.early_read && !p.create_contexts()) p.fail(p.ctx_err);
    p.start_encoders();
    p.write_blocks();
    p.join();
    if (!p.finish_archive()) return 1;
    p.release_or_leave();
    p.report();
    if (g_fast_exit) fast_exit(p.rc, o.verbose);   // (every thread joined, the archive closed)
    return p.rc;
}


// ---- decompression --------------------------------------------------------
uint64_t be(const uint8_t* p, int n)
{
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v = (v << 8) | p[i];
    return v;
}

// EBML VINT (Encap::getValue@0x420680): value and width
uint64_t vint(const uint8_t* p, const uint8_t* end, int& w)
{
    w = 1;
    if (p >= end) { w = 0; return 0; }
    while (w <= 8 && !(p[0] & (0x80 >> (w - 1)))) w++;
    if (w > 8 || end - p < w) { w = 0; return 0; }
    uint64_t v = p[0] & ((0x80u >> (w - 1)) - 1);
    for (int i = 1; i < w; i++) v = (v << 8) | p[i];
    return v;
}

// One decoded block, written as FASTQ records.  mate: -1 all reads in order,
// 0 / 1 only the r1 / r2 reads of a PE block (DecodePipeOutJob::recoverData*,
// mode 1 / 2); bare: '+' lines without the ID.
void write_reads(FILE* f, FILE* f2, const std::vector<uint8_t>& names, const std::vector<uint16_t>& nl,
                 const std::vector<uint8_t>& seq, const std::vector<int32_t>& sl, const std::vector<uint8_t>& qual,
                 uint32_t n, bool paired, int mate, bool bare)
{
    const uint8_t *nm = names.data(), *sq = seq.data(), *ql = qual.data();
    for (uint32_t r = 0; r < n; r++) {
        const size_t L = (size_t)sl[r], N = nl[r];
        const bool keep = mate < 0 || (int)(r & 1) == mate;
        FILE* o = (paired && mate < 0 && f2 && (r & 1)) ? f2 : f;
        if (keep) {
            fputc('@', o);
            fwrite(nm, 1, N, o);
            fputc('\n', o);
            fwrite(sq, 1, L, o);
            fputs("\n+", o);
            if (!bare) fwrite(nm, 1, N, o);
            fputc('\n', o);
            fwrite(ql, 1, L, o);
            fputc('\n', o);
        }
        nm += N;
        sq += L;
        ql += L;
    }
}

// SeqArc -d: SeqArcFile::readFileInfo@0x419660 (header, trailer params, block
// table), -t blocks decoded at once (ISeqArcDecodeThread::doJob@0x435580),
// written in block order.  Output names (SeqArcParam::getDecodeFile@0x405f70,
// appendname@0x405f10): PREFIX_1.fastq / PREFIX_2.fastq (PE) or PREFIX.fastq
// (SE); without a prefix the stored input names (3 more bytes cut when input 1
// was gzip, as the binary does).  -P writes to stdout instead.
int decompress(const Options& o)
{
    std::vector<uint8_t> a;
    {
        FILE* f = fopen(o.arc, "rb");
        if (!f) { fprintf(stderr, "Error:The file %s may be not exist!\n", o.arc); return 1; }
        fseek(f, 0, SEEK_END);
        a.resize((size_t)ftell(f));
        fseek(f, 0, SEEK_SET);
        if (fread(a.data(), 1, a.size(), f) != a.size()) { fclose(f); return 1; }
        fclose(f);
    }
    if (a.size() < 16 || memcmp(a.data(), ".arc", 4) || a[7] != 0x82) {
        fprintf(stderr, "seqarc_amd: %s is not a SeqArc 1.6 archive\n", o.arc);
        return 1;
    }
    const uint64_t region = be(a.data() + 8, 8) & ((1ull << 56) - 1);
    if (16 + region > a.size()) return 1;
    const uint8_t *t = a.data() + 16 + region, *end = a.data() + a.size();
    int w;
    if (vint(t, end, w) != 3 || !w) return 1;
    t += w + 4;
    // params encap (ID 1, 2-byte size): fields 1-18 (writeParam@0x416450)
    if (vint(t, end, w) != 1 || !w) return 1;
    t += w;
    const uint64_t psz = be(t, 2) & 0x3fff;
    t += 2;
    const uint8_t* pend = t + psz;
    uint8_t tmpl[512] = {0};
    int bare = 1, paired = 0, lossy = 0, md5 = 1, gz1 = 0, noref = 1;
    uint32_t nblocks = 0, insert = 0;
    // SeqArc's default (param+0x1b60); field 19 when the archive was made with
    // another; an archive without field 19 (SeqArc's own, made with a
    // seqarc.config maxmis, or an earlier build of this tool) takes -d --maxmis
    int maxmis = o.maxmis_set ? o.maxmis : 7;
    std::string name1, name2;
    while (t < pend) {
        const uint64_t id = vint(t, pend, w);
        if (!w) return 1;
        t += w;
        const int sw = id == 15 ? 2 : 1;
        const uint64_t ln = be(t, sw) & ((1ull << (7 * sw)) - 1);
        t += sw;
        if (t + ln > pend) return 1;
        if (id == 1) noref = t[0];
        else if (id == 10 && ln >= 2) insert = (uint32_t)(t[0] | t[1] << 8);
        else if (id == 2) bare = t[0];
        else if (id == 4) gz1 = t[0];
        else if (id == 11 && ln >= 4) nblocks = (uint32_t)(t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24);
        else if (id == 13) name1.assign((const char*)t, ln);
        else if (id == 14 && ln) { paired = 1; name2.assign((const char*)t, ln); }
        else if (id == 15 && ln == 512) memcpy(tmpl, t, 512);
        else if (id == 16) lossy = t[0];
        else if (id == 17) md5 = t[0];
        else if (id == 19 && ln >= 1) maxmis = t[0];   // (ours: a non-default --maxmis)
        t += ln;
    }
    // writeMd5@0x416b10: the reference FASTA's MD5 (ID 8), archives made with one
    uint8_t arc_md5[16] = {0};
    bool have_md5 = false;
    if (vint(t, end, w) == 8 && w) {
        t += w;
        if (t + 17 > end || (be(t, 1) & 0x7f) != 16) return 1;
        memcpy(arc_md5, t + 1, 16);
        have_md5 = true;
        t += 17;
    }
    // the genome of an archive made with a reference (Decompress::loadRef: the
    // index's packed bases, or the FASTA packed the same way)
    RefFiles rf;
    std::vector<uint32_t> gwords;
    uint64_t gbases = 0;
    if (!noref) {
        if (!o.ref) {
            fprintf(stderr, "seqarc_amd: %s was made with a reference: give ref.fa\n", o.arc);
            return 1;
        }
        if (!load_ref(o.ref, false, rf, o.shm, o.verbose)) return 1;
        if (have_md5 && memcmp(arc_md5, rf.md5, 16)) {   // checkMd5@0x416c40
            fprintf(stderr, "seqarc_amd: the reference %s is not the one %s was made with (MD5)\n", o.ref, o.arc);
            return 1;
        }
        if (rf.have_hash()) {   // K, bases, words, positions; words follow
            uint32_t hdr[4];
            memcpy(hdr, rf.hp, 16);
            if (16 + 4ull * hdr[2] > rf.hn) {
                fprintf(stderr, "seqarc_amd: %s.hash is truncated\n", o.ref);
                return 1;
            }
            gbases = hdr[1];
            gwords.resize(hdr[2]);
            memcpy(gwords.data(), rf.hp + 16, 4ull * hdr[2]);
            rf.drop_hash();
        } else if (!pack_fasta(rf.fasta, gwords, gbases)) {
            fprintf(stderr, "seqarc_amd: %s: not a FASTA file\n", o.ref);
            return 1;
        }
    }
    if (maxmis < 0 || maxmis > 8) {
        fprintf(stderr, "seqarc_amd: maxmis %d in the archive trailer (0..8 expected)\n", maxmis);
        return 1;
    }
    const sa_ref gref{gwords.data(), gbases, paired, maxmis, insert};
    if (vint(t, end, w) != 7 || !w) return 1;
    t += w;
    const uint64_t bt = be(t, 4) & 0x0fffffff;
    t += 4;
    const uint32_t rec = paired ? 40 : 32;
    if (bt != (uint64_t)rec * nblocks || t + bt > end) return 1;
    struct Blk { uint64_t off, size, text; uint32_t lng; };
    std::vector<Blk> blks(nblocks);
    for (uint32_t b = 0; b < nblocks; b++) {
        const uint8_t* r = t + (size_t)rec * b;
        const uint32_t s2 = r[0] | r[1] << 8 | r[2] << 16 | (uint32_t)r[3] << 24;
        uint64_t off = 0;
        for (int k = 7; k >= 0; k--) off = (off << 8) | r[0x10 + k];
        const uint64_t text = paired ? (uint64_t)(r[4] | r[5] << 8 | r[6] << 16 | (uint32_t)r[7] << 24) +
                                           (uint64_t)(r[8] | r[9] << 8 | r[10] << 16 | (uint32_t)r[11] << 24)
                                     : (uint64_t)(r[8] | r[9] << 8 | r[10] << 16 | (uint32_t)r[11] << 24);
        blks[b] = Blk{off, s2 >> 1, text, s2 & 1u};
        if (off + blks[b].size > 16 + region) return 1;
    }
    sa_cfg cfg = o.cfg;
    cfg.md5 = md5;
    cfg.lossy = lossy ? 1.0 : 0.0;
    cfg.bin_mode = tmpl[0];

    // --gpu-decode takes the blocks of a no-reference, lossless archive; any other archive runs as without the switch
    struct GpuDec {
        sa_decoder* h = nullptr;
        ~GpuDec() { sa_decoder_destroy(h); }
    } gdec;
    if (o.gpu_decode) {
        if (!noref || lossy) {
            if (o.verbose)
                fprintf(stderr, "seqarc_amd: --gpu-decode does not apply (%s): running without it\n",
                        !noref ? "the archive was made with a reference" : "the archive was made with -l");
        } else if (!(gdec.h = sa_decoder_create(o.device))) {
            fprintf(stderr, "seqarc_amd: --gpu-decode: no usable gfx950 device %d\n", o.device);
            return 1;
        }
    }

    // outputs
    FILE *o1 = nullptr, *o2 = nullptr;
    int mate = -1;
    if (o.pipe) {   // DecodePipeOutJob ctor@0x42fd00: SE -> all reads; PE: 1 -> r1, 2 -> r2, 3 -> pairs in order
        if (o.pipe < 1 || o.pipe > 3) return usage();
        o1 = stdout;
        mate = !paired ? -1 : o.pipe == 1 ? 0 : o.pipe == 2 ? 1 : -1;
    } else {
        const std::string dir = o.in_dir ? dir_of(o.arc) : std::string();
        auto name = [&](int i) {   // getDecodeFile(i)
            if (o.out && *o.out) {
                std::string p = o.out;
                if (o.in_dir && p.find('/') == std::string::npos) p = dir + p;
                return p + (i == 0 ? ".fastq" : i == 1 ? "_1.fastq" : "_2.fastq");
            }
            std::string s = i <= 1 ? name1 : name2;
            if (gz1 && s.size() >= 3) s = s.substr(0, s.size() - 3);
            // the archive's stored names (trailer fields 13/14) are untrusted: the
            // encoder only ever stores basenames (compressStr@0x4160f0), so keep the
            // part after the last '/' and refuse '.', '..' and control characters
            const size_t sl = s.rfind('/');
            if (sl != std::string::npos) s = s.substr(sl + 1);
            bool bad = s == "." || s == "..";
            for (unsigned char ch : s) bad |= ch < 0x20 || ch == 0x7f;
            if (bad || s == "@empty*" || s.empty())
                s = std::string("decode") + (i == 0 ? ".fastq" : i == 1 ? "_1.fastq" : "_2.fastq");
            return dir + s;
        };
        const std::string p1 = name(paired ? 1 : 0), p2 = paired ? name(2) : std::string();
        if (!may_write(p1, o.force) || (paired && !may_write(p2, o.force))) return 1;
        o1 = fopen(p1.c_str(), "wb");
        o2 = paired ? fopen(p2.c_str(), "wb") : nullptr;
        if (!o1 || (paired && !o2)) { fprintf(stderr, "seqarc_amd: cannot write %s\n", p1.c_str()); return 1; }
    }
    struct Dec {
        std::vector<uint8_t> names, seq, qual;
        std::vector<uint16_t> nl;
        std::vector<int32_t> sl;
        sa_decoded d{};
        int64_t rc = -1;
    };
    int rc = 0, bad_md5 = 0;
    const uint32_t nt = (uint32_t)std::max(1, o.threads > 0 ? o.threads : 1);
    auto arrays = [&](Dec& d, const Blk& bk) {
        const uint64_t cap = bk.text + 64;   // names, bases, qualities each fit the FASTQ text
        d.names.resize(cap); d.seq.resize(cap); d.qual.resize(cap);
        d.nl.resize(cap / 4 + 8); d.sl.resize(cap / 4 + 8);
        d.d = sa_decoded{d.names.data(), d.nl.data(), d.seq.data(), d.sl.data(), d.qual.data(), cap, cap,
                         (uint32_t)(cap / 4 + 8), 0, 0};
    };
    auto host_decode = [&](Dec& d, const Blk& bk) {
        d.rc = noref ? sa_decode_block(a.data() + bk.off, bk.size, &cfg, tmpl, (int32_t)bk.lng, &d.d)
                     : sa_decode_block_ref(a.data() + bk.off, bk.size, &cfg, tmpl, (int32_t)bk.lng, &gref, &d.d);
    };
    // --gpu-decode: the first window is -t blocks, the later ones the plan's blocks in flight (what the last call
    // reported), none more than a quarter of the host's memory in output arrays
    uint32_t win = nt;
    const uint64_t host_cap = (uint64_t)sysconf(_SC_PHYS_PAGES) * (uint64_t)sysconf(_SC_PAGESIZE) / 4;
    sa_decode_info gsum{};
    for (uint32_t b0 = 0, n = 0; b0 < nblocks && !rc; b0 += n) {
        n = std::min(nt, nblocks - b0);
        if (gdec.h) {
            uint64_t bytes = 0;
            for (n = 0; b0 + n < nblocks && n < win; n++) {   // (at least one block)
                bytes += 3 * (blks[b0 + n].text + 64);
                if (n && bytes > host_cap) break;
            }
        }
        std::vector<Dec> ds(n);
        std::vector<uint32_t> todo;   // the blocks host threads decode: all of them without --gpu-decode
        if (gdec.h) {
            std::vector<const uint8_t*> in(n);
            std::vector<uint64_t> len(n);
            std::vector<int32_t> lng(n);
            std::vector<sa_decoded> outs(n);
            std::vector<uint32_t> status(n, 0);
            for (uint32_t i0 = 0; i0 < n; i0 += nt) {   // (the arrays' pages are touched on -t threads, as below)
                std::vector<std::thread> th;
                for (uint32_t i = i0; i < std::min(n, i0 + nt); i++) th.emplace_back([&, i]() { arrays(ds[i], blks[b0 + i]); });
                for (auto& x : th) x.join();
            }
            for (uint32_t i = 0; i < n; i++) {
                const Blk& bk = blks[b0 + i];
                in[i] = a.data() + bk.off;
                len[i] = bk.size;
                lng[i] = (int32_t)bk.lng;
                outs[i] = ds[i].d;
            }
            const int bad = sa_decode_blocks(gdec.h, in.data(), len.data(), lng.data(), n, &cfg, tmpl, (int)nt, outs.data(), status.data());
            if (bad < 0) {
                fprintf(stderr, "seqarc_amd: --gpu-decode: %s\n", sa_decoder_error(gdec.h));
                rc = 1;
                break;
            }
            sa_decode_info gi;
            sa_decoder_info(gdec.h, &gi);
            gsum.groups += gi.groups; gsum.qual_launches += gi.qual_launches; gsum.seq_launches += gi.seq_launches;
            gsum.unsupported += gi.unsupported; gsum.inflight = std::max(gsum.inflight, gi.inflight); gsum.slice = gi.slice;
            gsum.init_ms += gi.init_ms; gsum.qual_ms += gi.qual_ms; gsum.place_ms += gi.place_ms; gsum.seq_ms += gi.seq_ms;
            gsum.h2d_ms += gi.h2d_ms; gsum.d2h_ms += gi.d2h_ms;
            win = std::max(nt, gi.inflight);
            for (uint32_t i = 0; i < n; i++) {
                ds[i].d = outs[i];
                ds[i].rc = status[i] ? -1 : (int64_t)outs[i].nreads;
                if (status[i] == SA_DEC_UNSUPPORTED || status[i] == SA_DEC_STUCK) {   // the host takes the block
                    if (o.verbose)
                        fprintf(stderr, "seqarc_amd: --gpu-decode: block %u %s: the host decodes it\n", b0 + i,
                                status[i] == SA_DEC_STUCK ? "did not end in its launches" : "is not supported on the device");
                    todo.push_back(i);
                }
            }
        } else {
            for (uint32_t i = 0; i < n; i++) todo.push_back(i);
        }
        for (size_t k0 = 0; k0 < todo.size(); k0 += nt) {
            std::vector<std::thread> th;
            for (size_t k = k0; k < std::min(todo.size(), k0 + nt); k++)
                th.emplace_back([&, k]() {
                    Dec& d = ds[todo[k]];
                    if (!gdec.h) arrays(d, blks[b0 + todo[k]]);
                    host_decode(d, blks[b0 + todo[k]]);
                });
            for (auto& x : th) x.join();
        }
        for (uint32_t i = 0; i < n && !rc; i++) {
            Dec& d = ds[i];
            if (d.rc < 0) { fprintf(stderr, "seqarc_amd: block %u does not decode\n", b0 + i); rc = 1; break; }
            if (!d.d.md5_ok)   // (-l archives: a range-coder desync fills the rest of the block with N)
                fprintf(stderr, "seqarc_amd: block %u: Name/Seq/Qual md5 unequal%s\n", b0 + i,
                        lossy ? " (made with -l: its bases past a desync are N)" : "");
            bad_md5 |= !d.d.md5_ok;
            write_reads(o1, o2, d.names, d.nl, d.seq, d.sl, d.qual, d.d.nreads, paired, mate, bare);
        }
    }
    if (gdec.h && o.verbose)
        fprintf(stderr, "seqarc_amd: sa_decode_blocks: groups %u, inflight %u, slice %u, qual_launches %u, seq_launches %u, "
                        "unsupported %u, init_ms %.2f, qual_ms %.2f, place_ms %.2f, seq_ms %.2f, h2d_ms %.2f, d2h_ms %.2f\n",
                gsum.groups, gsum.inflight, gsum.slice, gsum.qual_launches, gsum.seq_launches, gsum.unsupported, gsum.init_ms,
                gsum.qual_ms, gsum.place_ms, gsum.seq_ms, gsum.h2d_ms, gsum.d2h_ms);
    if (o1 && o1 != stdout) fclose(o1);
    else if (o1) fflush(o1);
    if (o2) fclose(o2);
    if (bad_md5) {   // blockMd5Verify@0x414e00: "Name/Seq/Qual md5 unequal"
        fprintf(stderr, "seqarc_amd: Name/Seq/Qual md5 unequal\n");
        rc = rc ? rc : 3;
    }
    return rc;
}

}  // namespace

int main(int argc, char** argv)
{
    g_main_s = mono_s();
    setenv("SA_SYNC", "block", 0);   // encoder threads sleep on their streams (sa_create)
    Options o;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        auto val = [&](void) -> const char* { return i + 1 < argc ? argv[++i] : nullptr; };
        auto ival = [&](int& dst, int lo) -> bool {
            const char* v = val();
            if (!v) return false;
            dst = std::max(lo, atoi(v));
            return true;
        };
        if (!strcmp(a, "-c")) o.compress = true;
        else if (!strcmp(a, "-d")) o.decompress = true;
        else if (!strcmp(a, "-1")) { if (!(o.f1 = val())) return usage(); }
        else if (!strcmp(a, "-2")) { if (!(o.f2 = val())) return usage(); }
        else if (!strcmp(a, "-o")) { if (!(o.out = val())) return usage(); }
        else if (!strcmp(a, "-n")) o.cfg.md5 = 0;
        else if (!strcmp(a, "-f")) o.force = true;
        else if (!strcmp(a, "-p")) o.in_dir = true;
        else if (!strcmp(a, "-l")) { const char* v = val(); if (!v) return usage(); o.cfg.lossy = atof(v); }
        else if (!strcmp(a, "-P")) { if (!ival(o.pipe, 0)) return usage(); }
        else if (!strcmp(a, "-t")) { if (!ival(o.threads, 1)) return usage(); }
        else if (!strcmp(a, "--slevel")) { if (!ival(o.cfg.slevel, 0)) return usage(); }
        else if (!strcmp(a, "--qlevel")) { if (!ival(o.cfg.qlevel, 0)) return usage(); }
        else if (!strcmp(a, "--device")) { if (!ival(o.device, 0)) return usage(); }
        else if (!strcmp(a, "--devices")) { if (!ival(o.devices, 1)) return usage(); }
        else if (!strcmp(a, "--contexts")) { if (!ival(o.contexts, 1)) return usage(); }
        else if (!strcmp(a, "--batch")) { if (!ival(o.batch, 1)) return usage(); }
        else if (!strcmp(a, "--block-size")) { if (!ival(o.block_mib, 1)) return usage(); }
        else if (!strcmp(a, "--share-device")) o.share_device = true;
        else if (!strcmp(a, "--host-only")) o.host_only = true;
        else if (!strcmp(a, "--ingest-only")) o.ingest_only = true;
        else if (!strcmp(a, "--ingest-crc")) o.ingest_crc = true;
        else if (!strcmp(a, "--gpu-inflate")) o.gpu_inflate = true;
        else if (!strcmp(a, "--gpu-gunzip")) o.gpu_gunzip = true;
        else if (!strcmp(a, "--gpu-text")) o.gpu_text = true;
        else if (!strcmp(a, "--gpu-decode")) o.gpu_decode = true;
        else if (!strcmp(a, "--read-threads")) { if (!ival(o.read_threads, 0)) return usage(); }
        else if (!strcmp(a, "--writers")) { if (!ival(o.writers, 1)) return usage(); }
        else if (!strcmp(a, "--no-ramp")) o.ramp = false;
        else if (!strcmp(a, "--ramp")) o.ramp = true;
        else if (!strcmp(a, "--release")) o.release = true;
        else if (!strcmp(a, "--stage-ahead")) o.stage_ahead = true;
        else if (!strcmp(a, "--host-parse")) o.host_parse = true;
        else if (!strcmp(a, "-v")) o.verbose = true;
        else if (!strcmp(a, "-i")) { o.index = true; if (!(o.ref = val())) return usage(); }
        else if (!strcmp(a, "-s")) o.shm = true;
        else if (!strcmp(a, "-q")) {   // -q -i: the minimizer index (MINI_INDEX) is not part of this build
            fprintf(stderr, "seqarc_amd: -q (minimizer index) is not part of this build; the HASH index is\n");
            return 2;
        }
        else if (!strcmp(a, "-I")) { if (!ival(o.insert, 0)) return usage(); o.insert = std::min(o.insert, 65535); }
        else if (!strcmp(a, "--maxmis")) {   // the Mis model (compressAlignInfo_Mis@0x425ff0) exists for 1..8
            if (!ival(o.maxmis, 0) || o.maxmis > 8) {
                fprintf(stderr, "seqarc_amd: --maxmis takes 0..8\n");
                return usage();
            }
            o.maxmis_set = true;
        }
        else if (a[0] != '-') pos.push_back(a);
        else return usage();
    }
    if (o.index) {
        if (o.compress || o.decompress || !pos.empty()) return usage();
        return build_index(o);
    }
    if (o.compress == o.decompress) return usage();
    if (o.compress && o.cfg.lossy > 0.0)   // (the reference's R-Block decoder loses sync on N / IUPAC bases)
        fprintf(stderr, "seqarc_amd: warning: -l: blocks with N / IUPAC bases may not decode back to their "
                        "bases (as in SeqArc 1.6); -d reports such blocks\n");
    // the first positional argument is the reference when it names a FASTA
    // (SeqArcParam::parseOptFromCmd@0x40b460: the argument before the inputs)
    if (!pos.empty() && is_fasta_name(pos[0])) {
        o.ref = pos[0];
        pos.erase(pos.begin());
    }
    if (o.decompress) {   // SeqArc -d [ref.fa] ARCHIVE [PREFIX]
        if (pos.empty() || pos.size() > 2) return usage();
        o.arc = pos[0];
        if (pos.size() == 2 && !o.out) o.out = pos[1];
        return decompress(o);
    }
    // SeqArc -c [ref.fa] -1 A [-2 B] OUT
    for (const char* p : pos) {
        if (o.out) return usage();
        o.out = p;
    }
    if (!o.f1 || !o.out) return usage();
    if (o.gpu_text && (o.ingest_only || o.host_only || o.host_parse || o.stage_ahead)) {
        fprintf(stderr, "seqarc_amd: --gpu-text keeps the text on the device: not with --ingest-only, --host-only, "
                        "--host-parse or --stage-ahead\n");
        return usage();
    }
    // one hardware queue per stream (four per context): with the runtime's
    // default of four queues (which the GPU boxes preset), the contexts' streams
    // share queues and one context's packets wait behind another's (DESIGN.md
    // 5); set before the device is used, overriding a preset value
    // (plan_hw_queues, cli_knobs.h)
    const cli::CliKnobs knobs = cli::parse_cli_knobs([](const char* n) -> const char* { return std::getenv(n); });
    setenv("GPU_MAX_HW_QUEUES", std::to_string(cli::plan_hw_queues(knobs, o.contexts)).c_str(), 1);   // (per device)
    const int rc = compress(o, knobs);
    if (o.verbose && !o.decompress)   // (a compression that released its buffers: the same stamps)
        fprintf(stderr, "seqarc_amd: monotonic clock: main %.6f, exit %.6f\n", g_main_s, mono_s());
    return rc;
}
