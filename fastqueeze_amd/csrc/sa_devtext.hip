// sa_devtext.hip -- an input's FASTQ text as a stream in device memory, and the
// reader's block cut done where the text is (sa_devtext_*, sa_devblock_*,
// sa_inflate_members_dev, sa_text_upload_dev).
// Included by sa_engine.hip after sa_parse.hip and sa_inflate.hip (needs DBuf,
// sa_ctx, PARSE_TILE, wg256_excl_scan, sa_inflater and k_inflate_bgzf).
//
// A devtext is one linear buffer [0, cap) with a read position rd and a write
// position wr, rd <= wr <= cap, and one newline count per 4 KiB tile of the
// buffer.  Text is appended at wr; when the room behind wr runs out the unread
// bytes [rd, wr) move to the front, and their tiles are counted again (the
// move does not keep rd's place within its tile, so the old counts do not
// apply to the moved bytes).
//
// Kernels (on the devtext's own stream):
//   k_dt_count  one tile per workgroup, 256 threads x 16 bytes: the tile's
//               newlines up to wr.  Runs once over the bytes of every append
//               (the tile that held the old wr is counted again, whole).
//   k_dt_cut    ONE wave: cuts the blocks of a call one after the other with
//               sa_devcut.h's dc_cut_blocks; reads the tile counts of whole
//               tiles and the bytes of partial ones, writes the lengths.
// Bounds: k_dt_count reads 16-byte groups that begin below wr, i.e. bytes
// below wr + 16 <= cap + 16 of a buffer of cap + 32 bytes, and writes
// tiles[t] for t <= (wr - 1) / 4096 < cap / 4096 + 1 of an array of
// cap / 4096 + 2.  k_dt_cut reads text below wr (dc_mask16: below the 16-byte
// boundary after it), tiles below wr / 4096, `first` below flen and writes
// len1 / len2 below max_blocks and res[0..2).
#include "sa_devcut.h"

namespace {

static_assert(DC_TILE == PARSE_TILE, "the devtext's tiles are the parse's tiles");

__global__ __launch_bounds__(256) void k_dt_count(const uint8_t* __restrict__ text, uint64_t tile0, uint64_t wr,
                                                  uint32_t* __restrict__ tiles)
{
    __shared__ uint32_t sh[4];
    const uint64_t tile = tile0 + blockIdx.x;
    const uint32_t n = dc_tile_thread_count(text, tile, wr, threadIdx.x);
    uint32_t ex;
    wg256_excl_scan(n, ex, sh);
    if (threadIdx.x == 255) tiles[tile] = ex + n;
}

// one wave; every loop of dc_cut_blocks is bounded (sa_devcut.h), none waits for another wave
__global__ __launch_bounds__(64) void k_dt_cut(DcSide s1, DcSide s2, uint32_t pe, uint64_t bs, const uint8_t* first,
                                               uint64_t flen, uint64_t* len1, uint64_t* len2, uint32_t max_blocks,
                                               uint32_t* res)
{
    const DcWaveLanes ln{threadIdx.x};
    int32_t end = 0;
    const uint32_t nb = dc_cut_blocks(ln, s1, s2, pe != 0, bs, first, flen, len1, len2, max_blocks, &end);
    if (threadIdx.x == 0) {
        res[0] = nb;
        res[1] = (uint32_t)end;
    }
}

// allocations of devblocks, per device, recycled (the command line's TextPool, in HBM)
struct DevBlockPool {
    std::mutex mu;
    std::vector<std::pair<void*, size_t>> idle;
};
DevBlockPool& devblock_pool(int device)
{
    static DevBlockPool pools[64];
    return pools[device & 63];
}

}  // namespace

struct sa_devtext {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    uint8_t* buf = nullptr;      // cap + 32 bytes
    uint32_t* tiles = nullptr;   // cap / DC_TILE + 2 counts
    uint8_t* bounce = nullptr;   // `piece` bytes, made by the first move that needs it
    uint64_t cap = 0, rd = 0, wr = 0, piece = 0;
    DBuf d_first, d_len1, d_len2, d_res;
    float count_ms = 0.f, cut_ms = 0.f;
    uint64_t count_bytes = 0;
    std::string err;
    ~sa_devtext()
    {
        for (DBuf* b : {&d_first, &d_len1, &d_len2, &d_res}) b->release();
        for (void* p : {(void*)buf, (void*)tiles, (void*)bounce})
            if (p) (void)hipFree(p);
        for (hipEvent_t e : {ev0, ev1, ev2, ev3})
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

struct sa_devblock {
    int device = 0;
    uint8_t* p = nullptr;
    size_t cap = 0;
    uint64_t len1 = 0, len2 = 0, off2 = 0;
    int pe = 0;
};

#define DT_CHECK(dt, expr)                                                  \
    do {                                                                    \
        hipError_t e_ = (expr);                                             \
        if (e_ != hipSuccess) {                                             \
            (dt)->err = std::string(#expr) + ": " + hipGetErrorString(e_);  \
            return -1;                                                      \
        }                                                                   \
    } while (0)

namespace {

// counts the tiles that hold [lo, hi) of a text that ends at hi; returns synchronised
int dt_count(sa_devtext* dt, uint64_t lo, uint64_t hi)
{
    if (lo >= hi) return 0;
    const uint64_t t0 = lo / DC_TILE, t1 = (hi + DC_TILE - 1) / DC_TILE;
    DT_CHECK(dt, hipEventRecord(dt->ev0, dt->st));
    hipLaunchKernelGGL(k_dt_count, dim3((uint32_t)(t1 - t0)), dim3(256), 0, dt->st, dt->buf, t0, hi, dt->tiles);
    DT_CHECK(dt, hipGetLastError());
    DT_CHECK(dt, hipEventRecord(dt->ev1, dt->st));
    DT_CHECK(dt, hipStreamSynchronize(dt->st));
    DT_CHECK(dt, hipEventElapsedTime(&dt->count_ms, dt->ev0, dt->ev1));
    dt->count_bytes = hi - t0 * DC_TILE;
    return 0;
}

// Room for n bytes behind wr: moves the unread bytes to the front when needed.
// Source [rd, wr) and destination [0, wr - rd) may overlap, and a device copy
// of overlapping ranges is undefined, so the move goes in pieces in ascending
// order on the stream, each piece's source and destination apart: pieces of rd
// bytes (a piece's destination ends where its source begins), or, when rd is
// smaller than `piece`, pieces through a bounce buffer.
int dt_make_room(sa_devtext* dt, uint64_t n)
{
    const uint64_t have = dt->wr - dt->rd;
    if (n > dt->cap - have) return -3;
    if (n <= dt->cap - dt->wr) return 0;
    if (have) {
        const uint64_t gap = dt->rd;   // > 0: wr + n > cap >= have + n
        if (gap >= have) {
            DT_CHECK(dt, hipMemcpyAsync(dt->buf, dt->buf + dt->rd, have, hipMemcpyDeviceToDevice, dt->st));
        } else if (gap >= dt->piece) {
            for (uint64_t o = 0; o < have; o += gap)
                DT_CHECK(dt, hipMemcpyAsync(dt->buf + o, dt->buf + dt->rd + o, std::min(gap, have - o),
                                            hipMemcpyDeviceToDevice, dt->st));
        } else {
            if (!dt->bounce) DT_CHECK(dt, hipMalloc((void**)&dt->bounce, dt->piece));
            for (uint64_t o = 0; o < have; o += dt->piece) {
                const uint64_t m = std::min(dt->piece, have - o);
                DT_CHECK(dt, hipMemcpyAsync(dt->bounce, dt->buf + dt->rd + o, m, hipMemcpyDeviceToDevice, dt->st));
                DT_CHECK(dt, hipMemcpyAsync(dt->buf + o, dt->bounce, m, hipMemcpyDeviceToDevice, dt->st));
            }
        }
        DT_CHECK(dt, hipStreamSynchronize(dt->st));
    }
    dt->rd = 0;
    dt->wr = have;
    return dt_count(dt, 0, have);
}

}  // namespace

extern "C" {

sa_devtext* sa_devtext_create(int device, uint64_t capacity)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || !capacity) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return nullptr;
    sa_devtext* dt = new sa_devtext();
    dt->device = device;
    dt->cap = capacity;
    // the move's piece: 1/256 of the buffer, 64 KiB .. 4 MiB (a 1 GiB buffer moves in at most 512 copies)
    dt->piece = std::min<uint64_t>(std::max<uint64_t>(capacity / 256 / DC_TILE * DC_TILE, 64u << 10), 4u << 20);
    const uint64_t ntiles = capacity / DC_TILE + 2;
    if (hipStreamCreateWithFlags(&dt->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&dt->ev0) != hipSuccess ||
        hipEventCreate(&dt->ev1) != hipSuccess || hipEventCreate(&dt->ev2) != hipSuccess ||
        hipEventCreate(&dt->ev3) != hipSuccess || hipMalloc((void**)&dt->buf, capacity + 32) != hipSuccess ||
        hipMalloc((void**)&dt->tiles, 4 * ntiles) != hipSuccess ||
        hipMemsetAsync(dt->tiles, 0, 4 * ntiles, dt->st) != hipSuccess || hipStreamSynchronize(dt->st) != hipSuccess) {
        delete dt;
        return nullptr;
    }
    return dt;
}

void sa_devtext_destroy(sa_devtext* dt)
{
    if (!dt) return;
    (void)hipSetDevice(dt->device);
    const int device = dt->device;
    delete dt;
    sa_devblock_pool_trim(device);
}

const char* sa_devtext_error(const sa_devtext* dt) { return dt ? dt->err.c_str() : "no devtext"; }

uint64_t sa_devtext_avail(const sa_devtext* dt) { return dt ? dt->wr - dt->rd : 0; }

uint64_t sa_devtext_room(const sa_devtext* dt) { return dt ? dt->cap - (dt->wr - dt->rd) : 0; }

void sa_devtext_kernel_ms(const sa_devtext* dt, float* count_ms, float* cut_ms)
{
    if (count_ms) *count_ms = dt ? dt->count_ms : 0.f;
    if (cut_ms) *cut_ms = dt ? dt->cut_ms : 0.f;
}

uint64_t sa_devtext_count_bytes(const sa_devtext* dt) { return dt ? dt->count_bytes : 0; }

int sa_devtext_append(sa_devtext* dt, const uint8_t* bytes, uint64_t n)
{
    if (!dt) return -1;
    dt->err.clear();
    if (n && !bytes) {
        dt->err = "sa_devtext_append: null argument";
        return -1;
    }
    if (n > sa_devtext_room(dt)) {
        dt->err = "sa_devtext_append: more bytes than sa_devtext_room";
        return -3;
    }
    if (!n) return 0;
    DT_CHECK(dt, hipSetDevice(dt->device));
    if (const int rc = dt_make_room(dt, n)) return rc;
    DT_CHECK(dt, hipMemcpyAsync(dt->buf + dt->wr, bytes, n, hipMemcpyHostToDevice, dt->st));
    if (dt_count(dt, dt->wr, dt->wr + n)) return -1;
    dt->wr += n;
    return 0;
}

int sa_inflate_members_dev(sa_inflater* f, const uint8_t* in, uint64_t in_bytes, const sa_bgzf_member* ms, uint32_t n,
                           sa_devtext* dt, uint32_t* status)
{
    if (!f) return -1;
#define INFL_CHECK(expr)                                                     \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            f->err = std::string(#expr) + ": " + hipGetErrorString(e_);      \
            return -1;                                                       \
        }                                                                    \
    } while (0)
    f->err.clear();
    f->kernel_ms = 0.f;
    if ((n && !ms) || (in_bytes && !in) || !dt || dt->device != f->device) {
        f->err = "sa_inflate_members_dev: null argument, or a devtext of another device";
        return -1;
    }
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        const sa_bgzf_member& m = ms[i];
        if (m.in_off > in_bytes || m.in_len > in_bytes - m.in_off || m.isize > INFL_MAX_ISIZE) {
            f->err = "sa_inflate_members_dev: member " + std::to_string(i) + " lies outside the input or is larger than 64 KiB";
            return -2;
        }
        total += m.isize;
    }
    if (total > sa_devtext_room(dt)) {
        f->err = "sa_inflate_members_dev: the members' text exceeds sa_devtext_room";
        return -3;
    }
    if (!n) return 0;
    INFL_CHECK(hipSetDevice(f->device));
    if (dt_make_room(dt, total)) {
        f->err = "sa_inflate_members_dev: " + dt->err;
        return -1;
    }
    // the members back to back from the write position: the kernel gets the devtext's base
    // (16-byte aligned) as `out`, so that out_off & 15 is the text's place mod 16
    std::vector<sa_bgzf_member> at(ms, ms + n);
    uint64_t o = dt->wr;
    for (sa_bgzf_member& m : at) {
        m.out_off = o;
        o += m.isize;   // <= wr + total <= cap
    }
    INFL_CHECK(f->d_in.ensure(in_bytes + 16));
    INFL_CHECK(f->d_ms.ensure(sizeof(sa_bgzf_member) * (size_t)n));
    INFL_CHECK(f->d_status.ensure(4ull * n));
    if (in_bytes) INFL_CHECK(hipMemcpyAsync(f->d_in.p, in, in_bytes, hipMemcpyHostToDevice, f->st));
    INFL_CHECK(hipMemcpyAsync(f->d_ms.p, at.data(), sizeof(sa_bgzf_member) * (size_t)n, hipMemcpyHostToDevice, f->st));
    INFL_CHECK(hipMemsetAsync(f->d_counter.p, 0, 4, f->st));
    INFL_CHECK(hipEventRecord(f->ev0, f->st));
    hipLaunchKernelGGL(k_inflate_bgzf, dim3(std::min(f->grid, n)), dim3(64), INFL_LDS_BYTES, f->st, f->d_in.as<uint8_t>(),
                       f->d_ms.as<sa_bgzf_member>(), n, dt->buf, f->d_status.as<uint32_t>(), f->d_counter.as<uint32_t>());
    INFL_CHECK(hipGetLastError());
    INFL_CHECK(hipEventRecord(f->ev1, f->st));
    f->h_status.resize(n);
    INFL_CHECK(hipMemcpyAsync(f->h_status.data(), f->d_status.p, 4ull * n, hipMemcpyDeviceToHost, f->st));
    INFL_CHECK(hipStreamSynchronize(f->st));   // (at.data() and the text are done with)
    INFL_CHECK(hipEventElapsedTime(&f->kernel_ms, f->ev0, f->ev1));
    int bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (status) status[i] = f->h_status[i];
        bad += f->h_status[i] != 0;
    }
    if (bad) return bad;
    if (dt_count(dt, dt->wr, dt->wr + total)) {
        f->err = "sa_inflate_members_dev: " + dt->err;
        return -1;
    }
    dt->wr += total;
    return 0;
#undef INFL_CHECK
}

int sa_devtext_peek(sa_devtext* dt, uint64_t off, uint8_t* out, uint64_t n)
{
    if (!dt) return -1;
    dt->err.clear();
    if ((n && !out) || off > dt->wr - dt->rd || n > dt->wr - dt->rd - off) {
        dt->err = "sa_devtext_peek: null argument, or bytes past the write position";
        return -1;
    }
    if (!n) return 0;
    DT_CHECK(dt, hipSetDevice(dt->device));
    DT_CHECK(dt, hipMemcpyAsync(out, dt->buf + dt->rd + off, n, hipMemcpyDeviceToHost, dt->st));
    DT_CHECK(dt, hipStreamSynchronize(dt->st));
    return 0;
}

int64_t sa_devtext_cut(sa_devtext* t1, int eof1, sa_devtext* t2, int eof2, uint64_t block_size, const uint8_t* first,
                       uint64_t flen, uint64_t* len1, uint64_t* len2, uint64_t max_blocks, int32_t* end)
{
    if (!t1) return -1;
    sa_devtext* dt = t1;
    dt->err.clear();
    if (!first || !flen || !len1 || !end || !max_blocks || (t2 && (!len2 || t2->device != t1->device || t2 == t1)) ||
        block_size < (t2 ? 2u : 1u) || flen > (64u << 20)) {
        dt->err = "sa_devtext_cut: invalid argument";
        return -1;
    }
    const uint32_t maxb = (uint32_t)std::min<uint64_t>(max_blocks, 1u << 20);
    DT_CHECK(dt, hipSetDevice(dt->device));
    DT_CHECK(dt, dt->d_first.ensure(flen));
    DT_CHECK(dt, dt->d_len1.ensure(8ull * maxb));
    DT_CHECK(dt, dt->d_len2.ensure(8ull * maxb));
    DT_CHECK(dt, dt->d_res.ensure(8));
    // (both devtexts are at rest: every call on them returned synchronised)
    const DcSide s1{t1->buf, t1->tiles, t1->rd, t1->wr, eof1 ? 1 : 0, 0};
    const DcSide s2 = t2 ? DcSide{t2->buf, t2->tiles, t2->rd, t2->wr, eof2 ? 1 : 0, 0} : s1;
    DT_CHECK(dt, hipMemcpyAsync(dt->d_first.p, first, flen, hipMemcpyHostToDevice, dt->st));
    DT_CHECK(dt, hipEventRecord(dt->ev2, dt->st));
    hipLaunchKernelGGL(k_dt_cut, dim3(1), dim3(64), 0, dt->st, s1, s2, t2 ? 1u : 0u, block_size, dt->d_first.as<uint8_t>(),
                       flen, dt->d_len1.as<uint64_t>(), dt->d_len2.as<uint64_t>(), maxb, dt->d_res.as<uint32_t>());
    DT_CHECK(dt, hipGetLastError());
    DT_CHECK(dt, hipEventRecord(dt->ev3, dt->st));
    uint32_t res[2] = {0, 0};
    DT_CHECK(dt, hipMemcpyAsync(res, dt->d_res.p, 8, hipMemcpyDeviceToHost, dt->st));
    DT_CHECK(dt, hipStreamSynchronize(dt->st));
    DT_CHECK(dt, hipEventElapsedTime(&dt->cut_ms, dt->ev2, dt->ev3));
    if (res[0] > maxb) {
        dt->err = "sa_devtext_cut: internal: more blocks than asked for";
        return -1;
    }
    if (res[0]) {
        DT_CHECK(dt, hipMemcpyAsync(len1, dt->d_len1.p, 8ull * res[0], hipMemcpyDeviceToHost, dt->st));
        if (t2) DT_CHECK(dt, hipMemcpyAsync(len2, dt->d_len2.p, 8ull * res[0], hipMemcpyDeviceToHost, dt->st));
        DT_CHECK(dt, hipStreamSynchronize(dt->st));
    }
    *end = (int32_t)res[1];
    return (int64_t)res[0];
}

sa_devblock* sa_devtext_take(sa_devtext* t1, uint64_t len1, sa_devtext* t2, uint64_t len2)
{
    if (!t1) return nullptr;
    t1->err.clear();
    if (len1 > t1->wr - t1->rd || (t2 && (len2 > t2->wr - t2->rd || t2->device != t1->device)) || (!t2 && len2)) {
        t1->err = "sa_devtext_take: more bytes than the devtext holds";
        return nullptr;
    }
    auto fail = [&](hipError_t e, const char* what) {
        t1->err = std::string(what) + ": " + hipGetErrorString(e);
        return (sa_devblock*)nullptr;
    };
    hipError_t e = hipSetDevice(t1->device);
    if (e != hipSuccess) return fail(e, "hipSetDevice");
    const uint64_t off2 = (len1 + 255) & ~255ull;
    const size_t need = (size_t)(off2 + len2 + 256);
    sa_devblock* b = new sa_devblock();
    b->device = t1->device;
    {   // the smallest idle allocation that is large enough
        DevBlockPool& P = devblock_pool(t1->device);
        std::lock_guard<std::mutex> g(P.mu);
        size_t best = P.idle.size();
        for (size_t i = 0; i < P.idle.size(); i++)
            if (P.idle[i].second >= need && (best == P.idle.size() || P.idle[i].second < P.idle[best].second)) best = i;
        if (best < P.idle.size()) {
            b->p = (uint8_t*)P.idle[best].first;
            b->cap = P.idle[best].second;
            P.idle.erase(P.idle.begin() + (long)best);
        }
    }
    if (!b->p) {
        // (room for a somewhat longer block of the same input: whole MiB, 1/8 on top)
        const size_t want = ((need + need / 8) + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
        e = hipMalloc((void**)&b->p, want);
        if (e != hipSuccess) {
            delete b;
            return fail(e, "hipMalloc (devblock)");
        }
        b->cap = want;
    }
    b->len1 = len1;
    b->len2 = len2;
    b->off2 = off2;
    b->pe = t2 ? 1 : 0;
    e = len1 ? hipMemcpyAsync(b->p, t1->buf + t1->rd, len1, hipMemcpyDeviceToDevice, t1->st) : hipSuccess;
    if (e == hipSuccess && t2 && len2)
        e = hipMemcpyAsync(b->p + off2, t2->buf + t2->rd, len2, hipMemcpyDeviceToDevice, t1->st);
    if (e == hipSuccess) e = hipStreamSynchronize(t1->st);
    if (e != hipSuccess) {
        sa_devblock_release(b);
        return fail(e, "sa_devtext_take: copy");
    }
    t1->rd += len1;
    if (t2) t2->rd += len2;
    return b;
}

void sa_devblock_release(sa_devblock* b)
{
    if (!b) return;
    if (b->p) {
        DevBlockPool& P = devblock_pool(b->device);
        std::lock_guard<std::mutex> g(P.mu);
        P.idle.emplace_back(b->p, b->cap);
    }
    delete b;
}

void sa_devblock_pool_trim(int device)
{
    DevBlockPool& P = devblock_pool(device);
    std::vector<std::pair<void*, size_t>> idle;
    {
        std::lock_guard<std::mutex> g(P.mu);
        idle.swap(P.idle);
    }
    if (idle.empty()) return;
    (void)hipSetDevice(device);
    for (auto& a : idle) (void)hipFree(a.first);
}

int sa_devblock_lens(const sa_devblock* b, uint64_t* len1, uint64_t* len2)
{
    if (len1) *len1 = b ? b->len1 : 0;
    if (len2) *len2 = b ? b->len2 : 0;
    return b ? b->pe : 0;
}

int sa_devblock_fetch(const sa_devblock* b, uint8_t* out1, uint8_t* out2)
{
    if (!b || (b->len1 && !out1)) return -1;
    if (hipSetDevice(b->device) != hipSuccess) return -1;
    if (b->len1 && hipMemcpy(out1, b->p, b->len1, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (out2 && b->len2 && hipMemcpy(out2, b->p + b->off2, b->len2, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

// sa_text_upload with a device source.  A helper thread may run this while
// sa_run of the same context runs, so it never writes c->err: its error text
// is c->upload_err, written and read under copy_mu.
int sa_text_upload_dev(sa_ctx* c, sa_input* I, int slot, int index, int nmax, const sa_devblock* blk, uint64_t stride)
{
    if (!c) return -1;
    if (!I) I = &c->own;
    stride = (stride + PARSE_TILE - 1) / PARSE_TILE * PARSE_TILE;
    std::lock_guard<std::mutex> g(c->copy_mu);   // (one uploader per context at a time)
    c->upload_err.clear();
    if (!blk || slot < 0 || slot > 1 || index < 0 || index >= nmax || !stride || blk->len1 > stride || blk->len2 > stride ||
        I->device != c->device || blk->device != c->device) {
        c->upload_err = "sa_text_upload_dev: invalid block, slot, index or stride";
        return -1;
    }
#define UP_CHECK(expr)                                                          \
    do {                                                                        \
        hipError_t e_ = (expr);                                                 \
        if (e_ != hipSuccess) {                                                 \
            c->upload_err = std::string(#expr) + ": " + hipGetErrorString(e_);  \
            return -1;                                                          \
        }                                                                       \
    } while (0)
    UP_CHECK(hipSetDevice(c->device));
    if (!c->st_copy) UP_CHECK(hipStreamCreateWithFlags(&c->st_copy, hipStreamNonBlocking));
    DBuf& arena = slot ? I->d_text_b : I->d_text;
    if (index == 0 && arena.cap < 2ull * (uint64_t)nmax * stride) UP_CHECK(arena.ensure(2ull * (uint64_t)nmax * stride));
    if (arena.cap < 2ull * (uint64_t)(index + 1) * stride) {
        c->upload_err = "sa_text_upload_dev: block 0 of the batch was not uploaded first";
        return -1;
    }
    uint8_t* d = arena.as<uint8_t>() + 2ull * (uint64_t)index * stride;
    if (blk->len1) UP_CHECK(hipMemcpyAsync(d, blk->p, blk->len1, hipMemcpyDeviceToDevice, c->st_copy));
    if (blk->pe && blk->len2)
        UP_CHECK(hipMemcpyAsync(d + stride, blk->p + blk->off2, blk->len2, hipMemcpyDeviceToDevice, c->st_copy));
    UP_CHECK(hipStreamSynchronize(c->st_copy));
    return 0;
#undef UP_CHECK
}

const char* sa_upload_error(sa_ctx* c)
{
    static thread_local std::string copy;
    if (!c) return "no context";
    std::lock_guard<std::mutex> g(c->copy_mu);
    copy = c->upload_err;
    return copy.c_str();
}

}  // extern "C"

#undef DT_CHECK
