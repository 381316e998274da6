// sa_decode.hip -- archive blocks decoded on the device (sa_decode_blocks): the
// kernels over sa_decode_logic.h and the device backend of sa_decoder.h's driver.
// A translation unit of its own beside sa_engine.hip: the encoder's kernels are
// compiled exactly as they are without this file.
//
//   k_dec_init   fresh tables of every block of the group (QUAL: the 288-byte
//                pattern of sm_init_entry repeated; SEQ: every byte 3), the output
//                region zeroed, the chain states and status words zeroed
//   k_dec_qual   one wave per block (blockIdx.x = the block's index in the group,
//                the grid is the group): loads the block's DecChain, returns if it
//                is done, else one dec_qual_slice of `slice` symbols, lane 0 stores
//                the DecChain back
//   k_dec_place  one thread per block: dec_block_place into the status word
//   k_dec_seq    as k_dec_qual, dec_seq_slice
// The mapping of blocks to waves is static: no device counter, no atomics.  NO
// kernel waits for another wave -- no spin, no polling of memory, no barrier
// between workgroups: what a launch needs of an earlier one is complete when it
// starts (one stream).  Every loop is bounded by `slice`, a read's length, the
// read count, DEC_RENORM_MAX or a table's size, and says so.  How many launches
// a group gets is the driver's count (sa_decoder.h), fixed before the first one.
// Every store to global memory is an ordinary vector store from a lane.
// Bounds: sa_decode_logic.h's; the descriptors' offsets are checked by the host
// against the arena before any launch (dec_desc_ok).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sa_decoder.h"

namespace {

using namespace sadec;

// inclusive add-scan of a wave64 on DPP (row shifts, then row broadcasts 15 / 31;
// sa_kernels.hip's wave_incl_scan_dpp): register to register
__device__ inline uint32_t dec_incl_scan_dpp(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31
    return v;
}

struct DBuf {   // a device buffer that grows on demand and is kept
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        const size_t want = std::max<size_t>(std::max(bytes + bytes / 16, cap + cap / 16), 256);
        const hipError_t e = hipMalloc(&p, want);
        cap = e == hipSuccess ? want : 0;
        return e;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// the device W of sa_decode_logic.h: one wave, each lane holds its own registers
struct WaveOps {
    static constexpr int N = 1;
    uint32_t lane;
    template <class F> __device__ void each(F f) { f(lane, 0u); }
    // exclusive prefix sum over the 64 lanes; the total (lane 63's inclusive sum) in every lane
    __device__ uint32_t scan(const uint32_t* in, uint32_t* out)
    {
        const uint32_t inc = dec_incl_scan_dpp(in[0]);
        out[0] = inc - in[0];
        return (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    __device__ uint32_t first(const uint32_t* a, uint32_t v)
    {
        const uint64_t m = __ballot(a[0] == v);
        return m ? (uint32_t)__builtin_ctzll(m) : 64u;
    }
    __device__ uint32_t get(const uint32_t* a, uint32_t src)
    {
        return (uint32_t)__builtin_amdgcn_readlane((int)a[0], (int)SAD_UNI(src & 63u));
    }
    // lane 0's load, broadcast (a vector load: the same wave stores to these bytes)
    __device__ uint32_t ld8(const uint8_t* p)
    {
        uint32_t v = 0;
        if (lane == 0) v = *p;
        return SAD_UNI(v);
    }
    __device__ uint32_t ld32(const uint32_t* p)
    {
        uint32_t v = 0;
        if (lane == 0) v = *p;
        return SAD_UNI(v);
    }
    __device__ void st8(uint8_t* p, uint8_t v)
    {
        if (lane == 0) *p = v;
    }
    __device__ void st32(uint32_t* p, uint32_t v)
    {
        if (lane == 0) *p = v;
    }
    __device__ void fill(uint8_t* p, uint32_t n, uint8_t v)
    {
        for (uint32_t i = lane; i < n; i += DEC_LANES) p[i] = v;   // bounded by n <= a read's length
    }
};

// a DecChain every lane loaded alike, said so to the compiler field by field (scalar registers)
__device__ inline uint64_t dec_uni64(uint64_t v) { return (uint64_t)SAD_UNI((uint32_t)(v >> 32)) << 32 | SAD_UNI((uint32_t)v); }
__device__ inline DecChain dec_chain_load(const DecChain* p)
{
    DecChain c = *p;
    c.low = dec_uni64(c.low);
    c.code = dec_uni64(c.code);
    c.off = dec_uni64(c.off);
    c.range = SAD_UNI(c.range);
    c.pos = SAD_UNI(c.pos);
    c.status = SAD_UNI(c.status);
    c.done = SAD_UNI(c.done);
    c.r = SAD_UNI(c.r);
    c.i = SAD_UNI(c.i);
    c.q1 = SAD_UNI(c.q1);
    c.q2 = SAD_UNI(c.q2);
    c.delta = SAD_UNI(c.delta);
    c.last = SAD_UNI(c.last);
    c.ctx = SAD_UNI(c.ctx);
    c.started = SAD_UNI(c.started);
    return c;
}

constexpr uint32_t DEC_INIT_THREADS = 256, DEC_INIT_WGS = 64;
constexpr uint32_t DEC_PAT_VECS = DEC_QM_STRIDE / 16;   // the fresh context as 18 x 16 bytes
static_assert(DEC_QM_STRIDE % 16 == 0 && DEC_PAD % 16 == 0, "k_dec_init stores 16 bytes a lane");

// grid (DEC_INIT_WGS, blocks of the group); out_off / out_bytes: the group's output region, multiples of DEC_PAD
__global__ __launch_bounds__(DEC_INIT_THREADS) void k_dec_init(uint8_t* __restrict__ base, const DecDesc* __restrict__ desc,
                                                               uint64_t out_off, uint64_t out_bytes, uint64_t qual_table,
                                                               uint64_t seq_table, DecChain* __restrict__ qchain,
                                                               DecChain* __restrict__ schain, uint32_t* __restrict__ status)
{
    __shared__ __align__(16) uint8_t pat[DEC_QM_STRIDE];
    const uint32_t b = blockIdx.y, nb = gridDim.y;
    const uint64_t t = (uint64_t)blockIdx.x * DEC_INIT_THREADS + threadIdx.x, nt = (uint64_t)gridDim.x * DEC_INIT_THREADS;
    if (threadIdx.x < DEC_QSYM) sm_init_entry(pat, threadIdx.x);
    __syncthreads();
    const DecDesc d = desc[b];
    const uint4* pv = reinterpret_cast<const uint4*>(pat);
    uint4* m = reinterpret_cast<uint4*>(base + d.models);
    for (uint64_t j = t; j < qual_table / 16; j += nt) m[j] = pv[j % DEC_PAT_VECS];   // bounded by the table's size
    uint32_t* tab = reinterpret_cast<uint32_t*>(base + d.tab);
    for (uint64_t j = t; j < seq_table / 4; j += nt) tab[j] = 0x03030303u;            // bounded by the table's size
    // the output region, this block row's share of it
    uint4* o = reinterpret_cast<uint4*>(base + out_off);
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint64_t j = (uint64_t)b * nt + t; j < out_bytes / 16; j += nt * nb) o[j] = z;   // bounded by the region's size
    if (blockIdx.x == 0 && threadIdx.x < sizeof(DecChain) / 4) {
        reinterpret_cast<uint32_t*>(qchain + b)[threadIdx.x] = 0;
        reinterpret_cast<uint32_t*>(schain + b)[threadIdx.x] = 0;
        if (threadIdx.x == 0) status[b] = 0;
    }
}

__global__ __launch_bounds__(64) void k_dec_qual(uint8_t* base, const DecDesc* __restrict__ desc, DecChain* chains, int32_t qlevel,
                                                 uint32_t slice)
{
    const uint32_t b = blockIdx.x;
    DecChain c = dec_chain_load(chains + b);
    if (c.done) return;
    const DecDesc d = desc[b];
    WaveOps w{threadIdx.x};
    uint32_t ev = 0;
    dec_block_qual(w, base, d, c, qlevel, slice, ev);   // at most `slice` symbols
    if (threadIdx.x == 0) chains[b] = c;
}

__global__ __launch_bounds__(64) void k_dec_seq(uint8_t* base, const DecDesc* __restrict__ desc, DecChain* chains, uint32_t mask,
                                                uint32_t slice)
{
    const uint32_t b = blockIdx.x;
    DecChain c = dec_chain_load(chains + b);
    if (c.done) return;
    const DecDesc d = desc[b];
    WaveOps w{threadIdx.x};
    uint32_t ev = 0;
    dec_block_seq(w, base, d, c, mask, slice, ev);   // at most `slice` positions
    if (threadIdx.x == 0) chains[b] = c;
}

// one thread per block: the walk over the tip reads (bounded by their count and lengths)
__global__ __launch_bounds__(64) void k_dec_place(uint8_t* base, const DecDesc* __restrict__ desc, const DecChain* __restrict__ qchain,
                                                  DecChain* schain, uint32_t* __restrict__ status, uint32_t nb)
{
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    const DecDesc d = desc[b];
    const DecChain qc = qchain[b];
    DecChain sc = schain[b];
    const uint32_t st = dec_block_place(base, d, qc, sc);
    status[b] = st;
    if (st) schain[b] = sc;
}

struct HBuf {   // a page-locked host buffer, kept between groups and calls
    uint8_t* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap && p) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        const size_t want = std::max<size_t>(bytes + bytes / 16, 4096);
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault);
        cap = e == hipSuccess ? want : 0;
        return e;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

}  // namespace

struct sa_decoder {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[12] = {};   // h2d, init, qual, place, seq, d2h: begin and end of each
    DBuf d_arena, d_desc, d_qchain, d_schain, d_status;
    HBuf h_up, h_out, h_chain;
    DecKnobs knobs;
    sa_decode_info info{};
    std::string err;
    ~sa_decoder()
    {
        for (DBuf* b : {&d_arena, &d_desc, &d_qchain, &d_schain, &d_status}) b->release();
        for (HBuf* b : {&h_up, &h_out, &h_chain}) b->release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

#define DEC_CHECK(expr)                                                  \
    do {                                                                 \
        hipError_t e_ = (expr);                                          \
        if (e_ != hipSuccess) {                                          \
            g.err = std::string(#expr) + ": " + hipGetErrorString(e_);   \
            return false;                                                \
        }                                                                \
    } while (0)

// dec_run's backend: every call of a group goes on the decoder's stream, and the
// host synchronises only where it reads something back (chains, download).
struct DecDevice {
    sa_decoder& g;
    uint32_t launches[2] = {0, 0};
    enum { H2D = 0, INIT = 2, QUAL = 4, PLACE = 6, SEQ = 8, D2H = 10 };

    uint64_t free_bytes()
    {
        size_t fr = 0, tot = 0;
        if (hipSetDevice(g.device) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) return 0;
        return (uint64_t)fr + g.d_arena.cap;   // (the arena of the last call is the decoder's to reuse)
    }
    bool alloc(uint64_t arena, uint64_t up, uint64_t out, uint32_t nb, uint8_t** h_up, uint8_t** h_out)
    {
        if (nb > 65535) {   // (k_dec_init's grid has the group in y)
            g.err = "sa_decode_blocks: more than 65535 blocks in a group";
            return false;
        }
        DEC_CHECK(hipSetDevice(g.device));
        if (arena > g.d_arena.cap) g.d_arena.release();   // (no second arena beside the first: the plan counted one)
        DEC_CHECK(g.d_arena.ensure(arena));
        DEC_CHECK(g.d_desc.ensure(sizeof(DecDesc) * (size_t)nb));
        DEC_CHECK(g.d_qchain.ensure(sizeof(DecChain) * (size_t)nb));
        DEC_CHECK(g.d_schain.ensure(sizeof(DecChain) * (size_t)nb));
        DEC_CHECK(g.d_status.ensure(4ull * nb));
        DEC_CHECK(g.h_up.ensure(up));
        DEC_CHECK(g.h_out.ensure(out));
        DEC_CHECK(g.h_chain.ensure((sizeof(DecChain) + 4) * (size_t)nb));
        *h_up = g.h_up.p;
        *h_out = g.h_out.p;
        launches[0] = launches[1] = 0;
        return true;
    }
    bool upload(const DecDesc* d, uint32_t nb, uint64_t up)
    {
        DEC_CHECK(hipEventRecord(g.ev[H2D], g.st));
        if (up) DEC_CHECK(hipMemcpyAsync(g.d_arena.p, g.h_up.p, up, hipMemcpyHostToDevice, g.st));
        DEC_CHECK(hipMemcpyAsync(g.d_desc.p, d, sizeof(DecDesc) * (size_t)nb, hipMemcpyHostToDevice, g.st));
        DEC_CHECK(hipEventRecord(g.ev[H2D + 1], g.st));
        return true;
    }
    bool init(uint32_t nb, uint64_t out_off, uint64_t out, uint64_t qual_table, uint64_t seq_table)
    {
        DEC_CHECK(hipEventRecord(g.ev[INIT], g.st));
        hipLaunchKernelGGL(k_dec_init, dim3(DEC_INIT_WGS, nb), dim3(DEC_INIT_THREADS), 0, g.st, g.d_arena.as<uint8_t>(),
                           g.d_desc.as<DecDesc>(), out_off, out, qual_table, seq_table, g.d_qchain.as<DecChain>(),
                           g.d_schain.as<DecChain>(), g.d_status.as<uint32_t>());
        DEC_CHECK(hipGetLastError());
        DEC_CHECK(hipEventRecord(g.ev[INIT + 1], g.st));
        return true;
    }
    bool qual_slice(uint32_t nb, int32_t qlevel, uint32_t slice)
    {
        if (!launches[0]++) DEC_CHECK(hipEventRecord(g.ev[QUAL], g.st));
        hipLaunchKernelGGL(k_dec_qual, dim3(nb), dim3(64), 0, g.st, g.d_arena.as<uint8_t>(), g.d_desc.as<DecDesc>(),
                           g.d_qchain.as<DecChain>(), qlevel, slice);
        DEC_CHECK(hipGetLastError());
        return true;
    }
    bool place(uint32_t nb)
    {
        DEC_CHECK(hipEventRecord(g.ev[PLACE], g.st));
        hipLaunchKernelGGL(k_dec_place, dim3((nb + 63) / 64), dim3(64), 0, g.st, g.d_arena.as<uint8_t>(), g.d_desc.as<DecDesc>(),
                           g.d_qchain.as<DecChain>(), g.d_schain.as<DecChain>(), g.d_status.as<uint32_t>(), nb);
        DEC_CHECK(hipGetLastError());
        DEC_CHECK(hipEventRecord(g.ev[PLACE + 1], g.st));
        return true;
    }
    bool seq_slice(uint32_t nb, uint32_t mask, uint32_t slice)
    {
        if (!launches[1]++) DEC_CHECK(hipEventRecord(g.ev[SEQ], g.st));
        hipLaunchKernelGGL(k_dec_seq, dim3(nb), dim3(64), 0, g.st, g.d_arena.as<uint8_t>(), g.d_desc.as<DecDesc>(),
                           g.d_schain.as<DecChain>(), mask, slice);
        DEC_CHECK(hipGetLastError());
        return true;
    }
    bool chains(int which, DecChain* c, uint32_t* status, uint32_t nb)
    {
        // (the end of the slice launches: the states are read once, after the last of them)
        DEC_CHECK(hipEventRecord(g.ev[(which ? SEQ : QUAL) + 1], g.st));
        const size_t cb = sizeof(DecChain) * (size_t)nb;
        DEC_CHECK(hipMemcpyAsync(g.h_chain.p, which ? g.d_schain.p : g.d_qchain.p, cb, hipMemcpyDeviceToHost, g.st));
        if (status) DEC_CHECK(hipMemcpyAsync(g.h_chain.p + cb, g.d_status.p, 4ull * nb, hipMemcpyDeviceToHost, g.st));
        DEC_CHECK(hipStreamSynchronize(g.st));
        memcpy(c, g.h_chain.p, cb);
        if (status) memcpy(status, g.h_chain.p + cb, 4ull * nb);
        return true;
    }
    bool download(uint64_t out_off, uint64_t out)
    {
        DEC_CHECK(hipEventRecord(g.ev[D2H], g.st));
        if (out) DEC_CHECK(hipMemcpyAsync(g.h_out.p, g.d_arena.as<uint8_t>() + out_off, out, hipMemcpyDeviceToHost, g.st));
        DEC_CHECK(hipEventRecord(g.ev[D2H + 1], g.st));
        DEC_CHECK(hipStreamSynchronize(g.st));
        return true;
    }
    bool finish(sa_decode_info& inf)
    {
        float* ms[6] = {&inf.h2d_ms, &inf.init_ms, &inf.qual_ms, &inf.place_ms, &inf.seq_ms, &inf.d2h_ms};
        for (int k = 0; k < 6; k++) {
            float v = 0.f;
            DEC_CHECK(hipEventElapsedTime(&v, g.ev[2 * k], g.ev[2 * k + 1]));
            *ms[k] += v;
        }
        return true;
    }
};
#undef DEC_CHECK

}  // namespace

extern "C" {

sa_decoder* sa_decoder_create(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return nullptr;
    sa_decoder* g = new sa_decoder();
    g->device = device;
    g->knobs = parse_dec_knobs([](const char* n) -> const char* { return std::getenv(n); });
    bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess;
    for (hipEvent_t& e : g->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        delete g;
        return nullptr;
    }
    return g;
}

void sa_decoder_destroy(sa_decoder* g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    delete g;
}

const char* sa_decoder_error(const sa_decoder* g) { return g ? g->err.c_str() : "no decoder"; }

void sa_decoder_info(const sa_decoder* g, sa_decode_info* info)
{
    if (info) *info = g ? g->info : sa_decode_info{};
}

int sa_decode_blocks(sa_decoder* g, const uint8_t* const* in, const uint64_t* len, const int32_t* long_reads, uint32_t n,
                     const sa_cfg* cfg, const uint8_t tmpl[512], int threads, sa_decoded* out, uint32_t* status)
{
    if (!g) return -1;
    g->err.clear();
    g->info = sa_decode_info{};
    if (n && (!in || !len || !cfg || !tmpl || !out || !status)) {
        g->err = "sa_decode_blocks: null argument";
        return -1;
    }
    DecDevice be{*g};
    return dec_run(be, in, len, long_reads, n, cfg, tmpl, threads, out, status, g->knobs, g->info, g->err);
}

}  // extern "C"
