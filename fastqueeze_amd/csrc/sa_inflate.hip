// sa_inflate.hip -- BGZF members inflated on the device (sa_inflate_members).
// Included by sa_engine.hip (needs DBuf).
//
// k_inflate_bgzf: one wave per member, one wave per workgroup; the waves take
// members from a device counter until none is left.  The wave runs
// sa_inflate.h's infl_member: every lane executes the same symbol loop on the
// same bit buffer (the branch conditions are wave-uniform), and the 64 lanes
// split the table fills, the match and stored-block copies, the CRC-32 and the
// final store.  LDS of a workgroup (69.1 KiB, two workgroups per CU):
//   [0, 65552)        the member's output (<= 64 KiB), placed so that its LDS
//                     address and its address in the output slab agree mod 16
//   [65552, +4.2 KiB) InflTabs: the block's decode tables
//   then 1 KiB        the CRC-32 byte table
// The output window stays in LDS until the member is complete: a match reads
// what other lanes of the wave stored a few instructions earlier, which LDS
// returns in issue order, and global memory sees each byte once, in 16-byte
// stores.  Bounds: see sa_inflate.h; the host has checked every descriptor
// against the slabs before the launch (sa_inflate_members).
#include "sa_inflate.h"

namespace {

constexpr uint32_t INFL_WIN_BYTES = INFL_MAX_ISIZE + 16;
constexpr uint32_t INFL_LDS_BYTES = INFL_WIN_BYTES + (uint32_t)sizeof(InflTabs) + 256 * 4;
static_assert(sizeof(InflTabs) % 16 == 0, "the CRC table follows the decode tables, 4-byte aligned");
static_assert(sizeof(sa_bgzf_member) == 32, "sa_bgzf_member is copied to the device as it is");

__global__ __launch_bounds__(64) void k_inflate_bgzf(const uint8_t* __restrict__ in, const sa_bgzf_member* __restrict__ ms,
                                                     uint32_t n, uint8_t* __restrict__ out, uint32_t* __restrict__ status,
                                                     uint32_t* __restrict__ counter)
{
    extern __shared__ __align__(16) uint8_t infl_lds[];
    InflTabs* tabs = reinterpret_cast<InflTabs*>(infl_lds + INFL_WIN_BYTES);
    uint32_t* crc_tab = reinterpret_cast<uint32_t*>(infl_lds + INFL_WIN_BYTES + sizeof(InflTabs));
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += 64) crc_tab[i] = crc32_entry(i);
    const uint32_t shift = crc32_chunk_shift(63 - lane);
    __syncthreads();
    for (;;) {
        uint32_t m = 0;
        if (lane == 0) m = atomicAdd(counter, 1u);
        m = __builtin_amdgcn_readfirstlane(m);
        if (m >= n) break;
        const uint64_t in_off = ms[m].in_off, out_off = ms[m].out_off;
        const uint32_t in_len = ms[m].in_len, isize = ms[m].isize, crc = ms[m].crc;
        uint32_t st;
        if (isize == 0) {
            // an empty member (the end-of-file marker) is inflated like any other: with no room in
            // the window a literal, a match or a stored byte is SA_INFL_SIZE, so it is good only
            // if its stream reaches the final end-of-block code having produced nothing
            st = infl_member(in + in_off, in_len, infl_lds, 0, *tabs, lane, 64);
            if (st == 0 && crc) st = SA_INFL_CRC;
        } else if (isize > INFL_MAX_ISIZE) {
            st = SA_INFL_SIZE;   // (the host rejects these before the launch)
        } else {
            uint8_t* win = infl_lds + (uint32_t)(out_off & 15u);
            st = infl_member(in + in_off, in_len, win, isize, *tabs, lane, 64);
            __syncthreads();
            if (st == 0) {
                uint32_t x = crc32_share(win, isize, lane, shift, crc_tab);
                for (int d = 32; d; d >>= 1) x ^= __shfl_xor(x, d, 64);
                if (~x != crc) st = SA_INFL_CRC;
                // the member to its place: bytes up to the slab's next 16-byte boundary, 16-byte
                // stores (LDS and slab addresses agree mod 16), the last bytes
                uint8_t* dst = out + out_off;
                const uint32_t gap = (16u - (uint32_t)(out_off & 15u)) & 15u;
                const uint32_t head = gap < isize ? gap : isize;
                const uint32_t nvec = (isize - head) >> 4;
                if (lane < head) dst[lane] = win[lane];
                const uint4* s4 = reinterpret_cast<const uint4*>(win + head);
                uint4* d4 = reinterpret_cast<uint4*>(dst + head);
                for (uint32_t v = lane; v < nvec; v += 64) d4[v] = s4[v];
                const uint32_t done = head + (nvec << 4);
                if (done + lane < isize) dst[done + lane] = win[done + lane];
            }
        }
        if (lane == 0) status[m] = st;
        __syncthreads();   // the window and the tables are the next member's
    }
}

}  // namespace

struct sa_inflater {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DBuf d_in, d_out, d_ms, d_status, d_counter;
    std::vector<uint32_t> h_status;
    uint32_t grid = 0;   // workgroups (SA_INFL_GRID; default two per CU, what the LDS allows)
    float kernel_ms = 0.f;
    std::string err;
    ~sa_inflater()
    {
        for (DBuf* b : {&d_in, &d_out, &d_ms, &d_status, &d_counter}) b->release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (st) (void)hipStreamDestroy(st);
    }
};

extern "C" {

int64_t sa_bgzf_scan(const uint8_t* buf, uint64_t have, sa_bgzf_member* ms, uint64_t max_members, uint64_t* consumed,
                     uint64_t* out_bytes)
{
    if (!buf && have) return -1;
    return bgzf_scan(buf, have, ms, max_members, consumed, out_bytes, INFL_MAX_ISIZE);
}

sa_inflater* sa_inflater_create(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return nullptr;
    sa_inflater* f = new sa_inflater();
    f->device = device;
    f->grid = 2u * (uint32_t)std::max(1, prop.multiProcessorCount);
    if (const char* e = std::getenv("SA_INFL_GRID")) f->grid = (uint32_t)std::min(std::max(std::atoi(e), 1), 1 << 16);   // (tests)
    if (hipStreamCreateWithFlags(&f->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&f->ev0) != hipSuccess ||
        hipEventCreate(&f->ev1) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_inflate_bgzf), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)INFL_LDS_BYTES) != hipSuccess ||
        f->d_counter.ensure(256) != hipSuccess) {
        delete f;
        return nullptr;
    }
    return f;
}

void sa_inflater_destroy(sa_inflater* f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    delete f;
}

const char* sa_inflater_error(const sa_inflater* f) { return f ? f->err.c_str() : "no inflater"; }

float sa_inflater_kernel_ms(const sa_inflater* f) { return f ? f->kernel_ms : 0.f; }

uint32_t sa_inflater_grid(const sa_inflater* f) { return f ? f->grid : 0; }

int sa_inflate_members(sa_inflater* f, const uint8_t* in, uint64_t in_bytes, const sa_bgzf_member* ms, uint32_t n,
                       uint8_t* out, uint64_t out_bytes, uint32_t* status)
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
    if ((n && !ms) || (in_bytes && !in) || (out_bytes && !out)) {
        f->err = "sa_inflate_members: null argument";
        return -1;
    }
    for (uint32_t i = 0; i < n; i++) {
        const sa_bgzf_member& m = ms[i];
        if (m.in_off > in_bytes || m.in_len > in_bytes - m.in_off || m.out_off > out_bytes ||
            m.isize > out_bytes - m.out_off || m.isize > INFL_MAX_ISIZE) {
            f->err = "sa_inflate_members: member " + std::to_string(i) + " lies outside the buffers or is larger than 64 KiB";
            return -2;
        }
    }
    if (!n) return 0;
    INFL_CHECK(hipSetDevice(f->device));
    INFL_CHECK(f->d_in.ensure(in_bytes + 16));
    INFL_CHECK(f->d_out.ensure(out_bytes + 16));
    INFL_CHECK(f->d_ms.ensure(sizeof(sa_bgzf_member) * (size_t)n));
    INFL_CHECK(f->d_status.ensure(4ull * n));
    if (in_bytes) INFL_CHECK(hipMemcpyAsync(f->d_in.p, in, in_bytes, hipMemcpyHostToDevice, f->st));
    INFL_CHECK(hipMemcpyAsync(f->d_ms.p, ms, sizeof(sa_bgzf_member) * (size_t)n, hipMemcpyHostToDevice, f->st));
    INFL_CHECK(hipMemsetAsync(f->d_counter.p, 0, 4, f->st));
    INFL_CHECK(hipEventRecord(f->ev0, f->st));
    hipLaunchKernelGGL(k_inflate_bgzf, dim3(std::min(f->grid, n)), dim3(64), INFL_LDS_BYTES, f->st, f->d_in.as<uint8_t>(),
                       f->d_ms.as<sa_bgzf_member>(), n, f->d_out.as<uint8_t>(), f->d_status.as<uint32_t>(),
                       f->d_counter.as<uint32_t>());
    INFL_CHECK(hipGetLastError());
    INFL_CHECK(hipEventRecord(f->ev1, f->st));
    f->h_status.resize(n);
    INFL_CHECK(hipMemcpyAsync(f->h_status.data(), f->d_status.p, 4ull * n, hipMemcpyDeviceToHost, f->st));
    if (out_bytes) INFL_CHECK(hipMemcpyAsync(out, f->d_out.p, out_bytes, hipMemcpyDeviceToHost, f->st));
    INFL_CHECK(hipStreamSynchronize(f->st));
    INFL_CHECK(hipEventElapsedTime(&f->kernel_ms, f->ev0, f->ev1));
    int bad = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (status) status[i] = f->h_status[i];
        bad += f->h_status[i] != 0;
    }
    return bad;
#undef INFL_CHECK
}

}  // extern "C"
