// sa_gunzip.hip -- ordinary gzip inflated on the device (sa_gunzip_run, and
// sa_gunzip_run_dev: the text into a devtext and never to the host).
// Included by sa_engine.hip after sa_devtext.hip (needs DBuf, sa_devtext,
// dt_make_room and dt_count).
//
// The stages of sa_gunzip.h as separate launches on one stream; NO kernel waits
// for another wave -- no spin, no flag polling, no cooperative launch: what a
// stage needs of another is complete when it starts.
//   k_gz_find     one wave per chunk (chunk 0 is the known start): the lanes
//                 test 64 consecutive bit positions a step (gz_precheck), the
//                 survivors go through infl_dynamic one at a time; cand[k]
//   (host)        compacts the candidates, sizes each wave's symbol range
//   k_gz_spec     one wave per start: gz_wave.  LDS of a workgroup (68.2 KiB,
//                 two workgroups per CU): the 32768-symbol ring, then InflTabs
//   k_gz_chain    one workgroup of 1024: the chain over the waves, serial; the
//                 threads split each 32 KiB window (two windows in LDS)
//   k_gz_resolve  symbols to text, data-parallel
//   k_gz_crc      one wave per task of <= 64 KiB of text (crc32_share)
// k_gz_find, k_gz_spec and k_gz_crc are one wave per workgroup
// (__launch_bounds__(64)) under sa_inflate.h's lockstep assumption and take
// their chunks / waves / tasks from a device counter.  Every store to global
// memory is an ordinary vector store from a lane.  Bounds: see sa_gunzip.h; the
// ranges come from gz_plan and the buffers are sized from the same plan.
#include "sa_gunzip.h"

namespace {

constexpr uint32_t GZ_SPEC_LDS = GZ_RING * 2 + (uint32_t)sizeof(InflTabs);
constexpr uint32_t GZ_CHAIN_LDS = 2 * GZ_RING;
constexpr uint32_t GZ_CRC_DATA = 64 * INFL_CRC_CHUNK + 16;
constexpr uint32_t GZ_CRC_LDS = GZ_CRC_DATA + 256 * 4;
constexpr uint32_t GZ_CHAIN_THREADS = 1024;

__device__ inline uint32_t gz_next_index(uint32_t* counter, uint32_t lane)
{
    uint32_t k = 0;
    if (lane == 0) k = atomicAdd(counter, 1u);
    return __builtin_amdgcn_readfirstlane(k);
}

__global__ __launch_bounds__(64) void k_gz_find(const uint8_t* __restrict__ in, uint32_t in_len, uint32_t chunk, uint32_t nchunks,
                                                uint32_t* __restrict__ cand, uint32_t* __restrict__ counter)
{
    __shared__ InflTabs tabs;
    const uint32_t lane = threadIdx.x;
    for (;;) {   // bounded by nchunks
        const uint32_t k = gz_next_index(counter, lane) + 1;   // (chunk 0 is the known start)
        if (k >= nchunks) break;
        const uint64_t from = 8ull * k * chunk;
        const uint64_t to = 8ull * (((uint64_t)k + 1) * chunk < in_len ? ((uint64_t)k + 1) * chunk : in_len);
        const uint32_t c = gz_find_first(in, in_len, (uint32_t)from, (uint32_t)to, tabs, lane, 64);
        if (lane == 0) cand[k] = c;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_gz_spec(const uint8_t* __restrict__ in, uint32_t in_len, const uint32_t* __restrict__ starts,
                                                uint32_t nw, const uint64_t* __restrict__ base, const uint32_t* __restrict__ cap,
                                                uint16_t* __restrict__ sym, const uint8_t* __restrict__ win0, uint32_t win_len,
                                                uint32_t at_header, GzWaveRes* __restrict__ res, uint32_t* __restrict__ counter)
{
    extern __shared__ __align__(16) uint8_t gz_lds[];
    uint16_t* ring = reinterpret_cast<uint16_t*>(gz_lds);
    InflTabs* tabs = reinterpret_cast<InflTabs*>(gz_lds + GZ_RING * 2);
    const uint32_t lane = threadIdx.x;
    for (;;) {   // bounded by nw
        const uint32_t j = gz_next_index(counter, lane);
        if (j >= nw) break;
        gz_wave(in, in_len, starts, nw, j, j == 0, j == 0 && at_header, win0, win_len, ring, *tabs, sym + base[j], cap[j], res + j,
                lane, 64);
        __syncthreads();   // the ring and the tables are the next wave's
    }
}

// win: nw + 1 slots of 32768 bytes; slot 0 holds the state's window, slot j
// receives wave j's, slot nw the one the next call starts from.
__global__ __launch_bounds__(GZ_CHAIN_THREADS) void k_gz_chain(const GzWaveRes* __restrict__ res, const uint32_t* __restrict__ starts,
                                                               uint32_t nw, const uint64_t* __restrict__ base,
                                                               const uint16_t* __restrict__ sym, uint8_t* __restrict__ win,
                                                               uint32_t win_len0, uint64_t out_cap, uint32_t first_header,
                                                               GzChainEnd* __restrict__ end, uint32_t* __restrict__ order,
                                                               uint64_t* __restrict__ woff, uint32_t* __restrict__ wwl)
{
    extern __shared__ __align__(16) uint8_t gz_lds[];
    uint8_t* cur = gz_lds;
    uint8_t* nxt = gz_lds + GZ_RING;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid * 16; i < GZ_RING; i += GZ_CHAIN_THREADS * 16)
        *reinterpret_cast<uint4*>(cur + i) = *reinterpret_cast<const uint4*>(win + i);
    __syncthreads();
    GzChainEnd e{};
    uint32_t j = 0, wl = win_len0, n = 0;
    for (;;) {   // j strictly increases (gz_chain_step: met > j): <= nw steps
        GzChainStep s{};
        const uint64_t off = e.text;
        if (!gz_chain_step(res[j], j, nw, starts, wl, out_cap, first_header != 0, e, s)) break;
        if (tid == 0) {
            order[n] = j;
            woff[n] = off;
            wwl[n] = wl;
        }
        n++;
        gz_window_next(cur, sym + base[j], res[j].lb_sym, nxt, tid, GZ_CHAIN_THREADS);
        __syncthreads();   // nxt is complete; nobody reads cur any more
        uint8_t* g = win + (size_t)s.next_slot * GZ_RING;
        for (uint32_t i = tid * 16; i < GZ_RING; i += GZ_CHAIN_THREADS * 16)
            *reinterpret_cast<uint4*>(g + i) = *reinterpret_cast<const uint4*>(nxt + i);
        // (the next step writes the old cur and reads nxt; the step after it writes nxt again, and
        // no thread gets there before every thread has passed the next step's barrier)
        uint8_t* t = cur;
        cur = nxt;
        nxt = t;
        if (s.last) break;
        j = s.next_slot;
        wl = s.next_len;
    }
    if (tid == 0) *end = e;
}

// blockIdx.y: the k-th confirmed wave
__global__ __launch_bounds__(256) void k_gz_resolve(const uint32_t* __restrict__ order, const uint64_t* __restrict__ woff,
                                                    const uint32_t* __restrict__ wwl, const GzWaveRes* __restrict__ res,
                                                    const uint64_t* __restrict__ base, const uint16_t* __restrict__ sym,
                                                    const uint8_t* __restrict__ win, uint8_t* __restrict__ text,
                                                    uint32_t* __restrict__ bad)
{
    const uint32_t k = blockIdx.y, j = order[k], n = res[j].lb_sym, wl = wwl[k];
    const uint16_t* s = sym + base[j];
    const uint8_t* w = win + (size_t)j * GZ_RING;
    uint8_t* t = text + woff[k];
    bool b = false;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) t[i] = gz_resolve_sym(s[i], w, wl, b);
    if (b) *bad = 1;
}

static_assert(sizeof(GzAccount::Task) == 16, "the CRC tasks are copied to the device as they are");

__global__ __launch_bounds__(64) void k_gz_crc(const uint8_t* __restrict__ text, const GzAccount::Task* __restrict__ tasks, uint32_t n,
                                               uint32_t* __restrict__ crcs, uint32_t* __restrict__ counter)
{
    extern __shared__ __align__(16) uint8_t gz_lds[];
    uint32_t* crc_tab = reinterpret_cast<uint32_t*>(gz_lds + GZ_CRC_DATA);
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += 64) crc_tab[i] = crc32_entry(i);
    const uint32_t shift = crc32_chunk_shift(63 - lane);
    __syncthreads();
    for (;;) {   // bounded by n
        const uint32_t t = gz_next_index(counter, lane);
        if (t >= n) break;
        const uint64_t off = tasks[t].off;
        const uint32_t len = tasks[t].len;   // 1 .. 65536
        // the task's bytes into LDS at the same address mod 16: bytes up to the next 16-byte
        // boundary, 16-byte loads, the last bytes
        uint8_t* data = gz_lds + (uint32_t)(off & 15u);
        const uint8_t* src = text + off;
        const uint32_t gap = (16u - (uint32_t)(off & 15u)) & 15u;
        const uint32_t head = gap < len ? gap : len;
        const uint32_t nvec = (len - head) >> 4;
        if (lane < head) data[lane] = src[lane];
        const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
        uint4* d4 = reinterpret_cast<uint4*>(data + head);
        for (uint32_t v = lane; v < nvec; v += 64) d4[v] = s4[v];
        const uint32_t done = head + (nvec << 4);
        if (done + lane < len) data[done + lane] = src[done + lane];
        __syncthreads();
        uint32_t x = crc32_share(data, len, lane, shift, crc_tab);
        for (int d = 32; d; d >>= 1) x ^= __shfl_xor(x, d, 64);
        if (lane == 0) crcs[t] = ~x;
        __syncthreads();   // the data is the next task's
    }
}

}  // namespace

struct sa_gunzipper {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[10] = {};
    DBuf d_in, d_cand, d_starts, d_base, d_cap, d_sym, d_res, d_win, d_counter, d_end, d_order, d_woff, d_wwl, d_text, d_bad, d_tasks,
        d_crcs;
    uint32_t grid = 0;            // workgroups of the one-wave kernels (SA_GUNZIP_GRID; default two per CU)
    uint32_t chunk = 64u << 10;   // SA_GUNZIP_CHUNK (the best of 64 KiB, 256 KiB and 1 MiB: scripts/gunzip_rate.py)
    uint32_t ratio = 8;           // SA_GUNZIP_RATIO
    float kernel_ms = 0.f;
    std::string err;
    ~sa_gunzipper()
    {
        for (DBuf* b : {&d_in, &d_cand, &d_starts, &d_base, &d_cap, &d_sym, &d_res, &d_win, &d_counter, &d_end, &d_order, &d_woff,
                        &d_wwl, &d_text, &d_bad, &d_tasks, &d_crcs})
            b->release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

namespace {

#define GZ_CHECK(expr)                                                   \
    do {                                                                 \
        hipError_t e_ = (expr);                                          \
        if (e_ != hipSuccess) {                                          \
            g.err = std::string(#expr) + ": " + hipGetErrorString(e_);   \
            return false;                                                \
        }                                                                \
    } while (0)

// gz_run's backend: the stages as kernels on the gunzipper's stream.  With a
// sink (sa_gunzip_run_dev) the text is resolved into the devtext at its write
// position and summed there, and never copied to the host.  The kernels get the
// devtext's base, which is 16-byte aligned (k_gz_crc's vector loads rely on it),
// and the write position is added to the offsets here: to the confirmed waves'
// (d_woff, which the chain wrote and the host has read) and to a copy of the
// CRC tasks.
struct GzDevice {
    sa_gunzipper& g;
    sa_devtext* sink = nullptr;
    std::vector<uint64_t> sink_woff;
    std::vector<GzAccount::Task> sink_tasks;
    uint32_t in_len = 0, nw = 0, nconf = 0, ntasks = 0;
    const sa_gunzip_state* state = nullptr;
    uint32_t h_bad = 0;
    bool ran[5] = {};

    bool upload(const uint8_t* in, uint32_t n, const sa_gunzip_state* s)
    {
        in_len = n;
        state = s;
        GZ_CHECK(hipSetDevice(g.device));
        GZ_CHECK(g.d_in.ensure((size_t)n + 16));
        GZ_CHECK(hipMemcpyAsync(g.d_in.p, in, n, hipMemcpyHostToDevice, g.st));
        return true;
    }
    bool find(uint32_t nchunks, uint32_t chunk, uint32_t* cand)
    {
        if (nchunks < 2) return true;
        if (nchunks > 65535) {
            g.err = "sa_gunzip_run: more than 65535 chunks in one call";
            return false;
        }
        GZ_CHECK(g.d_cand.ensure(4ull * nchunks));
        GZ_CHECK(hipMemsetAsync(g.d_cand.p, 0xff, 4ull * nchunks, g.st));
        GZ_CHECK(hipMemsetAsync(g.d_counter.p, 0, 4, g.st));
        GZ_CHECK(hipEventRecord(g.ev[0], g.st));
        hipLaunchKernelGGL(k_gz_find, dim3(std::min(g.grid, nchunks - 1)), dim3(64), 0, g.st, g.d_in.as<uint8_t>(), in_len, chunk,
                           nchunks, g.d_cand.as<uint32_t>(), g.d_counter.as<uint32_t>());
        GZ_CHECK(hipGetLastError());
        GZ_CHECK(hipEventRecord(g.ev[1], g.st));
        GZ_CHECK(hipMemcpyAsync(cand, g.d_cand.p, 4ull * nchunks, hipMemcpyDeviceToHost, g.st));
        GZ_CHECK(hipStreamSynchronize(g.st));
        ran[0] = true;
        return true;
    }
    bool spec(const GzPlan& p, bool at_header, uint32_t win_len)
    {
        nw = (uint32_t)p.starts.size();
        GZ_CHECK(g.d_starts.ensure(4ull * nw));
        GZ_CHECK(g.d_base.ensure(8ull * nw));
        GZ_CHECK(g.d_cap.ensure(4ull * nw));
        GZ_CHECK(g.d_res.ensure(sizeof(GzWaveRes) * (size_t)nw));
        GZ_CHECK(g.d_win.ensure((size_t)(nw + 1) * GZ_RING));
        GZ_CHECK(g.d_sym.ensure(p.total * 2 + 16));
        GZ_CHECK(hipMemcpyAsync(g.d_starts.p, p.starts.data(), 4ull * nw, hipMemcpyHostToDevice, g.st));
        GZ_CHECK(hipMemcpyAsync(g.d_base.p, p.base.data(), 8ull * nw, hipMemcpyHostToDevice, g.st));
        GZ_CHECK(hipMemcpyAsync(g.d_cap.p, p.cap.data(), 4ull * nw, hipMemcpyHostToDevice, g.st));
        GZ_CHECK(hipMemcpyAsync(g.d_win.p, state->window, GZ_RING, hipMemcpyHostToDevice, g.st));
        GZ_CHECK(hipMemsetAsync(g.d_res.p, 0, sizeof(GzWaveRes) * (size_t)nw, g.st));
        GZ_CHECK(hipMemsetAsync(g.d_counter.p, 0, 4, g.st));
        GZ_CHECK(hipEventRecord(g.ev[2], g.st));
        hipLaunchKernelGGL(k_gz_spec, dim3(std::min(g.grid, nw)), dim3(64), GZ_SPEC_LDS, g.st, g.d_in.as<uint8_t>(), in_len,
                           g.d_starts.as<uint32_t>(), nw, g.d_base.as<uint64_t>(), g.d_cap.as<uint32_t>(), g.d_sym.as<uint16_t>(),
                           g.d_win.as<uint8_t>(), win_len, at_header ? 1u : 0u, g.d_res.as<GzWaveRes>(), g.d_counter.as<uint32_t>());
        GZ_CHECK(hipGetLastError());
        GZ_CHECK(hipEventRecord(g.ev[3], g.st));
        ran[1] = true;
        return true;
    }
    bool chain(const GzPlan&, uint32_t win_len, uint64_t out_cap, bool first_header, GzChainEnd& e, std::vector<uint32_t>& order,
               std::vector<uint64_t>& woff, std::vector<uint32_t>& wwl, std::vector<GzWaveRes>& res)
    {
        GZ_CHECK(g.d_end.ensure(sizeof(GzChainEnd)));
        GZ_CHECK(g.d_order.ensure(4ull * nw));
        GZ_CHECK(g.d_woff.ensure(8ull * nw));
        GZ_CHECK(g.d_wwl.ensure(4ull * nw));
        GZ_CHECK(hipEventRecord(g.ev[4], g.st));
        hipLaunchKernelGGL(k_gz_chain, dim3(1), dim3(GZ_CHAIN_THREADS), GZ_CHAIN_LDS, g.st, g.d_res.as<GzWaveRes>(),
                           g.d_starts.as<uint32_t>(), nw, g.d_base.as<uint64_t>(), g.d_sym.as<uint16_t>(), g.d_win.as<uint8_t>(),
                           win_len, out_cap, first_header ? 1u : 0u, g.d_end.as<GzChainEnd>(), g.d_order.as<uint32_t>(),
                           g.d_woff.as<uint64_t>(), g.d_wwl.as<uint32_t>());
        GZ_CHECK(hipGetLastError());
        GZ_CHECK(hipEventRecord(g.ev[5], g.st));
        order.resize(nw);
        woff.resize(nw);
        wwl.resize(nw);
        res.resize(nw);
        GZ_CHECK(hipMemcpyAsync(&e, g.d_end.p, sizeof e, hipMemcpyDeviceToHost, g.st));
        GZ_CHECK(hipMemcpyAsync(order.data(), g.d_order.p, 4ull * nw, hipMemcpyDeviceToHost, g.st));
        GZ_CHECK(hipMemcpyAsync(woff.data(), g.d_woff.p, 8ull * nw, hipMemcpyDeviceToHost, g.st));
        GZ_CHECK(hipMemcpyAsync(wwl.data(), g.d_wwl.p, 4ull * nw, hipMemcpyDeviceToHost, g.st));
        GZ_CHECK(hipMemcpyAsync(res.data(), g.d_res.p, sizeof(GzWaveRes) * (size_t)nw, hipMemcpyDeviceToHost, g.st));
        GZ_CHECK(hipStreamSynchronize(g.st));
        ran[2] = true;
        if (e.nconf > nw || e.end_slot > nw) {
            g.err = "sa_gunzip_run: the chain's result is out of range";
            return false;
        }
        nconf = e.nconf;
        order.resize(nconf);
        woff.resize(nconf);
        wwl.resize(nconf);
        return true;
    }
    bool resolve(const GzPlan&, const std::vector<uint32_t>& order, const std::vector<uint64_t>& woff, const std::vector<uint32_t>&,
                 const std::vector<GzWaveRes>& res, uint8_t* out, uint64_t text)
    {
        uint8_t* d_text = nullptr;
        if (sink) {
            // (the caller made room for out_cap >= text bytes behind wr; a wave outside [0, text) would write
            // outside them)
            sink_woff.resize(nconf);
            for (uint32_t k = 0; k < nconf; k++) {
                if (order[k] >= nw || woff[k] > text || res[order[k]].lb_sym > text - woff[k] || sink->wr + text > sink->cap) {
                    g.err = "sa_gunzip_run_dev: a confirmed wave's text lies outside the call's";
                    return false;
                }
                sink_woff[k] = sink->wr + woff[k];
            }
            GZ_CHECK(hipMemcpyAsync(g.d_woff.p, sink_woff.data(), 8ull * nconf, hipMemcpyHostToDevice, g.st));
            d_text = sink->buf;
        } else {
            GZ_CHECK(g.d_text.ensure(text + 16));
            d_text = g.d_text.as<uint8_t>();
        }
        GZ_CHECK(g.d_bad.ensure(4));
        GZ_CHECK(hipMemsetAsync(g.d_bad.p, 0, 4, g.st));
        GZ_CHECK(hipEventRecord(g.ev[6], g.st));
        hipLaunchKernelGGL(k_gz_resolve, dim3(64, nconf), dim3(256), 0, g.st, g.d_order.as<uint32_t>(), g.d_woff.as<uint64_t>(),
                           g.d_wwl.as<uint32_t>(), g.d_res.as<GzWaveRes>(), g.d_base.as<uint64_t>(), g.d_sym.as<uint16_t>(),
                           g.d_win.as<uint8_t>(), d_text, g.d_bad.as<uint32_t>());
        GZ_CHECK(hipGetLastError());
        GZ_CHECK(hipEventRecord(g.ev[7], g.st));
        GZ_CHECK(hipMemcpyAsync(&h_bad, g.d_bad.p, 4, hipMemcpyDeviceToHost, g.st));
        if (text && !sink) GZ_CHECK(hipMemcpyAsync(out, g.d_text.p, text, hipMemcpyDeviceToHost, g.st));
        ran[3] = true;
        return true;
    }
    bool crc(const std::vector<GzAccount::Task>& tasks, const uint8_t*, std::vector<uint32_t>& crcs)
    {
        ntasks = (uint32_t)tasks.size();
        if (!ntasks) return true;
        GZ_CHECK(g.d_tasks.ensure(sizeof(GzAccount::Task) * (size_t)ntasks));
        GZ_CHECK(g.d_crcs.ensure(4ull * ntasks));
        const GzAccount::Task* h_tasks = tasks.data();
        if (sink) {
            sink_tasks = tasks;
            for (GzAccount::Task& t : sink_tasks) t.off += sink->wr;
            h_tasks = sink_tasks.data();
        }
        GZ_CHECK(hipMemcpyAsync(g.d_tasks.p, h_tasks, sizeof(GzAccount::Task) * (size_t)ntasks, hipMemcpyHostToDevice, g.st));
        GZ_CHECK(hipMemsetAsync(g.d_counter.p, 0, 4, g.st));
        GZ_CHECK(hipEventRecord(g.ev[8], g.st));
        hipLaunchKernelGGL(k_gz_crc, dim3(std::min(g.grid, ntasks)), dim3(64), GZ_CRC_LDS, g.st,
                           sink ? sink->buf : g.d_text.as<uint8_t>(), g.d_tasks.as<GzAccount::Task>(), ntasks, g.d_crcs.as<uint32_t>(), g.d_counter.as<uint32_t>());
        GZ_CHECK(hipGetLastError());
        GZ_CHECK(hipEventRecord(g.ev[9], g.st));
        GZ_CHECK(hipMemcpyAsync(crcs.data(), g.d_crcs.p, 4ull * ntasks, hipMemcpyDeviceToHost, g.st));
        ran[4] = true;
        return true;
    }
    bool window(uint32_t slot, uint8_t* dst)
    {
        GZ_CHECK(hipMemcpyAsync(dst, g.d_win.as<uint8_t>() + (size_t)slot * GZ_RING, GZ_RING, hipMemcpyDeviceToHost, g.st));
        return true;
    }
    bool finish(sa_gunzip_info& inf, bool& bad)
    {
        GZ_CHECK(hipStreamSynchronize(g.st));
        bad = h_bad != 0;
        float* ms[5] = {&inf.find_ms, &inf.spec_ms, &inf.chain_ms, &inf.resolve_ms, &inf.crc_ms};
        g.kernel_ms = 0.f;
        for (int i = 0; i < 5; i++) {
            if (!ran[i]) continue;
            GZ_CHECK(hipEventElapsedTime(ms[i], g.ev[2 * i], g.ev[2 * i + 1]));
            g.kernel_ms += *ms[i];
        }
        return true;
    }
};
#undef GZ_CHECK

}  // namespace

extern "C" {

sa_gunzipper* sa_gunzipper_create(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return nullptr;
    sa_gunzipper* g = new sa_gunzipper();
    g->device = device;
    g->grid = 2u * (uint32_t)std::max(1, prop.multiProcessorCount);
    if (const char* e = std::getenv("SA_GUNZIP_GRID")) g->grid = (uint32_t)std::min(std::max(std::atoi(e), 1), 1 << 16);   // (tests)
    if (const char* e = std::getenv("SA_GUNZIP_CHUNK")) g->chunk = (uint32_t)std::min(std::max(std::atoi(e), 4096), 16 << 20);
    if (const char* e = std::getenv("SA_GUNZIP_RATIO")) g->ratio = (uint32_t)std::min(std::max(std::atoi(e), 1), 1024);
    bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess;
    for (hipEvent_t& e : g->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gz_spec), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)GZ_SPEC_LDS) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gz_chain), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)GZ_CHAIN_LDS) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gz_crc), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)GZ_CRC_LDS) == hipSuccess &&
         g->d_counter.ensure(256) == hipSuccess;
    if (!ok) {
        delete g;
        return nullptr;
    }
    return g;
}

void sa_gunzipper_destroy(sa_gunzipper* g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    delete g;
}

const char* sa_gunzipper_error(const sa_gunzipper* g) { return g ? g->err.c_str() : "no gunzipper"; }

float sa_gunzipper_kernel_ms(const sa_gunzipper* g) { return g ? g->kernel_ms : 0.f; }

uint32_t sa_gunzipper_grid(const sa_gunzipper* g) { return g ? g->grid : 0; }

uint32_t sa_gunzipper_chunk(const sa_gunzipper* g) { return g ? g->chunk : 0; }

int sa_gunzip_run(sa_gunzipper* g, const uint8_t* in, uint64_t in_bytes, int eof, sa_gunzip_state* state, uint8_t* out,
                  uint64_t out_cap, uint64_t* out_bytes, uint64_t* in_used, sa_gunzip_info* info)
{
    if (!g) return -1;
    g->err.clear();
    g->kernel_ms = 0.f;
    if (!state || !out_bytes || !in_used || (in_bytes && !in) || (out_cap && !out)) {
        g->err = "sa_gunzip_run: null argument";
        return -1;
    }
    GzDevice be{*g};
    return gz_run(be, in, in_bytes, eof, state, out, out_cap, out_bytes, in_used, info, g->chunk, g->ratio, g->err);
}

// The gunzipper's kernels run on its stream and the devtext's move and count on
// the devtext's.  No event orders the two: dt_make_room and dt_count return
// synchronised, and so does gz_run (finish), so each step finds the other
// stream idle -- sa_inflate_members_dev's arrangement.
int sa_gunzip_run_dev(sa_gunzipper* g, const uint8_t* in, uint64_t in_bytes, int eof, sa_gunzip_state* state, sa_devtext* dt,
                      uint64_t out_cap, uint64_t* text_bytes, uint64_t* in_used, sa_gunzip_info* info)
{
    if (!g) return -1;
    g->err.clear();
    g->kernel_ms = 0.f;
    if (text_bytes) *text_bytes = 0;
    if (!state || !text_bytes || !in_used || (in_bytes && !in) || !dt || dt->device != g->device) {
        g->err = "sa_gunzip_run_dev: null argument, or a devtext of another device";
        return -1;
    }
    if (out_cap > sa_devtext_room(dt)) {
        g->err = "sa_gunzip_run_dev: out_cap exceeds sa_devtext_room";
        return -3;
    }
    dt->err.clear();
    if (hipSetDevice(g->device) != hipSuccess) {
        g->err = "sa_gunzip_run_dev: hipSetDevice failed";
        return -1;
    }
    if (dt_make_room(dt, out_cap)) {
        g->err = "sa_gunzip_run_dev: " + dt->err;
        return -1;
    }
    GzDevice be{*g, dt};
    uint64_t text = 0;
    const int rc = gz_run(be, in, in_bytes, eof, state, nullptr, out_cap, &text, in_used, info, g->chunk, g->ratio, g->err);
    if (rc != 0) return rc;   // (bytes behind the write position are scratch: it does not move)
    if (dt_count(dt, dt->wr, dt->wr + text)) {
        g->err = "sa_gunzip_run_dev: " + dt->err;
        return -1;
    }
    dt->wr += text;
    *text_bytes = text;
    return 0;
}

}  // extern "C"
