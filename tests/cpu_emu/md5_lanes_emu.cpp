// md5_lanes_emu.cpp -- k_md5_lanes (sa_kernels.hip) on the CPU, through the
// host+device logic of sa_md5_lanes.h: the host's grouping of a batch's
// messages into chain waves, then per wave the loader (each lane's 16-byte
// loads of its full blocks, its tail blocks from guarded reads, the words into
// the [slot][block][word][lane] LDS image a chunk ahead) and the chain (every
// lane's block from the LDS image, a lane past its last block keeping its
// state), chunk by chunk as the kernel's two waves do.
//
//   md5_lanes_emu digests <file>
//     file: u32 n, n x u32 byte lengths, then the messages' bytes back to back.
//     Every message lives in a heap block of exactly its length (16-byte
//     aligned, as the engine's are), so under -fsanitize=address a read at or
//     past ptr + len is reported.  Prints "order <task> ..." (the lane order)
//     and per task, in task order, "<task> <wave> <lane> <32 hex digits>".
//   md5_lanes_emu knobs
//     "md5_lanes <0|1> md5_pipe <0|1> path <sa_paths::md5 with MD5 on> path_off
//     <with MD5 off>" from the environment (parse_knobs, plan_paths).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastqueeze_amd/csrc/sa_md5_lanes.h"
#include "../../fastqueeze_amd/csrc/sa_plan.h"

using namespace sa;

namespace {

struct Msg {
    uint8_t* base = nullptr;   // the allocation
    const uint8_t* ptr = nullptr;
    uint64_t len = 0;
};

// a 16-byte aligned block of exactly len bytes (len 0: the end of a block)
Msg make_msg(const uint8_t* src, uint64_t len)
{
    Msg m;
    void* p = nullptr;
    if (posix_memalign(&p, 16, len ? len : 16)) std::abort();
    m.base = static_cast<uint8_t*>(p);
    m.ptr = len ? m.base : m.base + 16;
    m.len = len;
    if (len) std::memcpy(m.base, src, len);
    return m;
}

// One chain wave: the lanes' messages are tasks order[first .. first + n).
void run_wave(const std::vector<Msg>& msgs, const uint32_t* order, uint32_t n, uint32_t (*digests)[4])
{
    constexpr uint32_t CH = md5l::CHUNK, L = md5l::LANES, BLK_W = 16 * L;
    std::vector<uint32_t> lds(md5l::LDS_BYTES / 4, 0xdeadbeefu);   // [slot][block][word][lane]
    static_assert(md5l::LDS_BYTES == md5l::SLOTS * CH * BLK_W * 4, "LDS image");
    uint32_t h[L][4];
    uint64_t nfull[L], nblk[L], wb = 0;
    for (uint32_t l = 0; l < L; l++) {
        const bool have = l < n;
        const uint64_t len = have ? msgs[order[l]].len : 0;
        nfull[l] = md5l::full_blocks(len);
        nblk[l] = have ? md5l::total_blocks(len) : 0;
        wb = std::max(wb, nblk[l]);
        for (int k = 0; k < 4; k++) h[l][k] = md5l::H0[k];
    }
    const uint64_t nck = (wb + CH - 1) / CH;
    std::vector<uint32_t> q((size_t)L * CH * 16);   // the loader's registers: [lane][block][word]
    auto fetch = [&](uint64_t c) {
        for (uint32_t l = 0; l < n; l++) {
            if (!nfull[l]) continue;   // (the kernel: 16 bytes of the task table, unused)
            const uint8_t* p = msgs[order[l]].ptr;
            for (uint32_t k = 0; k < CH; k++) {
                const uint64_t at = std::min<uint64_t>(c * CH + k, nfull[l] - 1) * 64;
                for (uint32_t j = 0; j < 4; j++) std::memcpy(&q[((size_t)l * CH + k) * 16 + 4 * j], p + at + 16 * j, 16);
            }
        }
    };
    auto stash = [&](uint64_t c) {
        uint32_t* s = lds.data() + (c & 1) * CH * BLK_W;
        for (uint32_t l = 0; l < L; l++) {
            for (uint32_t k = 0; k < CH; k++)
                for (uint32_t w = 0; w < 16; w++) s[(k * 16 + w) * L + l] = q[((size_t)l * CH + k) * 16 + w];
            const uint64_t b0 = c * CH;
            if (l < n && b0 + CH > nfull[l] && b0 < nblk[l])
                for (uint32_t k = 0; k < CH; k++) {
                    const uint64_t bi = b0 + k;
                    if (bi < nfull[l] || bi >= nblk[l]) continue;
                    const Msg& m = msgs[order[l]];
                    for (uint32_t w = 0; w < 16; w++) s[(k * 16 + w) * L + l] = md5l::tail_word(m.ptr, m.len, bi, w);
                }
        }
    };
    fetch(0);
    stash(0);
    if (nck > 1) fetch(1);
    for (uint64_t c = 0; c < nck; c++) {
        // (the chain wave first: the loader writes the other slot)
        const uint64_t b0 = c * CH;
        const uint32_t nb = wb - b0 < CH ? (uint32_t)(wb - b0) : CH;
        const uint32_t* s = lds.data() + (c & 1) * CH * BLK_W;
        for (uint32_t k = 0; k < nb; k++)
            for (uint32_t l = 0; l < L; l++) {
                uint32_t m[16];
                for (uint32_t w = 0; w < 16; w++) m[w] = s[(k * 16 + w) * L + l];
                md5l::block_ref(h[l], m, b0 + k < nblk[l]);
            }
        if (c + 1 < nck) stash(c + 1);
        if (c + 2 < nck) fetch(c + 2);
    }
    for (uint32_t l = 0; l < n; l++)
        for (int k = 0; k < 4; k++) digests[order[l]][k] = h[l][k];
}

int digests_mode(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    uint32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return 2;
    std::vector<uint32_t> lens(n);
    if (n && std::fread(lens.data(), 4, n, f) != n) return 2;
    std::vector<Msg> msgs;
    for (uint32_t i = 0; i < n; i++) {
        std::vector<uint8_t> buf(lens[i]);
        if (lens[i] && std::fread(buf.data(), 1, lens[i], f) != lens[i]) return 2;
        msgs.push_back(make_msg(buf.data(), lens[i]));
    }
    std::fclose(f);
    const std::vector<uint32_t> order = md5l::lane_order(n, [&](uint32_t i) { return msgs[i].len; });
    std::vector<uint32_t> where(n, ~0u);
    std::printf("order");
    for (uint32_t s = 0; s < n; s++) {
        std::printf(" %u", order[s]);
        if (order[s] >= n || where[order[s]] != ~0u) return 3;   // every task placed exactly once
        where[order[s]] = s;
    }
    std::printf("\n");
    // (sentinel digests: a task no wave wrote shows)
    std::vector<uint32_t> dg((size_t)n * 4, 0xffffffffu);
    auto* d4 = reinterpret_cast<uint32_t(*)[4]>(dg.data());
    for (uint32_t w = 0; w < md5l::wave_count(n); w++)
        run_wave(msgs, order.data() + w * md5l::LANES, std::min(md5l::LANES, n - w * md5l::LANES), d4);
    for (uint32_t i = 0; i < n; i++) {
        std::printf("%u %u %u ", i, md5l::slot_wave(where[i]), md5l::slot_lane(where[i]));
        for (int k = 0; k < 4; k++)
            for (int b = 0; b < 4; b++) std::printf("%02x", (d4[i][k] >> (8 * b)) & 0xff);
        std::printf("\n");
    }
    for (Msg& m : msgs) std::free(m.base);
    return 0;
}

const char* env_get(const char* n) { return std::getenv(n); }

int knobs_mode()
{
    const EngineKnobs k = parse_knobs(env_get);
    const RunKnobs rk = parse_run_knobs(env_get, parse_sort_min_db(env_get));
    const BatchShape sh{1000, 150000, 2, false, true};
    const PathPlan on = plan_paths(k, rk, PathCfg{3, 2, false, true}, sh);
    const PathPlan off = plan_paths(k, rk, PathCfg{3, 2, false, false}, sh);
    std::printf("md5_lanes %d md5_pipe %d path %u path_off %u\n", k.md5_lanes, k.md5_pipe, on.md5, off.md5);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "digests")) return digests_mode(argv[2]);
    if (argc == 2 && !std::strcmp(argv[1], "knobs")) return knobs_mode();
    std::fprintf(stderr, "usage: md5_lanes_emu digests <file> | knobs\n");
    return 1;
}
