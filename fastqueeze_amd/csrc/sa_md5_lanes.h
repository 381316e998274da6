// sa_md5_lanes.h -- the host+device logic of the lane-per-message MD5
// (k_md5_lanes, sa_kernels.hip): which message goes to which lane of which
// chain wave, how many 64-byte blocks a message has, and the words of its
// last one or two (tail + padding) blocks from guarded byte reads.  Plain
// integer code for gfx950 and for the host: tests/cpu_emu/md5_lanes_emu.cpp
// runs the loader and the chain of one wave lane by lane through these
// functions and compares with known digests.
//
// RFC 1321 with the length field of the reference's MDString@0x4058f0: the
// u32 byte length x 8 as a 64-bit little-endian count.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef SA_HD
#define SA_HD __host__ __device__ inline
#endif
#else
#ifndef SA_HD
#define SA_HD inline
#endif
#endif

namespace sa {
namespace md5l {

constexpr uint32_t LANES = 64;    // messages per chain wave
constexpr uint32_t CHUNK = 8;     // blocks the loader hands over at a time
constexpr uint32_t SLOTS = 2;     // chunks in LDS (one read by the chain, one written)
// raw message words in LDS, [slot][block][word][lane]: 4 KiB a block
constexpr uint32_t LDS_BYTES = SLOTS * CHUNK * 16 * LANES * 4;
static_assert(LDS_BYTES <= 64 * 1024, "the workgroup stays within 64 KiB of LDS");

// ---- the grouping: tasks by length, longest first, stable; consecutive
//      tasks share a wave ----
SA_HD uint32_t wave_count(uint32_t ntasks) { return (ntasks + LANES - 1) / LANES; }
SA_HD uint32_t slot_wave(uint32_t slot) { return slot / LANES; }
SA_HD uint32_t slot_lane(uint32_t slot) { return slot % LANES; }

// order[slot] = the task that runs in lane slot % 64 of wave slot / 64
// (len(i): the byte length of task i)
template <class LenOf>
inline std::vector<uint32_t> lane_order(uint32_t ntasks, LenOf len)
{
    std::vector<uint32_t> order(ntasks);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return len(a) > len(b); });
    return order;
}

// ---- blocks of a message ----
SA_HD uint64_t full_blocks(uint64_t len) { return len / 64; }
// ... plus one padded block, or two when the 0x80 and the length do not fit
SA_HD uint64_t total_blocks(uint64_t len) { return len / 64 + ((len & 63) < 56 ? 1 : 2); }

// Byte j (0..127) of the message's tail: its last len % 64 bytes, 0x80, zeros,
// and the 8-byte bit count at the end of the one or two blocks.  Reads
// nothing at or past ptr + len.
SA_HD uint32_t tail_byte(const uint8_t* ptr, uint64_t len, uint32_t j)
{
    const uint32_t rem = (uint32_t)(len & 63);
    const uint32_t tl = rem < 56 ? 64u : 128u;
    const uint64_t bits = (uint64_t)(uint32_t)len << 3;
    if (j < rem) return ptr[(len - rem) + j];
    if (j == rem) return 0x80u;
    if (j >= tl - 8 && j < tl) return (uint32_t)(bits >> (8 * (j - (tl - 8)))) & 0xffu;
    return 0u;
}

// Word w (0..15) of block blk >= full_blocks(len) (little-endian, RFC 1321
// 3.4).  ptr is 4-byte aligned (the host aligns every message to 16): a word
// that lies wholly inside the message is one load.
SA_HD uint32_t tail_word(const uint8_t* ptr, uint64_t len, uint64_t blk, uint32_t w)
{
    const uint32_t j = (uint32_t)(blk - full_blocks(len)) * 64 + 4 * w;
    const uint32_t rem = (uint32_t)(len & 63);
    if (j + 4 <= rem) {
        uint32_t v;
        __builtin_memcpy(&v, __builtin_assume_aligned(ptr + (len - rem) + j, 4), 4);
        return v;
    }
    return tail_byte(ptr, len, j) | tail_byte(ptr, len, j + 1) << 8 | tail_byte(ptr, len, j + 2) << 16 |
           tail_byte(ptr, len, j + 3) << 24;
}

// ---- the chain's tables ----
constexpr uint32_t K[64] = {
    0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
    0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
    0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
    0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
    0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
    0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
    0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
    0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};
constexpr uint32_t H0[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};

// message word and rotation of step i
SA_HD constexpr uint32_t word_of_step(uint32_t i)
{
    return i < 16 ? i : i < 32 ? (5 * i + 1) & 15 : i < 48 ? (3 * i + 5) & 15 : (7 * i) & 15;
}
SA_HD constexpr uint32_t rot_of_step(uint32_t i)
{
    return i < 16   ? (i % 4 == 0 ? 7u : i % 4 == 1 ? 12u : i % 4 == 2 ? 17u : 22u)
           : i < 32 ? (i % 4 == 0 ? 5u : i % 4 == 1 ? 9u : i % 4 == 2 ? 14u : 20u)
           : i < 48 ? (i % 4 == 0 ? 4u : i % 4 == 1 ? 11u : i % 4 == 2 ? 16u : 23u)
                    : (i % 4 == 0 ? 6u : i % 4 == 1 ? 10u : i % 4 == 2 ? 15u : 21u);
}

// One block of one lane in plain C++ (the kernel's chain is the same steps
// with v_bitop3 / v_add3 / v_alignbit): a lane past its own last block keeps
// its state by a select.  (Host only: the CPU emulation's chain.)
inline void block_ref(uint32_t h[4], const uint32_t m[16], bool active)
{
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
    for (uint32_t i = 0; i < 64; i++) {
        const uint32_t f = i < 16 ? ((b & c) | (~b & d)) : i < 32 ? ((d & b) | (~d & c)) : i < 48 ? (b ^ c ^ d) : (c ^ (b | ~d));
        const uint32_t x = a + f + (m[word_of_step(i)] + K[i]);
        const uint32_t s = rot_of_step(i);
        const uint32_t t = d;
        d = c;
        c = b;
        b = b + ((x << s) | (x >> (32 - s)));
        a = t;
    }
    h[0] = active ? h[0] + a : h[0];
    h[1] = active ? h[1] + b : h[1];
    h[2] = active ? h[2] + c : h[2];
    h[3] = active ? h[3] + d : h[3];
}

}  // namespace md5l
}  // namespace sa
