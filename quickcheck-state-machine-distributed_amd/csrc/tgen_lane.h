// tgen_lane.h -- what the generator kernels of tgen.hip and ktgen.hip share:
// the per-lane RNG, the n-th set bit, and the LDS layouts of the byte columns
// and the staged 16-bit events (described at the head of tgen.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qsmd {

namespace {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kEvStride = 65;      // words per row of the staged events

struct TRng {   // gen.cpp's xoshiro256** / splitmix64
    uint64_t s0, s1, s2, s3;
    __device__ static uint64_t splitmix(uint64_t& x) {
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    __device__ TRng(uint64_t seed, uint64_t index) {
        uint64_t x = seed ^ (index * 0xD1B54A32D192ED03ull);
        s0 = splitmix(x);
        s1 = splitmix(x);
        s2 = splitmix(x);
        s3 = splitmix(x);
    }
    __device__ static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    __device__ uint64_t next() {
        const uint64_t r = rotl(s1 * 5, 7) * 9, t = s1 << 17;
        s2 ^= s0;
        s3 ^= s1;
        s1 ^= s2;
        s0 ^= s3;
        s2 ^= t;
        s3 = rotl(s3, 45);
        return r;
    }
    // (n > 0 at every call site but below(n_resp - 1) of a one-response model,
    // which the bug never reaches)
    __device__ uint32_t below(uint32_t n) { return (uint32_t)(((next() >> 32) * (uint64_t)n) >> 32); }
};

// the n-th set bit of m, ascending (n < popcount(m)): five halvings
__device__ __forceinline__ uint32_t nth_bit(uint32_t m, uint32_t n) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t sh = 16; sh; sh >>= 1) {
        const uint32_t low = m & ((1u << sh) - 1u);
        const uint32_t c = (uint32_t)__popc(low);
        const bool up = n >= c;
        n -= up ? c : 0u;
        m = up ? m >> sh : low;
        pos += up ? sh : 0u;
    }
    return pos;
}

// byte x of a lane's column, four to a word: [x / 4][lane][x & 3]
__device__ __forceinline__ uint32_t col8(uint32_t x, uint32_t lane) {
    return (((x >> 2) * kLanes + lane) << 2) | (x & 3u);
}
// 16-bit staged event e of a lane: [e / 2][lane][e & 1], rows of kEvStride words
__device__ __forceinline__ uint32_t ev16(uint32_t e, uint32_t lane) {
    return (((e >> 1) * kEvStride + lane) << 1) | (e & 1u);
}

// two events as they are stored: {kp, code, a, 0}, val = 0, twice (a
// qsmd_event array is 4-byte aligned, no more)
struct alignas(4) EvPair {
    uint32_t w[4];
};

}  // namespace

}  // namespace qsmd
