// scatter_map.h -- the load map of the packed scatter (lane.h
// stage_packed_body, 16-B path, power-of-two length): which 16-byte event
// pair of a packed block a lane loads, and where its two words land in the
// [event][history] LDS image.  Plain functions of (lane, u, N0) shared by
// the kernels and by the host check tools/scatter_map_check.cpp (no HIP
// needed to include it).
//
// A step covers 256 consecutive pairs of the block in 4 loads (u = 0..3) of
// 64 pairs.  In block order (lane L of load u takes pair 64 u + L) 16
// consecutive lanes of a 32-event history write one LDS column, i.e. one
// bank: each 32-lane half of the two stores of a ds_write2 is a 16-way
// conflict.  Here a lane quad still loads 64 contiguous bytes (4 pairs of
// one history), but the 16 quads of a load take as many histories as the
// step holds, so a 32-lane half writes 8 columns, 4 rows each: 4-way, the
// least a quad on 8 consecutive events of one history allows.
//
// pair of (lane, u) within the step = sm_lane_pair(lane) + sm_load_pair(u):
// a per-lane constant plus a wave-uniform term, a bijection onto 0..255.
// With P = N0 / 2 pairs per history and H = 256 / P histories per step,
// t = lane / 4, r = lane % 4:
//   P >= 16 (H <= 16)  history t % H, quad 4 (u (16 / H) + t / H) + r
//   P == 8  (H == 32)  history t + 16 (u % 2), pair 4 (u / 2) + r
//   P <= 4             block order (a quad already spans whole histories)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define QSMD_SM_FN __host__ __device__ __forceinline__
#else
#define QSMD_SM_FN inline
#endif

namespace qsmd {

constexpr uint32_t kScatterLoads = 4;     // loads of 64 pairs per step

// lp = log2(P) = log2(N0) - 1, 0..5
QSMD_SM_FN uint32_t sm_lane_pair(uint32_t lane, uint32_t lp) {
    const uint32_t t = lane >> 2, r = lane & 3u;
    if (lp <= 2u) return lane;
    if (lp == 3u) return (t << 3) + r;
    const uint32_t lh = 8u - lp;                        // log2(H): 4 or 3
    return ((t & ((1u << lh) - 1u)) << lp) + ((t >> lh) << 2) + r;
}
QSMD_SM_FN uint32_t sm_load_pair(uint32_t u, uint32_t lp) {
    if (lp <= 2u) return u << 6;
    if (lp == 3u) return ((u & 1u) << 7) + ((u >> 1) << 2);
    return u << (lp - 2u);                              // u * 64 / H
}
// the LDS word index (row e, column c of a [..][64] image: e * 64 + c) of
// the first event of pair q, q below 2^15; sh = log2(N0).  For the two
// terms above index(a + b) = index(a) + index(b): neither the event nor the
// history part carries.
QSMD_SM_FN uint32_t sm_index(uint32_t q, uint32_t sh) {
    const uint32_t g = 2u * q;
    return ((g & ((1u << sh) - 1u)) << 6) + (g >> sh);
}

// Any other length keeps block order; the history (= column) and the event
// of block event g by a multiply: exact for g < 2^16 (g * N0 < 2^21 << 2^32)
QSMD_SM_FN uint32_t sm_magic(uint32_t N0) { return (uint32_t)(0xFFFFFFFFull / N0) + 1u; }
QSMD_SM_FN uint32_t sm_col_magic(uint32_t g, uint32_t N0, uint32_t mg, uint32_t& e) {
    const uint32_t hh = (uint32_t)(((uint64_t)g * mg) >> 32);
    e = g - hh * N0;
    return hh;
}

}  // namespace qsmd
