// Host check of the packed scatter's load map (csrc/scatter_map.h as used by
// lane.h stage_packed_body): no GPU.
//
//   g++ -O1 -std=c++17 -Iquickcheck-state-machine-distributed_amd/csrc tools/scatter_map_check.cpp -o scatter_map_check
//   ./scatter_map_check            (may also be built with -fsanitize=address,undefined)
//
// For every common length 2..64, group size 1, 2, 63, 64 and both parities
// of the block's first event it replays the stage's steps lane by lane --
// the 16-byte path (power-of-two lengths through the map, the others in
// block order) or the 8-byte path of an unaligned block -- and checks that
// every event of the block is loaded exactly once and stored at
// [event][history] of the 64-column image, and nothing else is stored.  It
// prints, per length, the worst bank-conflict degree of one store
// instruction: the most distinct addresses on one of the 32 banks within a
// 32-lane half (how the LDS serves a 4-byte store), beside the degree of
// block order.  Exit status 0 when every case holds.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <vector>

#include "scatter_map.h"

using namespace qsmd;

namespace {

constexpr uint32_t LANES = 64, ROWS = 64, U = kScatterLoads;

struct Image {
    int32_t ev[ROWS][LANES];          // block event stored here, -1: none
    std::vector<uint32_t> loads;      // times each block event was loaded
    bool ok = true;
    uint32_t worst = 0;               // conflict degree over the store instructions
    void reset(uint32_t total) {
        memset(ev, 0xFF, sizeof ev);
        loads.assign(total, 0);
        ok = true;
        worst = 0;
    }
    void store(uint32_t idx, uint32_t g) {
        if (idx >= ROWS * LANES || ev[idx / LANES][idx % LANES] != -1) {
            ok = false;
            return;
        }
        ev[idx / LANES][idx % LANES] = (int32_t)g;
    }
};

// one store instruction: idx[lane] (word index) for the lanes of `exec`
void degree(Image& im, const uint32_t* idx, uint64_t exec) {
    for (uint32_t half = 0; half < 2; ++half) {
        std::set<uint32_t> bank[32];
        for (uint32_t l = half * 32; l < half * 32 + 32; ++l)
            if ((exec >> l) & 1u) bank[idx[l] % 32u].insert(idx[l]);
        for (auto& b : bank) im.worst = std::max(im.worst, (uint32_t)b.size());
    }
}

// the 16-byte path; mapped: power-of-two lengths through scatter_map.h,
// otherwise block order with the same index arithmetic
void path16(Image& im, uint32_t N0, uint32_t nh, bool mapped) {
    const bool pow2 = (N0 & (N0 - 1u)) == 0u && N0 >= 2u;
    const uint32_t total = nh * N0, nq = total / 2u;
    const uint32_t sh = pow2 ? (uint32_t)__builtin_ctz(N0) : 0u, lp = mapped ? sh - 1u : 0u;
    const uint32_t mg = pow2 ? 0u : sm_magic(N0);
    auto step = [&](uint32_t k0, bool guard) {
        for (uint32_t u = 0; u < U; ++u) {
            uint32_t i0[LANES], i1[LANES];
            uint64_t exec = 0;
            for (uint32_t lane = 0; lane < LANES; ++lane) {
                uint32_t q;
                if (pow2) {
                    const uint32_t q_lane = sm_lane_pair(lane, lp), i_lane = sm_index(q_lane, sh);
                    q = k0 + sm_load_pair(u, lp) + q_lane;
                    i0[lane] = ((2u * k0) >> sh) + sm_index(sm_load_pair(u, lp), sh) + i_lane;
                    i1[lane] = i0[lane] + LANES;
                } else {
                    q = k0 + u * 64u + lane;
                    uint32_t e0, e1;
                    const uint32_t c0 = sm_col_magic(2u * q, N0, mg, e0), c1 = sm_col_magic(2u * q + 1u, N0, mg, e1);
                    i0[lane] = e0 * LANES + c0;
                    i1[lane] = e1 * LANES + c1;
                }
                if (guard && q >= nq) continue;
                if (q >= nq) {          // a full step never leaves the block
                    im.ok = false;
                    continue;
                }
                exec |= 1ull << lane;
                ++im.loads[2u * q];
                ++im.loads[2u * q + 1u];
                im.store(i0[lane], 2u * q);
                im.store(i1[lane], 2u * q + 1u);
            }
            degree(im, i0, exec);
            degree(im, i1, exec);
        }
    };
    uint32_t k0 = 0;
    for (; k0 + U * 64u <= nq; k0 += U * 64u) step(k0, false);
    if (k0 < nq) step(k0, true);
}

// the 8-byte path of a block with an odd first event or an odd event count
void path8(Image& im, uint32_t N0, uint32_t nh) {
    const bool pow2 = (N0 & (N0 - 1u)) == 0u && N0 >= 2u;
    const uint32_t total = nh * N0;
    const uint32_t sh = pow2 ? (uint32_t)__builtin_ctz(N0) : 0u, mg = pow2 ? 0u : sm_magic(N0);
    auto step = [&](uint32_t k0, bool guard) {
        for (uint32_t u = 0; u < 2u * U; ++u) {
            uint32_t i0[LANES];
            uint64_t exec = 0;
            for (uint32_t lane = 0; lane < LANES; ++lane) {
                const uint32_t g = k0 + u * 64u + lane;
                uint32_t e, c;
                if (pow2) {
                    e = g & (N0 - 1u);
                    c = g >> sh;
                } else {
                    c = sm_col_magic(g, N0, mg, e);
                }
                i0[lane] = e * LANES + c;
                if (guard && g >= total) continue;
                if (g >= total) {
                    im.ok = false;
                    continue;
                }
                exec |= 1ull << lane;
                ++im.loads[g];
                im.store(i0[lane], g);
            }
            degree(im, i0, exec);
        }
    };
    uint32_t k0 = 0;
    for (; k0 + 2u * U * 64u <= total; k0 += 2u * U * 64u) step(k0, false);
    if (k0 < total) step(k0, true);
}

bool verify(const Image& im, uint32_t N0, uint32_t nh) {
    if (!im.ok) return false;
    for (uint32_t x : im.loads)
        if (x != 1u) return false;
    for (uint32_t e = 0; e < ROWS; ++e)
        for (uint32_t c = 0; c < LANES; ++c) {
            const int32_t want = (e < N0 && c < nh) ? (int32_t)(c * N0 + e) : -1;
            if (im.ev[e][c] != want) return false;
        }
    return true;
}

}  // namespace

int main() {
    static Image im;
    const uint32_t sizes[] = {1, 2, 63, 64};
    int failed = 0, cases = 0;
    printf("length  full group, 16-byte path: worst conflict degree per store (block order)\n");
    for (uint32_t N0 = 2; N0 <= 64; ++N0) {
        const bool pow2 = (N0 & (N0 - 1u)) == 0u;
        for (uint32_t nh : sizes)
            for (uint32_t off0 = 0; off0 < 2; ++off0) {
                const uint32_t total = nh * N0;
                const bool wide = ((off0 | total) & 1u) == 0u;
                im.reset(total);
                if (wide) path16(im, N0, nh, pow2);
                else path8(im, N0, nh);
                ++cases;
                if (!verify(im, N0, nh)) {
                    ++failed;
                    printf("FAIL length %u group %u first event %u (%s path)\n", N0, nh, off0, wide ? "16-byte" : "8-byte");
                }
                if (nh == 64 && off0 == 0) {
                    const uint32_t w = im.worst;
                    im.reset(total);
                    path16(im, N0, nh, false);
                    if (!verify(im, N0, nh)) {
                        ++failed;
                        printf("FAIL length %u block order\n", N0);
                    }
                    printf("%6u  %2u (%2u)%s\n", N0, w, im.worst, pow2 ? "" : "  block order kept");
                }
            }
    }
    printf("%d cases, %d failed\n", cases, failed);
    return failed ? 1 : 0;
}
