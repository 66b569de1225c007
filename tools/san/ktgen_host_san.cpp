// Stand-alone sanitizer run of the host keyed-table generator
// (csrc/gen/ktgen.cpp): a few thousand histories from seeded random
// components on 1..8 keys, through every schedule setting, with unit and
// non-unit inv and key weights.  Host code only; build and run on a CPU:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/san/ktgen_host_san.cpp quickcheck-state-machine-distributed_amd/csrc/gen/ktgen.cpp \
//       -o /tmp/ktgen_host_san -lpthread && /tmp/ktgen_host_san
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "qsmd_gen.h"

int main() {
    std::mt19937_64 rng(54321);
    unsigned long long total = 0, stuck = 0, bugs = 0, keys_seen = 0;
    for (int round = 0; round < 32; ++round) {
        const uint32_t ns = round % 3 ? 256 : 7, ni = round % 3 ? 32 : 3, nr = round % 3 ? 32 : (round % 2 ? 5 : 1);
        const uint32_t n_keys = 1 + (uint32_t)(round % 8);
        std::vector<uint8_t> inv8(ns * ni), resp8(ns * nr);
        std::vector<uint32_t> post((size_t)ns * ni), err((size_t)ns * ni), weight(ni), key_weight(n_keys);
        for (auto& x : inv8) x = (uint8_t)(rng() % ns);
        for (auto& x : resp8) x = (uint8_t)(rng() % ns);
        for (auto& x : post) x = (uint32_t)(rng() & rng() & rng());
        for (auto& x : err) x = (uint32_t)(rng() & rng());
        // weights: rounds 0-1 of four none, round 2 of four 0 and 1 only, round 3 of four any small value
        for (auto& x : weight) x = (uint32_t)(rng() % (round % 4 == 2 ? 2 : 4));
        for (auto& x : key_weight) x = (uint32_t)(rng() % (round % 4 == 2 ? 2 : 5));
        weight[0] = 1;
        key_weight[n_keys - 1] = 1;
        qsmd_table_model tm{ns, ni, nr, (uint32_t)(rng() % ns), inv8.data(), resp8.data(), post.data(),
                            round % 4 ? err.data() : nullptr};
        qsmd_gen_ktable_params p{};
        p.n_keys = n_keys;
        p.n_clients = 1 + (uint32_t)(rng() % 32);
        p.n_ops = round % 5 == 0 ? 64 : 1 + (uint32_t)(rng() % 64);
        p.prefix_ops = (uint32_t)(rng() % (p.n_ops + 2));
        p.lin_policy = (round >> 1) & 1;
        p.pid_mode = (round >> 2) & 1;
        p.overlap = (uint32_t)(rng() % 4);
        p.p_bug = round % 3 ? 0.5 : 1.0;
        p.seed = rng();
        p.inv_weight = round % 4 >= 2 ? weight.data() : nullptr;
        p.key_weight = round % 4 >= 2 || round % 8 == 1 ? key_weight.data() : nullptr;
        const uint64_t n = 1500, first = round % 2 ? (1ull << 33) + 5 : 0;
        std::vector<qsmd_hdr> hdr(n);
        std::vector<qsmd_event> ev(n * 2 * p.n_ops);
        std::vector<uint8_t> fl(n);
        const int rc = qsmd_gen_ktable_batch(&p, &tm, first, n, 1000, hdr.data(), ev.data(), fl.data(),
                                             round % 2 ? 4 : 1);
        if (rc != 0) {
            std::fprintf(stderr, "round %d: rc %d\n", round, rc);
            return 1;
        }
        uint32_t keys = 0;
        for (uint64_t i = 0; i < n; ++i) {
            stuck += (fl[i] >> 1) & 1;
            bugs += fl[i] & 1;
            for (uint32_t e = 0; e < 2 * p.n_ops; ++e) {
                const qsmd_event& x = ev[i * 2 * p.n_ops + e];
                const bool resp = x.kp & QSMD_EV_RESP;
                if (x.code >= (resp ? nr : ni) || (x.kp & QSMD_EV_PID_MASK) >= p.n_clients ||
                    x.a >= (resp ? 1u : n_keys) || (!resp && p.key_weight && key_weight[x.a] == 0) ||
                    (!resp && p.inv_weight && weight[x.code] == 0)) {
                    std::fprintf(stderr, "round %d history %llu: symbol, key or pid out of range\n", round,
                                 (unsigned long long)i);
                    return 1;
                }
                if (!resp) keys |= 1u << x.a;
            }
        }
        keys_seen += (unsigned long long)__builtin_popcount(keys);
        total += n;
    }
    // the refusals write nothing: buffers of one entry would overflow under the sanitizer
    {
        uint8_t one8[1] = {0};
        uint32_t one32[1] = {1};
        qsmd_table_model tm{1, 1, 1, 0, one8, one8, one32, nullptr};
        qsmd_gen_ktable_params p{};
        p.n_keys = 9;
        p.n_clients = 4;
        p.n_ops = 16;
        qsmd_hdr h;
        qsmd_event e;
        if (qsmd_gen_ktable_batch(&p, &tm, 0, 1000, 0, &h, &e, nullptr, 4) != QSMD_ERR_ARG) return 1;
        p.n_keys = 8;
        p.n_ops = 65;
        if (qsmd_gen_ktable_batch(&p, &tm, 0, 1000, 0, &h, &e, nullptr, 4) != QSMD_ERR_ARG) return 1;
    }
    std::printf("ok: %llu histories, %llu stuck, %llu with a bug, %llu keys in use over the rounds\n", total, stuck,
                bugs, keys_seen);
    return 0;
}
