// tgen_stream.h -- what the table generators of libqsmd_gen.so share
// (tgen.cpp: models 3 and 4; ktgen.cpp: model 5): the RNG, the schedule of
// include/qsmd_gen.h ("table-model generator", Schedule 1-4) over any machine
// that can request and execute, the checks of the schedule's parameters and
// the index-sharded driver that writes the headers.  No HIP.
//
// A machine M has
//   typename M::State, typename M::Sym (an invocation symbol, trivially copyable)
//   State    init() const
//   Sym      request(Rng&, const State&) const            one draw
//   uint32_t execute(Rng&, State&, Sym, uint8_t& flags) const   one draw; the response
//   uint32_t n_resp() const
//   qsmd_event inv_event(uint8_t kp, Sym) const            the invocation event
#pragma once

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "qsmd_gen.h"

namespace qsmd_tgen {

struct Rng {  // xoshiro256** seeded by splitmix64 (gen.cpp's)
    uint64_t s[4];
    static uint64_t splitmix(uint64_t& x) {
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    Rng(uint64_t seed, uint64_t index) {
        uint64_t x = seed ^ (index * 0xD1B54A32D192ED03ull);
        for (auto& v : s) v = splitmix(x);
    }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    uint64_t next() {
        const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3];
        s[2] ^= t; s[3] = rotl(s[3], 45);
        return r;
    }
    uint32_t below(uint32_t n) { return n ? (uint32_t)((next() >> 32) * n >> 32) : 0; }
    double unit() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
};

// the schedule's parameters: the fields qsmd_gen_table_params and
// qsmd_gen_ktable_params have in common
struct Sched {
    uint32_t n_clients, n_ops, prefix_ops, lin_policy, pid_mode, overlap;
    double p_bug;
    uint64_t seed;
};

// the parameter ranges and the event-offset overflow of qsmd_gen_table_batch
inline bool sched_ok(const Sched& p, uint64_t n_hist, uint32_t ev_base) {
    if (p.n_clients < 1 || p.n_clients > 32 || p.n_ops < 1 || 2 * p.n_ops > QSMD_MAX_EVENTS) return false;
    if (p.lin_policy > 1 || p.pid_mode > 1) return false;
    if (!(p.p_bug >= 0.0 && p.p_bug <= 1.0)) return false;       // (NaN fails both)
    const uint32_t per = 2 * p.n_ops;
    if ((uint64_t)ev_base + n_hist * (uint64_t)per > 0xFFFFFFFFull || n_hist > 0xFFFFFFFFull) return false;
    return true;
}

// one history: 2 * n_ops events at ev, the flag byte at flag_out (nullable)
template <class M>
void gen_one(const Sched& p, const M& m, uint64_t index, qsmd_event* ev, uint8_t* flag_out) {
    using Sym = typename M::Sym;
    Rng r(p.seed, index);
    const uint32_t C = p.n_clients, K = p.n_ops;
    const uint32_t P = std::min(p.prefix_ops, K), S = K - P;
    const uint32_t overlap = p.overlap ? p.overlap : C;
    const bool shared = p.pid_mode == QSMD_GEN_PID_SHARED;
    typename M::State s = m.init();
    uint8_t flags = 0;
    uint32_t ne = 0;
    auto emit_inv = [&](uint32_t c, Sym i) { ev[ne++] = m.inv_event((uint8_t)(shared ? 0u : c), i); };
    auto emit_resp = [&](uint32_t c, uint32_t code) {
        ev[ne++] = qsmd_event{(uint8_t)(QSMD_EV_RESP | (shared ? 0u : c)), (uint8_t)code, 0, 0, 0};
    };

    for (uint32_t k = 0; k < P; ++k) {
        const uint32_t c = r.below(C);
        const Sym i = m.request(r, s);
        const uint32_t x = m.execute(r, s, i, flags);
        emit_inv(c, i);
        emit_resp(c, x);
    }

    uint32_t queued[32] = {}, resp[32] = {};
    Sym inv[32] = {};
    uint8_t st[32] = {};                      // 0 idle, 1 invoked, 2 executed
    for (uint32_t k = 0; k < S; ++k) queued[r.below(C)]++;
    uint32_t outstanding = 0, done = 0;
    uint32_t act[32];
    while (done < S) {
        uint32_t n_act = 0;
        for (uint32_t c = 0; c < C; ++c)
            if (st[c] ? true : (queued[c] && outstanding < overlap)) act[n_act++] = c;
        const uint32_t c = act[r.below(n_act)];
        if (st[c] == 0) {
            inv[c] = m.request(r, s);
            emit_inv(c, inv[c]);
            queued[c]--;
            outstanding++;
            if (p.lin_policy == QSMD_GEN_LIN_AT_INVOKE) {
                resp[c] = m.execute(r, s, inv[c], flags);
                st[c] = 2;
            } else {
                st[c] = 1;
            }
        } else if (st[c] == 1) {
            resp[c] = m.execute(r, s, inv[c], flags);
            st[c] = 2;
        } else {
            emit_resp(c, resp[c]);
            st[c] = 0;
            outstanding--;
            done++;
        }
    }

    if (p.p_bug > 0 && r.unit() < p.p_bug && S >= 1) {
        uint32_t at[64], n = 0;               // the suffix responses' positions
        for (uint32_t e = 2 * P; e < ne; ++e)
            if (ev[e].kp & QSMD_EV_RESP) at[n++] = e;
        const uint32_t n_resp = m.n_resp();
        const bool two = n_resp >= 2;
        const uint32_t coin = two && S >= 2 ? r.below(2) : 0u;
        if (two && (S < 2 || coin == 0)) {
            const uint32_t e = at[r.below(S)];
            ev[e].code = (uint8_t)((ev[e].code + 1u + r.below(n_resp - 1)) % n_resp);
            flags |= 1u;
        } else if (S >= 2) {
            const uint32_t k1 = r.below(S);
            uint32_t k2 = r.below(S);
            if (k2 == k1) k2 = (k1 + 1) % S;
            std::swap(ev[at[k1]].code, ev[at[k2]].code);
            flags |= 1u;
        }
    }
    if (flag_out) *flag_out = flags;
}

// histories [first, first + n_hist): the headers and gen_one, by index shard
template <class M>
void gen_batch(const Sched& p, const M& m, uint32_t model_id, uint64_t first, uint64_t n_hist, uint32_t ev_base,
               qsmd_hdr* hdr, qsmd_event* events, uint8_t* bug_out, int n_threads) {
    const uint32_t per = 2 * p.n_ops;
    if (n_threads < 1) n_threads = 1;
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            qsmd_hdr& h = hdr[i];
            std::memset(&h, 0, sizeof(h));
            h.ev_off = ev_base + (uint32_t)(i * per);
            h.n_ev = (uint16_t)per;
            h.n_pid = (uint8_t)(p.pid_mode == QSMD_GEN_PID_SHARED ? 1 : p.n_clients);
            h.model_id = (uint8_t)model_id;
            h.tag = (uint32_t)(first + i);
            gen_one(p, m, first + i, events + i * per, bug_out ? bug_out + i : nullptr);
        }
    };
    if (n_threads == 1 || n_hist < 1024) { work(0, n_hist); return; }
    std::vector<std::thread> th;
    const uint64_t chunk = (n_hist + n_threads - 1) / n_threads;
    for (int t = 0; t < n_threads; ++t) {
        const uint64_t lo = t * chunk, hi = std::min<uint64_t>(n_hist, lo + chunk);
        if (lo >= hi) break;
        th.emplace_back(work, lo, hi);
    }
    for (auto& x : th) x.join();
}

}  // namespace qsmd_tgen
