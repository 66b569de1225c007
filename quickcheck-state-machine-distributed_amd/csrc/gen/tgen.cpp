// tgen.cpp -- seeded history generator for the table models
// (qsmd_gen_table_batch, include/qsmd_gen.h).
//
// gen.cpp's scheduler policy and RNG with the table as the implementation:
// requests are drawn among the invocations the current state accepts a
// response for, and an operation's response is drawn among the accepted ones
// at its linearisation point.  The header's comment is the definition; this
// file follows it line by line (the device kernel, csrc/tgen.hip, keeps the
// same stream in registers and LDS).
#include "qsmd_gen.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

namespace {

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

// Either table behind one face: acc(s, i) as post_words words.
struct Model {
    uint32_t n_states, n_inv, n_resp, init_state, post_words;
    bool wide;
    const void* on_inv;
    const void* on_resp;
    const uint32_t* post;
    const uint32_t* post_err;

    uint32_t inv_to(uint32_t s, uint32_t i) const {
        const size_t k = (size_t)s * n_inv + i;
        return wide ? static_cast<const uint16_t*>(on_inv)[k] : static_cast<const uint8_t*>(on_inv)[k];
    }
    uint32_t resp_to(uint32_t s, uint32_t r) const {
        const size_t k = (size_t)s * n_resp + r;
        return wide ? static_cast<const uint16_t*>(on_resp)[k] : static_cast<const uint8_t*>(on_resp)[k];
    }
    // acc(s, i) into a[0 .. post_words); returns its popcount
    uint32_t acc(uint32_t s, uint32_t i, uint32_t* a) const {
        const size_t k = ((size_t)s * n_inv + i) * post_words;
        uint32_t n = 0;
        for (uint32_t w = 0; w < post_words; ++w) {
            uint32_t x = post[k + w];
            if (post_err) x &= ~post_err[k + w];
            const uint32_t left = n_resp - 32u * w;        // bits of this word below n_resp
            if (left < 32u) x &= (1u << left) - 1u;
            a[w] = x;
            n += (uint32_t)__builtin_popcount(x);
        }
        return n;
    }
};

struct Gen {
    const qsmd_gen_table_params& p;
    const Model& m;
    const uint32_t* weight;        // n_inv entries
    uint32_t w_all;                // the sum of all weights

    uint32_t request(Rng& r, uint32_t s) const {
        uint32_t a[QSMD_WTABLE_MAX_RESP / 32];
        uint8_t en[QSMD_WTABLE_MAX_INV];
        uint32_t W = 0;
        for (uint32_t i = 0; i < m.n_inv; ++i) {
            en[i] = weight[i] > 0 && m.acc(s, i, a) != 0;
            if (en[i]) W += weight[i];
        }
        if (W == 0) {
            for (uint32_t i = 0; i < m.n_inv; ++i) en[i] = weight[i] > 0;
            W = w_all;
        }
        const uint32_t w = r.below(W);
        uint64_t run = 0;
        for (uint32_t i = 0; i < m.n_inv; ++i) {
            if (!en[i]) continue;
            run += weight[i];
            if (run > w) return i;
        }
        return m.n_inv - 1;   // (not reached: run ends at W > w)
    }

    uint32_t execute(Rng& r, uint32_t& s, uint32_t i, uint8_t& flags) const {
        uint32_t a[QSMD_WTABLE_MAX_RESP / 32];
        const uint32_t n = m.acc(s, i, a);
        uint32_t resp;
        if (n) {
            uint32_t k = r.below(n);
            resp = 0;
            for (uint32_t b = 0; b < m.n_resp; ++b) {
                if (!((a[b >> 5] >> (b & 31u)) & 1u)) continue;
                if (k-- == 0) { resp = b; break; }
            }
        } else {
            resp = r.below(m.n_resp);
            flags |= 2u;
        }
        s = m.resp_to(m.inv_to(s, i), resp);
        return resp;
    }

    void one(uint64_t index, qsmd_event* ev, uint8_t* flag_out) const {
        Rng r(p.seed, index);
        const uint32_t C = p.n_clients, K = p.n_ops;
        const uint32_t P = std::min(p.prefix_ops, K), S = K - P;
        const uint32_t overlap = p.overlap ? p.overlap : C;
        const bool shared = p.pid_mode == QSMD_GEN_PID_SHARED;
        uint32_t s = m.init_state;
        uint8_t flags = 0;
        uint32_t ne = 0;
        auto emit = [&](uint32_t c, bool resp, uint32_t code) {
            ev[ne++] = qsmd_event{(uint8_t)((resp ? QSMD_EV_RESP : 0u) | (shared ? 0u : c)), (uint8_t)code, 0, 0, 0};
        };

        for (uint32_t k = 0; k < P; ++k) {
            const uint32_t c = r.below(C);
            const uint32_t i = request(r, s);
            const uint32_t x = execute(r, s, i, flags);
            emit(c, false, i);
            emit(c, true, x);
        }

        uint32_t queued[32] = {}, inv[32] = {}, resp[32] = {};
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
                inv[c] = request(r, s);
                emit(c, false, inv[c]);
                queued[c]--;
                outstanding++;
                if (p.lin_policy == QSMD_GEN_LIN_AT_INVOKE) {
                    resp[c] = execute(r, s, inv[c], flags);
                    st[c] = 2;
                } else {
                    st[c] = 1;
                }
            } else if (st[c] == 1) {
                resp[c] = execute(r, s, inv[c], flags);
                st[c] = 2;
            } else {
                emit(c, true, resp[c]);
                st[c] = 0;
                outstanding--;
                done++;
            }
        }

        if (p.p_bug > 0 && r.unit() < p.p_bug && S >= 1) {
            uint32_t at[64], n = 0;               // the suffix responses' positions
            for (uint32_t e = 2 * P; e < ne; ++e)
                if (ev[e].kp & QSMD_EV_RESP) at[n++] = e;
            const bool two = m.n_resp >= 2;
            const uint32_t coin = two && S >= 2 ? r.below(2) : 0u;
            if (two && (S < 2 || coin == 0)) {
                const uint32_t e = at[r.below(S)];
                ev[e].code = (uint8_t)((ev[e].code + 1u + r.below(m.n_resp - 1)) % m.n_resp);
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
};

template <class T, class S>
bool model_ok(const T* t, uint32_t max_states, uint32_t max_sym) {
    if (!t || !t->on_inv || !t->on_resp || !t->post) return false;
    if (t->n_states == 0 || t->n_states > max_states || t->n_inv == 0 || t->n_inv > max_sym || t->n_resp == 0 ||
        t->n_resp > max_sym || t->init_state >= t->n_states)
        return false;
    const uint64_t si = (uint64_t)t->n_states * t->n_inv, sr = (uint64_t)t->n_states * t->n_resp;
    const S* a = static_cast<const S*>(t->on_inv);
    const S* b = static_cast<const S*>(t->on_resp);
    for (uint64_t k = 0; k < si; ++k)
        if (a[k] >= t->n_states) return false;
    for (uint64_t k = 0; k < sr; ++k)
        if (b[k] >= t->n_states) return false;
    return true;
}

}  // namespace

extern "C" int qsmd_gen_table_batch(const qsmd_gen_table_params* p, const void* model, uint64_t first,
                                    uint64_t n_hist, uint32_t ev_base, qsmd_hdr* hdr, qsmd_event* events,
                                    uint8_t* bug_out, int n_threads) {
    if (!p || !model || !hdr || !events) return QSMD_ERR_ARG;
    Model m{};
    if (p->model_id == QSMD_MODEL_TABLE) {
        const auto* t = static_cast<const qsmd_table_model*>(model);
        if (!model_ok<qsmd_table_model, uint8_t>(t, QSMD_TABLE_MAX_STATES, QSMD_TABLE_MAX_INV)) return QSMD_ERR_ARG;
        m = Model{t->n_states, t->n_inv, t->n_resp, t->init_state, 1u, false, t->on_inv, t->on_resp, t->post,
                  t->post_err};
    } else if (p->model_id == QSMD_MODEL_WTABLE) {
        const auto* t = static_cast<const qsmd_wtable_model*>(model);
        if (!model_ok<qsmd_wtable_model, uint16_t>(t, QSMD_WTABLE_MAX_STATES, QSMD_WTABLE_MAX_INV))
            return QSMD_ERR_ARG;
        m = Model{t->n_states, t->n_inv, t->n_resp, t->init_state, (t->n_resp + 31u) / 32u, true, t->on_inv,
                  t->on_resp, t->post, t->post_err};
    } else {
        return QSMD_ERR_ARG;
    }
    if (p->n_clients < 1 || p->n_clients > 32 || p->n_ops < 1 || 2 * p->n_ops > QSMD_MAX_EVENTS) return QSMD_ERR_ARG;
    if (p->lin_policy > 1 || p->pid_mode > 1) return QSMD_ERR_ARG;
    if (!(p->p_bug >= 0.0 && p->p_bug <= 1.0)) return QSMD_ERR_ARG;       // (NaN fails both)
    const uint32_t per = 2 * p->n_ops;
    if ((uint64_t)ev_base + n_hist * (uint64_t)per > 0xFFFFFFFFull || n_hist > 0xFFFFFFFFull) return QSMD_ERR_ARG;
    std::vector<uint32_t> weight(m.n_inv, 1u);
    if (p->inv_weight) std::copy(p->inv_weight, p->inv_weight + m.n_inv, weight.begin());
    uint64_t w_all = 0;
    for (uint32_t w : weight) w_all += w;
    if (w_all == 0 || w_all > 0xFFFFFFFFull) return QSMD_ERR_ARG;

    const Gen g{*p, m, weight.data(), (uint32_t)w_all};
    if (n_threads < 1) n_threads = 1;
    auto work = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            qsmd_hdr& h = hdr[i];
            std::memset(&h, 0, sizeof(h));
            h.ev_off = ev_base + (uint32_t)(i * per);
            h.n_ev = (uint16_t)per;
            h.n_pid = (uint8_t)(p->pid_mode == QSMD_GEN_PID_SHARED ? 1 : p->n_clients);
            h.model_id = (uint8_t)p->model_id;
            h.tag = (uint32_t)(first + i);
            g.one(first + i, events + i * per, bug_out ? bug_out + i : nullptr);
        }
    };
    if (n_threads == 1 || n_hist < 1024) { work(0, n_hist); return 0; }
    std::vector<std::thread> th;
    const uint64_t chunk = (n_hist + n_threads - 1) / n_threads;
    for (int t = 0; t < n_threads; ++t) {
        const uint64_t lo = t * chunk, hi = std::min<uint64_t>(n_hist, lo + chunk);
        if (lo >= hi) break;
        th.emplace_back(work, lo, hi);
    }
    for (auto& x : th) x.join();
    return 0;
}
