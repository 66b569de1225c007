// ktgen.cpp -- seeded history generator for the keyed table models
// (qsmd_gen_ktable_batch, include/qsmd_gen.h "keyed-table-model generator").
//
// tgen.cpp's stream on the product of n_keys copies of one narrow component,
// kept factored: the state is a vector of component states, an invocation is
// a pair (key, component invocation), request() takes one draw over the pairs
// key-major, execute() moves one key.  The schedule, the RNG and the driver
// are tgen_stream.h's; the device kernel (csrc/ktgen.hip) keeps the same
// stream in registers and LDS.
#include "tgen_stream.h"

namespace {

using qsmd_tgen::Rng;

struct Pair {
    uint32_t k, i;
};

struct KGen {
    struct State {
        uint8_t s[QSMD_KTABLE_MAX_KEYS];
    };
    using Sym = Pair;
    const qsmd_table_model& c;
    uint32_t n_keys;
    const uint64_t* weight;        // [n_keys][n_inv]: key_weight[k] * inv_weight[i]
    uint32_t w_all;                // the sum of all of them

    State init() const {
        State v{};
        for (uint32_t k = 0; k < n_keys; ++k) v.s[k] = (uint8_t)c.init_state;
        return v;
    }
    uint32_t n_resp() const { return c.n_resp; }
    qsmd_event inv_event(uint8_t kp, Pair x) const { return qsmd_event{kp, (uint8_t)x.i, (uint8_t)x.k, 0, 0}; }

    // the component's acc(s, i)
    uint32_t acc(uint32_t s, uint32_t i) const {
        const size_t at = (size_t)s * c.n_inv + i;
        uint32_t x = c.post[at];
        if (c.post_err) x &= ~c.post_err[at];
        if (c.n_resp < 32u) x &= (1u << c.n_resp) - 1u;
        return x;
    }

    Pair request(Rng& r, const State& v) const {
        const uint32_t n = n_keys * c.n_inv;
        uint8_t en[QSMD_KTABLE_MAX_KEYS * QSMD_TABLE_MAX_INV];
        uint64_t W = 0;
        for (uint32_t k = 0, x = 0; k < n_keys; ++k)
            for (uint32_t i = 0; i < c.n_inv; ++i, ++x) {
                en[x] = weight[x] > 0 && acc(v.s[k], i) != 0;
                if (en[x]) W += weight[x];
            }
        if (W == 0) {
            for (uint32_t x = 0; x < n; ++x) en[x] = weight[x] > 0;
            W = w_all;
        }
        const uint32_t w = r.below((uint32_t)W);
        uint64_t run = 0;
        for (uint32_t x = 0; x < n; ++x) {
            if (!en[x]) continue;
            run += weight[x];
            if (run > w) return Pair{x / c.n_inv, x % c.n_inv};
        }
        return Pair{n_keys - 1, c.n_inv - 1};   // (not reached: run ends at W > w)
    }

    uint32_t execute(Rng& r, State& v, Pair x, uint8_t& flags) const {
        const uint32_t s = v.s[x.k], a = acc(s, x.i);
        uint32_t resp;
        if (a) {
            uint32_t k = r.below((uint32_t)__builtin_popcount(a));
            resp = 0;
            for (uint32_t b = 0; b < c.n_resp; ++b) {
                if (!((a >> b) & 1u)) continue;
                if (k-- == 0) { resp = b; break; }
            }
        } else {
            resp = r.below(c.n_resp);
            flags |= 2u;
        }
        v.s[x.k] = c.on_resp[(size_t)c.on_inv[(size_t)s * c.n_inv + x.i] * c.n_resp + resp];
        return resp;
    }
};

// what qsmd_ktable_set (csrc/ktable_host.h ktable_build) rejects
bool component_ok(const qsmd_table_model* m, uint32_t n_keys) {
    if (n_keys == 0 || n_keys > QSMD_KTABLE_MAX_KEYS) return false;
    if (!m || !m->on_inv || !m->on_resp || !m->post) return false;
    if (m->n_states == 0 || m->n_states > QSMD_TABLE_MAX_STATES || m->n_inv == 0 || m->n_inv > QSMD_TABLE_MAX_INV ||
        m->n_resp == 0 || m->n_resp > QSMD_TABLE_MAX_RESP || m->init_state >= m->n_states)
        return false;
    const uint32_t si = m->n_states * m->n_inv, sr = m->n_states * m->n_resp;
    for (uint32_t k = 0; k < si; ++k)
        if (m->on_inv[k] >= m->n_states) return false;
    for (uint32_t k = 0; k < sr; ++k)
        if (m->on_resp[k] >= m->n_states) return false;
    return true;
}

}  // namespace

extern "C" int qsmd_gen_ktable_batch(const qsmd_gen_ktable_params* p, const qsmd_table_model* component,
                                     uint64_t first, uint64_t n_hist, uint32_t ev_base, qsmd_hdr* hdr,
                                     qsmd_event* events, uint8_t* bug_out, int n_threads) {
    if (!p || !hdr || !events) return QSMD_ERR_ARG;
    if (!component_ok(component, p->n_keys)) return QSMD_ERR_ARG;
    const qsmd_tgen::Sched sc{p->n_clients, p->n_ops, p->prefix_ops, p->lin_policy, p->pid_mode, p->overlap,
                              p->p_bug, p->seed};
    if (!qsmd_tgen::sched_ok(sc, n_hist, ev_base)) return QSMD_ERR_ARG;
    const uint32_t n_inv = component->n_inv;
    std::vector<uint64_t> weight((size_t)p->n_keys * n_inv);
    uint64_t w_all = 0;       // at most 256 products, each held to 2^32 - 1
    for (uint32_t k = 0; k < p->n_keys; ++k)
        for (uint32_t i = 0; i < n_inv; ++i) {
            const uint64_t w = (uint64_t)(p->key_weight ? p->key_weight[k] : 1u) *
                               (uint64_t)(p->inv_weight ? p->inv_weight[i] : 1u);
            if (w > 0xFFFFFFFFull) return QSMD_ERR_ARG;
            weight[(size_t)k * n_inv + i] = w;
            w_all += w;
        }
    if (w_all == 0 || w_all > 0xFFFFFFFFull) return QSMD_ERR_ARG;

    const KGen g{*component, p->n_keys, weight.data(), (uint32_t)w_all};
    qsmd_tgen::gen_batch(sc, g, QSMD_MODEL_KTABLE, first, n_hist, ev_base, hdr, events, bug_out, n_threads);
    return 0;
}
