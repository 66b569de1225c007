// tgen.cpp -- seeded history generator for the table models
// (qsmd_gen_table_batch, include/qsmd_gen.h).
//
// gen.cpp's scheduler policy and RNG with the table as the implementation:
// requests are drawn among the invocations the current state accepts a
// response for, and an operation's response is drawn among the accepted ones
// at its linearisation point.  The header's comment is the definition; this
// file follows it line by line (the device kernel, csrc/tgen.hip, keeps the
// same stream in registers and LDS).
#include "tgen_stream.h"

namespace {

using qsmd_tgen::Rng;

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
    using State = uint32_t;
    using Sym = uint32_t;
    const Model& m;
    const uint32_t* weight;        // n_inv entries
    uint32_t w_all;                // the sum of all weights

    State init() const { return m.init_state; }
    uint32_t n_resp() const { return m.n_resp; }
    qsmd_event inv_event(uint8_t kp, Sym i) const { return qsmd_event{kp, (uint8_t)i, 0, 0, 0}; }

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
    const qsmd_tgen::Sched sc{p->n_clients, p->n_ops, p->prefix_ops, p->lin_policy, p->pid_mode, p->overlap,
                              p->p_bug, p->seed};
    if (!qsmd_tgen::sched_ok(sc, n_hist, ev_base)) return QSMD_ERR_ARG;
    std::vector<uint32_t> weight(m.n_inv, 1u);
    if (p->inv_weight) std::copy(p->inv_weight, p->inv_weight + m.n_inv, weight.begin());
    uint64_t w_all = 0;
    for (uint32_t w : weight) w_all += w;
    if (w_all == 0 || w_all > 0xFFFFFFFFull) return QSMD_ERR_ARG;

    const Gen g{m, weight.data(), (uint32_t)w_all};
    qsmd_tgen::gen_batch(sc, g, p->model_id, first, n_hist, ev_base, hdr, events, bug_out, n_threads);
    return 0;
}
