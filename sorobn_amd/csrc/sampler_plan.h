// Host side of the sampling family (mibn_gibbs, mibn_gibbs_shard, mibn_gibbs_conditional, mibn_sample, mibn_sample_probe,
// mibn_sampling_query): everything gibbs_run and sample_run decide before their first HIP call, in plain C++17 - no HIP header, so
// that tools/sampler_plan_sim.cpp runs it on a CPU (tests/test_sampler_plan_host.py) the way prog_sim runs the planner.  The two
// layout functions are the ONE description of the kernels' dynamic LDS: gibbs_kernel, gibbs_kernel8 and sample_kernel take their
// pointers from them, the plans take the launch's size from them.
//
// The Gibbs launch takes one of six forms (GibbsForm; each with a drawing and a COND instantiation).  With
//     waves_ok = (n_chains + 63) / 64 <= 512        - at most two rounds of one-wave workgroups over the 256 CUs
//     fits(x)  = gibbs_layout(...).total with x in LDS <= 160 KiB
// the rules are, in this order:
//     tables in LDS    gibbs_lds != 0, waves_ok, fits(state + histogram + every CPT)
//     FAST records     tables in LDS, and every variable of the cycle has at most 8 states, at most 4 factors (its CPT and its
//                      children's) and at most two other variables in each of them, and fits(.. + the 1.0 cell + 28 words per
//                      cycle position)
//     8 lanes a chain  FAST, gibbs_lds == 1 and (n_chains + 7) / 8 <= 512          (gibbs_lds == 2: never)
//     programs in LDS  FAST, or: gibbs_lds != 0, waves_ok, fits(.. + update programs + their offsets + the cycle)
//  => Fast8 | Fast | PoolProgLds | PoolLds (the programs do not fit beside the tables) | ProgLds (the tables do not fit) | L2.
// State + histogram above 150 KiB is MIBN_E_LIMIT whatever the form.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mibn.h"
#include "planner.h"

#if defined(__HIPCC__)
#define MIBN_HD __host__ __device__
#else
#define MIBN_HD
#endif

namespace mibn {

struct GibbsVar {
    int32_t card, table_off, scope_begin, scope_len, child_begin, child_len, is_evidence, ev_code;
};

constexpr int kFastWords = 28;  // words of one cycle position's update record in the FAST format (gibbs_kernel)
constexpr size_t kSamplerStateLimit = 150 * 1024;  // chain state + histogram
constexpr size_t kSamplerLdsLimit = 160 * 1024;    // the LDS of a CU
// the largest histogram any launch holds (4 bytes a cell below kSamplerStateLimit); a cell product stops growing above it
constexpr int64_t kMaxHistCells = (int64_t)kSamplerStateLimit / 4;

// (I: the kernels compute their offsets in int, as wide as their arguments; the plans in size_t, where a table too large for any
// launch must not wrap before it is refused)
template <typename I>
MIBN_HD inline I lds_align16(I x) { return (x + 15) & ~I(15); }

// ------------------------------------------------------------------------------------------------------------ LDS layouts
// gibbs_kernel / gibbs_kernel8:  state[n_vars * 64] | hist[hist_cells] u32 | pool[pool_cells] f64 | programs i32
// (byte offsets; the state starts at 0).  pool_cells = 0: the tables stay in global memory; prog_words = 0: the programs do.
// FAST: one more cell behind the tables (the 1.0 of an unused factor slot), then the records, 16-byte aligned for their
// four-word reads.  Generic programs follow the tables directly (4-byte reads); `total` rounds their start up all the same.
template <typename I>
struct GibbsLayout {
    I hist, pool, prog, total;
};
template <typename I>
MIBN_HD inline GibbsLayout<I> gibbs_layout(I n_vars, I hist_cells, I pool_cells, bool fast, I prog_words) {
    GibbsLayout<I> L;
    L.hist = lds_align16(n_vars * 64);
    L.pool = lds_align16(L.hist + hist_cells * 4);
    if (fast) {
        L.prog = L.pool + lds_align16((pool_cells + 1) * 8);
        L.total = L.prog + prog_words * 4;
    } else {
        L.prog = L.pool + pool_cells * 8;
        L.total = prog_words ? lds_align16(L.prog) + prog_words * 4 : pool_cells ? L.prog : L.hist + hist_cells * 4;
    }
    return L;
}

// sample_kernel:  state[n_vars * 64] | hsum[hist_cells] f64 | hcnt[hist_cells] u32
template <typename I>
struct SampleLayout {
    I hsum, hcnt, total;
};
template <typename I>
MIBN_HD inline SampleLayout<I> sample_layout(I n_vars, I hist_cells) {
    SampleLayout<I> L;
    L.hsum = lds_align16(n_vars * 64);
    L.hcnt = L.hsum + hist_cells * 8;
    L.total = L.hcnt + hist_cells * 4;
    return L;
}

// ---------------------------------------------------------------------------------------------------- the shared pieces
// Everything a launch reads besides the CPTs: the variables and ONE int32 pack (put() returns a part's word offset).
struct SamplerPack {
    std::vector<GibbsVar> vars;
    std::vector<int32_t> words;
    size_t put(const int32_t *a, size_t n) {
        const size_t o = words.size();
        words.insert(words.end(), a, a + n);
        return o;
    }
    size_t put(const std::vector<int32_t> &a) { return put(a.data(), a.size()); }
};

// vars[v] and the flattened CPT scopes; `ch` (Gibbs): the children lists as well.  who: "gibbs" / "sampling".  topological
// (forward sampling walks the variables in id order): every parent must have a smaller id (true for BayesNet.nodes).
inline int pack_vars(const Network &net, const char *who, bool topological, std::vector<std::vector<int32_t>> *ch, SamplerPack &P,
                     size_t &o_sv, size_t &o_ss, size_t &o_ch, std::string &err) {
    const int n = net.n_vars;
    std::vector<int32_t> scope_var, scope_stride, children;
    if (ch) {
        ch->assign(n, {});
        for (int v = 0; v < n; ++v)
            for (size_t k = 0; k + 1 < net.scope[v].size(); ++k) (*ch)[net.scope[v][k]].push_back(v);
    }
    P.vars.assign(n, GibbsVar{});
    for (int v = 0; v < n; ++v) {
        if (net.card[v] > 255) { err = std::string(who) + ": cardinality above 255"; return MIBN_E_LIMIT; }
        for (size_t k = 0; topological && k + 1 < net.scope[v].size(); ++k)
            if (net.scope[v][k] >= v) { err = std::string(who) + ": variable ids are not in topological order"; return MIBN_E_ARG; }
        GibbsVar &g = P.vars[v];
        g.card = net.card[v];
        g.table_off = (int32_t)net.pool_off[v];
        g.scope_begin = (int32_t)scope_var.size();
        g.scope_len = (int32_t)net.scope[v].size();
        for (size_t k = 0; k < net.scope[v].size(); ++k) {
            scope_var.push_back(net.scope[v][k]);
            scope_stride.push_back((int32_t)net.cstride[v][k]);
        }
        if (ch) {
            g.child_begin = (int32_t)children.size();
            g.child_len = (int32_t)(*ch)[v].size();
            children.insert(children.end(), (*ch)[v].begin(), (*ch)[v].end());
        }
    }
    o_sv = P.put(scope_var);
    o_ss = P.put(scope_stride);
    o_ch = P.put(children);
    return MIBN_OK;
}

// (variable, code) pairs forced to a value.  what: "evidence" / "clamped".
inline int apply_clamps(const Network &net, const char *who, const char *what, int32_t n, const int32_t *ids, const int32_t *codes,
                      std::vector<GibbsVar> &vars, std::string &err) {
    for (int i = 0; i < n; ++i) {
        const int v = ids[i];
        if (v < 0 || v >= net.n_vars) { err = std::string(who) + ": unknown " + what + " variable"; return MIBN_E_ARG; }
        if (codes[i] < 0 || codes[i] >= net.card[v]) { err = std::string(who) + ": " + what + " label outside the domain"; return MIBN_E_ARG; }
        vars[v].is_evidence = 1;
        vars[v].ev_code = codes[i];
    }
    return MIBN_OK;
}

// C-order strides of the joint query histogram -> its cells.  The product stops at the first value above kMaxHistCells (at most
// 255 times it: no overflow however long the query), which every caller's "too large" check refuses.  false: an unknown id.
inline bool query_cells(const Network &net, int32_t n_q, const int32_t *q_vars, std::vector<int32_t> &qstride, int64_t &cells) {
    qstride.assign((size_t)std::max(0, n_q), 0);
    cells = 1;
    for (int i = n_q - 1; i >= 0; --i) {
        if (q_vars[i] < 0 || q_vars[i] >= net.n_vars) return false;
        if (cells > kMaxHistCells) continue;
        qstride[i] = (int32_t)cells;
        cells *= net.card[q_vars[i]];
    }
    return true;
}

constexpr const char *kGibbsTooLarge = "gibbs: network/query too large for the LDS-resident chain state";
constexpr const char *kSamplingTooLarge = "sampling: network/query too large for the LDS-resident state";

// The all-zero histogram of a call that launches nothing (an empty Gibbs shard, a rejection event nobody can draw).
inline int zero_histogram(const Network &net, int32_t n_q, const int32_t *q_vars, const char *too_large, int64_t *counts, std::string &err) {
    std::vector<int32_t> qstride;
    int64_t cells;
    if (!query_cells(net, n_q, q_vars, qstride, cells)) { err = "unknown query variable"; return MIBN_E_ARG; }
    if (cells > kMaxHistCells) { err = too_large; return MIBN_E_LIMIT; }
    std::fill(counts, counts + cells, (int64_t)0);
    return MIBN_OK;
}

// ------------------------------------------------------------------------------------------------------------------ Gibbs
enum class GibbsForm { L2, PoolLds, ProgLds, PoolProgLds, Fast, Fast8 };
constexpr int kGibbsForms = 6;
inline const char *gibbs_form_name(GibbsForm f) {
    static const char *const names[kGibbsForms] = {"L2", "PoolLds", "ProgLds", "PoolProgLds", "Fast", "Fast8"};
    return names[(int)f];
}

struct GibbsPlan {
    SamplerPack pack;
    size_t o_sv = 0, o_ss = 0, o_ch = 0, o_cy = 0, o_q = 0, o_qs = 0, o_up = 0, o_uo = 0;  // word offsets into pack.words
    int32_t n_cycle = 0, hist_cells = 0, pool_cells = 0;
    int32_t uprog_words = 0;  // words of the update programs alone (FAST: the records)
    int32_t prog_words = 0;   // words copied to LDS: programs + their offsets + the cycle (FAST: the records); 0: none
    int32_t cond_pos = 0;
    GibbsForm form = GibbsForm::L2;
    GibbsLayout<size_t> lds{};
    unsigned blocks = 0;  // of 64 lanes: 64 chains, Fast8: 8 chains
};

// lds_mode (the gibbs_lds option): 0 tables in L2, 1 LDS, 2 LDS without the 8-lane form.  cond_var >= 0 (mibn_gibbs_conditional):
// the cycle position of that variable in cond_pos.  cycle_in: the caller's update order or null (ascending ids; the reference
// cycles through sorted(nodes - event), bayes_net.py:697,718).
inline int gibbs_plan(const Network &net, int lds_mode, int32_t n_q, const int32_t *q_vars, int32_t n_e, const int32_t *e_vars,
                      const int32_t *e_codes, const int32_t *cycle_in, int64_t n_chains, int32_t cond_var, GibbsPlan &G, std::string &err) {
    const int n = net.n_vars;
    SamplerPack &P = G.pack;
    std::vector<std::vector<int32_t>> ch;
    if (int rc = pack_vars(net, "gibbs", false, &ch, P, G.o_sv, G.o_ss, G.o_ch, err)) return rc;
    if (int rc = apply_clamps(net, "gibbs", "evidence", n_e, e_vars, e_codes, P.vars, err)) return rc;
    std::vector<int32_t> cycle;
    if (cycle_in) {
        int n_free = 0;
        for (int v = 0; v < n; ++v) n_free += !P.vars[v].is_evidence;
        std::vector<char> seen(n, 0);
        for (int i = 0; i < n_free; ++i) {
            const int v = cycle_in[i];
            if (v < 0 || v >= n || P.vars[v].is_evidence || seen[v]) { err = "gibbs: cycle must list every non-evidence variable once"; return MIBN_E_ARG; }
            seen[v] = 1;
            cycle.push_back(v);
        }
    } else {
        for (int v = 0; v < n; ++v)
            if (!P.vars[v].is_evidence) cycle.push_back(v);
    }
    if (cycle.empty()) { err = "gibbs: every variable is evidence"; return MIBN_E_ARG; }
    G.cond_pos = 0;
    if (cond_var >= 0) {
        G.cond_pos = -1;
        for (size_t i = 0; i < cycle.size(); ++i)
            if (cycle[i] == cond_var) G.cond_pos = (int)i;
        if (G.cond_pos < 0) { err = "gibbs conditional: the variable is evidence or unknown"; return MIBN_E_ARG; }
    }
    // update programs, one per cycle position: card, n_factors, {table_off, stride of v, n_other, {var, stride}*}*
    std::vector<int32_t> uprog, uprog_off;
    for (int v : cycle) {
        uprog_off.push_back((int32_t)uprog.size());
        uprog.push_back(net.card[v]);
        uprog.push_back(1 + (int32_t)ch[v].size());
        auto factor = [&](int c) {  // CPT of c as a function of v's value
            int32_t sv = 0;
            std::vector<int32_t> others;
            for (size_t k = 0; k < net.scope[c].size(); ++k) {
                const int u = net.scope[c][k];
                if (u == v) sv = (int32_t)net.cstride[c][k];
                else { others.push_back(u); others.push_back((int32_t)net.cstride[c][k]); }
            }
            uprog.push_back((int32_t)net.pool_off[c]);
            uprog.push_back(sv);
            uprog.push_back((int32_t)(others.size() / 2));
            uprog.insert(uprog.end(), others.begin(), others.end());
        };
        factor(v);
        for (int c : ch[v]) factor(c);
    }
    std::vector<int32_t> qstride;
    int64_t cells;
    if (!query_cells(net, n_q, q_vars, qstride, cells)) { err = "gibbs: unknown query variable"; return MIBN_E_ARG; }
    if (cells > kMaxHistCells || gibbs_layout<size_t>(n, cells, 0, false, 0).total > kSamplerStateLimit) { err = kGibbsTooLarge; return MIBN_E_LIMIT; }
    const size_t pool_cells = net.pool.size();
    // (eight chains a workgroup: (n_chains + 7) / 8 <= 512 means at most 4 096 chains, so waves_ok holds wherever want8 does)
    const bool want8 = lds_mode == 1 && (n_chains + 7) / 8 <= 512;
    const bool waves_ok = (n_chains + 63) / 64 <= 512;
    const bool pool_lds = lds_mode != 0 && waves_ok && gibbs_layout<size_t>(n, cells, pool_cells, false, 0).total <= kSamplerLdsLimit;
    // fixed-size records: [v, card, n_factors, is a query variable, then four of (table base, stride of v, other variable 0, its
    // stride, other variable 1, its stride)]; an unused slot points at the 1.0 behind the tables with all strides 0
    bool fast = pool_lds;
    std::vector<int32_t> fprog;
    for (size_t ci = 0; ci < cycle.size() && fast; ++ci) {
        const int v = cycle[ci];
        if (net.card[v] > 8 || 1 + ch[v].size() > 4) { fast = false; break; }
        int32_t is_query = 0;
        for (int i = 0; i < n_q; ++i) is_query |= q_vars[i] == v;
        const int32_t head[4] = {v, net.card[v], 1 + (int32_t)ch[v].size(), is_query};
        fprog.insert(fprog.end(), head, head + 4);
        int slots = 0;
        auto record = [&](int c) {
            int32_t rec[6] = {(int32_t)net.pool_off[c], 0, 0, 0, 0, 0};
            int n_other = 0;
            for (size_t k = 0; k < net.scope[c].size(); ++k) {
                const int u = net.scope[c][k];
                if (u == v) rec[1] = (int32_t)net.cstride[c][k];
                else if (n_other < 2) { rec[2 + 2 * n_other] = u; rec[3 + 2 * n_other] = (int32_t)net.cstride[c][k]; ++n_other; }
                else fast = false;
            }
            fprog.insert(fprog.end(), rec, rec + 6);
            ++slots;
        };
        record(v);
        for (int c : ch[v]) record(c);
        for (; slots < 4; ++slots) {
            const int32_t rec[6] = {(int32_t)pool_cells, 0, 0, 0, 0, 0};
            fprog.insert(fprog.end(), rec, rec + 6);
        }
    }
    if (fast && gibbs_layout<size_t>(n, cells, pool_cells, true, fprog.size()).total > kSamplerLdsLimit) fast = false;
    if (fast) uprog = fprog;
    const size_t prog_words = fast ? uprog.size() : uprog.size() + 2 * cycle.size();
    const bool prog_lds = fast || (lds_mode != 0 && waves_ok &&
                                   gibbs_layout<size_t>(n, cells, pool_lds ? pool_cells : 0, false, prog_words).total <= kSamplerLdsLimit);
    G.form = fast ? (want8 ? GibbsForm::Fast8 : GibbsForm::Fast)
                  : pool_lds ? (prog_lds ? GibbsForm::PoolProgLds : GibbsForm::PoolLds) : (prog_lds ? GibbsForm::ProgLds : GibbsForm::L2);
    G.lds = gibbs_layout<size_t>(n, cells, pool_lds ? pool_cells : 0, fast, prog_lds ? prog_words : 0);
    G.blocks = G.form == GibbsForm::Fast8 ? (unsigned)((n_chains + 7) / 8) : (unsigned)((n_chains + 63) / 64);
    G.n_cycle = (int32_t)cycle.size();
    G.hist_cells = (int32_t)cells;
    G.pool_cells = (int32_t)pool_cells;
    G.uprog_words = (int32_t)uprog.size();
    G.prog_words = prog_lds ? (int32_t)prog_words : 0;
    G.o_cy = P.put(cycle);
    G.o_q = P.put(q_vars, (size_t)n_q);
    G.o_qs = P.put(qstride);
    G.o_up = P.put(uprog);
    G.o_uo = P.put(uprog_off);
    return MIBN_OK;
}

// ------------------------------------------------------------------------------------------------------- forward sampling
constexpr int kSampleMode = 0, kRejectionMode = 1, kLikelihoodMode = 2;
// PROBE (mibn_sample_probe, parity hook): the walk of the kernel over GIVEN joint states - same offsets, same row sums, same
// running sums a draw compares its uniform with, same likelihood product - written out instead of drawn from / histogrammed
constexpr int kProbeMode = 3;

struct SamplePlan {
    SamplerPack pack;
    size_t o_sv = 0, o_ss = 0, o_q = 0, o_qs = 0, o_ev = 0, o_ec = 0;
    int64_t cells = 1;       // of the query histogram (1 without a query)
    int32_t hist_cells = 0;  // of the launch: SAMPLE and PROBE keep no histogram
    SampleLayout<size_t> lds{};
    unsigned blocks = 1;
    // the output buffer: SAMPLE states[n_samples][n_vars]; PROBE the given states (padded to 8 bytes) | likelihoods | running sums;
    // REJECTION / LIKELIHOOD wsum[cells] f64 | counts[cells] u64
    size_t probe_states = 0, out_bytes = 0;
};

// clamp_*: variables forced to a value (sample's `init`, likelihood weighting's event); ev_*: the event rejection sampling
// filters on.
inline int sample_plan(const Network &net, int mode, int32_t n_q, const int32_t *q_vars, int32_t n_clamp, const int32_t *clamp_vars,
                       const int32_t *clamp_codes, int32_t n_ev, const int32_t *ev_vars, const int32_t *ev_codes, int64_t n_samples,
                       int32_t cdf_stride, SamplePlan &S, std::string &err) {
    const size_t n = (size_t)net.n_vars;
    SamplerPack &P = S.pack;
    size_t o_ch;
    if (int rc = pack_vars(net, "sampling", true, nullptr, P, S.o_sv, S.o_ss, o_ch, err)) return rc;
    if (int rc = apply_clamps(net, "sampling", "clamped", n_clamp, clamp_vars, clamp_codes, P.vars, err)) return rc;
    std::vector<int32_t> qstride;
    if (!query_cells(net, n_q, q_vars, qstride, S.cells)) { err = "sampling: unknown query variable"; return MIBN_E_ARG; }
    if (S.cells > kMaxHistCells || sample_layout<size_t>(n, S.cells).total > kSamplerStateLimit) { err = kSamplingTooLarge; return MIBN_E_LIMIT; }
    S.o_q = P.put(q_vars, (size_t)n_q);
    S.o_qs = P.put(qstride);
    S.o_ev = P.put(ev_vars, (size_t)n_ev);
    S.o_ec = P.put(ev_codes, (size_t)n_ev);
    S.hist_cells = (mode == kSampleMode || mode == kProbeMode) ? 0 : (int32_t)S.cells;
    S.lds = sample_layout<size_t>(n, S.hist_cells);
    S.blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_samples + 63) / 64, 256 * 16));
    S.probe_states = ((size_t)n_samples * n + 7) & ~size_t(7);
    S.out_bytes = mode == kSampleMode ? (size_t)n_samples * n
                  : mode == kProbeMode ? S.probe_states + (size_t)n_samples * 8 * (1 + n * (size_t)cdf_stride) : (size_t)S.cells * 16;
    return MIBN_OK;
}

}  // namespace mibn
