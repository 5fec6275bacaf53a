// Host side of loopy belief propagation (mibn_bp_batch, mibn_bp_mpe_batch, mibn_bp_evidence_batch): everything the call decides before its first HIP call, in plain C++17 - no
// HIP header, so that tools/bp_plan_sim.cpp runs it on a CPU (tests/test_bp_host.py) the way sampler_plan_sim runs sampler_plan.h.
// bp_layout is the ONE description of a request's message state: bp_kernel takes its pointers from it - into dynamic LDS or into the
// request's slab of the arena -, the plan takes the launch's LDS size and the slab size from it.
//
// The factor graph: one factor per variable v, its CPT, with the scope S_v = (parents.., v) as mibn_set_network received it.  Every CPT
// takes part.  Edge e = (f, k) joins factor f and variable u = S_f[k]; edges are numbered by ascending factor, then ascending scope
// position, so the edges of factor f are vars[f].edge_begin .. + scope_len.  Each edge owns card(u) cells at cell offset moff in every
// message array (mu of the previous step, mu of this step, nu).  N(u): the edges of variable u in ascending edge number.  lambda of
// variable u: card(u) cells at loff = sum of the cards below u, which is also where u's belief goes in a request's output row.
//
// The launch takes one of two forms:
//     MsgLds      the message arrays and lambda of a request in the LDS of its workgroup     bp_lds != 0 and bp_layout(..).total <= 160 KiB
//     MsgGlobal   the same arrays in a slab of the arena, one per request of the launch        otherwise
// Either way the CPTs, the records below and the request's evidence are read from global memory.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mibn.h"
#include "planner.h"
#include "sampler_plan.h"  // MIBN_HD, pack_vars, kSamplerLdsLimit

namespace mibn {

struct BpEdge {
    int32_t factor, pos, var, card;  // e = (factor, pos); var = S_factor[pos] and its cardinality
    int32_t moff;                    // first message cell
    int32_t table_off;               // the factor's CPT in the pool
    int32_t stride;                  // C-order stride of `pos` in that table
    int32_t loff;                    // first lambda cell of var
};
struct BpVar {
    int32_t card, loff;
    int32_t nb_begin, nb_len;        // N(v) in nbr / nbr_moff
    int32_t edge_begin, scope_len;   // the edges of factor v
    int32_t table_off, table_cells;  // its CPT
};

// ------------------------------------------------------------------------------------------------------------ the state of a request
// mu0[cells] | mu1[cells] | nu[cells] | lambda[lam_cells] f64 | red (byte offsets).  red: the workgroup's reduction slots - always in LDS;
// a slab has the room and leaves it unused.
constexpr int kBpMaxWaves = 4;
constexpr size_t kBpRedBytes = 64;  // kBpMaxWaves doubles (the waves' residual maxima) + as many ints (their zero-mass flags)
template <typename I>
struct BpLayout {
    I mu0, mu1, nu, lam, red, total;
};
template <typename I>
MIBN_HD inline BpLayout<I> bp_layout(I cells, I lam_cells) {
    BpLayout<I> L;
    L.mu0 = 0;
    L.mu1 = cells * 8;
    L.nu = 2 * cells * 8;
    L.lam = 3 * cells * 8;
    L.red = L.lam + lam_cells * 8;
    L.total = L.red + (I)kBpRedBytes;
    return L;
}

enum class BpForm { MsgLds, MsgGlobal };
inline const char *bp_form_name(BpForm f) { return f == BpForm::MsgLds ? "MsgLds" : "MsgGlobal"; }

// Threads of a workgroup: the work items of both phases are edges, so one lane per edge in whole waves, 64 .. 256.  A small network
// (Asia: 18 edges) gets one wave - its two barriers an iteration cost nothing and four of its workgroups share a CU's SIMDs -, anything
// above 192 edges the full 256.
inline int bp_threads(int64_t n_edges) { return (int)std::min<int64_t>(64 * kBpMaxWaves, std::max<int64_t>(64, (n_edges + 63) / 64 * 64)); }

struct BpPlan {
    std::vector<BpEdge> edges;
    std::vector<BpVar> vars;
    std::vector<int32_t> nbr, nbr_moff;  // flattened N(v): edge numbers, and the moff of each
    int32_t cells = 0, lam_cells = 0;
    BpLayout<size_t> lds{};
    size_t slab_bytes = 0;   // MsgGlobal: stride of a request's slab (16-byte multiple)
    double iter_bytes = 0;   // bytes of CPT cells one iteration of one request reads: 8 * sum over factors of scope_len * table cells
    BpForm form = BpForm::MsgLds;
    int threads = 64;
};

// max_iterations >= 1, 0 <= damping < 1, tol >= 0 (NaN fails every comparison)
inline int bp_check_args(int32_t max_iterations, double tol, double damping, std::string &err) {
    if (max_iterations < 1) { err = "bp: max_iterations must be at least 1"; return MIBN_E_ARG; }
    if (!(damping >= 0.0 && damping < 1.0)) { err = "bp: damping must be in [0, 1)"; return MIBN_E_ARG; }
    if (!(tol >= 0.0)) { err = "bp: tol must be a number >= 0"; return MIBN_E_ARG; }
    return MIBN_OK;
}

// lds_mode: the bp_lds option (0 forces MsgGlobal)
inline int bp_plan(const Network &net, int lds_mode, BpPlan &P, std::string &err) {
    const int n = net.n_vars;
    SamplerPack pack;
    size_t o_sv = 0, o_ss = 0, o_ch = 0;
    if (int rc = pack_vars(net, "bp", false, nullptr, pack, o_sv, o_ss, o_ch, err)) return rc;  // (cardinality above 255: MIBN_E_LIMIT)
    if (net.pool.size() > (size_t)INT32_MAX) { err = "bp: the CPTs have more than 2^31 cells"; return MIBN_E_LIMIT; }
    P.edges.clear();
    P.vars.assign((size_t)n, BpVar{});
    int64_t cells = 0, lam = 0;
    std::vector<std::vector<int32_t>> nb((size_t)n);
    for (int f = 0; f < n; ++f) {
        const GibbsVar &g = pack.vars[(size_t)f];
        BpVar &V = P.vars[(size_t)f];
        V.card = g.card;
        V.loff = (int32_t)lam;
        lam += g.card;
        V.edge_begin = (int32_t)P.edges.size();
        V.scope_len = g.scope_len;
        V.table_off = g.table_off;
        int64_t tc = 1;
        for (int k = 0; k < g.scope_len; ++k) tc *= net.card[(size_t)pack.words[o_sv + (size_t)g.scope_begin + (size_t)k]];
        V.table_cells = (int32_t)tc;  // (a part of the pool: below 2^31)
        P.iter_bytes += 8.0 * (double)g.scope_len * (double)tc;
        for (int k = 0; k < g.scope_len; ++k) {
            const int32_t u = pack.words[o_sv + (size_t)g.scope_begin + (size_t)k];
            if (cells > (int64_t)INT32_MAX - 255) { err = "bp: more than 2^31 message cells"; return MIBN_E_LIMIT; }
            BpEdge E;
            E.factor = f; E.pos = k; E.var = u; E.card = net.card[(size_t)u];
            E.moff = (int32_t)cells;
            E.table_off = g.table_off;
            E.stride = pack.words[o_ss + (size_t)g.scope_begin + (size_t)k];
            E.loff = 0;
            nb[(size_t)u].push_back((int32_t)P.edges.size());
            P.edges.push_back(E);
            cells += E.card;
        }
    }
    for (BpEdge &E : P.edges) E.loff = P.vars[(size_t)E.var].loff;
    P.nbr.clear();
    P.nbr_moff.clear();
    for (int v = 0; v < n; ++v) {
        P.vars[(size_t)v].nb_begin = (int32_t)P.nbr.size();
        P.vars[(size_t)v].nb_len = (int32_t)nb[(size_t)v].size();
        for (int32_t e : nb[(size_t)v]) { P.nbr.push_back(e); P.nbr_moff.push_back(P.edges[(size_t)e].moff); }
    }
    P.cells = (int32_t)cells;
    P.lam_cells = (int32_t)lam;
    P.lds = bp_layout<size_t>((size_t)cells, (size_t)lam);
    P.slab_bytes = lds_align16(P.lds.total);
    P.form = lds_mode != 0 && P.lds.total <= kSamplerLdsLimit ? BpForm::MsgLds : BpForm::MsgGlobal;
    P.threads = bp_threads((int64_t)P.edges.size());
    return MIBN_OK;
}

// Requests of one launch: at most `chunk`, and in the global form as many slabs as the budget holds.  0: one slab does not fit.
inline int64_t bp_launch_requests(BpForm form, size_t slab_bytes, int64_t chunk, double budget_bytes) {
    chunk = std::max<int64_t>(1, chunk);
    if (form == BpForm::MsgLds) return chunk;
    const double fit = std::floor(budget_bytes / (double)slab_bytes);
    return fit < 1.0 ? 0 : (int64_t)std::min((double)chunk, fit);
}
inline int64_t bp_launch_requests(const BpPlan &P, int64_t chunk, double budget_bytes) { return bp_launch_requests(P.form, P.slab_bytes, chunk, budget_bytes); }

// ------------------------------------------------------------------------------------- max-product with a decoder (mibn_bp_mpe_batch)
// The state of a request: the message arrays and lambda exactly as above, then what the decoder keeps -
//     term[n_vars] f64 | part[64] f64 | cur[n_vars] i32 | kept[n_vars] i32 | (pad to 8) | red
// term: the score terms of the assignment being scored; part: the 64 partial sums of the pinned score order; cur: the decode of this
// step; kept: the best candidate so far, which the polish then moves.  red: the reduction slots of bp_kernel, then as many again for
// the decoder's own reductions (zero flag, moves of a sweep) and the slot every lane reads the score from - always in LDS.
constexpr int kBpScoreLanes = 64;
constexpr size_t kBpMpeRedBytes = 2 * kBpRedBytes;
template <typename I>
struct BpMpeLayout {
    I mu0, mu1, nu, lam, term, part, cur, kept, red, total;
};
template <typename I>
MIBN_HD inline BpMpeLayout<I> bp_mpe_layout(I cells, I lam_cells, I n_vars) {
    const BpLayout<I> S = bp_layout<I>(cells, lam_cells);
    BpMpeLayout<I> L;
    L.mu0 = S.mu0;
    L.mu1 = S.mu1;
    L.nu = S.nu;
    L.lam = S.lam;
    L.term = S.red;
    L.part = L.term + n_vars * 8;
    L.cur = L.part + (I)kBpScoreLanes * 8;
    L.kept = L.cur + n_vars * 4;
    L.red = (L.kept + n_vars * 4 + 7) / 8 * 8;
    L.total = L.red + (I)kBpMpeRedBytes;
    return L;
}

// The colouring of the moral graph for the polish: u and v are adjacent when some CPT scope holds both.  Greedy - ascending v, the
// smallest colour no already-coloured neighbour has -, so a colour's members share no factor.  members: CSR by colour, ascending v.
struct BpColouring {
    std::vector<int32_t> colour, off, members;
    int32_t n_colours = 0;
};
inline void bp_colour(const BpPlan &P, BpColouring &C) {
    const size_t n = P.vars.size();
    C.colour.assign(n, -1);
    C.n_colours = 0;
    std::vector<char> used;
    for (size_t v = 0; v < n; ++v) {
        used.assign((size_t)C.n_colours + 1, 0);
        const BpVar &V = P.vars[v];
        for (int i = 0; i < V.nb_len; ++i) {  // the factors v is in, and everything in their scopes
            const BpVar &F = P.vars[(size_t)P.edges[(size_t)P.nbr[(size_t)(V.nb_begin + i)]].factor];
            for (int j = 0; j < F.scope_len; ++j) {
                const int32_t c = C.colour[(size_t)P.edges[(size_t)(F.edge_begin + j)].var];
                if (c >= 0) used[(size_t)c] = 1;
            }
        }
        int32_t c = 0;
        while (used[(size_t)c]) ++c;
        C.colour[v] = c;
        C.n_colours = std::max(C.n_colours, c + 1);
    }
    C.off.assign((size_t)C.n_colours + 1, 0);
    for (size_t v = 0; v < n; ++v) ++C.off[(size_t)C.colour[v] + 1];
    for (int32_t c = 0; c < C.n_colours; ++c) C.off[(size_t)c + 1] += C.off[(size_t)c];
    C.members.assign(n, 0);
    std::vector<int32_t> at(C.off.begin(), C.off.end() - 1);
    for (size_t v = 0; v < n; ++v) C.members[(size_t)at[(size_t)C.colour[v]]++] = (int32_t)v;
}

struct BpMpePlan {
    BpPlan bp;  // the records, threads and iter_bytes; its lds / slab_bytes / form are mibn_bp_batch's and unused here
    BpColouring col;
    BpMpeLayout<size_t> lds{};
    size_t slab_bytes = 0;
    BpForm form = BpForm::MsgLds;
};

// bp_check_args, and polish_sweeps >= 0
inline int bp_mpe_check_args(int32_t max_iterations, double tol, double damping, int32_t polish_sweeps, std::string &err) {
    if (int rc = bp_check_args(max_iterations, tol, damping, err)) return rc;
    if (polish_sweeps < 0) { err = "bp: polish_sweeps must be at least 0"; return MIBN_E_ARG; }
    return MIBN_OK;
}

// The same rule as bp_plan's on the larger state: in LDS when bp_lds != 0 and the whole of it fits 160 KiB.
inline int bp_mpe_plan(const Network &net, int lds_mode, BpMpePlan &M, std::string &err) {
    if (int rc = bp_plan(net, lds_mode, M.bp, err)) return rc;
    bp_colour(M.bp, M.col);
    M.lds = bp_mpe_layout<size_t>((size_t)M.bp.cells, (size_t)M.bp.lam_cells, (size_t)net.n_vars);
    M.slab_bytes = lds_align16(M.lds.total);
    M.form = lds_mode != 0 && M.lds.total <= kSamplerLdsLimit ? BpForm::MsgLds : BpForm::MsgGlobal;
    return MIBN_OK;
}

// ------------------------------------------------------------------ Bethe log Z and family beliefs (mibn_bp_evidence_batch)
// The state of a request: the message arrays and lambda exactly as above, then what the final phase keeps -
//     zf[n_vars] f64 | term[n_vars] f64 | part[64] f64 | red
// zf: the normaliser of every factor's belief, which the family-belief cells divide by; term: the Bethe term of every variable; part:
// the 64 partial sums of the pinned order (the score rule's).  red: the reduction slots of bp_kernel, then as many again for the
// final phase's own reduction - always in LDS.
constexpr size_t kBpEvRedBytes = 2 * kBpRedBytes;
template <typename I>
struct BpEvLayout {
    I mu0, mu1, nu, lam, zf, term, part, red, total;
};
template <typename I>
MIBN_HD inline BpEvLayout<I> bp_ev_layout(I cells, I lam_cells, I n_vars) {
    const BpLayout<I> S = bp_layout<I>(cells, lam_cells);
    BpEvLayout<I> L;
    L.mu0 = S.mu0;
    L.mu1 = S.mu1;
    L.nu = S.nu;
    L.lam = S.lam;
    L.zf = S.red;
    L.term = L.zf + n_vars * 8;
    L.part = L.term + n_vars * 8;
    L.red = L.part + (I)kBpScoreLanes * 8;
    L.total = L.red + (I)kBpEvRedBytes;
    return L;
}

struct BpEvPlan {
    BpPlan bp;  // the records, threads and iter_bytes; its lds / slab_bytes / form are mibn_bp_batch's and unused here
    BpEvLayout<size_t> lds{};
    size_t slab_bytes = 0;
    BpForm form = BpForm::MsgLds;
    std::vector<int32_t> foff;  // [n_vars + 1]: factor v's cells in a family-belief row - the tables back to back, not the pool's layout
    int32_t fcells = 0;         // cells of a family-belief row
};

// The same rule as bp_plan's on the larger state: in LDS when bp_lds != 0 and the whole of it fits 160 KiB.
inline int bp_ev_plan(const Network &net, int lds_mode, BpEvPlan &E, std::string &err) {
    if (int rc = bp_plan(net, lds_mode, E.bp, err)) return rc;
    E.lds = bp_ev_layout<size_t>((size_t)E.bp.cells, (size_t)E.bp.lam_cells, (size_t)net.n_vars);
    E.slab_bytes = lds_align16(E.lds.total);
    E.form = lds_mode != 0 && E.lds.total <= kSamplerLdsLimit ? BpForm::MsgLds : BpForm::MsgGlobal;
    E.foff.assign(E.bp.vars.size() + 1, 0);
    int64_t at = 0;  // (at most the pool: below 2^31)
    for (size_t v = 0; v < E.bp.vars.size(); ++v) {
        E.foff[v] = (int32_t)at;
        at += E.bp.vars[v].table_cells;
    }
    E.foff.back() = E.fcells = (int32_t)at;
    return MIBN_OK;
}

// n_acc must be the family-belief row's length; every weight a finite number >= 0.  `weight` may be null (all ones).
inline int bp_ev_check_acc(const BpEvPlan &E, bool has_acc, int64_t n_acc, const double *weight, int64_t B, std::string &err) {
    if (has_acc && n_acc != (int64_t)E.fcells) {
        err = "bp: n_acc is " + std::to_string(n_acc) + ", the family tables have " + std::to_string(E.fcells) + " cells";
        return MIBN_E_ARG;
    }
    for (int64_t b = 0; weight && b < B; ++b)
        if (!(weight[b] >= 0.0) || std::isinf(weight[b])) { err = "request " + std::to_string(b) + ": weight must be a finite number >= 0"; return MIBN_E_ARG; }
    return MIBN_OK;
}

// Requests of one launch: at most `chunk`, and as many as have, in the budget, a slab (MsgGlobal) plus a family-belief row
// (`rows`: the call returns family beliefs or accumulates them).  0: one request does not fit.
inline int64_t bp_ev_launch_requests(const BpEvPlan &E, bool rows, int64_t chunk, double budget_bytes) {
    chunk = std::max<int64_t>(1, chunk);
    const double per = (E.form == BpForm::MsgGlobal ? (double)E.slab_bytes : 0.0) + (rows ? 8.0 * (double)E.fcells : 0.0);
    if (per == 0.0) return chunk;
    const double fit = std::floor(budget_bytes / per);
    return fit < 1.0 ? 0 : (int64_t)std::min((double)chunk, fit);
}

}  // namespace mibn
