// Host side of mibn_best_dag (exact structure learning by dynamic programming over variable subsets) and of mibn_arc_posteriors
// (the same DP with the maximum replaced by a sum): the argument check, the pass schedule, the index functions and - as MIBN_HD
// inlines - the BODIES of the passes and levels.  The kernels of dag_kernel.hip.h / dag_post_kernel.hip.h and the CPU programs
// tools/dag_plan_sim.cpp / tools/dag_post_sim.cpp (tests/test_exact_host.py, tests/test_arc_posterior_host.py) call the same
// bodies: a kernel adds its lane-to-work mapping, its LDS arrays and its barrier, a CPU program runs them with one lane.  Plain
// C++17 - no HIP header.
//
// Phase A turns the table of child v - 2^(n-1) entries (score, parent mask), entry i = the candidate whose parent set, with bit v
// squeezed out, is exactly i - into its superset maximum: entry i = the best candidate with parents inside i.  That is one step
// per index bit b, entry[i | 1 << b] = better(entry[i | 1 << b], entry[i]), and the steps of different bits commute because
// `better` is the maximum of a TOTAL order (higher score, then the smaller mask): whatever order and grouping the bits are taken
// in, every entry ends as the maximum over the same set of candidates, and a maximum has one value.  So the schedule cannot
// change a bit of the result - which is what lets the device take the bits in tiles.
//
// A pass (b0, g, c) covers the g bits [b0, b0 + g).  A tile of the pass is 2^(g + c) entries of one child: 2^g runs of 2^c
// consecutive entries, the runs 2^b0 entries apart.  Local entry e of tile t lies at dag_gather(P, t, e); the pass's bits are the
// bits [c, c + g) of e.  The first pass has b0 = 0, c = 0: 2^g consecutive entries.  With tile_bits T and group_bits G:
//     first pass   g = min(T, n - 1)
//     then         g = min(G, bits left), c = min(b0, max(0, T - g))       (a tile holds 2^max(T, g) entries at most)
// The defaults T = 12, G = 6 give 4 096-entry tiles (48 KiB of LDS: three workgroups per CU) and runs of 2^6 entries - 512 bytes of
// scores, 256 of masks - in the later passes; n = 20 is three passes (12 + 6 + 1 bits), n = 24 three (12 + 6 + 5).
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mibn.h"

#if defined(__HIPCC__)
#define MIBN_HD __host__ __device__
#else
#define MIBN_HD
#endif
// First statement of a body whose sums must round where they are written: no contraction into FMAs.  (g++ has no such pragma:
// tools/dag_post_sim.cpp is built with -ffp-contract=off.)
#if defined(__clang__)
#define MIBN_FP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MIBN_FP_NO_CONTRACT
#endif

namespace mibn {

constexpr int kDagMaxTileBits = 12;  // the kernel's LDS arrays: 2^12 x (8 + 4) bytes
constexpr int kDagTileBits = 12;     // option dag_tile_bits
constexpr int kDagGroupBits = 6;     // option dag_group_bits
constexpr uint32_t kDagNoMask = 0xFFFFFFFFu;
constexpr int kDagNoSink = 255;

// C (a subset of the columns without v) -> the index of child v's table: bit v squeezed out
MIBN_HD inline uint32_t dag_squeeze(uint32_t C, int v) { return (C & ((1u << v) - 1u)) | ((C >> (v + 1)) << v); }
// the entry of child v for the subset `mask` (without v) in a child-major table of n children (64 bits: 2.0e8 entries at n = 24)
MIBN_HD inline int64_t dag_entry(int v, uint32_t mask, int32_t n) { return ((int64_t)v << (n - 1)) + dag_squeeze(mask, v); }

// the total order of phase A: is (sa, ma) better than (sb, mb)?  Higher score first; at equal score the smaller mask.
MIBN_HD inline bool dag_better(double sa, uint32_t ma, double sb, uint32_t mb) { return sa > sb || (sa == sb && ma < mb); }

struct DagPass {
    int32_t b0, g, c;
    MIBN_HD int tile_size() const { return 1 << (g + c); }  // entries of a tile
};

// local entry e of tile t -> index in the child's table
MIBN_HD inline int64_t dag_gather(const DagPass &P, int64_t t, int64_t e) {
    const int64_t r = e & ((int64_t(1) << P.c) - 1), j = e >> P.c;
    const int mid_bits = P.b0 - P.c;
    const int64_t mid = t & ((int64_t(1) << mid_bits) - 1), hi = t >> mid_bits;
    return r | (mid << P.c) | (j << P.b0) | (hi << (P.b0 + P.g));
}

// One tile of one pass, by `lanes` lanes of which the caller is `lane`: load the tile (dag_tile_load), then (dag_tile_run) run
// the pass's bits over it (size = P.tile_size(), taken once by whoever calls the two halves apart) - for each bit the entry pairs (e0, e1 = e0 | bit), a pair by one lane, a sync() before the first
// bit and after every bit - and store it.  kUp: combine into e1 (subset sums and maxima); else into e0 (superset sums).  A
// workgroup passes (threadIdx.x, its size, a barrier), a CPU (0, 1, DagNoSync).  Tile is a policy over the tile's storage and the
// tables behind it (DagMaxTile below; DagSumTile and the load-only DagGapTile further down):
//     load(e, i) / store(e, i)    local entry e <- / -> entry i of the child's table
//     combine(dst, src)           local entry dst <- dst (+) src
struct DagNoSync {
    MIBN_HD void operator()() const {}
};
template <class Tile>
MIBN_HD inline void dag_tile_load(const Tile &T, const DagPass &P, int size, int64_t t, int lane, int lanes) {
    for (int e = lane; e < size; e += lanes) T.load(e, dag_gather(P, t, e));
}
template <bool kUp, class Tile, class Sync>
MIBN_HD inline void dag_tile_run(const Tile &T, const DagPass &P, int size, int64_t t, int lane, int lanes, Sync sync) {
    sync();
    for (int b = P.c; b < P.c + P.g; ++b) {
        const int low = (1 << b) - 1;
        for (int p = lane; p < size / 2; p += lanes) {
            const int e0 = (p & low) | ((p & ~low) << 1), e1 = e0 | (1 << b);
            if constexpr (kUp) T.combine(e1, e0);
            else T.combine(e0, e1);
        }
        sync();
    }
    for (int e = lane; e < size; e += lanes) T.store(e, dag_gather(P, t, e));
}
template <bool kUp, class Tile, class Sync>
MIBN_HD inline void dag_tile_pass(const Tile &T, const DagPass &P, int64_t t, int lane, int lanes, Sync sync) {
    const int size = P.tile_size();
    dag_tile_load(T, P, size, t, lane, lanes);
    dag_tile_run<kUp>(T, P, size, t, lane, lanes, sync);
}

// mibn_best_dag's tile: (score, mask) entries as two arrays of 2^kDagMaxTileBits; combine = the better of the two (dag_better)
struct DagMaxTile {
    double *score;  // the tables; the child's entries from `base`
    uint32_t *mask;
    int64_t base;
    double *s_score;  // the tile
    uint32_t *s_mask;
    MIBN_HD void load(int e, int64_t i) const {
        const int64_t at = base + i;  // (one sum for both arrays: written apart, the base is folded into both pointers per workgroup)
        s_score[e] = score[at];
        s_mask[e] = mask[at];
    }
    MIBN_HD void store(int e, int64_t i) const {
        const int64_t at = base + i;
        score[at] = s_score[e];
        mask[at] = s_mask[e];
    }
    MIBN_HD void combine(int dst, int src) const {
        const double s = s_score[src];
        const uint32_t m = s_mask[src];
        if (dag_better(s, m, s_score[dst], s_mask[dst])) {
            s_score[dst] = s;
            s_mask[dst] = m;
        }
    }
};

// Phase B, one subset S: best[S] = max over the members v of S of best[S \ v] + bps_v(S \ v), the first v in ascending order at
// a tie; the empty set has 0 and no sink.  `score`: the table phase A left.
struct DagSink {
    double top;
    int who;
};
MIBN_HD inline DagSink dag_sink(uint32_t S, int32_t n, const double *score, const double *best) {
    DagSink r{S ? -HUGE_VAL : 0.0, kDagNoSink};
    for (uint32_t rest = S; rest; rest &= rest - 1) {
        const int v = __builtin_ctz(rest);
        const uint32_t C = S ^ (1u << v);
        const double term = best[C] + score[dag_entry(v, C, n)];
        if (term > r.top) {
            r.top = term;
            r.who = v;
        }
    }
    return r;
}

// The traceback: peel the sinks from V; parents_out[n], order_out[n] (roots first), *total_out = best[V].  No DAG from the
// candidates: every parents entry kDagNoMask, every order entry -1.
MIBN_HD inline void dag_traceback(const uint32_t *mask, const double *best, const uint8_t *sink, int32_t n, uint32_t *parents_out, int32_t *order_out,
                                  double *total_out) {
    uint32_t S = n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u;
    *total_out = best[S];
    if (sink[S] == kDagNoSink) {
        for (int v = 0; v < n; ++v) {
            parents_out[v] = kDagNoMask;
            order_out[v] = -1;
        }
        return;
    }
    for (int k = n - 1; k >= 0; --k) {
        const int v = sink[S];
        S ^= 1u << v;
        parents_out[v] = mask[dag_entry(v, S, n)];
        order_out[k] = v;
    }
}

struct DagPlan {
    int32_t n = 0;
    int64_t entries = 0;  // of one child: 2^(n - 1)
    std::vector<DagPass> passes;
    // workgroups of a pass: every child's tiles
    int64_t tiles_per_child(const DagPass &P) const { return entries >> (P.g + P.c); }
    int64_t grid(const DagPass &P) const { return (int64_t)n * tiles_per_child(P); }
};

inline int dag_clamp_bits(int64_t v) { return (int)(v < 1 ? 1 : v > kDagMaxTileBits ? kDagMaxTileBits : v); }

inline DagPlan dag_plan(int32_t n, int tile_bits, int group_bits) {
    DagPlan D;
    D.n = n;
    D.entries = int64_t(1) << (n - 1);
    const int T = dag_clamp_bits(tile_bits), G = dag_clamp_bits(group_bits), m = n - 1;
    for (int b0 = 0; b0 < m;) {
        DagPass P;
        P.b0 = b0;
        P.g = b0 == 0 ? (T < m ? T : m) : (G < m - b0 ? G : m - b0);
        const int room = T > P.g ? T - P.g : 0;
        P.c = b0 < room ? b0 : room;
        D.passes.push_back(P);
        b0 += P.g;
    }
    return D;
}

// what mibn_best_dag and mibn_arc_posteriors refuse before anything is launched (include/mibn.h has the contract); `who`: the
// call's name in the message ("best_dag", "arc_posteriors")
inline int dag_check(const std::string &who, int32_t n_vars, int64_t n_fam, const int32_t *child, const uint32_t *parents, const double *score, std::string &err) {
    if (n_vars < 1) { err = who + ": n_vars must be at least 1"; return MIBN_E_ARG; }
    if (n_vars > MIBN_BEST_DAG_MAX_VARS) {
        err = who + ": " + std::to_string(n_vars) + " variables (at most " + std::to_string(MIBN_BEST_DAG_MAX_VARS) + ": the tables double with every variable)";
        return MIBN_E_LIMIT;
    }
    const int64_t entries = int64_t(1) << (n_vars - 1);
    std::vector<uint64_t> seen((size_t)((n_vars * entries + 63) / 64), 0);
    for (int64_t f = 0; f < n_fam; ++f) {
        const std::string cand = who + ": candidate " + std::to_string(f);
        const int32_t v = child[f];
        if (v < 0 || v >= n_vars) { err = cand + ": child outside [0, n_vars)"; return MIBN_E_ARG; }
        if (n_vars < 32 && (parents[f] >> n_vars)) { err = cand + ": a parent bit at or above n_vars"; return MIBN_E_ARG; }
        if ((parents[f] >> v) & 1u) { err = cand + ": the child is its own parent"; return MIBN_E_ARG; }
        if (!std::isfinite(score[f])) { err = cand + ": its score is not finite"; return MIBN_E_ARG; }
        const int64_t at = dag_entry(v, parents[f], n_vars);
        if ((seen[(size_t)(at >> 6)] >> (at & 63)) & 1u) { err = cand + ": the same (child, parent set) is listed twice"; return MIBN_E_ARG; }
        seen[(size_t)(at >> 6)] |= uint64_t(1) << (at & 63);
    }
    return MIBN_OK;
}

// ---- mibn_arc_posteriors (dag_post_kernel.hip.h): the same tables and the same pass schedule with the maximum replaced by a sum
// in log space.  A sum of doubles has no total order behind it: its last bits DO depend on the order the index bits are taken in,
// so - unlike mibn_best_dag - the options dag_tile_bits / dag_group_bits are allowed to move the last bits of its results (within
// the bound of include/mibn.h); under fixed options a call is bit-for-bit repeatable.  (dag_plan takes the bits in ascending order
// under every tiling, so every entry goes through the same chain of operations and today's schedules agree bit for bit; a planner
// that reorders bits would not, and nothing may rely on it.)  What device, tools/dag_post_sim.cpp and the tests share:

// log(exp(a) + exp(b)), pinned: m + log1p(exp(-|a - b|)) with m = max(a, b); m itself when the other operand is -inf (or both
// are): a single term passes through bit for bit and no NaN can form.  Never called with +inf or NaN.
MIBN_HD inline double dag_logaddexp(double a, double b) {
    const double m = a > b ? a : b, o = a > b ? b : a;
    if (o == -HUGE_VAL) return m;
    return m + ::log1p(::exp(-::fabs(a - b)));
}

// index in child v's table -> the subset: bit v put back as 0 (the inverse of dag_squeeze)
MIBN_HD inline uint32_t dag_unsqueeze(uint32_t i, int v) { return (i & ((1u << v) - 1u)) | ((i >> v) << (v + 1)); }

// The level kernel gives lane k of level l the k-th subset of l members in colexicographic order - the combinatorial number
// system: S = {c_l > .. > c_1}, k = C(c_l, l) + .. + C(c_1, 1) - so that every lane of a wave has a subset of the level (of 64
// consecutive masks at most 20 share a popcount).  binom[c * kDagBinomStride + i] = C(c, i) for c, i in [0, 24]; at most
// C(24, 12) = 2 704 156.
constexpr int kDagBinomStride = 25;
inline std::vector<uint32_t> dag_binomials() {
    std::vector<uint32_t> binom((size_t)kDagBinomStride * kDagBinomStride);
    for (int c = 0; c < kDagBinomStride; ++c)
        for (int i = 0; i < kDagBinomStride; ++i)
            binom[c * kDagBinomStride + i] = i == 0 ? 1u : c == 0 ? 0u : binom[(c - 1) * kDagBinomStride + i - 1] + binom[(c - 1) * kDagBinomStride + i];
    return binom;
}
// k in [0, C(n, level)) -> the subset; n <= 24
MIBN_HD inline uint32_t dag_unrank(uint32_t k, int level, int n, const uint32_t *binom) {
    uint32_t S = 0;
    int c = n - 1;
    for (int i = level; i >= 1; --i) {
        while (binom[c * kDagBinomStride + i] > k) --c;  // (ends at c = i - 1 at the latest: C(i - 1, i) = 0)
        S |= 1u << c;
        k -= binom[c * kDagBinomStride + i];
        --c;
    }
    return S;
}

// Centring.  c_v = the maximum score among child v's candidates, 0 without one; the tables hold s' = s - c_v (one subtraction, the
// same wherever it is made).  log_evidence = L(V) + c_0 + c_1 + .. added one by one in ascending v.
inline void dag_centres(int32_t n, int64_t n_fam, const int32_t *child, const double *score, double *c) {
    std::vector<char> any((size_t)n, 0);
    for (int v = 0; v < n; ++v) c[v] = 0.0;
    for (int64_t f = 0; f < n_fam; ++f) {
        const int v = child[f];
        if (!any[(size_t)v] || score[f] > c[v]) c[v] = score[f];
        any[(size_t)v] = 1;
    }
}
MIBN_HD inline double dag_centred(double s, double c) { return s - c; }
inline double dag_log_evidence(double l_full, int32_t n, const double *c) {
    double e = l_full;
    for (int v = 0; v < n; ++v) e += c[v];
    return e;
}

// mibn_arc_posteriors' tile (dag_tile_pass): one array of 2^kDagMaxTileBits doubles over one child's table; combine = dag_logaddexp.
// The subset sum turns s' into alpha_v (kUp), the superset sum g_v into Gamma_v (not kUp).
struct DagSumTile {
    double *table;  // the child's entries from `base`
    int64_t base;
    double *s_val;  // the tile
    MIBN_HD void load(int e, int64_t i) const { s_val[e] = table[base + i]; }
    MIBN_HD void store(int e, int64_t i) const { table[base + i] = s_val[e]; }
    MIBN_HD void combine(int dst, int src) const {
        MIBN_FP_NO_CONTRACT
        s_val[dst] = dag_logaddexp(s_val[dst], s_val[src]);
    }
};
// What the FIRST pass of the superset sum loads its tile with (dag_tile_load; the pass goes on over a DagSumTile): nothing is read
// from the table, entry S of child v is formed as g_v(S) = L(S) + R(V \ S \ {v}) - g never exists in memory.
struct DagGapTile {
    double *s_val;  // the tile
    const double *L, *R;
    int v;
    uint32_t others;  // V \ {v}
    MIBN_HD DagGapTile(double *tile, const double *L_, const double *R_, int v_, int32_t n)
        : s_val(tile), L(L_), R(R_), v(v_), others(((1u << n) - 1u) ^ (1u << v_)) {}
    MIBN_HD void load(int e, int64_t i) const {
        MIBN_FP_NO_CONTRACT
        const uint32_t S = dag_unsqueeze((uint32_t)i, v);
        s_val[e] = L[S] + R[others ^ S];
    }
};

// L and R of one subset S, the terms of either sum in ascending v; the empty set has 0:
//     L(S) = (+) over v in S of L(S \ v) + alpha_v(S \ v)           R(S) = (+) over v in S of alpha_v(V \ S) + R(S \ v)
struct DagLR {
    double l, r;
};
MIBN_HD inline DagLR dag_level(uint32_t S, int32_t n, const double *alpha, const double *L, const double *R) {
    MIBN_FP_NO_CONTRACT
    const uint32_t outside = ((1u << n) - 1u) ^ S;  // (n <= 24)
    DagLR x{S ? -HUGE_VAL : 0.0, S ? -HUGE_VAL : 0.0};
    for (uint32_t rest = S; rest; rest &= rest - 1) {
        const int v = __builtin_ctz(rest);
        const uint32_t C = S ^ (1u << v);
        x.l = dag_logaddexp(x.l, L[C] + alpha[dag_entry(v, C, n)]);
        x.r = dag_logaddexp(x.r, alpha[dag_entry(v, outside, n)] + R[C]);
    }
    return x;
}

// log posterior of the candidate (v, pm) with score s: (s' + Gamma_v(pm)) - L(V); -inf when no structure exists (never -inf - -inf)
MIBN_HD inline double dag_log_post(int v, uint32_t pm, double s, double centre_v, const double *gamma, double whole, int32_t n) {
    MIBN_FP_NO_CONTRACT
    const double g = gamma[dag_entry(v, pm, n)];
    return whole == -HUGE_VAL ? whole : (dag_centred(s, centre_v) + g) - whole;
}

// The order of the arc sums, a function of the candidate list alone.  The list is cut into segments of kDagArcSegment consecutive
// candidates.  For the arc u -> v and segment j, lane t of kDagArcLanes adds exp(log_post[f]) over the segment's candidates
// f = first + t, first + t + kDagArcLanes, .. in ascending f, starting from 0.0 - a candidate of another child, or without u
// among its parents, adds +0.0, which changes no bit of a non-negative sum; the lanes' sums are folded in a tree, lane[t] +=
// lane[t + h] for h = kDagArcLanes / 2, .., 1; arc[u * n + v] = the segments' results added in ascending j, starting from 0.0.
constexpr int kDagArcLanes = 256;
constexpr int64_t kDagArcSegment = int64_t(1) << 16;
MIBN_HD inline int64_t dag_arc_segments(int64_t n_fam) { return n_fam > 0 ? (n_fam + kDagArcSegment - 1) / kDagArcSegment : 1; }

// the same order on a CPU (tools/dag_post_sim.cpp); arc: n * n, row = from
inline void dag_arc_reduce(int32_t n, int64_t n_fam, const int32_t *child, const uint32_t *parents, const double *log_post, double *arc) {
    std::vector<double> lane((size_t)n * (size_t)n * kDagArcLanes);
    for (int k = 0; k < n * n; ++k) arc[k] = 0.0;
    for (int64_t j = 0; j < dag_arc_segments(n_fam); ++j) {
        std::fill(lane.begin(), lane.end(), 0.0);
        const int64_t first = j * kDagArcSegment, last = first + kDagArcSegment < n_fam ? first + kDagArcSegment : n_fam;
        for (int64_t f = first; f < last; ++f) {
            const double p = ::exp(log_post[f]);
            for (int u = 0; u < n; ++u)
                if ((parents[f] >> u) & 1u) lane[((size_t)u * (size_t)n + (size_t)child[f]) * kDagArcLanes + (size_t)((f - first) % kDagArcLanes)] += p;
        }
        for (int k = 0; k < n * n; ++k) {
            double *s = &lane[(size_t)k * kDagArcLanes];
            for (int h = kDagArcLanes / 2; h >= 1; h /= 2)
                for (int t = 0; t < h; ++t) s[t] += s[t + h];
            arc[k] += s[0];
        }
    }
}

}  // namespace mibn
