// Host side of mibn_best_dag (exact structure learning by dynamic programming over variable subsets): the argument check, the
// pass schedule of phase A and the index functions the kernels of dag_kernel.hip.h share with it, in plain C++17 - no HIP header,
// so that tools/dag_plan_sim.cpp executes the same schedule, tile by tile, on a CPU (tests/test_exact_host.py).
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

namespace mibn {

constexpr int kDagMaxTileBits = 12;  // the kernel's LDS arrays: 2^12 x (8 + 4) bytes
constexpr int kDagTileBits = 12;     // option dag_tile_bits
constexpr int kDagGroupBits = 6;     // option dag_group_bits
constexpr uint32_t kDagNoMask = 0xFFFFFFFFu;
constexpr int kDagNoSink = 255;

// C (a subset of the columns without v) -> the index of child v's table: bit v squeezed out
MIBN_HD inline uint32_t dag_squeeze(uint32_t C, int v) { return (C & ((1u << v) - 1u)) | ((C >> (v + 1)) << v); }

// the total order of phase A: is (sa, ma) better than (sb, mb)?  Higher score first; at equal score the smaller mask.
MIBN_HD inline bool dag_better(double sa, uint32_t ma, double sb, uint32_t mb) { return sa > sb || (sa == sb && ma < mb); }

struct DagPass {
    int32_t b0, g, c;
    MIBN_HD int64_t tile_entries() const { return int64_t(1) << (g + c); }
};

// local entry e of tile t -> index in the child's table
MIBN_HD inline int64_t dag_gather(const DagPass &P, int64_t t, int64_t e) {
    const int64_t r = e & ((int64_t(1) << P.c) - 1), j = e >> P.c;
    const int mid_bits = P.b0 - P.c;
    const int64_t mid = t & ((int64_t(1) << mid_bits) - 1), hi = t >> mid_bits;
    return r | (mid << P.c) | (j << P.b0) | (hi << (P.b0 + P.g));
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

// what mibn_best_dag refuses before anything is launched (include/mibn.h has the contract)
inline int dag_check(int32_t n_vars, int64_t n_fam, const int32_t *child, const uint32_t *parents, const double *score, std::string &err) {
    if (n_vars < 1) { err = "best_dag: n_vars must be at least 1"; return MIBN_E_ARG; }
    if (n_vars > MIBN_BEST_DAG_MAX_VARS) {
        err = "best_dag: " + std::to_string(n_vars) + " variables (at most " + std::to_string(MIBN_BEST_DAG_MAX_VARS) + ": the tables double with every variable)";
        return MIBN_E_LIMIT;
    }
    const int64_t entries = int64_t(1) << (n_vars - 1);
    std::vector<uint64_t> seen((size_t)((n_vars * entries + 63) / 64), 0);
    for (int64_t f = 0; f < n_fam; ++f) {
        const std::string who = "best_dag: candidate " + std::to_string(f);
        const int32_t v = child[f];
        if (v < 0 || v >= n_vars) { err = who + ": child outside [0, n_vars)"; return MIBN_E_ARG; }
        if (n_vars < 32 && (parents[f] >> n_vars)) { err = who + ": a parent bit at or above n_vars"; return MIBN_E_ARG; }
        if ((parents[f] >> v) & 1u) { err = who + ": the child is its own parent"; return MIBN_E_ARG; }
        if (!std::isfinite(score[f])) { err = who + ": its score is not finite"; return MIBN_E_ARG; }
        const int64_t at = (int64_t)v * entries + dag_squeeze(parents[f], v);
        if ((seen[(size_t)(at >> 6)] >> (at & 63)) & 1u) { err = who + ": the same (child, parent set) is listed twice"; return MIBN_E_ARG; }
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
inline void dag_binomials(uint32_t *binom /* kDagBinomStride x kDagBinomStride */) {
    for (int c = 0; c < kDagBinomStride; ++c)
        for (int i = 0; i < kDagBinomStride; ++i)
            binom[c * kDagBinomStride + i] = i == 0 ? 1u : c == 0 ? 0u : binom[(c - 1) * kDagBinomStride + i - 1] + binom[(c - 1) * kDagBinomStride + i];
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
