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

}  // namespace mibn
