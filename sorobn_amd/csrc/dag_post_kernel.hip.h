// Kernels of mibn_arc_posteriors: the posterior probability of every candidate parent set and of every arc, averaged over all
// DAGs under an order-modular prior, by the sum-product form of the subset DP (Koivisto and Sood 2004, Koivisto 2006).
// include/mibn.h pins what is computed; dag_plan.h has the pass schedule - mibn_best_dag's, unchanged -, dag_logaddexp, the centring,
// the order of the arc sums and the bodies of the tile pass, a level's subset and a candidate's posterior - shared with
// tools/dag_post_sim.cpp; a kernel here is its lane-to-work mapping, its LDS array and its stores.  Plain HIP for gfx950, wave64,
// fp64: no inline assembly, no atomics, no scratch; contraction into FMAs is off in this arithmetic (MIBN_FP_NO_CONTRACT), so that
// device, tools/dag_post_sim.cpp and the numpy twin round at the same places.
//
// Tables (every offset in 64 bits: 2.0e8 entries of alpha at n = 24; 8 n 2^(n-1) + 16 2^n bytes in all, 1.9 GB there):
//   alpha[v * 2^(n-1) + i] fp64     i = the subset with bit v squeezed out (dag_squeeze) - dag_kernel's score layout, no mask array;
//                                   first s', then alpha_v, and - alpha being dead once L and R exist - Gamma_v
//   L[S], R[S] fp64                 S = subset of the n variables as a bit mask
//
//   dag_post_fill_kernel       every alpha entry <- -inf
//   dag_post_scatter_kernel    one lane per candidate writes s' = s - c_v (duplicates were refused on the host)
//   dag_post_subset_kernel     one pass of the subset sum: dag_subset_kernel's tile pass over a DagSumTile, entry[e | bit] = entry[e | bit] (+) entry[e]
//   dag_post_level_kernel      L and R of one popcount level, both in one launch (they do not depend on each other)
//                              - a lane per subset OF THE LEVEL, found from its rank (dag_unrank), not a lane per mask
//   dag_post_superset_kernel   one pass of the superset sum, entry[e] = entry[e] (+) entry[e | bit]; the FIRST pass reads no table
//                              but forms g_v(S) = L(S) + R(V \ S \ {v}) while it loads its tile: g never exists in memory
//   dag_post_candidate_kernel  one lane per candidate: log_post[f] = (s'_f + Gamma_v(P_f)) - L(V)
//   dag_post_arc_kernel        the arc sums of one child and one segment of the candidate list, in the order dag_plan.h pins
//   dag_post_arc_sum_kernel    the segments' results added in ascending order: arc[u * n + v]
// Unlike dag_subset_kernel's maximum, a sum's last bits depend on the order of its terms: the options dag_tile_bits /
// dag_group_bits may change the last bits of the results here (within include/mibn.h's bound), never more; dag_plan.h says why
// today's schedules do not.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dag_kernel.hip.h"
#include "dag_plan.h"

namespace mibn {

static_assert(kDagArcLanes == kDagWG, "dag_post_arc_kernel: one lane of the pinned order per thread");
constexpr int kDagPostMaxVars = MIBN_ARC_POSTERIOR_MAX_VARS;

__global__ __launch_bounds__(kDagWG) void dag_post_fill_kernel(double *__restrict__ alpha, int64_t total) {
    const int64_t step = (int64_t)gridDim.x * kDagWG;
    for (int64_t i = (int64_t)blockIdx.x * kDagWG + threadIdx.x; i < total; i += step) alpha[i] = -__builtin_huge_val();
}

__global__ __launch_bounds__(kDagWG) void dag_post_scatter_kernel(const int32_t *__restrict__ child, const uint32_t *__restrict__ parents,
                                                                  const double *__restrict__ fam_score, const double *__restrict__ centre,
                                                                  int64_t n_fam, int32_t n, double *__restrict__ alpha) {
    MIBN_FP_NO_CONTRACT
    const int64_t f = (int64_t)blockIdx.x * kDagWG + threadIdx.x;
    if (f >= n_fam) return;
    const int v = child[f];
    alpha[dag_entry(v, parents[f], n)] = dag_centred(fam_score[f], centre[v]);
}

// grid: n * tiles_per_child workgroups, child-major
__global__ __launch_bounds__(kDagWG) void dag_post_subset_kernel(double *__restrict__ alpha, DagPass P, int32_t n, int64_t tiles_per_child) {
    __shared__ double s_val[1 << kDagMaxTileBits];
    const int64_t wg = blockIdx.x;
    const int64_t v = wg / tiles_per_child, t = wg - v * tiles_per_child;
    dag_tile_pass<true>(DagSumTile{alpha, v << (n - 1), s_val}, P, t, threadIdx.x, kDagWG, DagBarrier{});
}

// level = popcount of the subsets that take part; level 0 writes L[0] = R[0] = 0.
// grid: C(n, level) lanes - lane k takes the k-th subset of the level (dag_unrank), so no lane of a wave idles while others work.
__global__ __launch_bounds__(kDagWG) void dag_post_level_kernel(const double *__restrict__ alpha, double *__restrict__ L, double *__restrict__ R,
                                                                const uint32_t *__restrict__ binom, int32_t n, int32_t level) {
    const uint32_t k = blockIdx.x * kDagWG + threadIdx.x;
    if (k >= binom[n * kDagBinomStride + level]) return;
    const uint32_t S = dag_unrank(k, level, n, binom);
    const DagLR x = dag_level(S, n, alpha, L, R);
    L[(int64_t)S] = x.l;
    R[(int64_t)S] = x.r;
}

// grid: n * tiles_per_child workgroups, child-major.  first != 0: the tile is formed from L and R, nothing is read from gamma.
__global__ __launch_bounds__(kDagWG) void dag_post_superset_kernel(double *__restrict__ gamma, const double *__restrict__ L, const double *__restrict__ R,
                                                                   DagPass P, int32_t n, int64_t tiles_per_child, int32_t first) {
    __shared__ double s_val[1 << kDagMaxTileBits];
    const int64_t wg = blockIdx.x;
    const int64_t v = wg / tiles_per_child, t = wg - v * tiles_per_child;
    const DagSumTile T{gamma, v << (n - 1), s_val};
    const int size = P.tile_size();
    if (first) dag_tile_load(DagGapTile(s_val, L, R, (int)v, n), P, size, t, threadIdx.x, kDagWG);
    else dag_tile_load(T, P, size, t, threadIdx.x, kDagWG);
    dag_tile_run<false>(T, P, size, t, threadIdx.x, kDagWG, DagBarrier{});
}

__global__ __launch_bounds__(kDagWG) void dag_post_candidate_kernel(const int32_t *__restrict__ child, const uint32_t *__restrict__ parents,
                                                                    const double *__restrict__ fam_score, const double *__restrict__ centre,
                                                                    const double *__restrict__ gamma, const double *__restrict__ L, int64_t n_fam,
                                                                    int32_t n, double *__restrict__ log_post) {
    const int64_t f = (int64_t)blockIdx.x * kDagWG + threadIdx.x;
    if (f >= n_fam) return;
    const int v = child[f];
    log_post[f] = dag_log_post(v, parents[f], fam_score[f], centre[v], gamma, L[(int64_t(1) << n) - 1], n);
}

// grid (segments, n): workgroup (j, v) writes part[(j * n + u) * n + v] for every u.  A lane keeps one sum per u in registers (the
// loops over u have a compile-time bound: no array is indexed by a run-time value).
__global__ __launch_bounds__(kDagWG) void dag_post_arc_kernel(const int32_t *__restrict__ child, const uint32_t *__restrict__ parents,
                                                              const double *__restrict__ log_post, int64_t n_fam, int32_t n, double *__restrict__ part) {
    MIBN_FP_NO_CONTRACT
    __shared__ double s_lane[kDagWG];
    const int64_t j = blockIdx.x;
    const int v = blockIdx.y;
    const int64_t first = j * kDagArcSegment, last = first + kDagArcSegment < n_fam ? first + kDagArcSegment : n_fam;
    double acc[kDagPostMaxVars];
#pragma unroll
    for (int u = 0; u < kDagPostMaxVars; ++u) acc[u] = 0.0;
    for (int64_t f = first + threadIdx.x; f < last; f += kDagWG) {
        if (child[f] != v) continue;
        const uint32_t pm = parents[f];
        const double p = exp(log_post[f]);
#pragma unroll
        for (int u = 0; u < kDagPostMaxVars; ++u) acc[u] += (pm >> u) & 1u ? p : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kDagPostMaxVars; ++u) {
        if (u < n) {  // (uniform)
            s_lane[threadIdx.x] = acc[u];
            __syncthreads();
            for (int h = kDagWG / 2; h >= 1; h /= 2) {
                if ((int)threadIdx.x < h) s_lane[threadIdx.x] += s_lane[threadIdx.x + h];
                __syncthreads();
            }
            if (threadIdx.x == 0) part[(j * n + u) * n + v] = s_lane[0];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kDagWG) void dag_post_arc_sum_kernel(const double *__restrict__ part, int64_t segments, int32_t n, double *__restrict__ arc) {
    MIBN_FP_NO_CONTRACT
    const int k = blockIdx.x * kDagWG + threadIdx.x;
    if (k >= n * n) return;
    double sum = 0.0;
    for (int64_t j = 0; j < segments; ++j) sum += part[j * n * n + k];
    arc[k] = sum;
}

}  // namespace mibn
