// Kernels of mibn_best_dag: the best-scoring DAG by dynamic programming over variable subsets (Silander and Myllymaki 2006).
// include/mibn.h pins what is computed; dag_plan.h has the pass schedule of phase A, why it cannot change a bit, the index
// functions and the bodies of the tile pass, a level's subset and the traceback - shared with tools/dag_plan_sim.cpp; a kernel
// here is its lane-to-work mapping, its LDS arrays and its stores.  Plain HIP for gfx950, wave64: no inline assembly, no atomics,
// no scratch.
//
// Tables (every offset in 64 bits: 2.0e8 entries and 1.6e9 bytes at n = 24):
//   score[v * 2^(n-1) + i] fp64, mask[..] uint32    bps of child v, i = the subset with bit v squeezed out (dag_squeeze)
//   best[S] fp64, sink[S] uint8                     S = subset of the n variables as a bit mask
//
//   dag_fill_kernel       every bps entry <- (-inf, none)
//   dag_scatter_kernel    one lane per candidate writes its entry (duplicates were refused on the host: no two lanes share one)
//   dag_subset_kernel     one pass of phase A: a workgroup loads a tile (dag_gather) into LDS - scores and masks as two arrays -,
//                         runs the pass's bits over it with a barrier between bits, and writes it back (dag_tile_pass, DagMaxTile)
//   dag_sink_kernel       one level of phase B: the lanes run over all subsets, those of `level` members take part
//   dag_traceback_kernel  one lane peels the sinks from V and writes parents, order and total
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dag_plan.h"

namespace mibn {

constexpr int kDagWG = 256;

__global__ __launch_bounds__(kDagWG) void dag_fill_kernel(double *__restrict__ score, uint32_t *__restrict__ mask, int64_t total) {
    const int64_t step = (int64_t)gridDim.x * kDagWG;
    for (int64_t i = (int64_t)blockIdx.x * kDagWG + threadIdx.x; i < total; i += step) {
        score[i] = -__builtin_huge_val();
        mask[i] = kDagNoMask;
    }
}

__global__ __launch_bounds__(kDagWG) void dag_scatter_kernel(const int32_t *__restrict__ child, const uint32_t *__restrict__ parents,
                                                             const double *__restrict__ fam_score, int64_t n_fam, int32_t n,
                                                             double *__restrict__ score, uint32_t *__restrict__ mask) {
    const int64_t f = (int64_t)blockIdx.x * kDagWG + threadIdx.x;
    if (f >= n_fam) return;
    const uint32_t pm = parents[f];
    const int64_t at = dag_entry(child[f], pm, n);
    score[at] = fam_score[f];
    mask[at] = pm;
}

// a workgroup's barrier as dag_tile_pass's sync
struct DagBarrier {
    __device__ void operator()() const { __syncthreads(); }
};

// grid: n * tiles_per_child workgroups, child-major
__global__ __launch_bounds__(kDagWG) void dag_subset_kernel(double *__restrict__ score, uint32_t *__restrict__ mask, DagPass P, int32_t n,
                                                            int64_t tiles_per_child) {
    __shared__ double s_score[1 << kDagMaxTileBits];
    __shared__ uint32_t s_mask[1 << kDagMaxTileBits];
    const int64_t wg = blockIdx.x;
    const int64_t v = wg / tiles_per_child, t = wg - v * tiles_per_child;
    const int64_t base = v << (n - 1);
    dag_tile_pass<true>(DagMaxTile{score, mask, base, s_score, s_mask}, P, t, threadIdx.x, kDagWG, DagBarrier{});
}

// level = popcount of the subsets that take part; level 0 writes best[0] = 0
__global__ __launch_bounds__(kDagWG) void dag_sink_kernel(const double *__restrict__ score, double *__restrict__ best, uint8_t *__restrict__ sink,
                                                          int32_t n, int32_t level) {
    const int64_t S64 = (int64_t)blockIdx.x * kDagWG + threadIdx.x;
    if (S64 >= (int64_t(1) << n)) return;
    if (__builtin_popcount((uint32_t)S64) != level) return;
    const DagSink r = dag_sink((uint32_t)S64, n, score, best);
    best[S64] = r.top;
    sink[S64] = (uint8_t)r.who;
}

// out: parents uint32[n] | order int32[n] (as words), total in `total_out`
__global__ void dag_traceback_kernel(const uint32_t *__restrict__ mask, const double *__restrict__ best, const uint8_t *__restrict__ sink, int32_t n,
                                     uint32_t *__restrict__ parents_out, int32_t *__restrict__ order_out, double *__restrict__ total_out) {
    if (blockIdx.x || threadIdx.x) return;
    dag_traceback(mask, best, sink, n, parents_out, order_out, total_out);
}

}  // namespace mibn
