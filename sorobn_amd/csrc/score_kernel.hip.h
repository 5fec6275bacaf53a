// Decomposable family scores for score-based structure learning (hill climbing over add / delete / reverse): the second phase
// of mibn_score_families.  The first phase is count_kernel / count_big_kernel (count_kernel.hip.h) over the resident code matrix,
// writing the dense contingency table of every family - parents first, CHILD LAST - into a device buffer of 64-bit counts.  The
// kernels here reduce every table to one fp64 score, so that one double per family goes back to the host.
//
// With the child last the r = card(child) cells of one parent configuration j are contiguous: N_j is their (exact, integer) sum.
// Natural logs; q = number of parent configurations (1 without parents), N = n_rows:
//   loglik  LL = sum over cells with N_jk > 0 of N_jk * (ln N_jk - ln N_j)
//   bic     LL - 0.5 * ln(max(N, 1)) * q * (r - 1)
//   aic     LL - q * (r - 1)
//   bdeu    sum_j [lgamma(a/q) - lgamma(a/q + N_j)] + sum_jk [lgamma(a/(q r) + N_jk) - lgamma(a/(q r))]      (a = ess)
//   k2      sum_j [lgamma(r) - lgamma(r + N_j)] + sum_jk lgamma(1 + N_jk)
// A configuration with N_j = 0 and a cell with N_jk = 0 contribute exactly 0: they are skipped, not computed and cancelled.
//
// THE ADDITION ORDER IS A FUNCTION OF THE TABLE'S SHAPE (q, r) ALONE - not of the grid, of the other families of the call or of
// any option - so the same family on the same data gives the same bits in any call:
//   * a configuration's value is  head_j + (((t_0 + t_1) + ...) + t_{r-1})  over its non-zero cells in ascending k;
//   * a table of at most kScoreWaveCells cells is reduced by ONE wave: lane l adds the configurations l, l + 64, ... in ascending
//     order, then a xor butterfly (32, 16, ..., 1) over the 64 lanes; the penalty is added last;
//   * a larger table is cut into chunks of score_chunk_configs(r) = max(1, kScoreChunkCells / r) configurations.  One 256-thread
//     workgroup per chunk: thread t adds the chunk's configurations t, t + 256, ..., the butterfly per wave, then
//     ((w0 + w1) + w2) + w3 -> one partial per chunk.  score_finish_kernel reduces a table's partials with one wave exactly as a
//     small table reduces its configurations, and adds the penalty.
// No atomics on doubles anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mibn.h"

namespace mibn {

constexpr int64_t kScoreWaveCells = 4096;    // one wave: at most 64 cells per lane (32 KiB of counts)
constexpr int64_t kScoreChunkCells = 16384;  // one workgroup of the chunked form: the same 64 cells per thread
constexpr int kScoreWG = 256;

inline int64_t score_chunk_configs(int32_t r) { return kScoreChunkCells / r > 1 ? kScoreChunkCells / r : 1; }

struct ScoreFam {
    int64_t off;  // first cell of the table in `counts`
    int64_t q;    // parent configurations
    int32_t r;    // child states
    int32_t out;  // index in `scores`
};

struct ScoreChunk {
    int32_t fam;   // index in `big`
    int32_t part;  // index in `parts`
    int64_t j0;    // first configuration
};

struct ScoreBig {
    int32_t part0, n_parts;
};

struct ScoreArgs {
    const unsigned long long *counts;
    const ScoreFam *small;    // tables of at most kScoreWaveCells cells
    const ScoreFam *big;      // the others
    const ScoreChunk *chunk;
    const ScoreBig *big_parts;
    double *parts;
    double *scores;
    double ess;
    int64_t n_rows;
    int32_t kind;
    int32_t n_small, n_big;
};

// what a family adds per configuration / cell, with the constants of its shape
struct ScoreTerms {
    int32_t kind;
    double head0, cell0, a_q, a_qr;  // bdeu: lgamma(a/q), lgamma(a/(q r)), a/q, a/(q r); k2: head0 = lgamma(r)
    __device__ ScoreTerms(int32_t kind_, double ess, int64_t q, int32_t r) : kind(kind_), head0(0), cell0(0), a_q(0), a_qr(0) {
        if (kind == MIBN_SCORE_BDEU) {
            a_q = ess / (double)q;
            a_qr = ess / ((double)q * (double)r);
            head0 = lgamma(a_q);
            cell0 = lgamma(a_qr);
        } else if (kind == MIBN_SCORE_K2) {
            head0 = lgamma((double)r);
        }
    }
    // value of configuration j: cells c[0 .. r)
    __device__ double config(const unsigned long long *c, int32_t r) const {
        unsigned long long nj = 0;
        for (int k = 0; k < r; ++k) nj += c[k];
        if (nj == 0) return 0.0;
        double cells = 0.0;
        if (kind == MIBN_SCORE_BDEU) {
            for (int k = 0; k < r; ++k)
                if (c[k]) cells += lgamma(a_qr + (double)c[k]) - cell0;
            return (head0 - lgamma(a_q + (double)nj)) + cells;
        }
        if (kind == MIBN_SCORE_K2) {
            for (int k = 0; k < r; ++k)
                if (c[k]) cells += lgamma(1.0 + (double)c[k]);
            return (head0 - lgamma((double)r + (double)nj)) + cells;
        }
        const double ln_nj = log((double)nj);
        for (int k = 0; k < r; ++k)
            if (c[k]) cells += (double)c[k] * (log((double)c[k]) - ln_nj);
        return cells;
    }
    // the part that does not depend on the counts, added last
    __device__ double finish(double sum, int64_t q, int32_t r, int64_t n_rows) const {
        if (kind == MIBN_SCORE_BIC) return sum - 0.5 * log((double)(n_rows > 1 ? n_rows : 1)) * (double)q * (double)(r - 1);
        if (kind == MIBN_SCORE_AIC) return sum - (double)q * (double)(r - 1);
        return sum;
    }
};

__device__ inline double score_wave_sum(double x) {
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// blockIdx.x * 4 + wave = small table; one wave each
__global__ __launch_bounds__(kScoreWG) void score_kernel(const ScoreArgs A) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * (kScoreWG / 64) + (threadIdx.x >> 6);
    if (f >= A.n_small) return;  // (the whole wave)
    const ScoreFam F = A.small[f];
    const ScoreTerms T(A.kind, A.ess, F.q, F.r);
    double acc = 0.0;
    for (int64_t j = lane; j < F.q; j += 64) acc += T.config(A.counts + F.off + j * F.r, F.r);
    acc = score_wave_sum(acc);
    if (lane == 0) A.scores[F.out] = T.finish(acc, F.q, F.r, A.n_rows);
}

// blockIdx.x = chunk of a big table -> parts[chunk.part]
__global__ __launch_bounds__(kScoreWG) void score_chunk_kernel(const ScoreArgs A) {
    __shared__ double wave_sum[kScoreWG / 64];
    const ScoreChunk C = A.chunk[blockIdx.x];
    const ScoreFam F = A.big[C.fam];
    const ScoreTerms T(A.kind, A.ess, F.q, F.r);
    const int64_t per = kScoreChunkCells / F.r > 1 ? kScoreChunkCells / F.r : 1;
    const int64_t j1 = C.j0 + per < F.q ? C.j0 + per : F.q;
    double acc = 0.0;
    for (int64_t j = C.j0 + threadIdx.x; j < j1; j += kScoreWG) acc += T.config(A.counts + F.off + j * F.r, F.r);
    acc = score_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) A.parts[C.part] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// blockIdx.x * 4 + wave = big table: its partials, one wave each
__global__ __launch_bounds__(kScoreWG) void score_finish_kernel(const ScoreArgs A) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * (kScoreWG / 64) + (threadIdx.x >> 6);
    if (f >= A.n_big) return;
    const ScoreFam F = A.big[f];
    const ScoreBig B = A.big_parts[f];
    const ScoreTerms T(A.kind, A.ess, F.q, F.r);
    double acc = 0.0;
    for (int i = lane; i < B.n_parts; i += 64) acc += A.parts[B.part0 + i];
    acc = score_wave_sum(acc);
    if (lane == 0) A.scores[F.out] = T.finish(acc, F.q, F.r, A.n_rows);
}

}  // namespace mibn
