// Conditional-independence tests for constraint-based structure learning (PC-stable): the second phase of mibn_ci_tests.  The first
// phase is count_kernel / count_big_kernel (count_kernel.hip.h) over the resident code matrix, writing the dense contingency table
// of every test - conditioning columns Z_1 .. Z_m first, X, then Y LAST and fastest - into a device buffer of 64-bit counts.  The
// kernels here reduce every table to one fp64 statistic and one exact int64 degree-of-freedom count.
//
// A stratum z (one configuration of Z; q = prod card(Z), 1 without Z) is a contiguous block of s = rx * ry cells.  With N_z the sum
// of the stratum, N_xz its row sums and N_yz its column sums (all exact integers):
//   MIBN_CI_G2   2 * sum over cells with N_xyz > 0 of N_xyz * ln((N_xyz * N_z) / (N_xz * N_yz))
//                the logarithm of the quotient of the two integer products, each exact in a double while N < 2^26 - never the
//                four-logarithm or the entropy form, which cancel at magnitude N ln N; an independent cell has quotient exactly 1
//   MIBN_CI_X2   sum over cells with N_xz * N_yz > 0 of (N_xyz * N_z - N_xz * N_yz)^2 / (N_z * N_xz * N_yz)
//                the difference in 64-bit integers (exact for N < 2^31): every term is >= 0, an independent table gives exactly 0
//   adj_dof      sum over strata with N_z > 0 of (rows with N_xz > 0 - 1) * (columns with N_yz > 0 - 1)
// Empty strata, rows and columns contribute exactly 0: they are skipped, not computed and cancelled.
//
// THE ADDITION ORDER IS A FUNCTION OF THE TABLE'S SHAPE (q, rx, ry) ALONE - not of the grid, of the other tests of the call, of the
// sub-batch cut or of any option - so the same test on the same rows gives the same bits in any call:
//   * LANE FORM, s <= kCiLaneCells.  One lane owns a stratum: its value is ((R_0 + R_1) + ...) over the rows x ascending with
//     R_x = ((t_0 + t_1) + ...) over the cells y ascending (row sums kept in the outer loop, column sums recomputed).
//       - a table of at most kCiWaveCells cells is reduced by a GROUP of g = ci_group(q) lanes, the smallest power of two >= min(q, 64):
//         lane l of the group adds the strata l, l + g, ... in ascending order, then a xor butterfly (g/2, ..., 1) over the group.
//         Groups are packed 64 / g to a wave (ci_lane_kernel), so a level-0 test of PC (q = 1) costs a lane, not a wave;
//       - a larger table is cut into chunks of ci_chunk_strata(s) = kCiWaveCells / s whole strata (the last one ragged); a chunk is
//         reduced exactly as above by a group of 64 lanes -> one partial per chunk.
//   * WAVE FORM, s > kCiLaneCells.  One wave owns a stratum: row and column sums in LDS (at most 256 + 256 32-bit counts, integer
//     atomics), lane l adds the cells l, l + 64, ... of the stratum in ascending order.
//       - a table of at most kCiWaveCells cells: one wave walks the strata 0 .. q - 1, every lane keeps adding to the same
//         accumulator, ONE butterfly (32, ..., 1) at the end;
//       - a larger table: chunks of max(1, kCiWaveCells / s) whole strata, each reduced like that -> one partial per chunk.
//   * ci_finish_kernel reduces a chunked table's partials with one wave: lane l adds the partials l, l + 64, ..., then the butterfly.
// adj_dof is integer arithmetic throughout.  No atomics on doubles anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mibn.h"
#include "score_kernel.hip.h"

namespace mibn {

constexpr int32_t kCiLaneCells = 64;                // a stratum of at most this many cells is one lane's
constexpr int64_t kCiWaveCells = kScoreWaveCells;   // what one group / one wave reduces: a table up to here is not chunked
constexpr int kCiWG = 256;                          // ci_lane_kernel, ci_finish_kernel
constexpr int kCiClasses = 7;                       // group sizes 64, 32, ..., 1

inline int64_t ci_chunk_strata(int64_t s) { return kCiWaveCells / s > 1 ? kCiWaveCells / s : 1; }
inline int32_t ci_group(int64_t q) {
    int32_t g = 1;
    while (g < 64 && g < q) g <<= 1;
    return g;
}

// a run of whole strata of one table: a small table, or a chunk of a large one
struct CiItem {
    int64_t off;  // first cell of the run in `counts`
    int32_t nz;   // strata in the run
    int32_t rx, ry;
    int32_t out;  // index in `stat` / `dof`: the test's own slot, or a partial's
};

struct CiBig {
    int32_t part0, n_parts;  // in `stat` / `dof`
    int32_t out;
};

struct CiArgs {
    const unsigned long long *counts;
    const CiItem *lane_items;  // sorted by group size, 64 first: item i of class k owns the lanes lane0[k] + (i - item0[k]) * (64 >> k) ...
    const CiItem *wave_items;
    const CiBig *big;
    double *stat;    // [tests of the call | partials of the sub-batch]
    long long *dof;  // the same layout
    int32_t kind;
    int32_t n_wave, n_big;
    int32_t lane0[kCiClasses + 1], item0[kCiClasses + 1];
};

__device__ inline double ci_g2_term(unsigned long long n, unsigned long long nz, unsigned long long nx, unsigned long long ny) {
    return 2.0 * (double)n * log(((double)n * (double)nz) / ((double)nx * (double)ny));
}

__device__ inline double ci_x2_term(unsigned long long n, unsigned long long nz, unsigned long long nx, unsigned long long ny) {
    const long long d = (long long)(n * nz) - (long long)(nx * ny);
    return ((double)d * (double)d) / ((double)nz * (double)nx * (double)ny);
}

// lane form: value and degrees of freedom of the stratum c[0 .. rx * ry)
__device__ inline void ci_lane_stratum(const unsigned long long *c, int32_t rx, int32_t ry, int32_t kind, double &stat, long long &dof) {
    unsigned long long nz = 0;
    int cols = 0;
    for (int y = 0; y < ry; ++y) {
        unsigned long long ny = 0;
        for (int x = 0; x < rx; ++x) ny += c[x * ry + y];
        cols += ny > 0;
        nz += ny;
    }
    if (nz == 0) return;
    int rows = 0;
    double v = 0.0;
    for (int x = 0; x < rx; ++x) {
        unsigned long long nx = 0;
        for (int y = 0; y < ry; ++y) nx += c[x * ry + y];
        if (nx == 0) continue;
        ++rows;
        double r = 0.0;
        for (int y = 0; y < ry; ++y) {
            const unsigned long long n = c[x * ry + y];
            if (kind == MIBN_CI_G2 && n == 0) continue;
            unsigned long long ny = 0;
            for (int k = 0; k < rx; ++k) ny += c[k * ry + y];
            if (ny == 0) continue;
            r += kind == MIBN_CI_G2 ? ci_g2_term(n, nz, nx, ny) : ci_x2_term(n, nz, nx, ny);
        }
        v += r;
    }
    stat += v;
    dof += (long long)(rows - 1) * (long long)(cols - 1);
}

// one lane of the grid = one lane of a group (CiArgs::lane_items)
__global__ __launch_bounds__(kCiWG) void ci_lane_kernel(const CiArgs A) {
    const int32_t L = blockIdx.x * kCiWG + threadIdx.x;
    int k = 0;
    int32_t first_lane = A.lane0[0], first_item = A.item0[0];
#pragma unroll
    for (int j = 1; j < kCiClasses; ++j)
        if (L >= A.lane0[j]) {
            k = j;
            first_lane = A.lane0[j];
            first_item = A.item0[j];
        }
    const bool live = L < A.lane0[kCiClasses];
    const int g = live ? 64 >> k : 1;
    const int32_t rel = live ? L - first_lane : 0;
    double stat = 0.0;
    long long dof = 0;
    CiItem I;
    I.out = -1;
    if (live) {
        I = A.lane_items[first_item + rel / g];
        const int64_t s = (int64_t)I.rx * I.ry;
        for (int32_t z = rel & (g - 1); z < I.nz; z += g) ci_lane_stratum(A.counts + I.off + z * s, I.rx, I.ry, A.kind, stat, dof);
    }
    for (int m = 32; m >= 1; m >>= 1) {  // (every lane of the wave shuffles; a group adds only its own steps)
        const double o = __shfl_xor(stat, m, 64);
        const long long d = __shfl_xor(dof, m, 64);
        if (m < g) {
            stat += o;
            dof += d;
        }
    }
    if (live && (rel & (g - 1)) == 0) {
        A.stat[I.out] = stat;
        A.dof[I.out] = dof;
    }
}

__device__ inline unsigned long long ci_wave_sum_u64(unsigned long long x) {
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// blockIdx.x = wave item: ONE wave per workgroup, so the workgroup barrier is the wave's own
__global__ __launch_bounds__(64) void ci_wave_kernel(const CiArgs A) {
    __shared__ unsigned int row[256], col[256];
    const int lane = threadIdx.x;
    const CiItem I = A.wave_items[blockIdx.x];
    const int32_t s = I.rx * I.ry;
    double stat = 0.0;
    long long dof = 0;
    for (int32_t z = 0; z < I.nz; ++z) {
        const unsigned long long *c = A.counts + I.off + (int64_t)z * s;
        for (int i = lane; i < I.rx; i += 64) row[i] = 0;
        for (int i = lane; i < I.ry; i += 64) col[i] = 0;
        __syncthreads();
        for (int32_t i = lane; i < s; i += 64) {
            const unsigned int n = (unsigned int)c[i];  // (n_rows < 2^31)
            if (n) {
                atomicAdd(&row[i / I.ry], n);
                atomicAdd(&col[i % I.ry], n);
            }
        }
        __syncthreads();
        unsigned long long packed = 0;  // N_z | rows in use << 40 | columns in use << 52
        for (int i = lane; i < I.rx; i += 64) packed += (unsigned long long)row[i] + ((unsigned long long)(row[i] > 0) << 40);
        for (int i = lane; i < I.ry; i += 64) packed += (unsigned long long)(col[i] > 0) << 52;
        packed = ci_wave_sum_u64(packed);
        const unsigned long long nz = packed & ((1ull << 40) - 1);
        if (nz) {  // (the whole wave)
            dof += (long long)(((packed >> 40) & 0xfff) - 1) * (long long)((packed >> 52) - 1);
            for (int32_t i = lane; i < s; i += 64) {
                const unsigned long long n = c[i];
                const unsigned long long nx = row[i / I.ry], ny = col[i % I.ry];
                if (nx == 0 || ny == 0 || (A.kind == MIBN_CI_G2 && n == 0)) continue;
                stat += A.kind == MIBN_CI_G2 ? ci_g2_term(n, nz, nx, ny) : ci_x2_term(n, nz, nx, ny);
            }
        }
        __syncthreads();
    }
    stat = score_wave_sum(stat);
    if (lane == 0) {
        A.stat[I.out] = stat;
        A.dof[I.out] = dof;
    }
}

// blockIdx.x * 4 + wave = chunked table: its partials, one wave each
__global__ __launch_bounds__(kCiWG) void ci_finish_kernel(const CiArgs A) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * (kCiWG / 64) + (threadIdx.x >> 6);
    if (f >= A.n_big) return;  // (the whole wave)
    const CiBig B = A.big[f];
    double stat = 0.0;
    unsigned long long dof = 0;
    for (int i = lane; i < B.n_parts; i += 64) {
        stat += A.stat[B.part0 + i];
        dof += (unsigned long long)A.dof[B.part0 + i];
    }
    stat = score_wave_sum(stat);
    dof = ci_wave_sum_u64(dof);
    if (lane == 0) {
        A.stat[B.out] = stat;
        A.dof[B.out] = (long long)dof;
    }
}

}  // namespace mibn
