// Expected counts on gfx950 - the fractional twin of count_kernel (the E-step of BayesNet.fit_em, mibn_expect_batch).
// Input: the device-resident results of an unnormalised query call - request b's slice of P(q_b, e_b), C-order over its
// query variables - and per request a target: a base cell in one float64 accumulation buffer `acc` and one stride per
// query variable.  With s_b = the sum of the slice = P(e_b):
//     acc[base_b + sum_k idx_k * stride_{b,k}] += w_b * slice_b[idx] / s_b      (nothing when s_b == 0)
//     p_out[b] = s_b
//
// Bitwise repeatable: no floating-point atomics, every addition order is a function of the request arrays alone.
//   * The host cuts the requests, in the caller's order, into slabs of consecutive requests whose targets together span at
//     most kExpectLdsCells cells (a caller that lays its requests out target-table major gets slabs inside one table).
//   * expect_kernel: one wave = one workgroup per slab.  It walks the requests of its slab IN ORDER; the lanes cover the cells of
//     the current slice - distinct target cells within a request, so plain LDS read-add-writes - into a wave-private LDS image of
//     the slab's span.  The slice sum is a fixed-shape reduction (lane-strided partial sums, then a xor butterfly).  The image
//     goes to global memory as the slab's partial.
//   * expect_reduce_kernel: one thread per cell of `acc` adds the partials of the slabs that cover the cell in slab order (the
//     host lists them per block of 256 cells).
//   * A request whose own targets span more than kExpectLdsCells cells (a family table too large for the LDS image) takes
//     expect_big_kernel: thread t owns the cells congruent to t modulo the thread count and walks the big requests in order,
//     adding the cells it owns straight into `acc` - one owner per cell, program order per owner.  It runs after the reduction.
//
// kExpectLdsCells = 2048 float64 cells = 16 KiB per wave (count_kernel: 16 384 uint32 cells = 64 KiB shared by a 256-lane workgroup):
// a slab is walked by ONE wave and its latency is hidden only by other waves, so the image is sized for ten resident workgroups per
// CU (160 KiB of LDS), not for the largest table; 2048 cells hold a four-state child with four four-state parents.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mibn.h"

namespace mibn {

constexpr int kExpectLdsCells = 2048;  // float64 cells of a slab's LDS image (16 KiB per wave)
constexpr int kExpectSlabMax = 64;     // requests per slab at most
constexpr int kExpectMaxQ = 8;         // query variables of a request at most (missing members of one family)
constexpr int kExpectBigWG = 256;

struct ExpectReq {
    int64_t res_off;  // first cell of the slice in the results
    int64_t base;     // LDS path: target base relative to the slab's first cell; big path: absolute cell of acc
    int32_t cells;    // slice cells
    int32_t nq;       // query variables (0: only p_out)
    int32_t dim;      // first entry in dim_card / dim_stride
    int32_t out;      // the request's index in the call (p_out, weight)
};

struct ExpectArgs {
    const double *results;
    const ExpectReq *req;
    const int32_t *dim_card;
    const int64_t *dim_stride;
    const double *weight;        // per request of the call, or nullptr
    const int32_t *slab_begin;   // [n_slabs + 1] into req
    const int32_t *slab_cells;   // [n_slabs] cells of the slab's span
    const int64_t *slab_part;    // [n_slabs] offset of the slab's partial
    double *part;
    double *p_out;
};

__device__ __forceinline__ double expect_wave_sum(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

__device__ __forceinline__ int64_t expect_target(int idx, int nq, const int32_t *card, const int64_t *stride) {
    int64_t off = 0;
    for (int k = nq - 1; k >= 0; --k) {
        const int c = card[k];
        const int d = idx % c;
        idx /= c;
        off += (int64_t)d * stride[k];
    }
    return off;
}

__global__ __launch_bounds__(64) void expect_kernel(const ExpectArgs A) {
    __shared__ double image[kExpectLdsCells];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int span = A.slab_cells[s];
    for (int i = lane; i < span; i += 64) image[i] = 0.0;
    __syncthreads();
    for (int r = A.slab_begin[s]; r < A.slab_begin[s + 1]; ++r) {
        const ExpectReq R = A.req[r];
        const double *slice = A.results + R.res_off;
        double part = 0.0;
        for (int i = lane; i < R.cells; i += 64) part += slice[i];
        const double sum = expect_wave_sum(part);
        if (lane == 0) A.p_out[R.out] = sum;
        if (R.nq == 0 || !(sum > 0.0)) continue;
        const double w = A.weight ? A.weight[R.out] : 1.0;
        const int32_t *card = A.dim_card + R.dim;
        const int64_t *stride = A.dim_stride + R.dim;
        for (int i = lane; i < R.cells; i += 64) {
            const int cell = (int)(R.base + expect_target(i, R.nq, card, stride));
            image[cell] += w * (slice[i] / sum);
        }
        __syncthreads();  // (one wave: orders this request's LDS writes before the next request's reads)
    }
    double *out = A.part + A.slab_part[s];
    for (int i = lane; i < span; i += 64) out[i] = image[i];
}

struct ExpectReduceArgs {
    const double *part;
    const int32_t *blk_begin;   // [n_blocks + 1] into blk_slab
    const int32_t *blk_slab;    // slabs that cover a block of 256 cells, ascending
    const int64_t *slab_lo;     // first cell of acc of every slab's span
    const int32_t *slab_cells;
    const int64_t *slab_part;
    double *acc;
    int64_t cell0;              // first cell of block 0
    int64_t n_acc;
};

__global__ __launch_bounds__(256) void expect_reduce_kernel(const ExpectReduceArgs A) {
    const int64_t c = A.cell0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= A.n_acc) return;
    double v = A.acc[c];
    bool any = false;
    for (int k = A.blk_begin[blockIdx.x]; k < A.blk_begin[blockIdx.x + 1]; ++k) {
        const int s = A.blk_slab[k];
        const int64_t rel = c - A.slab_lo[s];
        if (rel >= 0 && rel < A.slab_cells[s]) { v += A.part[A.slab_part[s] + rel]; any = true; }
    }
    if (any) A.acc[c] = v;
}

struct ExpectBigArgs {
    const double *results;
    const ExpectReq *req;  // the big requests, in the caller's order
    const int32_t *dim_card;
    const int64_t *dim_stride;
    const double *weight;
    double *acc;
    double *p_out;
    int32_t n_req;
};

__global__ __launch_bounds__(kExpectBigWG) void expect_big_kernel(const ExpectBigArgs A) {
    const int64_t n_threads = (int64_t)gridDim.x * kExpectBigWG;
    const int64_t me = (int64_t)blockIdx.x * kExpectBigWG + threadIdx.x;
    for (int r = 0; r < A.n_req; ++r) {
        const ExpectReq R = A.req[r];
        const double *slice = A.results + R.res_off;
        // every thread forms the same sum in the same order (no cross-lane step: blocks do not share one)
        double sum = 0.0;
        for (int i = 0; i < R.cells; ++i) sum += slice[i];
        if (me == 0) A.p_out[R.out] = sum;
        if (!(sum > 0.0)) continue;
        const double w = A.weight ? A.weight[R.out] : 1.0;
        const int32_t *card = A.dim_card + R.dim;
        const int64_t *stride = A.dim_stride + R.dim;
        for (int i = 0; i < R.cells; ++i) {
            const int64_t cell = R.base + expect_target(i, R.nq, card, stride);
            if (cell % n_threads == me) A.acc[cell] += w * (slice[i] / sum);
        }
    }
}

// The host's side: slabs, the reduction lists and the big requests of one call.  Everything here is a function of the request
// arrays alone (never of thread counts or timing): the addition order it fixes is the call's.
struct ExpectPlan {
    std::vector<ExpectReq> req, big;
    std::vector<int32_t> dim_card;
    std::vector<int64_t> dim_stride;
    std::vector<int32_t> slab_begin{0}, slab_cells, blk_begin{0}, blk_slab;
    std::vector<int64_t> slab_lo, slab_part;
    int64_t part_cells = 0, cell0 = 0, n_blocks = 0;
};

// Validates the targets (MIBN_E_ARG when one leaves [0, n_acc)) and builds the plan.  out_off: the slices of the call's results.
inline int expect_plan(int64_t B, const int64_t *q_off, const int32_t *q_vars, const int32_t *card, const int64_t *out_off, const int64_t *acc_base,
                       const int64_t *acc_stride, int64_t n_acc, ExpectPlan &P, std::string &err) {
    P = ExpectPlan{};
    P.req.reserve((size_t)B);
    int64_t lo = 0, hi = -1;  // span of the slab in progress (hi < lo: empty)
    int32_t in_slab = 0;
    auto close = [&]() {
        if (!in_slab) return;
        const int32_t first = P.slab_begin.back();
        for (size_t r = (size_t)first; r < P.req.size(); ++r)
            if (P.req[r].nq) P.req[r].base -= lo;
        P.slab_begin.push_back((int32_t)P.req.size());
        P.slab_cells.push_back(hi >= lo ? (int32_t)(hi - lo + 1) : 0);
        P.slab_lo.push_back(lo);
        P.slab_part.push_back(P.part_cells);
        P.part_cells += hi >= lo ? hi - lo + 1 : 0;
        in_slab = 0;
        lo = 0;
        hi = -1;
    };
    for (int64_t b = 0; b < B; ++b) {
        const int64_t nq = q_off[b + 1] - q_off[b];
        if (nq > kExpectMaxQ) { err = "request " + std::to_string(b) + ": more than " + std::to_string(kExpectMaxQ) + " query variables"; return MIBN_E_LIMIT; }
        ExpectReq R;
        R.res_off = out_off[b] - out_off[0];
        R.cells = (int32_t)(out_off[b + 1] - out_off[b]);
        R.nq = (int32_t)nq;
        R.dim = (int32_t)P.dim_card.size();
        R.out = (int32_t)b;
        R.base = 0;
        if (nq == 0) {  // only p_out: joins the slab in progress, adds nothing to its span
            if (in_slab == kExpectSlabMax) close();
            P.req.push_back(R);
            ++in_slab;
            continue;
        }
        int64_t t_lo = acc_base[b], t_hi = acc_base[b];
        for (int64_t k = 0; k < nq; ++k) {
            const int32_t c = card[q_vars[q_off[b] + k]];
            const int64_t st = acc_stride[q_off[b] + k];
            // (|stride| * card beyond any buffer: refused before the products below could overflow)
            if (st > n_acc || st < -n_acc) { err = "request " + std::to_string(b) + ": target outside the accumulation buffer"; return MIBN_E_ARG; }
            if (st >= 0) t_hi += st * (c - 1); else t_lo += st * (c - 1);
            P.dim_card.push_back(c);
            P.dim_stride.push_back(st);
        }
        if (acc_base[b] < 0 || acc_base[b] >= n_acc || t_lo < 0 || t_hi >= n_acc) { err = "request " + std::to_string(b) + ": target outside the accumulation buffer"; return MIBN_E_ARG; }
        R.base = acc_base[b];
        if (t_hi - t_lo + 1 > kExpectLdsCells) {  // the global path
            P.big.push_back(R);
            continue;
        }
        const int64_t n_lo = hi >= lo ? std::min(lo, t_lo) : t_lo, n_hi = hi >= lo ? std::max(hi, t_hi) : t_hi;
        if (in_slab == kExpectSlabMax || n_hi - n_lo + 1 > kExpectLdsCells) {
            close();
            lo = t_lo;
            hi = t_hi;
        } else {
            lo = n_lo;
            hi = n_hi;
        }
        P.req.push_back(R);
        ++in_slab;
    }
    close();
    // per block of 256 cells of acc (from the first cell any slab touches): the slabs that cover it, ascending
    const size_t n_slabs = P.slab_cells.size();
    int64_t a_lo = n_acc, a_hi = -1;
    for (size_t s = 0; s < n_slabs; ++s)
        if (P.slab_cells[s]) { a_lo = std::min(a_lo, P.slab_lo[s]); a_hi = std::max(a_hi, P.slab_lo[s] + P.slab_cells[s] - 1); }
    if (a_hi >= a_lo) {
        P.cell0 = a_lo;
        P.n_blocks = (a_hi - a_lo) / 256 + 1;
        std::vector<int32_t> count((size_t)P.n_blocks + 1, 0);
        for (size_t s = 0; s < n_slabs; ++s)
            if (P.slab_cells[s])
                for (int64_t k = (P.slab_lo[s] - a_lo) / 256; k <= (P.slab_lo[s] + P.slab_cells[s] - 1 - a_lo) / 256; ++k) ++count[(size_t)k + 1];
        for (int64_t k = 0; k < P.n_blocks; ++k) count[(size_t)k + 1] += count[(size_t)k];
        P.blk_begin = count;
        P.blk_slab.resize((size_t)count[(size_t)P.n_blocks]);
        std::vector<int32_t> fill(count.begin(), count.end() - 1);
        for (size_t s = 0; s < n_slabs; ++s)
            if (P.slab_cells[s])
                for (int64_t k = (P.slab_lo[s] - a_lo) / 256; k <= (P.slab_lo[s] + P.slab_cells[s] - 1 - a_lo) / 256; ++k) P.blk_slab[(size_t)fill[(size_t)k]++] = (int32_t)s;
    }
    return MIBN_OK;
}

}  // namespace mibn
