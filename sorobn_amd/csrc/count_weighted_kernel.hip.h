// Counting under integer row weights on gfx950 - the weighted twin of count_kernel.hip.h, under mibn_score_families_w,
// mibn_ci_tests_w and mibn_count_tables_w, and the draw of bootstrap weight sets (mibn_dataset_bootstrap).
//
// A weight set is uint32[n_rows]; the sets of a data set lie back to back (set-major).  Every table names a set (tbl_wset, -1 = every
// row once): its contingency table counts row i w_s[i] times.  The shape is count_kernel's: tables packed into groups of at most
// kCountLdsCells cells, a workgroup per (group, row block), consecutive lanes on consecutive rows - the code columns AND the weight
// column are 256 B / 1 KiB coalesced wave loads that stay in L1 across the tables of the group - ds_add_u32 of the weight into the
// LDS histogram, one 64-bit global atomic per non-zero cell at the end.  A row of weight 0 issues NO atomic (37 % of the rows of a
// bootstrap set).  The host guarantees W_s <= 2^32 - 1, so no 32-bit partial sum overflows.
//
// In a bootstrap sweep the same scope is counted under many sets.  A table flagged tbl_same has the scope of the table before it in
// its group: the row's cell index (one byte load and one multiply-add per column) is then kept, not recomputed - only the weight load
// and the atomic remain per (scope, set).  The flag is uniform over the workgroup (a scalar load and a scalar branch).
//
// Integer atomics only: every result is independent of launch geometry and scheduling.  No scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mibn.h"
#include "count_kernel.hip.h"
#include "device_mem.h"
#include "gibbs_kernel.hip.h"  // philox_uniform

namespace mibn {

struct CountWArgs {
    CountArgs c;                // what count_kernel reads, with the same meaning
    const int32_t *tbl_wset;    // per table: weight set, -1 = every row once
    const int32_t *tbl_same;    // per table: 1 = the scope of the table before it (never set on a group's first table)
    const uint32_t *weights;    // [n_sets][n_rows]
};

__global__ __launch_bounds__(256) void count_weighted_kernel(const CountWArgs W) {
    __shared__ unsigned int hist[kCountLdsCells];
    const CountArgs &A = W.c;
    const int g = blockIdx.y;
    const int t0 = A.grp_begin[g], t1 = A.grp_begin[g + 1];
    const int cells = A.tbl_lds[t1] - A.tbl_lds[t0];
    for (int i = threadIdx.x; i < cells; i += 256) hist[i] = 0u;
    __syncthreads();
    const int base = A.tbl_lds[t0];
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < A.n_rows; row += (int64_t)gridDim.x * 256) {
        int rel = 0;
        for (int t = t0; t < t1; ++t) {
            if (!W.tbl_same[t]) {
                rel = 0;
                for (int k = A.tbl_begin[t]; k < A.tbl_begin[t + 1]; ++k)
                    rel += (int)A.codes[(int64_t)A.tbl_col[k] * A.n_rows + row] * A.tbl_stride[k];
            }
            const int s = W.tbl_wset[t];
            const unsigned int w = s < 0 ? 1u : W.weights[(int64_t)s * A.n_rows + row];
            if (w) atomicAdd(&hist[A.tbl_lds[t] - base + rel], w);
        }
    }
    __syncthreads();
    for (int t = t0; t < t1; ++t) {
        const int lo = A.tbl_lds[t] - base, n = A.tbl_lds[t + 1] - A.tbl_lds[t];
        for (int i = threadIdx.x; i < n; i += 256)
            if (hist[lo + i]) atomicAdd(&A.counts[A.tbl_out[t] + i], (unsigned long long)hist[lo + i]);
    }
}

// tables above kCountLdsCells cells: straight into HBM, as count_big_kernel (blockIdx.y = table)
struct CountBigWArgs {
    CountBigArgs c;
    const int32_t *tbl_wset;
    const uint32_t *weights;
};

__global__ __launch_bounds__(256) void count_big_weighted_kernel(const CountBigWArgs W) {
    const CountBigArgs &A = W.c;
    const int t = blockIdx.y;
    const int k0 = A.tbl_begin[t], k1 = A.tbl_begin[t + 1];
    const int s = W.tbl_wset[t];
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < A.n_rows; row += (int64_t)gridDim.x * 256) {
        const unsigned int w = s < 0 ? 1u : W.weights[(int64_t)s * A.n_rows + row];
        if (!w) continue;
        int64_t cell = A.tbl_out[t];
        for (int k = k0; k < k1; ++k) cell += (int64_t)A.codes[(int64_t)A.tbl_col[k] * A.n_rows + row] * A.tbl_stride[k];
        atomicAdd(&A.counts[cell], (unsigned long long)w);
    }
}

// A lane per (set, draw) over a ZEROED block w[n_sets][n_rows]: set s, draw j -> row min(floor(u * n_rows), n_rows - 1) with
// u = philox_uniform(j, s, k0, k1), the product in fp64 (include/mibn.h pins the rule; tests/weights_check.py is its numpy twin).
__global__ __launch_bounds__(256) void bootstrap_weights_kernel(uint32_t *w, int64_t n_rows, int64_t total, uint32_t k0, uint32_t k1) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t s = i / n_rows, j = i - s * n_rows;
        const double u = philox_uniform((uint64_t)j, (uint32_t)s, k0, k1);
        int64_t idx = (int64_t)floor(u * (double)n_rows);
        idx = idx < n_rows - 1 ? idx : n_rows - 1;
        atomicAdd(&w[s * n_rows + idx], 1u);
    }
}

inline hipError_t bootstrap_weights_launch(hipStream_t stream, uint32_t *d_w, int64_t n_rows, int64_t n_sets, uint64_t seed) {
    const int64_t total = n_rows * n_sets;
    if (total <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(d_w, 0, 4 * (size_t)total, stream);
    if (e != hipSuccess) return e;
    const unsigned bx = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(bootstrap_weights_kernel, dim3(bx), dim3(256), 0, stream, d_w, n_rows, total, (uint32_t)seed,
                       (uint32_t)(seed >> 32) ^ 0x85EBCA6Bu);
    return hipGetLastError();
}

// W_s of every set, checked: <= 2^32 - 1 each
inline int weight_sums(const uint32_t *weights, int64_t n_sets, int64_t n_rows, std::vector<int64_t> &sums, std::string &err) {
    sums.assign((size_t)n_sets, 0);
    for (int64_t s = 0; s < n_sets; ++s) {
        uint64_t run = 0;
        const uint32_t *w = weights + s * n_rows;
        for (int64_t i = 0; i < n_rows; ++i) run += w[i];
        if (run > 0xffffffffull) { err = "weights: set " + std::to_string(s) + " sums to more than 2^32 - 1"; return MIBN_E_LIMIT; }
        sums[(size_t)s] = (int64_t)run;
    }
    return MIBN_OK;
}

// The weighted half of a packed call: count_pack's layout with three arrays appended to P.i32 (so the pack still goes up in one
// copy) - the weight set of every LDS table, its same-scope flag, the weight set of every big table.  `wset` has one entry per table
// of the call, already checked; share = false never sets a flag (every table computes its own cell index).
struct CountWeightsPack {
    size_t o_ws = 0, o_same = 0, o_wb = 0;
};

inline void count_pack_weights(CountPack &P, int32_t n_tables, const int64_t *scope_off, const int32_t *scope_cols, const int64_t *counts_off,
                               const int32_t *wset, bool share, CountWeightsPack &E) {
    std::vector<int32_t> ws, same, wb;
    std::vector<int> small;
    for (int t = 0; t < n_tables; ++t) {
        if (counts_off[t + 1] - counts_off[t] <= kCountLdsCells) { small.push_back(t); ws.push_back(wset[t]); }
        else wb.push_back(wset[t]);
    }
    same.assign(small.size() + 1, 0);
    for (int g = 0; share && g < P.n_groups; ++g)
        for (int i = P.i32[P.o_gb + (size_t)g] + 1; i < P.i32[P.o_gb + (size_t)g + 1]; ++i) {
            const int a = small[(size_t)i - 1], b = small[(size_t)i];
            const int64_t n = scope_off[a + 1] - scope_off[a];
            same[(size_t)i] = n == scope_off[b + 1] - scope_off[b] && std::equal(scope_cols + scope_off[a], scope_cols + scope_off[a] + n, scope_cols + scope_off[b]);
        }
    ws.push_back(-1);  // (never read: keeps the arrays non-empty)
    wb.push_back(-1);
    auto put = [&](const std::vector<int32_t> &a) { size_t o = P.i32.size(); P.i32.insert(P.i32.end(), a.begin(), a.end()); return o; };
    E.o_ws = put(ws); E.o_same = put(same); E.o_wb = put(wb);
}

// count_launch's twin: the same grids, the weighted kernels; d_weights: the data set's block [n_sets][n_rows]
inline hipError_t count_weighted_launch(hipStream_t stream, const uint8_t *d_codes, int64_t n_rows, const CountPack &P, const CountWeightsPack &E,
                                        const int32_t *d_i32, const int64_t *d_i64, const uint32_t *d_weights, unsigned long long *counts0) {
    if (n_rows > 0 && P.n_big > 0) {
        CountBigWArgs Bg;
        Bg.c.codes = d_codes;
        Bg.c.tbl_begin = d_i32 + P.o_bb;
        Bg.c.tbl_col = d_i32 + P.o_bc;
        Bg.c.tbl_stride = d_i64 + P.o_bs;
        Bg.c.tbl_out = d_i64 + P.o_bo;
        Bg.c.counts = counts0;
        Bg.c.n_rows = n_rows;
        Bg.tbl_wset = d_i32 + E.o_wb;
        Bg.weights = d_weights;
        const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_rows + 255) / 256, 1024));
        hipLaunchKernelGGL(count_big_weighted_kernel, dim3(bx, (unsigned)P.n_big), dim3(256), 0, stream, Bg);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (n_rows > 0 && P.n_small > 0) {
        CountWArgs A;
        A.c.codes = d_codes;
        A.c.tbl_begin = d_i32 + P.o_tb;
        A.c.tbl_col = d_i32 + P.o_tc;
        A.c.tbl_stride = d_i32 + P.o_ts;
        A.c.tbl_lds = d_i32 + P.o_tl;
        A.c.tbl_out = d_i64;
        A.c.grp_begin = d_i32 + P.o_gb;
        A.c.counts = counts0;
        A.c.n_rows = n_rows;
        A.c.n_groups = P.n_groups;
        A.tbl_wset = d_i32 + E.o_ws;
        A.tbl_same = d_i32 + E.o_same;
        A.weights = d_weights;
        const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_rows + 255) / 256, std::max(1, 256 * 8 / std::max(1, P.n_groups))));
        hipLaunchKernelGGL(count_weighted_kernel, dim3(bx, (unsigned)P.n_groups), dim3(256), 0, stream, A);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// mibn_count_tables_w's driver: count_run with every table under the one weight vector (set 0)
inline int count_run_weighted(hipStream_t stream, int64_t n_rows, int32_t n_cols, const uint8_t *codes, bool row_major, const int32_t *card,
                              int32_t n_tables, const int64_t *scope_off, const int32_t *scope_cols, const int64_t *counts_off,
                              const uint32_t *weights, int64_t *counts, std::string &err) {
    CountPack P;
    CountWeightsPack E;
    std::vector<int64_t> sums;
    int rc = count_pack(n_cols, card, n_tables, scope_off, scope_cols, counts_off, P, err);
    if (rc != MIBN_OK) return rc;
    if ((rc = weight_sums(weights, 1, n_rows, sums, err)) != MIBN_OK) return rc;
    const std::vector<int32_t> wset((size_t)std::max(1, n_tables), 0);
    count_pack_weights(P, n_tables, scope_off, scope_cols, counts_off, wset.data(), true, E);
    const size_t total = (size_t)std::max<int64_t>(1, counts_off[n_tables] - counts_off[0]);
    const size_t code_bytes = (size_t)n_rows * (size_t)n_cols;
    DevBuf<uint8_t> d_codes, d_rows;
    DevBuf<int32_t> d_i32;
    DevBuf<int64_t> d_i64;
    DevBuf<uint32_t> d_w;
    DevBuf<unsigned long long> d_counts;
    std::vector<unsigned long long> host(total);
    hipError_t e = d_codes.reset(std::max<size_t>(16, code_bytes));
    if (e == hipSuccess) e = d_i32.reset(P.i32.size());
    if (e == hipSuccess) e = d_i64.reset(std::max<size_t>(1, P.i64.size()));
    if (e == hipSuccess) e = d_w.reset((size_t)std::max<int64_t>(1, n_rows));
    if (e == hipSuccess) e = d_counts.reset(total);
    if (e == hipSuccess && row_major && code_bytes) e = d_rows.reset(code_bytes);
    if (e == hipSuccess) e = count_upload_codes(stream, n_rows, n_cols, codes, row_major, d_codes, d_rows);
    if (e == hipSuccess) e = hipMemcpyAsync(d_i32, P.i32.data(), 4 * P.i32.size(), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && !P.i64.empty()) e = hipMemcpyAsync(d_i64, P.i64.data(), 8 * P.i64.size(), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && n_rows) e = hipMemcpyAsync(d_w, weights, 4 * (size_t)n_rows, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, 8 * total, stream);
    if (e == hipSuccess) e = count_weighted_launch(stream, d_codes, n_rows, P, E, d_i32, d_i64, d_w, d_counts - counts_off[0]);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_counts, 8 * total, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { err = std::string("count: ") + hipGetErrorString(e); return MIBN_E_HIP; }
    for (int64_t i = 0; i < counts_off[n_tables] - counts_off[0]; ++i) counts[i] = (int64_t)host[(size_t)i];
    return MIBN_OK;
}

}  // namespace mibn
