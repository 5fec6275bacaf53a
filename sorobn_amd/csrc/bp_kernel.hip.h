// Loopy belief propagation on gfx950 (mibn_bp_batch): sum-product message passing on the factor graph of the CPTs, flooding schedule,
// fp64.  One workgroup per request, every iteration in ONE launch:
//     phase 1   nu_e   = lambda_u * prod of the other mu^(t-1) at u, normalised          work item: edge, strided over the workgroup
//     barrier
//     phase 2   mu^t_e = sum over the factor's cells of f * prod of the other nu, normalised, damped; r = max |mu^t - mu^(t-1)|
//     reduce    r and the zero-mass flag over the workgroup: DPP-free butterfly in the wave, one LDS slot per wave, barrier
//     swap
// and every lane leaves the loop on the same r <= tol.  Addition and multiplication orders are the ones include/mibn.h pins (ascending
// edge, ascending cell, ascending state) and contraction into FMAs is off in this file's arithmetic, so a request's result is the same
// bits alone or in any batch, in either memory form, and equals the numpy twin's (tests/bp_check.py) up to the division's last bit.
// The message arrays live where bp_plan.h's form says: in dynamic LDS (MsgLds) or in the request's slab of the arena (MsgGlobal); one
// body serves both.  CPTs, edge records and the request's evidence come from global memory: they are shared by every request of the
// launch and stay in L2.  No atomics, no arrays in registers (no scratch).
#pragma once
#include <hip/hip_runtime.h>

#include "bp_plan.h"

namespace mibn {

struct BpArgs {
    const double *pool;
    const BpEdge *edges;
    const BpVar *vars;
    const int32_t *nbr_moff;   // flattened N(v): the moff of each neighbour edge (an edge's moff names it: every edge has cells)
    const int64_t *e_off;      // [n + 1], relative to this launch's e_vars / e_codes
    const int32_t *e_vars, *e_codes;
    const int64_t *l_off;      // [n + 1] over l_vars, or null: no findings
    const int32_t *l_vars;
    const int64_t *v_off;      // [findings + 1] over values
    const double *values;
    unsigned char *slabs;      // MsgGlobal
    size_t slab_bytes;
    double *beliefs;           // [n][lam_cells]
    int32_t *iterations;       // [n]
    double *residual;          // [n]
    int32_t n_vars, n_edges, cells, lam_cells, max_iterations;
    double tol, damping;
};

// max of r and any of z over the workgroup, the same in every lane.  Between two calls there must be a barrier (the slots are reused).
__device__ __forceinline__ void bp_reduce(double &r, bool &z, double *red, int *zred) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(r, m, 64);
        r = o > r ? o : r;
    }
    const bool any = __ballot(z) != 0;
    if (lane == 0) { red[wave] = r; zred[wave] = any; }
    __syncthreads();
    r = red[0];
    z = zred[0] != 0;
    for (int w = 1; w < n_waves; ++w) {
        r = red[w] > r ? red[w] : r;
        z = z || zred[w] != 0;
    }
}

template <bool LDS>
__global__ __launch_bounds__(64 * kBpMaxWaves) void bp_kernel(const BpArgs A) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BpLayout<size_t> L = bp_layout<size_t>((size_t)A.cells, (size_t)A.lam_cells);
    const size_t req = blockIdx.x;
    unsigned char *base = LDS ? smem : A.slabs + req * A.slab_bytes;
    double *mu_prev = reinterpret_cast<double *>(base + L.mu0);
    double *mu_next = reinterpret_cast<double *>(base + L.mu1);
    double *nu = reinterpret_cast<double *>(base + L.nu);
    double *lam = reinterpret_cast<double *>(base + L.lam);
    double *red = reinterpret_cast<double *>(smem + (LDS ? L.red : 0));
    int *zred = reinterpret_cast<int *>(red + kBpMaxWaves);
    const int tid = threadIdx.x, nt = blockDim.x;
    double *out = A.beliefs + req * (size_t)A.lam_cells;

    // lambda = 1, mu^0 = 1 / card; then the request's evidence (one-hot; a code outside the domain: all zeros) and findings
    for (int i = tid; i < A.lam_cells; i += nt) lam[i] = 1.0;
    for (int e = tid; e < A.n_edges; e += nt) {
        const BpEdge E = A.edges[e];
        const double u = 1.0 / (double)E.card;
        for (int x = 0; x < E.card; ++x) mu_prev[E.moff + x] = u;
    }
    __syncthreads();
    {
        const int64_t e0 = A.e_off[req], e1 = A.e_off[req + 1];
        for (int64_t i = e0 + tid; i < e1; i += nt) {
            const BpVar V = A.vars[A.e_vars[i]];
            const int c = A.e_codes[i];
            for (int x = 0; x < V.card; ++x) lam[V.loff + x] = x == c ? 1.0 : 0.0;
        }
        if (A.l_off) {
            const int64_t l0 = A.l_off[req], l1 = A.l_off[req + 1];
            for (int64_t k = l0 + tid; k < l1; k += nt) {
                const BpVar V = A.vars[A.l_vars[k]];
                const double *w = A.values + A.v_off[k];
                for (int x = 0; x < V.card; ++x) lam[V.loff + x] = w[x];
            }
        }
    }
    __syncthreads();
    double r = 0.0;
    bool z = false;
    for (int v = tid; v < A.n_vars; v += nt) {
        const BpVar V = A.vars[v];
        double s = 0.0;
        for (int x = 0; x < V.card; ++x) s += lam[V.loff + x];
        z = z || s == 0.0;
    }
    bp_reduce(r, z, red, zred);
    int it = 0;
    if (!z) {
        for (it = 1;; ++it) {
            // ---- phase 1: variable -> factor
            for (int e = tid; e < A.n_edges; e += nt) {
                const BpEdge E = A.edges[e];
                const BpVar V = A.vars[E.var];
                double s = 0.0;
                for (int x = 0; x < E.card; ++x) {
                    double p = lam[E.loff + x];
                    for (int i = 0; i < V.nb_len; ++i) {
                        const int mo = A.nbr_moff[V.nb_begin + i];
                        if (mo != E.moff) p *= mu_prev[mo + x];
                    }
                    nu[E.moff + x] = p;
                    s += p;
                }
                if (s == 0.0) z = true;
                else
                    for (int x = 0; x < E.card; ++x) nu[E.moff + x] = nu[E.moff + x] / s;
            }
            __syncthreads();
            // ---- phase 2: factor -> variable, damping, residual
            r = 0.0;
            for (int e = tid; e < A.n_edges; e += nt) {
                const BpEdge E = A.edges[e];
                const BpVar F = A.vars[E.factor];
                const double *table = A.pool + F.table_off;
                const int span = E.stride * E.card, n_hi = F.table_cells / span;
                double s = 0.0;
                for (int x = 0; x < E.card; ++x) {
                    double acc = 0.0;
                    for (int hi = 0; hi < n_hi; ++hi)
                        for (int lo = 0; lo < E.stride; ++lo) {
                            const int c = hi * span + x * E.stride + lo;
                            double t = table[c];
                            for (int j = 0; j < F.scope_len; ++j) {
                                if (j == E.pos) continue;
                                const BpEdge J = A.edges[F.edge_begin + j];
                                t *= nu[J.moff + (c / J.stride) % J.card];
                            }
                            acc += t;
                        }
                    mu_next[E.moff + x] = acc;
                    s += acc;
                }
                if (s == 0.0) {
                    z = true;
                    continue;
                }
                for (int x = 0; x < E.card; ++x) {
                    const double prev = mu_prev[E.moff + x];
                    double m = mu_next[E.moff + x] / s;
                    if (A.damping > 0.0) m = (1.0 - A.damping) * m + A.damping * prev;
                    mu_next[E.moff + x] = m;
                    const double d = fabs(m - prev);
                    r = d > r ? d : r;
                }
            }
            bp_reduce(r, z, red, zred);  // (its barrier also orders this step's mu before the next step's reads)
            double *t = mu_prev; mu_prev = mu_next; mu_next = t;
            if (z || r <= A.tol || it == A.max_iterations) break;  // the same in every lane
        }
    }
    // ---- beliefs (a request without mass: zeros)
    if (!z) {
        for (int v = tid; v < A.n_vars; v += nt) {
            const BpVar V = A.vars[v];
            double s = 0.0;
            for (int x = 0; x < V.card; ++x) {
                double p = lam[V.loff + x];
                for (int i = 0; i < V.nb_len; ++i) p *= mu_prev[A.nbr_moff[V.nb_begin + i] + x];
                out[V.loff + x] = p;
                s += p;
            }
            if (s == 0.0) z = true;
            else
                for (int x = 0; x < V.card; ++x) out[V.loff + x] = out[V.loff + x] / s;
        }
        __syncthreads();
        double unused = 0.0;
        bp_reduce(unused, z, red, zred);
    }
    if (z) {
        for (int i = tid; i < A.lam_cells; i += nt) out[i] = 0.0;
        r = 0.0;
    }
    if (tid == 0) {
        A.iterations[req] = it;
        A.residual[req] = r;
    }
}

typedef void (*BpKernel)(const BpArgs);
inline BpKernel bp_kernel_of(BpForm form) { return form == BpForm::MsgLds ? bp_kernel<true> : bp_kernel<false>; }

// dynamic LDS of a launch: the whole state, or the reduction slots alone
inline size_t bp_lds_bytes(const BpPlan &P) { return P.form == BpForm::MsgLds ? P.lds.total : kBpRedBytes; }

}  // namespace mibn
