// Loopy belief propagation on gfx950 (mibn_bp_batch, mibn_bp_mpe_batch): message passing on the factor graph of the CPTs, flooding
// schedule, fp64.  One workgroup per request, every iteration in ONE launch:
//     phase 1   nu_e   = lambda_u * prod of the other mu^(t-1) at u, normalised          work item: edge, strided over the workgroup
//     barrier
//     phase 2   mu^t_e = sum (bp_kernel) or max (bp_max_kernel) over the factor's cells of f * prod of the other nu, normalised, damped;
//               r = max |mu^t - mu^(t-1)|
//     reduce    r and the zero-mass flag over the workgroup: DPP-free butterfly in the wave, one LDS slot per wave, barrier
//     swap
// and every lane leaves the loop on the same r <= tol.  Addition and multiplication orders are the ones include/mibn.h pins (ascending
// edge, ascending cell, ascending state) and contraction into FMAs is off in this file's arithmetic, so a request's result is the same
// bits alone or in any batch, in either memory form, and equals the numpy twin's (tests/bp_check.py) up to the division's last bit.
// The message arrays live where bp_plan.h's form says: in dynamic LDS (MsgLds) or in the request's slab of the arena (MsgGlobal); one
// body serves both.  CPTs, edge records and the request's evidence come from global memory: they are shared by every request of the
// launch and stay in L2.  No atomics, no arrays in registers (no scratch).
//
// bp_start, bp_phase1 and bp_phase2 are the ONE copy of the start and of the two message phases; both kernels are made of them.
// bp_max_kernel adds, after the reduce of every step, the decoder of include/mibn.h - max-marginals, decode, score in the pinned order,
// keep the best candidate - and after the loop the polish (iterated conditional modes, colour by colour) and the final score.
// bp_evidence_kernel adds, after bp_kernel's loop, the final phase of mibn_bp_evidence_batch: the Bethe log Z and the family beliefs.
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
    double *beliefs;           // [n][lam_cells]  (bp_kernel)
    int32_t *iterations;       // [n]
    double *residual;          // [n]
    int32_t n_vars, n_edges, cells, lam_cells, max_iterations;
    double tol, damping;
};

// what bp_max_kernel takes besides
struct BpMaxArgs {
    BpArgs bp;
    const int32_t *nbr;        // flattened N(v): edge numbers
    const int32_t *col_off;    // [n_colours + 1] over col_members
    const int32_t *col_members;
    int32_t n_colours, polish_sweeps;
    int32_t *codes;            // [n][n_vars]
    double *log_p;             // [n]
    int32_t *info;             // [n][3]: best_iteration, sweeps run, moves made
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

// the sum of m over the workgroup, the same in every lane (integers: any order).  Slots and barrier rule as bp_reduce.
__device__ __forceinline__ int bp_reduce_sum(int m, int *slots) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) m += __shfl_xor(m, k, 64);
    if (lane == 0) slots[wave] = m;
    __syncthreads();
    int s = slots[0];
    for (int w = 1; w < n_waves; ++w) s += slots[w];
    return s;
}

// lambda = 1, mu^0 = 1 / card; then the request's evidence (one-hot; a code outside the domain: all zeros) and findings; z: some
// lambda has no mass
__device__ __forceinline__ void bp_start(const BpArgs &A, size_t req, double *mu_prev, double *lam, double *red, int *zred, bool &z) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x;
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
    z = false;
    for (int v = tid; v < A.n_vars; v += nt) {
        const BpVar V = A.vars[v];
        double s = 0.0;
        for (int x = 0; x < V.card; ++x) s += lam[V.loff + x];
        z = z || s == 0.0;
    }
    bp_reduce(r, z, red, zred);
}

// ---- phase 1: variable -> factor
__device__ __forceinline__ void bp_phase1(const BpArgs &A, const double *lam, const double *mu_prev, double *nu, bool &z) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x;
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
}

// ---- phase 2: factor -> variable (MAX: the maximum over the cells in place of their sum), damping, residual
template <bool MAX>
__device__ __forceinline__ void bp_phase2(const BpArgs &A, const double *mu_prev, double *mu_next, const double *nu, double &r, bool &z) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x;
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
                    if (MAX) acc = t > acc ? t : acc;
                    else acc += t;
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

    double r = 0.0;
    bool z = false;
    bp_start(A, req, mu_prev, lam, red, zred, z);
    int it = 0;
    if (!z) {
        for (it = 1;; ++it) {
            bp_phase1(A, lam, mu_prev, nu, z);
            __syncthreads();
            bp_phase2<false>(A, mu_prev, mu_next, nu, r, z);
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

// ------------------------------------------------------------------------------------------------------------------ the decoder
// The score of `codes` in the order include/mibn.h pins: term_v parallel over the variables, the 64 partials by wave 0, their sum by
// lane 0, every lane reads it from `slot`.  Starts after a barrier that made `codes` visible; ends with one.
__device__ __forceinline__ double bp_score(const BpArgs &A, const double *lam, const int32_t *codes, double *term, double *part, double *slot) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int v = tid; v < A.n_vars; v += nt) {
        const BpVar V = A.vars[v];
        int cell = 0;
        for (int j = 0; j < V.scope_len; ++j) {
            const BpEdge J = A.edges[V.edge_begin + j];
            cell += codes[J.var] * J.stride;
        }
        term[v] = log(A.pool[V.table_off + cell]) + log(lam[V.loff + codes[v]]);
    }
    __syncthreads();
    if (tid < kBpScoreLanes) {
        double s = 0.0;
        for (int v = tid; v < A.n_vars; v += kBpScoreLanes) s += term[v];
        part[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s = part[0];
        for (int l = 1; l < kBpScoreLanes; ++l) s += part[l];
        *slot = s;
    }
    __syncthreads();
    return *slot;
}

template <bool LDS>
__global__ __launch_bounds__(64 * kBpMaxWaves) void bp_max_kernel(const BpMaxArgs M) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BpArgs &A = M.bp;
    const BpMpeLayout<size_t> L = bp_mpe_layout<size_t>((size_t)A.cells, (size_t)A.lam_cells, (size_t)A.n_vars);
    const size_t req = blockIdx.x;
    unsigned char *base = LDS ? smem : A.slabs + req * A.slab_bytes;
    double *mu_prev = reinterpret_cast<double *>(base + L.mu0);
    double *mu_next = reinterpret_cast<double *>(base + L.mu1);
    double *nu = reinterpret_cast<double *>(base + L.nu);
    double *lam = reinterpret_cast<double *>(base + L.lam);
    double *term = reinterpret_cast<double *>(base + L.term);
    double *part = reinterpret_cast<double *>(base + L.part);
    int32_t *cur = reinterpret_cast<int32_t *>(base + L.cur);
    int32_t *kept = reinterpret_cast<int32_t *>(base + L.kept);
    double *red = reinterpret_cast<double *>(smem + (LDS ? L.red : 0));
    int *zred = reinterpret_cast<int *>(red + kBpMaxWaves);
    double *dred = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(red) + kBpRedBytes);  // the decoder's own slots
    int *dslots = reinterpret_cast<int *>(dred + kBpMaxWaves);
    double *slot = reinterpret_cast<double *>(dslots + kBpMaxWaves);
    const int tid = threadIdx.x, nt = blockDim.x;
    int32_t *out = M.codes + req * (size_t)A.n_vars;

    double r = 0.0, best = 0.0;
    bool z = false;
    bp_start(A, req, mu_prev, lam, red, zred, z);
    int it = 0, best_it = 0, sweeps = 0, moves = 0;
    if (!z) {
        for (it = 1;; ++it) {
            bp_phase1(A, lam, mu_prev, nu, z);
            __syncthreads();
            bp_phase2<true>(A, mu_prev, mu_next, nu, r, z);
            bp_reduce(r, z, red, zred);
            double *t = mu_prev; mu_prev = mu_next; mu_next = t;
            if (z) break;
            // ---- max-marginals and decode: the lowest state of maximal lambda * prod mu, compared before the division
            bool zd = false;
            for (int v = tid; v < A.n_vars; v += nt) {
                const BpVar V = A.vars[v];
                double s = 0.0, top = -1.0;
                int arg = 0;
                for (int x = 0; x < V.card; ++x) {
                    double p = lam[V.loff + x];
                    for (int i = 0; i < V.nb_len; ++i) p *= mu_prev[A.nbr_moff[V.nb_begin + i] + x];
                    s += p;
                    if (p > top) { top = p; arg = x; }
                }
                zd = zd || s == 0.0;
                cur[v] = arg;
            }
            double unused = 0.0;
            bp_reduce(unused, zd, dred, dslots);  // (its barrier publishes cur)
            if (zd) { z = true; break; }
            const double sc = bp_score(A, lam, cur, term, part, slot);
            if (it == 1 || sc > best) {  // the same in every lane: all read one slot
                best = sc;
                best_it = it;
                for (int v = tid; v < A.n_vars; v += nt) kept[v] = cur[v];  // (the lane that decoded v)
            }
            if (r <= A.tol || it == A.max_iterations) break;
        }
    }
    if (!z) {
        __syncthreads();
        // ---- polish: iterated conditional modes on the kept candidate, colour by colour
        for (int s = 1; s <= M.polish_sweeps; ++s) {
            int moved = 0;
            for (int c = 0; c < M.n_colours; ++c) {
                for (int i = M.col_off[c] + tid; i < M.col_off[c + 1]; i += nt) {
                    const int v = M.col_members[i];
                    const BpVar V = A.vars[v];
                    const int now = kept[v];
                    double top = -1.0, at_now = 0.0;
                    int arg = 0;
                    for (int x = 0; x < V.card; ++x) {
                        double p = lam[V.loff + x];
                        for (int k = 0; k < V.nb_len; ++k) {
                            const BpEdge E = A.edges[M.nbr[V.nb_begin + k]];
                            const BpVar F = A.vars[E.factor];
                            int cell = x * E.stride;
                            for (int j = 0; j < F.scope_len; ++j) {
                                if (j == E.pos) continue;
                                const BpEdge J = A.edges[F.edge_begin + j];
                                cell += kept[J.var] * J.stride;
                            }
                            p *= A.pool[F.table_off + cell];
                        }
                        if (p > top) { top = p; arg = x; }
                        if (x == now) at_now = p;
                    }
                    if (top > at_now) { kept[v] = arg; ++moved; }
                }
                __syncthreads();
            }
            moved = bp_reduce_sum(moved, dslots);
            sweeps = s;
            moves += moved;
            if (moved == 0) break;  // the same in every lane
        }
        best = bp_score(A, lam, kept, term, part, slot);
        for (int v = tid; v < A.n_vars; v += nt) out[v] = kept[v];
    } else {
        // no mass: -1 everywhere, then the evidence as it was given
        for (int v = tid; v < A.n_vars; v += nt) out[v] = -1;
        __syncthreads();
        const int64_t e0 = A.e_off[req], e1 = A.e_off[req + 1];
        for (int64_t i = e0 + tid; i < e1; i += nt) out[A.e_vars[i]] = A.e_codes[i];
        r = 0.0;
        best = -INFINITY;
        best_it = 0;
    }
    if (tid == 0) {
        A.iterations[req] = it;
        A.residual[req] = r;
        M.log_p[req] = best;
        M.info[req * 3 + 0] = best_it;
        M.info[req * 3 + 1] = sweeps;
        M.info[req * 3 + 2] = moves;
    }
}

// ------------------------------------------------------------------------------------------- Bethe log Z and family beliefs
// bp_evidence_kernel: bp_kernel's loop, then the final phase include/mibn.h pins for mibn_bp_evidence_batch - nu* from the final mu,
// then a lane per variable v for Z_(f_v) (every cell of the factor, ascending), Z_v with v's belief, the Z_e of factor v's edges and
// term_v; the 64 partials and their sum as in bp_score; and the family-belief cells, a wave per factor and a lane per cell, each
// recomputing its t_c in the pinned order and dividing by the published Z_f.
struct BpEvArgs {
    BpArgs bp;                 // beliefs may be null
    const int32_t *foff;       // [n_vars + 1]: factor v's cells in a family-belief row
    int32_t fcells;
    double *log_z;             // [n]
    double *fbeliefs;          // [n][fcells] or null
};

// t_c of factor F: f[c] times nu_(f,j)(c_j) for ascending j
__device__ __forceinline__ double bp_family_cell(const BpArgs &A, const BpVar &F, const double *nu, int c) {
#pragma clang fp contract(off)
    double t = A.pool[F.table_off + c];
    for (int j = 0; j < F.scope_len; ++j) {
        const BpEdge J = A.edges[F.edge_begin + j];
        t *= nu[J.moff + (c / J.stride) % J.card];
    }
    return t;
}

template <bool LDS>
__global__ __launch_bounds__(64 * kBpMaxWaves) void bp_evidence_kernel(const BpEvArgs M) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const BpArgs &A = M.bp;
    const BpEvLayout<size_t> L = bp_ev_layout<size_t>((size_t)A.cells, (size_t)A.lam_cells, (size_t)A.n_vars);
    const size_t req = blockIdx.x;
    unsigned char *base = LDS ? smem : A.slabs + req * A.slab_bytes;
    double *mu_prev = reinterpret_cast<double *>(base + L.mu0);
    double *mu_next = reinterpret_cast<double *>(base + L.mu1);
    double *nu = reinterpret_cast<double *>(base + L.nu);
    double *lam = reinterpret_cast<double *>(base + L.lam);
    double *zf = reinterpret_cast<double *>(base + L.zf);
    double *term = reinterpret_cast<double *>(base + L.term);
    double *part = reinterpret_cast<double *>(base + L.part);
    double *red = reinterpret_cast<double *>(smem + (LDS ? L.red : 0));
    int *zred = reinterpret_cast<int *>(red + kBpMaxWaves);
    double *fred = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(red) + kBpRedBytes);  // the final phase's own slots
    int *fzred = reinterpret_cast<int *>(fred + kBpMaxWaves);
    const int tid = threadIdx.x, nt = blockDim.x;
    double *out = A.beliefs ? A.beliefs + req * (size_t)A.lam_cells : nullptr;
    double *fout = M.fbeliefs ? M.fbeliefs + req * (size_t)M.fcells : nullptr;

    double r = 0.0;
    bool z = false;
    bp_start(A, req, mu_prev, lam, red, zred, z);
    int it = 0;
    if (!z) {
        for (it = 1;; ++it) {
            bp_phase1(A, lam, mu_prev, nu, z);
            __syncthreads();
            bp_phase2<false>(A, mu_prev, mu_next, nu, r, z);
            bp_reduce(r, z, red, zred);
            double *t = mu_prev; mu_prev = mu_next; mu_next = t;
            if (z || r <= A.tol || it == A.max_iterations) break;  // the same in every lane
        }
    }
    if (!z) {
        // ---- final phase 1: nu* from the final mu
        bp_phase1(A, lam, mu_prev, nu, z);
        __syncthreads();
        for (int v = tid; v < A.n_vars; v += nt) {
            const BpVar V = A.vars[v];
            double s = 0.0;  // Z_f of factor v
            for (int c = 0; c < V.table_cells; ++c) s += bp_family_cell(A, V, nu, c);
            zf[v] = s;
            z = z || s == 0.0;
            double tv = log(s);
            s = 0.0;  // Z_v, and v's belief as bp_kernel forms it
            for (int x = 0; x < V.card; ++x) {
                double p = lam[V.loff + x];
                for (int i = 0; i < V.nb_len; ++i) p *= mu_prev[A.nbr_moff[V.nb_begin + i] + x];
                if (out) out[V.loff + x] = p;
                s += p;
            }
            z = z || s == 0.0;
            if (out && s != 0.0)
                for (int x = 0; x < V.card; ++x) out[V.loff + x] = out[V.loff + x] / s;
            tv += log(s);
            for (int j = 0; j < V.scope_len; ++j) {  // Z_e of the edges of factor v
                const BpEdge J = A.edges[V.edge_begin + j];
                s = 0.0;
                for (int x = 0; x < J.card; ++x) s += mu_prev[J.moff + x] * nu[J.moff + x];
                z = z || s == 0.0;
                tv -= log(s);
            }
            term[v] = tv;
        }
        double unused = 0.0;
        bp_reduce(unused, z, fred, fzred);  // (its barrier publishes zf and term)
    }
    double log_z = -INFINITY;
    if (!z) {
        if (tid < kBpScoreLanes) {
            double s = 0.0;
            for (int v = tid; v < A.n_vars; v += kBpScoreLanes) s += term[v];
            part[tid] = s;
        }
        __syncthreads();
        if (tid == 0) {
            log_z = part[0];
            for (int l = 1; l < kBpScoreLanes; ++l) log_z += part[l];
        }
        if (fout) {
            const int lane = tid & 63, wave = tid >> 6, n_waves = (nt + 63) >> 6;
            for (int v = wave; v < A.n_vars; v += n_waves) {
                const BpVar V = A.vars[v];
                const double s = zf[v];
                for (int c = lane; c < V.table_cells; c += 64) fout[M.foff[v] + c] = bp_family_cell(A, V, nu, c) / s;
            }
        }
    } else {
        if (out)
            for (int i = tid; i < A.lam_cells; i += nt) out[i] = 0.0;
        if (fout)
            for (int i = tid; i < M.fcells; i += nt) fout[i] = 0.0;
        r = 0.0;
    }
    if (tid == 0) {
        A.iterations[req] = it;
        A.residual[req] = r;
        M.log_z[req] = log_z;
    }
}

// acc[c] = acc[c] + weight[b] * b_f(c) for the launch's requests b ascending, one addition after the other: a lane per cell
__global__ __launch_bounds__(256) void bp_accumulate_kernel(double *acc, const double *fbeliefs, const double *weight, int64_t n, int32_t fcells) {
#pragma clang fp contract(off)
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= fcells) return;
    double a = acc[c];
    for (int64_t b = 0; b < n; ++b) a = a + (weight ? weight[b] : 1.0) * fbeliefs[b * fcells + c];
    acc[c] = a;
}

typedef void (*BpKernel)(const BpArgs);
typedef void (*BpEvKernel)(const BpEvArgs);
inline BpEvKernel bp_evidence_kernel_of(BpForm form) { return form == BpForm::MsgLds ? bp_evidence_kernel<true> : bp_evidence_kernel<false>; }
inline size_t bp_lds_bytes(const BpEvPlan &E) { return E.form == BpForm::MsgLds ? E.lds.total : kBpEvRedBytes; }
inline BpKernel bp_kernel_of(BpForm form) { return form == BpForm::MsgLds ? bp_kernel<true> : bp_kernel<false>; }
typedef void (*BpMaxKernel)(const BpMaxArgs);
inline BpMaxKernel bp_max_kernel_of(BpForm form) { return form == BpForm::MsgLds ? bp_max_kernel<true> : bp_max_kernel<false>; }

// dynamic LDS of a launch: the whole state, or the reduction slots alone
inline size_t bp_lds_bytes(const BpPlan &P) { return P.form == BpForm::MsgLds ? P.lds.total : kBpRedBytes; }
inline size_t bp_lds_bytes(const BpMpePlan &M) { return M.form == BpForm::MsgLds ? M.lds.total : kBpMpeRedBytes; }

}  // namespace mibn
