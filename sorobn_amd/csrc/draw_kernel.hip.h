// CDNA4 (gfx950) kernels of exact posterior sampling (mibn_posterior_sample_batch): forward filtering, backward sampling.
//
// A draw program (planner.h, "DRAW programs") is a GENERIC-only sum program whose intermediates all stay in the arena.
// `ve_sum_kernel` (elim_kernel.hip.h) runs one level of its schedule - the level body of the step-wise kinds around the level
// kernel's own step code with MAX = false; the FINAL step carries the RAW flag, so segment_wave leaves the mass of the evidence as
// it is.
//
// `posterior_draw_kernel` then walks the request's draw record once per sample: ONE SAMPLE PER LANE.  A request has thousands of
// samples and the walk is a chain of dependent gathers (the value just drawn addresses the next table), so occupancy is the only
// latency hiding there is.  A workgroup serves samples of one request: the record is wave-uniform and is read with scalar loads
// straight from the program buffer (staging its ~30 KB for a 10 x 10 grid in LDS would cost more occupancy than the scalar
// cache misses it saves: the state below is what the LDS is for), the lanes' codes live in LDS as state[var][lane] (bytes when
// every cardinality fits, else 16 bits), tables are read with plain global loads (read-only here, L2-resident after the first
// wave for all but the largest frontier tables) and the finished rows leave through coalesced vector stores.  No atomics, no
// scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "elim_kernel.hip.h"
#include "gibbs_kernel.hip.h"

namespace mibn {

constexpr int kDrawWG = 256;  // samples per workgroup: four waves share one staging of the evidence and one row write-out

struct DrawItem {
    uint32_t req;    // request index within the wave
    uint32_t count;  // samples of this workgroup, <= kDrawWG
    uint64_t g;      // global row index of its first sample: the Philox counter
    uint64_t row;    // its first row in `codes`
};

struct DrawArgs {
    const uint32_t *prog;       // the chunk's draw programs (each followed by its draw record)
    const uint64_t *prog_off;   // word offset of request i's program
    const uint64_t *arena_off;  // offset (doubles) of request i's arena (its kept tables)
    const double *arena;
    const double *pool;         // the CPTs
    const double *m;            // m[i] = the mass of request i's evidence: its FINAL cell (1 for a program without steps)
    const DrawItem *items;
    int32_t *codes;             // [rows][n_vars]
    int32_t n_vars;
    uint32_t k0, k1;            // Philox key (the key of mibn_sample)
};

// w_x = prod_j phi_j[base_j + x * xs_j] in input order, rounded after every product (no contraction: the host twin,
// tools/prog_sim.cpp draw, computes the same bits)
template <int NIN>
__device__ __forceinline__ double draw_weight(const double *const (&tab)[kMaxIn], const int64_t (&base)[kMaxIn], const int64_t (&xs)[kMaxIn],
                                              const int n_in, const int x) {
    double w = tab[0][base[0] + (int64_t)x * xs[0]];
#pragma unroll
    for (int j = 1; j < NIN; ++j)
        if (j < n_in) w = __dmul_rn(w, tab[j][base[j] + (int64_t)x * xs[j]]);
    return w;
}

// Per sample: codes of the evidence, then per record entry (backward entries, last eliminated first, then forward entries in id
// order)  x ~ w_x / total:  total = sum_x w_x in code order, u = uniform(g, 2 + x) * total against the running sum, the first x
// with u < acc, else (rounding) the last x of positive weight.  Mass 0 gives -1 for every non-evidence variable; so does a
// total that is not positive (cannot happen at positive mass: an internal error, never a draw).
template <typename ST>
__global__ __launch_bounds__(kDrawWG) void posterior_draw_kernel(const DrawArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char draw_smem[];
    ST *st = reinterpret_cast<ST *>(draw_smem);  // [n_vars][kDrawWG]
    const int lane = threadIdx.x;
    const int n = A.n_vars;
    const DrawItem it = A.items[blockIdx.x];
    const uint32_t r = it.req;
    const uint32_t *p = A.prog + A.prog_off[r];
    // (record_offset(p), written out: through the helper the compiler orders a few independent instructions of this kernel
    //  differently, and the kernel is to stay instruction for instruction what the recorded profiles measured)
    const uint32_t n_steps = p[0];
    uint64_t off = 1;
    for (uint32_t s = 0; s < n_steps; ++s) off += p[off + 6];
    const uint32_t *rec = p + off;
    const uint32_t n_ent = rec[0] + rec[1], n_ev = rec[2];
    rec += 3;
    const double m = A.m[r];
    bool bad = !(m > 0.0);
    for (int v = 0; v < n; ++v) st[v * kDrawWG + lane] = (ST)0;
    for (uint32_t k = 0; k < n_ev; ++k) {
        const uint32_t v = rec[2 * k];
        if (v < (uint32_t)n) st[v * kDrawWG + lane] = (ST)rec[2 * k + 1];
    }
    const uint32_t *ev_rec = rec;
    rec += 2 * n_ev;
    if (!bad) {  // (wave-uniform: m belongs to the request)
        const double *arena = A.arena + A.arena_off[r];
        const uint64_t g = it.g + (uint64_t)lane;
        for (uint32_t e = 0; e < n_ent; ++e) {
            const int x = (int)rec[0], cx = (int)rec[1], n_in = (int)rec[2];
            rec += 3;
            const double *tab[kMaxIn];
            int64_t base[kMaxIn], xs[kMaxIn];
#pragma unroll
            for (int j = 0; j < kMaxIn; ++j) {
                tab[j] = A.pool;
                base[j] = 0;
                xs[j] = 0;
                if (j < n_in) {
                    const uint64_t o = (uint64_t)rec[0] | ((uint64_t)rec[1] << 32);
                    tab[j] = (o & kConstFlag) ? A.pool + (o & ~kConstFlag) : arena + o;
                    xs[j] = (int64_t)rec[2];
                    const uint32_t n_ax = rec[3];
                    int64_t idx = 0;
                    for (uint32_t a = 0; a < n_ax; ++a) idx += (int64_t)st[rec[4 + 2 * a] * kDrawWG + lane] * (int64_t)rec[5 + 2 * a];
                    base[j] = idx;
                    rec += 4 + 2 * n_ax;
                }
            }
            double total = 0.0, acc = 0.0;
            int val = -1, last_pos = 0;
            const double u01 = philox_uniform(g, 2u + (uint32_t)x, A.k0, A.k1);
            if (cx <= 4) {  // the weights stay in registers
                double w[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) w[c] = c < cx ? draw_weight<kMaxIn>(tab, base, xs, n_in, c) : 0.0;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < cx) total = __dadd_rn(total, w[c]);
                const double u = __dmul_rn(u01, total);
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < cx) {
                        acc = __dadd_rn(acc, w[c]);
                        if (w[c] > 0.0) last_pos = c;
                        if (val < 0 && u < acc) val = c;
                    }
            } else {  // two passes over the same loads: the same bits both times
                for (int c = 0; c < cx; ++c) total = __dadd_rn(total, draw_weight<kMaxIn>(tab, base, xs, n_in, c));
                const double u = __dmul_rn(u01, total);
                for (int c = 0; c < cx; ++c) {
                    const double w = draw_weight<kMaxIn>(tab, base, xs, n_in, c);
                    acc = __dadd_rn(acc, w);
                    if (w > 0.0) last_pos = c;
                    if (val < 0 && u < acc) val = c;
                }
            }
            if (val < 0) val = last_pos;
            if (!(total > 0.0)) { bad = true; val = 0; }
            st[x * kDrawWG + lane] = (ST)val;
        }
    }
    // rows out: the workgroup's rows are contiguous in `codes`, consecutive lanes write consecutive words.  A lane's own
    // verdict (`bad`) has to reach whoever writes its row: one flag byte per lane behind the state.
    unsigned char *sh_bad = draw_smem + (size_t)n * kDrawWG * sizeof(ST);
    sh_bad[lane] = bad ? 1 : 0;
    __syncthreads();
    if (n <= 0) return;
    int32_t *out = A.codes + it.row * (uint64_t)n;
    const uint32_t total_words = it.count * (uint32_t)n;
    for (uint32_t i = (uint32_t)lane; i < total_words; i += kDrawWG) {
        const uint32_t s = i / (uint32_t)n, v = i - s * (uint32_t)n;
        int32_t c = (int32_t)st[v * kDrawWG + s];
        if (sh_bad[s]) {  // (evidence keeps its code as given - it may lie outside the domain -, everything else is -1)
            c = -1;
            for (uint32_t k = 0; k < n_ev; ++k)
                if (ev_rec[2 * k] == v) c = (int32_t)ev_rec[2 * k + 1];
        }
        out[i] = c;
    }
}

inline size_t draw_lds_bytes(int n_vars, bool wide) { return (size_t)n_vars * kDrawWG * (wide ? 2 : 1) + kDrawWG; }

}  // namespace mibn
