// CDNA4 (gfx950) kernels of the step-wise program kinds (planner.h: MAX, DRAW and MAP programs): one level body, one traceback.
//
// Such a program is a step program whose every step is GENERIC: the schedule of build_schedule cuts it into SEGMENT items (runs of
// small steps, one wave each) and GENERIC tiles (big steps, one workgroup per tile) exactly like a sum program, and one launch of
// its level kernel runs one level of it.  The step code is the level kernel's own (generic_body); only FIBER / OUTER / CHAIN /
// SWEEP do not exist here - these programs never contain them.  The three level kernels are `elim_level` under three names, one
// per ElimMode (ve_kernel.hip.h):
//   ve_sum_kernel  (mibn_posterior_sample_batch)  draw programs: every step sums (MAX = false); the FINAL step carries the RAW
//                  flag, so segment_wave leaves the mass of the evidence as it is.
//   ve_max_kernel  (mibn_mpe_batch)  max programs: max instead of +, the lowest maximising value of the eliminated variable
//                  stored per output cell in the step's argmax table (MAX = true).
//   ve_map_kernel  (mibn_map_batch, m* = argmax_m sum_h P(m, h, e))  map programs: unflagged steps that sum the hidden variables
//                  out, then steps flagged kFlagMax that maximise the MAP variables out, each with its argmax table.  MAX = true
//                  for a flagged step, MAX = false for every other one (a product-only step has nothing to reduce and takes the
//                  sum body).  The choice is wave-uniform and made per STEP - a segment of a small network holds the whole
//                  program, sums and maxima alike - and per tile in the workgroup path.  The FINAL step, one cell, is never
//                  normalised.
//
// `mpe_traceback_kernel` / `map_traceback_kernel` then decode the assignment from the argmax tables, which never leave the device:
// one wave per request, lane 0 walks the request's traceback record (about one dependent 2-byte load per variable - latency, not
// bandwidth), the codes live in LDS and the wave writes them out with ordinary vector stores - all n_vars of them (MPE), or those
// of the request's MAP variables: the gather list behind the record, in the caller's order, into its slice of the output (MAP).
#pragma once
#include <hip/hip_runtime.h>

#include "ve_kernel.hip.h"

namespace mibn {

// One level of a schedule: workgroup b runs item wg_item[b] - a group of kSegPerWg segments or a tile of a big GENERIC step.
// The segments' descriptor copies and offset tables take the whole 12 KB buffer; a tile uses its first 3 KB.
template <ElimMode M>
__device__ __forceinline__ void elim_level(const LevelArgs &A) {
    __shared__ __attribute__((aligned(16))) unsigned char sh_buf[kSegPerWg * (kMaxStepWords * 4 + kMaxIn * kTileMax * 4)];
    const int tid = threadIdx.x;
    const uint32_t wg = blockIdx.x + A.wg_base;
    const uint32_t item_idx = (uint32_t)uni((int)A.wg_item[wg]);
    Item it;
    it.req = (uint32_t)uni((int)A.items[item_idx].req);
    it.rel_off = (uint32_t)uni((int)A.items[item_idx].rel_off);
    it.a = (uint32_t)uni((int)A.items[item_idx].a);
    it.b = (uint32_t)uni((int)A.items[item_idx].b);
    if (it.a & kItemSegment) {
        segment_wave<M>(A, item_idx, (int)it.b, reinterpret_cast<double *>(sh_buf), tid);
        return;
    }
    uint32_t *sh_step = reinterpret_cast<uint32_t *>(sh_buf);
    int (*sh_hoff)[kTileMax] = reinterpret_cast<int (*)[kTileMax]>(sh_buf + kMaxStepWords * 4);
    const uint64_t ao = A.arena_off[it.req], po = A.prog_off[it.req];
    double *slot = A.arena + (((uint64_t)(uint32_t)uni((int)(ao >> 32)) << 32) | (uint32_t)uni((int)(ao & 0xffffffffu)));
    const uint32_t *p = A.prog + (((uint64_t)(uint32_t)uni((int)(po >> 32)) << 32) | (uint32_t)uni((int)(po & 0xffffffffu))) + it.rel_off;
    const int words = (int)p[6];
    for (int i = tid; i < words; i += kWG) sh_step[i] = p[i];
    __syncthreads();
    const int h0 = (int)((wg - it.b) * it.a);
    const int h1 = min((int)sh_step[3], h0 + (int)it.a);
    if (M == ElimMode::Max || (M == ElimMode::Map && ((sh_step[1] >> 16) & kFlagMax)))
        generic_dispatch<kWG, true>((sh_step[0] >> 8) & 0xff, sh_step, sh_hoff, A.pool, slot, A.results, tid, h0, h1);
    else generic_dispatch<kWG, false>((sh_step[0] >> 8) & 0xff, sh_step, sh_hoff, A.pool, slot, A.results, tid, h0, h1);
}

__global__ __launch_bounds__(kWG, 4) void ve_sum_kernel(const LevelArgs A) { elim_level<ElimMode::Sum>(A); }
__global__ __launch_bounds__(kWG, 4) void ve_max_kernel(const LevelArgs A) { elim_level<ElimMode::Max>(A); }
__global__ __launch_bounds__(kWG, 4) void ve_map_kernel(const LevelArgs A) { elim_level<ElimMode::Map>(A); }

struct TracebackArgs {
    const uint32_t *prog;       // the chunk's programs (each followed by its traceback record and, a map program, its gather list)
    const uint64_t *prog_off;   // word offset of request i's program
    const uint64_t *arena_off;  // offset (doubles) of request i's arena (its argmax tables)
    const double *arena;
    const double *m;            // m[i] = the FINAL cell of request i: max_x P(x, e_i) / max_m sum_h P(m, h, e_i)
    const int64_t *m_off;       // MAP: [n_req + 1] request i's codes go to codes[m_off[i] .. m_off[i + 1]); unused for MPE
    int32_t *codes;             // MPE: [n_req][n_vars]
    double *log_p;              // [n_req]
    uint32_t n_req;
    int32_t n_vars;             // <= kMaxVars
};

constexpr int kTracebackWG = 64;  // one wave per request

// Per request: log_p = log m; then, per record (last eliminated first), x* = argmax[sum_v code[v] * stride_v] - every axis of a
// max step is a variable eliminated later, so the reverse walk has decoded it.
//   MPE (GATHER = false): m = 0 (zero-probability evidence, or a code outside its domain: the program is empty and m stays 0)
//     gives log_p = -inf and code -1 for every non-evidence variable.  Variables neither eliminated nor evidence (single-state
//     ones) take code 0.  All n_vars codes of the request are stored.
//   MAP (GATHER = true): codes[m_off + k] = the code of the k-th entry of the gather list.  m not positive (zero-mass evidence, or
//     a code outside its domain: the program is empty, has no gather list, and m stays 0) gives log_p = -inf and code -1 for every
//     MAP variable.  A MAP variable that no step eliminates (a single state) takes code 0.
template <bool GATHER>
__device__ __forceinline__ void traceback(const TracebackArgs &A) {
    __shared__ int32_t sh_code[kMaxVars];
    __shared__ uint32_t sh_gather;  // GATHER: word offset of the gather list inside the request's program
    const uint32_t r = blockIdx.x;
    const int lane = threadIdx.x;
    if (r >= A.n_req) return;
    const int n = A.n_vars;
    const double m = A.m[r];
    const bool zero = !(m > 0.0);
    for (int v = lane; v < n; v += kTracebackWG) sh_code[v] = !GATHER && zero ? -1 : 0;
    __syncthreads();
    const uint32_t *p = A.prog + A.prog_off[r];
    if (lane == 0) {
        uint32_t g = 0;
        if (!GATHER || !zero) {
            const uint32_t *rec = p + record_offset(p);
            const uint32_t n_rec = rec[0], n_ev = rec[1];
            rec += 2;
            if constexpr (!GATHER)
                for (uint32_t k = 0; k < n_ev; ++k) {
                    const int v = (int)rec[2 * k];
                    if (v >= 0 && v < n) sh_code[v] = (int32_t)rec[2 * k + 1];
                }
            rec += 2 * n_ev;
            if (!zero) {
                const uint16_t *arena = reinterpret_cast<const uint16_t *>(A.arena + A.arena_off[r]);
                for (uint32_t k = 0; k < n_rec; ++k) {
                    const uint64_t am = (uint64_t)rec[0] | ((uint64_t)rec[1] << 32);
                    const int x = (int)rec[2];
                    const uint32_t n_out = rec[3];
                    int64_t idx = 0;
                    for (uint32_t a = 0; a < n_out; ++a) idx += (int64_t)sh_code[rec[4 + 2 * a]] * (int64_t)rec[5 + 2 * a];
                    sh_code[x] = (int32_t)arena[4 * am + (uint64_t)idx];
                    rec += 4 + 2 * n_out;
                }
                g = (uint32_t)(rec - p) + 1;  // (rec[0] = the length of the list: m_off knows it already)
            }
        }
        if constexpr (GATHER) sh_gather = g;
        A.log_p[r] = zero ? -__builtin_inf() : log(m);
    }
    __syncthreads();
    if constexpr (GATHER) {
        const int64_t o0 = A.m_off[r];
        const int n_m = (int)(A.m_off[r + 1] - o0);
        const uint32_t *list = p + sh_gather;
        for (int k = lane; k < n_m; k += kTracebackWG) A.codes[o0 + k] = zero ? -1 : sh_code[list[k]];
    } else {
        for (int v = lane; v < n; v += kTracebackWG) A.codes[(size_t)r * (size_t)n + v] = sh_code[v];
    }
}

__global__ __launch_bounds__(kTracebackWG) void mpe_traceback_kernel(const TracebackArgs A) { traceback<false>(A); }
__global__ __launch_bounds__(kTracebackWG) void map_traceback_kernel(const TracebackArgs A) { traceback<true>(A); }

}  // namespace mibn
