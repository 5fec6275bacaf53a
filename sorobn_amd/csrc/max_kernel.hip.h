// CDNA4 (gfx950) kernels of the most-probable-explanation path (mibn_mpe_batch).
//
// A max program (planner.h, "MAX programs") is a step program whose every step is GENERIC: the schedule of build_schedule cuts it
// into SEGMENT items (runs of small steps, one wave each) and GENERIC tiles (big steps, one workgroup per tile) exactly like a sum
// program, and one launch of `ve_max_kernel` runs one level of it.  The step code is the level kernel's own (generic_body with
// MAX = true: max instead of +, the lowest maximising value of the eliminated variable stored per output cell in the step's argmax
// table); only FIBER / OUTER / CHAIN / SWEEP do not exist here - max programs never contain them.
//
// `mpe_traceback_kernel` then decodes the assignment from the argmax tables, which never leave the device: one wave per request,
// lane 0 walks the request's traceback record (about one dependent 2-byte load per variable - latency, not bandwidth), the codes
// live in LDS and the wave writes them out with ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include "ve_kernel.hip.h"

namespace mibn {

// One level of a max schedule: workgroup b runs item wg_item[b] - a group of kSegPerWg segments or a tile of a big GENERIC step.
// The segments' descriptor copies and offset tables take the whole 12 KB buffer; a tile uses its first 3 KB.
__global__ __launch_bounds__(kWG, 4) void ve_max_kernel(const LevelArgs A) {
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
        segment_wave<1>(A, item_idx, (int)it.b, reinterpret_cast<double *>(sh_buf), tid);
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
    generic_dispatch<kWG, true>((sh_step[0] >> 8) & 0xff, sh_step, sh_hoff, A.pool, slot, A.results, tid, h0, h1);
}

struct TracebackArgs {
    const uint32_t *prog;       // the chunk's max programs (each followed by its traceback record)
    const uint64_t *prog_off;   // word offset of request i's program
    const uint64_t *arena_off;  // offset (doubles) of request i's arena (its argmax tables)
    const double *arena;
    const double *m;            // m[i] = max_x P(x, e_i): the FINAL cell of request i
    int32_t *codes;             // [n_req][n_vars]
    double *log_p;              // [n_req]
    uint32_t n_req;
    int32_t n_vars;             // <= kMaxVars
};

constexpr int kTracebackWG = 64;  // one wave per request

// Per request:  q* / m = the FINAL cell (no query variable: a scalar), log_p = log m; then, per record (last eliminated first),
// x* = argmax[sum_v code[v] * stride_v].  m = 0 (zero-probability evidence, or a code outside its domain: the program is empty
// and m stays 0) gives log_p = -inf and code -1 for every non-evidence variable.  Variables neither eliminated nor evidence
// (single-state ones) take code 0.
__global__ __launch_bounds__(kTracebackWG) void mpe_traceback_kernel(const TracebackArgs A) {
    __shared__ int32_t sh_code[kMaxVars];
    const uint32_t r = blockIdx.x;
    const int lane = threadIdx.x;
    if (r >= A.n_req) return;
    const int n = A.n_vars;
    const double m = A.m[r];
    const bool zero = !(m > 0.0);
    for (int v = lane; v < n; v += kTracebackWG) sh_code[v] = zero ? -1 : 0;
    __syncthreads();
    if (lane == 0) {
        const uint32_t *p = A.prog + A.prog_off[r];
        const uint32_t n_steps = p[0];
        uint64_t off = 1;
        for (uint32_t s = 0; s < n_steps; ++s) off += p[off + 6];
        const uint32_t *rec = p + off;
        const uint32_t n_rec = rec[0], n_ev = rec[1];
        rec += 2;
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
        }
        A.log_p[r] = zero ? -__builtin_inf() : log(m);
    }
    __syncthreads();
    for (int v = lane; v < n; v += kTracebackWG) A.codes[(size_t)r * (size_t)n + v] = sh_code[v];
}

}  // namespace mibn
