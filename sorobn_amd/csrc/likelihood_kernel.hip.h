// Likelihood findings (Pearl's virtual evidence) on the planned path: the seeds of a wave of requests.
//
// A finding (X, lambda) is a one-axis factor of the request that carries it (emit_begin, emit_core.h): the planner gives it a SEED
// offset - the first cells of the request's private arena, in the order of the findings, each padded to 16 cells - and every
// elimination kernel then reads it like any intermediate table.  What no step writes, this kernel does: before the first level of a
// wave it copies the weights of every finding of the wave's requests from the chunk's packed weight array to
//     arena + arena_off[request - r0] + seed_off.
// An arena is re-used by the next wave, so the seeds are written again for every wave of a chunk.
//
// One 64-lane wave per record, lanes striding the cells (a variable of more than 64 states takes several strides), four waves per
// workgroup, grid-stride over the records.  Plain vector loads and stores: no atomics, no LDS.  A few hundred bytes per request
// against the megabytes its program moves: not HBM-bound, roofline n/a.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mibn {

struct SeedRec {        // one finding of one request of a chunk
    uint32_t req;       // request index within the chunk
    uint32_t seed_off;  // offset (doubles) of the seed in the request's arena
    uint32_t src_off;   // offset (doubles) of its weights in the chunk's packed weight array
    uint32_t cells;     // card(X)
};
static_assert(sizeof(SeedRec) == 16, "a record is 16 bytes");

struct SeedArgs {
    const SeedRec *recs;        // the records of the wave's requests [r0, r1): ascending by request
    const double *values;       // the chunk's packed weights
    double *arena;
    const uint64_t *arena_off;  // per request of the wave: offset (doubles) of its private arena
    uint32_t n_recs, r0;
};

constexpr int kSeedWG = 256;  // four waves

__global__ __launch_bounds__(kSeedWG) void likelihood_seed_kernel(const SeedArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * (kSeedWG / 64) + (threadIdx.x >> 6), n_waves = gridDim.x * (kSeedWG / 64);
    for (uint32_t k = wave; k < A.n_recs; k += n_waves) {
        const SeedRec r = A.recs[k];
        double *__restrict__ dst = A.arena + A.arena_off[r.req - A.r0] + r.seed_off;
        const double *__restrict__ src = A.values + r.src_off;
        for (uint32_t c = lane; c < r.cells; c += 64) dst[c] = src[c];
    }
}

inline unsigned seed_grid(uint32_t n_recs, int n_cu) {
    const unsigned want = (n_recs + kSeedWG / 64 - 1) / (kSeedWG / 64);
    const unsigned cap = (unsigned)(n_cu > 0 ? n_cu : 1) * 8u;
    return want < 1u ? 1u : (want < cap ? want : cap);
}

}  // namespace mibn
