// Forward (ancestral) sampling on gfx950 and the two approximate-inference loops built on it (SURVEY.md section 8f
// rank 2): BayesNet.sample / _forward_sample (sorobn/bayes_net.py:518-575), _rejection_sampling (577-619) and
// _llh_weighting (621-663).
//
// One sample per lane and trip: every lane walks the variables in topological order (= variable-id order, the order
// of `BayesNet.nodes`, bayes_net.py:319-322), looks up P(v | parents) in the dense CPT, draws v by inverse-CDF from a
// Philox4x32-10 uniform keyed by (seed, sample index, variable) - or takes the clamped `init` value - and multiplies
// the *likelihood* by P(value | parents) for EVERY node, clamped or not, exactly as the reference does (541-546).
//   mode SAMPLE     states[sample][v] = value code                                   (sample(n, init))
//   mode REJECTION  nothing is clamped; samples that agree with the event are counted per query cell   (606-619)
//   mode LIKELIHOOD the event is clamped; per query cell the likelihoods are summed and the samples counted - the
//                   reference returns groupby(query).mean() of the likelihood, normalised (658-663)
// The chain state of a lane lives in LDS (state[var][lane] bytes), histograms are accumulated per workgroup in LDS
// and flushed with one global atomic per cell.  Latency-bound like the Gibbs kernel.  Parity with the reference's stream
// is unpinned (it depends on the absent third-party `vose` sampler, oracle/README.md); our own stream is pinned by
// tests/sample_check.py - its numpy twin, which the samples and histograms have to equal exactly.
// The packed words, the LDS layout (sample_layout), the grid and the output buffer of a call are decided in sampler_plan.h
// (sample_plan: host-only, pinned on a CPU by tests/test_sampler_plan_host.py); sample_run below is plan, allocate, upload,
// launch, download.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/mibn.h"
#include "device_mem.h"
#include "gibbs_kernel.hip.h"
#include "planner.h"

namespace mibn {

struct SampleArgs {
    const double *pool;
    const GibbsVar *vars;         // is_evidence / ev_code = clamped (init) variables
    const int32_t *scope_var;
    const int32_t *scope_stride;
    const int32_t *qvars;
    const int32_t *qstride;
    const int32_t *evars;         // REJECTION: the event to agree with
    const int32_t *ecodes;
    uint8_t *states;              // SAMPLE: [n_samples][n_vars] (out); PROBE: the given joint states (in)
    double *cdf;                  // PROBE: [n_samples][n_vars][cdf_stride] running sums of the conditional row a draw of v compares u * total with
    double *lik;                  // PROBE: [n_samples] the likelihood of the given state
    int32_t cdf_stride;
    double *wsum;                 // LIKELIHOOD: sum of likelihoods per query cell
    unsigned long long *counts;   // samples per query cell (REJECTION: accepted ones)
    int32_t n_vars, n_q, n_e, hist_cells, mode;
    int64_t n_samples;
    uint64_t seed;
};

__global__ __launch_bounds__(64) void sample_kernel(const SampleArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const SampleLayout<int> L = sample_layout<int>(A.n_vars, A.hist_cells);
    uint8_t *st = smem;                                                          // n_vars * 64 bytes
    double *hsum = (double *)(smem + L.hsum);                                    // hist_cells
    unsigned int *hcnt = (unsigned int *)(smem + L.hcnt);                        // hist_cells
    for (int i = lane; i < A.hist_cells; i += 64) { hsum[i] = 0.0; hcnt[i] = 0u; }
    __syncthreads();
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32) ^ 0x85EBCA6Bu;
    for (int64_t s0 = (int64_t)blockIdx.x * 64; s0 < A.n_samples; s0 += (int64_t)gridDim.x * 64) {
        const int64_t s = s0 + lane;
        const bool active = s < A.n_samples;
        double likelihood = 1.0;
        for (int v = 0; v < A.n_vars; ++v) {
            const GibbsVar V = A.vars[v];
            int off = V.table_off;
            for (int k = 0; k + 1 < V.scope_len; ++k)
                off += (int)st[A.scope_var[V.scope_begin + k] * 64 + lane] * A.scope_stride[V.scope_begin + k];
            int val = V.ev_code;
            const bool probe = A.mode == kProbeMode;
            if (!V.is_evidence || probe) {
                // P.cdt.sample(): a draw from the (possibly unnormalised / sparse) conditional row (bayes_net.py:28-42)
                double total = 0;
                for (int x = 0; x < V.card; ++x) total += A.pool[off + x];
                const double u = philox_uniform((uint64_t)s, 2u + (uint32_t)v, k0, k1) * total;
                double acc = 0;
                val = V.card - 1;
                for (int x = 0; x < V.card; ++x) {
                    acc += A.pool[off + x];
                    if (probe) { if (active) A.cdf[((size_t)s * A.n_vars + v) * A.cdf_stride + x] = acc; continue; }
                    if (u < acc) { val = x; break; }
                }
                if (probe) val = active ? (int)A.states[(size_t)s * A.n_vars + v] : 0;
            }
            st[v * 64 + lane] = (uint8_t)val;
            likelihood *= A.pool[off + val];  // P.get(node_value, 0): absent rows are 0 in the dense table
        }
        if (!active) continue;
        if (A.mode == kProbeMode) { A.lik[s] = likelihood; continue; }
        if (A.mode == kSampleMode) {
            for (int v = 0; v < A.n_vars; ++v) A.states[s * A.n_vars + v] = st[v * 64 + lane];
            continue;
        }
        bool keep = true;
        if (A.mode == kRejectionMode)
            for (int i = 0; i < A.n_e; ++i) keep = keep && (int)st[A.evars[i] * 64 + lane] == A.ecodes[i];
        if (keep) {
            int cell = 0;
            for (int q = 0; q < A.n_q; ++q) cell += (int)st[A.qvars[q] * 64 + lane] * A.qstride[q];
            atomicAdd(&hcnt[cell], 1u);
            if (A.mode == kLikelihoodMode) atomicAdd(&hsum[cell], likelihood);
        }
    }
    __syncthreads();
    if (A.mode != kSampleMode)
        for (int i = lane; i < A.hist_cells; i += 64) {
            if (hcnt[i]) atomicAdd(&A.counts[i], (unsigned long long)hcnt[i]);
            if (A.mode == kLikelihoodMode && hsum[i] != 0.0) atomicAdd(&A.wsum[i], hsum[i]);
        }
}

// host driver: plan (sampler_plan.h), allocate, upload, launch, download - per-call buffers, blocking; returns MIBN_* code.
// clamp_*: variables forced to a value (sample's `init`, likelihood weighting's event); ev_*: the event rejection sampling
// filters on.
inline int sample_run(const Network &net, const double *d_pool, hipStream_t stream, int mode, int32_t n_q, const int32_t *q_vars,
                      int32_t n_clamp, const int32_t *clamp_vars, const int32_t *clamp_codes, int32_t n_ev, const int32_t *ev_vars,
                      const int32_t *ev_codes, int64_t n_samples, uint64_t seed, uint8_t *states, double *wsum, int64_t *counts,
                      std::string &err, int32_t cdf_stride = 0, double *probe_lik = nullptr, double *probe_cdf = nullptr) {
    SamplePlan S;
    if (int rc = sample_plan(net, mode, n_q, q_vars, n_clamp, clamp_vars, clamp_codes, n_ev, ev_vars, ev_codes, n_samples, cdf_stride, S, err)) return rc;
    const size_t n = (size_t)net.n_vars, out_bytes = S.out_bytes, buf_bytes = std::max<size_t>(16, out_bytes);
    const std::vector<int32_t> &pack = S.pack.words;
    DevBuf<GibbsVar> d_vars;
    DevBuf<int32_t> d_i32;
    DevBuf<unsigned char> d_out_buf;  // states | wsum + counts
    auto fail = [&](hipError_t e) { err = std::string("sampling: ") + hipGetErrorString(e); return MIBN_E_HIP; };
    hipError_t e;
    if ((e = d_vars.reset(std::max<size_t>(1, n))) != hipSuccess) return fail(e);
    if ((e = d_i32.reset(std::max<size_t>(1, pack.size()))) != hipSuccess) return fail(e);
    if ((e = d_out_buf.reset(buf_bytes)) != hipSuccess) return fail(e);
    unsigned char *const d_out = d_out_buf.get();
    if ((e = hipMemcpyAsync(d_vars, S.pack.vars.data(), sizeof(GibbsVar) * n, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
    if ((e = hipMemcpyAsync(d_i32, pack.data(), 4 * pack.size(), hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(d_out, 0, buf_bytes, stream)) != hipSuccess) return fail(e);
    if (mode == kProbeMode && (e = hipMemcpyAsync(d_out, states, (size_t)n_samples * n, hipMemcpyHostToDevice, stream)) != hipSuccess) return fail(e);
    SampleArgs A;
    A.pool = d_pool;
    A.vars = d_vars;
    A.scope_var = d_i32 + S.o_sv;
    A.scope_stride = d_i32 + S.o_ss;
    A.qvars = d_i32 + S.o_q;
    A.qstride = d_i32 + S.o_qs;
    A.evars = d_i32 + S.o_ev;
    A.ecodes = d_i32 + S.o_ec;
    A.states = d_out;
    A.wsum = (double *)d_out;
    A.counts = (unsigned long long *)(d_out + (size_t)S.cells * 8);
    A.lik = (double *)(d_out + S.probe_states);
    A.cdf = A.lik + n_samples;
    A.cdf_stride = cdf_stride;
    A.n_vars = net.n_vars;
    A.n_q = n_q;
    A.n_e = n_ev;
    A.hist_cells = S.hist_cells;
    A.mode = mode;
    A.n_samples = n_samples;
    A.seed = seed;
    if (S.lds.total > 64 * 1024) {
        if ((e = hipFuncSetAttribute((const void *)sample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.lds.total)) != hipSuccess) return fail(e);
    }
    hipLaunchKernelGGL(sample_kernel, dim3(S.blocks), dim3(64), S.lds.total, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e);
    std::vector<unsigned char> host(buf_bytes);
    if ((e = hipMemcpyAsync(host.data(), d_out, host.size(), hipMemcpyDeviceToHost, stream)) != hipSuccess) return fail(e);
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return fail(e);
    if (mode == kSampleMode) {
        std::memcpy(states, host.data(), out_bytes);
    } else if (mode == kProbeMode) {
        std::memcpy(probe_lik, host.data() + S.probe_states, (size_t)n_samples * 8);
        std::memcpy(probe_cdf, host.data() + S.probe_states + (size_t)n_samples * 8, (size_t)n_samples * 8 * n * cdf_stride);
    } else {
        const double *ws = (const double *)host.data();
        const unsigned long long *cn = (const unsigned long long *)(host.data() + (size_t)S.cells * 8);
        for (int64_t i = 0; i < S.cells; ++i) { if (wsum) wsum[i] = ws[i]; counts[i] = (int64_t)cn[i]; }
    }
    return MIBN_OK;
}

}  // namespace mibn
