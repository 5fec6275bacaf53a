// The adaptive planning policy of the query driver (engine.hip, option "adaptive") and the share rule of the device planner: the
// state and the decisions, as plain values.  No HIP, no mibn_ctx, no clock: the engine measures and passes the numbers in, and applies
// what comes back (tools/plan_policy_sim.cpp drives the same code from scripted sequences: tests/test_plan_policy_host.py).
#pragma once
#include <algorithm>
#include <cstdint>

#ifndef MIBN_HOST_KEEPS_UP
#define MIBN_HOST_KEEPS_UP 1.25  // adaptive policy: (requests the host plans per ms) x (kernel ms per request) at or above which the device planner is dropped
#endif
#ifndef MIBN_POLICY_WINDOW_MS
#define MIBN_POLICY_WINDOW_MS 150.0  // adaptive policy: planning and retired kernel time a window must hold before it is judged (ranks of more than four planning threads)
#endif
#ifndef MIBN_HOST_BOUND_RATIO
#define MIBN_HOST_BOUND_RATIO 1.15  // adaptive policy: planner wall time over GPU kernel time above which a stream of calls counts as host-bound
#endif

namespace mibn {

// adaptive planning (option "adaptive"): when planning, not the GPU, bounds a stream of calls (few host cores per
// GPU), the elimination-order search - 40 % of the planning time - moves to the device (order_kernel); for networks the
// device search does not cover (> 128 variables) the greedy min-fill search is reserved for ever more expensive
// requests instead; both are given back when the host has slack again
struct PlanPolicy {
    int adaptive = 0;
    bool auto_search = false;  // gpu_search was switched on by the adaptive policy
    bool auto_emit = false;    // gpu_emit was
    int host_bound_streak = 0;
    bool adaptive_seeded = false;
    double base_minfill = 5e6, seen_plan_ms = 0, seen_kernel_ms = 0;  // (minfill_above: 2e7 up to round 6's last day; with order_effort 1 min-fill also supplies the opening candidate - 5e6: 1.7 % less GPU time per step for a tenth more planning, profiles/r06_cd_ab.log)
    double base_second_above = 2e7;  // option second_above (the calls the device plans run without the second emission: query_setup)
    double seen_requests = 0;        // retired requests (the unit of kernel_ms in the policy's windows) at the last adjustment
    double host_rate = 0;            // requests per ms the host's workers planned beside the device planner (smoothed; 0: not measured)
    double kernel_ms_per_req = 0;    // retired kernel time per request over the policy's last windows (smoothed; 0: not measured)
    double fixed_ms_per_req = 0;     // the host's side of a call besides planning - validation, schedule - per request (smoothed)
    double emit_share = 0.75;        // the device's share of a chunk, the host's workers plan the rest meanwhile: follows the two measured
                                     // rates so that both finish together (option emit_share: 0 < x <= 1 pins it)
    double emit_share_opt = -1;

    // what the policy turns: options gpu_emit and gpu_search, and the network's minfill_above
    struct Knobs {
        int gpu_emit, gpu_search;
        double minfill_above;
    };

    // Start of call number `call` (from 1) of a context with `threads` planning threads: the running totals of planning ms, retired
    // kernel ms and retired requests against the marks of the last adjustment.  Returns the new knobs.
    Knobs call_start(uint64_t call, int threads, double total_plan_ms, double total_kernel_ms, double retired_requests, bool order_net_ok,
                     bool emit_net_ok, Knobs k) {
        if (!adaptive) return k;
        if (!adaptive_seeded) {
            // A rank with a handful of planning threads (8 ranks on a 16-CPU quota: 2-4 each) cannot plan a stream like C3 at the rate
            // its GPU executes it (67 / 133 k queries/s at 2 / 4 threads against 280 k): it starts with the device planner instead of
            // finding that out over several host-bound calls; the share controller gives the planning back where the host keeps up.
            adaptive_seeded = true;
            if (threads <= 4 && order_net_ok && emit_net_ok && !k.gpu_emit) { k.gpu_emit = 1; auto_emit = true; }
        }
        // over the calls since the last adjustment: host planning wall time against GPU kernel time (retired launches)
        const double dp = total_plan_ms - seen_plan_ms, dk = total_kernel_ms - seen_kernel_ms;
        if (call <= 2) {  // the first calls pay one-time costs (thread pool, pinned buffers, first kernel load): not a trend
            seen_plan_ms = total_plan_ms;
            seen_kernel_ms = total_kernel_ms;
            seen_requests = retired_requests;
        } else if (dp > 20.0 && dk > 20.0 && (threads <= 4 || (dp > MIBN_POLICY_WINDOW_MS && dk > MIBN_POLICY_WINDOW_MS))) {
            // (a rank that is not starved judges windows of at least MIBN_POLICY_WINDOW_MS of planning AND of retired kernel time - two
            //  to three calls: the kernel time of a call is booked when its launches retire, up to two calls late, and a window of one
            //  call saw "100 ms of planning, 136 ms of kernels" as often as "100 against 68" on a steadily host-bound stream - n_evidence
            //  = 16 in round 5's session D: the two host-bound windows in a row the switch asks for came once in twelve calls)
            const double dreq = retired_requests - seen_requests;
            if (dreq > 0) kernel_ms_per_req = kernel_ms_per_req > 0 ? 0.5 * kernel_ms_per_req + 0.5 * dk / dreq : dk / dreq;
            // The device planner goes again where the host ALONE would keep up: the requests its workers plan per ms (measured
            // beside the device planner) x the kernel time per request must cover a request with a margin - the margin also
            // absorbs that the kernels of device-planned chunks run ~ 17 % longer than they would without the planner's kernels.
            // (Up to session S the rule was "the device's share has fallen to 0.3": a 6-thread rank - share 0.33 - oscillated
            // around it, 219 k queries/s; a fixed lower bar, 0.2, kept the device planner on a full-quota rank that had
            // switched it on during its first calls: 278 k instead of 300 k.  profiles/r04_s_policy.log, r04_t_policy.log)
            if (auto_emit && host_rate > 0 && dreq > 0 && host_rate * (dk / dreq) >= MIBN_HOST_KEEPS_UP) {
                k.gpu_emit = 0;
                auto_emit = false;
                host_bound_streak = 0;
            } else if (dp > MIBN_HOST_BOUND_RATIO * dk && ++host_bound_streak >= 2) {  // (round 6: twice in a row for every rank - a full-quota rank used to switch on one window, and the window behind a step's barrier, with the first call's planning exposed, tripped it for a per mille of the requests: profiles/r06_ce_ab.log, r06_cf_ab.log)  // (twice in a row: the kernel time of a call is booked when its
                                                                          // launches retire, up to two calls late - one window can mislead)
                // host-bound: first hand the order search to the device (same orders, no more bytes); networks it does
                // not cover give up the min-fill search for ever more expensive requests instead
                if (order_net_ok && emit_net_ok && !k.gpu_emit) {  // the whole planning, not only the search
                    k.gpu_emit = 1;
                    auto_emit = true;
                    host_rate = 0;  // (measured afresh beside the device planner: a rate left over from another workload - the line's
                                    //  n_evidence = 1 variant plans 1 000 requests per ms, n_evidence = 16 500 - made "the host alone would
                                    //  keep up" drop the device planner one window after every switch: round 5's session ZZ)
                }
                else if (order_net_ok && !emit_net_ok && !k.gpu_search) { k.gpu_search = 1; auto_search = true; }
                else if (!order_net_ok) k.minfill_above = std::min(k.minfill_above * 8.0, 1e18);
            } else if (dp <= MIBN_HOST_BOUND_RATIO * dk) {
                host_bound_streak = 0;
            }
            if (dp < 0.3 * dk) {
                if (k.minfill_above > base_minfill) k.minfill_above = std::max(k.minfill_above / 8.0, base_minfill);
                else if (auto_search) { k.gpu_search = 0; auto_search = false; }
            }
            seen_plan_ms = total_plan_ms;
            seen_kernel_ms = total_kernel_ms;
            seen_requests = retired_requests;
        }
        return k;
    }

    // The device's share of a chunk of n requests: [0, nd) planned by the device, the rest by the host's workers meanwhile.  `whole`:
    // option gpu_emit = 2, the device plans every request; `wave`: the chunk goes through wave_plan_kernel.
    int64_t device_share(int64_t n, bool whole, bool wave) const {
        int64_t nd = whole ? n : std::min<int64_t>(n, std::max<int64_t>(64, (int64_t)((double)n * std::min(emit_share, emit_share_opt > 0 ? 1.0 : (wave ? 0.99 : 0.95)) + 0.5)));
        if (n - nd < 256) nd = n;  // (without a pinned share the host keeps at least a twentieth: its rate stays measured)
        return nd;
    }

    // What the wave-mode share rule worked with (the engine's "[mibn share]" trace line); `ruled`: that rule moved the share.
    struct ShareStep {
        bool ruled = false;
        double ih = 0, kv = 0, kp = 0, fixed = 0, target = 0;
    };

    // After a chunk of n requests of which the device planned nd < n in dev_ms (its kernels) and the host's workers the rest in host_ms;
    // `chunk`: option chunk.  Updates host_rate and emit_share:
    // the share that would have let both finish together (the device's kernels ran beside the chunk in flight, like they will)
    // The planner's kernels are latency-bound - one request per lane, their duration hardly depends on how many
    // requests they plan - so the host's share is what its workers plan in that time, at the rate just measured.
    // (whole chunks only: the tail of a call - 20 624 requests behind seven chunks of 32 768 in bench.py's 250 000-request
    //  steps - gives the latency-bound device a smaller fraction than it takes of a full chunk; fed into the average,
    //  the tails pushed the share below the switch-off threshold of the policy above and the planning of a 4-thread
    //  rank oscillated between the device and the host alone: 187 k queries/s, profiles/r04_h_threads.log)
    // (host_ms > 0.02, not > 1: a stream answered from plan templates - n_evidence = 1 once its 9 900 shapes are stored - plans
    //  its 13 000 requests in 0.7 ms; with the old bar its rate was never measured, "the host alone would keep up" never
    //  fired and the device planner stayed on at three quarters of every chunk: 430 instead of 550 k queries/s, session N)
    ShareStep after_mixed_chunk(int64_t n, int64_t nd, double host_ms, double dev_ms, int64_t chunk, bool wave) {
        ShareStep s;
        if (host_ms > 0.02) host_rate = host_rate > 0 ? (wave ? 0.75 : 0.5) * host_rate + (wave ? 0.25 : 0.5) * (double)(n - nd) / host_ms : (double)(n - nd) / host_ms;
        if (emit_share_opt <= 0 && host_ms > 0.02 && dev_ms > 1.0 && 4 * n >= 3 * chunk) {
            if (wave && kernel_ms_per_req > 0) {
                // wave_plan_kernel's time grows with the requests it is given, and it is GPU time taken from the VE kernels: the
                // device gets what the host cannot plan while the GPU works through the chunk -
                //   fixed + (n - nd) ih  <=  0.85 (kv n + kp nd)     ih: ms per request of the host's workers, kv: kernel ms per
                // request (retired launches, the adaptive policy's windows), kp: planner ms per request (just measured, beside
                // the kernels), fixed: the host's side of a call besides planning (validation, the schedule).  (The planning
                // rates alone left a two-thread rank host-bound - 223 against 262 k queries/s; a feedback rule on the policy's
                // planner-wall / kernel-time ratio counted the waits for the device as host time and ended at a share of 0.99:
                // profiles/r06_r_ab.log, r06_s_ab.log)
                // (ih: the smoothed rate and the slower of it and this chunk's - the workers of a rank with the whole CPU quota plan in
                //  bursts, 35 000 n_evidence = 16 requests in 38 ms one call and 74 ms the next: profiles/r06_x_share16.log)
                const double ih = std::max(host_ms / (double)(n - nd), host_rate > 0 ? 1.0 / host_rate : 0.0), kv = kernel_ms_per_req, kp = dev_ms / (double)nd;
                const double fixed = fixed_ms_per_req * (double)n;
                const double target = std::max(0.03, std::min(0.99, ((double)n * ih + fixed - 0.85 * kv * (double)n) / ((ih + 0.85 * kp) * (double)n)));
                emit_share = 0.5 * emit_share + 0.5 * target;
                s.ruled = true; s.ih = ih; s.kv = kv; s.kp = kp; s.fixed = fixed; s.target = target;
            } else {
                const double host_n = (double)(n - nd) / host_ms * dev_ms;
                emit_share = std::max(0.25, std::min(1.0, 0.5 * emit_share + 0.5 * (1.0 - host_n / (double)n)));
            }
        }
        return s;
    }

    // End of a call of B > 0 requests whose host side besides planning took call_fixed_ms.
    void call_end(int64_t B, double call_fixed_ms) {
        fixed_ms_per_req = fixed_ms_per_req > 0 ? 0.5 * fixed_ms_per_req + 0.5 * call_fixed_ms / (double)B : call_fixed_ms / (double)B;
    }
};

}  // namespace mibn
