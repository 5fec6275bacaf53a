"""What loopy belief propagation (mibn_bp_batch) costs and how far its answers are from the exact ones.

    python tools/bench_bp.py [--requests 32768] [--seconds 2] [--seed 1] [--big 1024]

One JSON line per row:

  c3        the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), the evidence of netspec.c3_requests (4 evidence
            variables), calls of the whole batch at the defaults (100 iterations, tol 1e-9, no damping): requests/s, mean iterations,
            share converged, bp_kernel's time, its time per executed request-iteration and the rate of its algorithmic bytes (CPT
            cells read: they come from L2, so the rate is to be read against L2's, not HBM's).
  c3 error  on the first 256 requests, max and mean |belief - exact posterior| over every non-evidence variable.  That is the error of
            the APPROXIMATION on this loopy grid, not the kernel's (the kernel is within 1e-12 of its numpy twin: tests/test_bp.py).
  gibbs     mibn_gibbs on the same 256 requests (64 chains each, the request's query variable), its iteration count chosen so that
            the 256 calls take about as long as ONE belief propagation call over all --requests requests - which already answers
            every variable of 128 times as many requests -, and its error on that variable beside belief propagation's on the same.
  grid NxN  20 x 20 and 30 x 30 four-state grids, --big requests, 30 iterations: requests/s, mean iterations, the form (MsgGlobal
            books its slabs under arena_bytes); for 20 x 20 also under bp_lds = 0 and the time ratio.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import golden_util as gu  # noqa: E402
import netspec  # noqa: E402
import sorobn_amd  # noqa: E402


def timed(fn, seconds, sync):
    fn()  # warm-up
    sync()
    n = 0
    t0 = time.perf_counter()
    while True:
        out = fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    sync()
    return n, time.perf_counter() - t0, out


def bp_row(eng, name, evars, ecodes, max_iterations, tol, seconds):
    requests = len(evars)
    n, dt, (bel, it, res) = timed(lambda: eng.bp(evars, ecodes, max_iterations, tol, 0.0), seconds, eng.synchronize)
    st = eng.stats()
    ks = {k["name"]: k for k in eng.kernel_stats()}["bp_kernel"]
    out = {"row": name, "requests_per_s": round(n * requests / dt, 1), "calls": n, "window_s": round(dt, 3),
           "mean_iterations": round(float(it.mean()), 2), "share_converged": round(float((res <= tol).mean()), 4),
           "form": "MsgGlobal" if st["arena_bytes"] > 0 else "MsgLds", "bp_kernel_launches": ks["launches"], "bp_kernel_ms": round(ks["ms"], 3),
           "ns_per_request_iteration": round(ks["ms"] * 1e6 / max(1.0, float(it.sum())), 2),
           "alg_GB_per_s": round(ks["alg_bytes"] / max(ks["ms"], 1e-9) / 1e6, 1), "last_call_total_ms": round(st["total_ms"], 2)}
    print(json.dumps(out), flush=True)
    return out, bel


def grid_rows(R, K, requests, seconds, seed):
    bn = netspec.build(netspec.grid_spec(R, R, K, seed=3), sorobn_amd.BayesNet).use_device(0)
    eng = bn.backend.engine
    ids = np.array([bn.backend.var_id(f"{i:03d}") for i in range(R * R)], np.int32)
    _, ev, ec = netspec.c3_requests(R * R, K, requests, 4, seed=seed)
    a, _ = bp_row(eng, f"grid {R}x{R}", ids[ev], ec, 30, 1e-9, seconds)
    if a["form"] == "MsgLds":
        eng.set_option("bp_lds", 0)
        b, _ = bp_row(eng, f"grid {R}x{R} bp_lds=0", ids[ev], ec, 30, 1e-9, seconds)
        eng.set_option("bp_lds", 1)
        print(json.dumps({"row": f"grid {R}x{R} MsgGlobal / MsgLds", "kernel_time_ratio": round(b["bp_kernel_ms"] / a["bp_kernel_ms"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32768)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--big", type=int, default=1024)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    be = bn.backend
    eng = be.engine
    card = eng.card
    q, ev, ec = netspec.c3_requests(100, 4, a.requests, 4, seed=a.seed)
    ids = np.array([be.var_id(f"{i:03d}") for i in range(100)], np.int32)
    evars, qvars = ids[ev], ids[q]
    c3, bel = bp_row(eng, "c3", evars, ec, 100, 1e-9, a.seconds)
    # ---- the approximation's error on the first 256 requests: every non-evidence variable against the exact query
    n_err = min(256, a.requests)
    off = np.concatenate([[0], np.cumsum(card, dtype=np.int64)])
    errs = []
    for v in range(100):
        rows = np.flatnonzero(~(evars[:n_err] == v).any(axis=1))
        exact = eng.query_fixed(np.full((len(rows), 1), v, np.int32), evars[rows], ec[rows])
        errs.append(np.abs(bel[rows, off[v]:off[v + 1]] - exact).reshape(-1))
    errs = np.concatenate(errs)
    print(json.dumps({"row": "c3 error", "requests": n_err, "max_abs_err": float(errs.max()), "mean_abs_err": float(errs.mean())}), flush=True)
    # ---- Gibbs on the same requests, given the wall time of one belief propagation call
    lbp_call_s = c3["window_s"] / c3["calls"]
    exact_q = eng.query_fixed(qvars[:n_err].reshape(-1, 1), evars[:n_err], ec[:n_err])
    lbp_q = np.stack([bel[b, off[qvars[b]]:off[qvars[b]] + 4] for b in range(n_err)])

    def gibbs(iters):
        t0 = time.perf_counter()
        est = np.stack([eng.gibbs([int(qvars[b])], evars[b], ec[b], 64, iters, seed=b).astype(np.float64) for b in range(n_err)])
        return est / est.sum(axis=1, keepdims=True), time.perf_counter() - t0
    gibbs(96)
    _, t_lo = gibbs(96)
    _, t_hi = gibbs(9600)
    per_iter = max(1e-12, (t_hi - t_lo) / (9600 - 96))
    iters = int(max(96, min(2_000_000, 96 + (lbp_call_s - t_lo) / per_iter)))
    est, t = gibbs(iters)
    print(json.dumps({"row": "gibbs", "requests": n_err, "chains": 64, "iterations": iters, "wall_s_256_calls": round(t, 4),
                      "wall_s_256_calls_at_96_iterations": round(t_lo, 4), "lbp_wall_s_one_call_all_requests": round(lbp_call_s, 4),
                      "gibbs_max_abs_err": float(np.abs(est - exact_q).max()), "gibbs_mean_abs_err": float(np.abs(est - exact_q).mean()),
                      "lbp_max_abs_err_same_variable": float(np.abs(lbp_q - exact_q).max()),
                      "lbp_mean_abs_err_same_variable": float(np.abs(lbp_q - exact_q).mean())}), flush=True)
    # ---- beyond the reach of the exact calls
    for R in (20, 30):
        grid_rows(R, 4, a.big, a.seconds / 2, a.seed)


if __name__ == "__main__":
    main()
