"""What approximate MPE by max-product belief propagation (mibn_bp_mpe_batch) costs and how far its answers are from the exact ones.

    python tools/bench_bp_mpe.py [--requests 32768] [--seconds 2] [--seed 1] [--big 1024] [--iterations 40]

One JSON line per row:

  c3          the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), the evidence of netspec.c3_requests (4 evidence
              variables), calls of the whole batch at --iterations, tol 1e-9, damping 0.5, polish 10: requests/s, bp_max_kernel's time a
              call and per executed request-iteration, mean iterations, share converged, mean sweeps and moves.
  c3 sum      mibn_bp_batch on the same batch at the same iteration cap and damping - the yardstick: bp_kernel's time per
              request-iteration, and the ratio of the two.
  c3 quality  on the first 256 requests against the exact mpe: the share that hits the exact log_p (within 1e-9), mean and max of
              log_p_exact - log_p; the same for polish 0 and for the argmax of the sum-product marginals scored by mibn_bp_mpe_batch's
              own rule (every variable observed: the call returns the log-probability of that assignment).
  grid NxN    20 x 20 and 30 x 30 four-state grids, --big requests: requests/s, the form, time per request-iteration beside
              bp_kernel's, mean log_p with polish 10 and 0; for a grid in MsgLds also under bp_lds = 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import golden_util as gu  # noqa: E402
import netspec  # noqa: E402
import sorobn_amd  # noqa: E402
from bench_bp import timed  # noqa: E402

TOL, DAMPING, POLISH = 1e-9, 0.5, 10


def kernel_row(eng, name):
    return {k["name"]: k for k in eng.kernel_stats()}[name]


def mpe_row(eng, name, evars, ecodes, iterations, seconds, polish=POLISH):
    requests = len(evars)
    n, dt, (codes, log_p, it, res, info) = timed(lambda: eng.bp_mpe(evars, ecodes, iterations, TOL, DAMPING, polish), seconds, eng.synchronize)
    st, ks = eng.stats(), kernel_row(eng, "bp_max_kernel")
    out = {"row": name, "requests": requests, "requests_per_s": round(n * requests / dt, 1), "calls": n, "window_s": round(dt, 3),
           "form": "MsgGlobal" if st["arena_bytes"] > 0 else "MsgLds", "bp_max_kernel_launches": ks["launches"],
           "bp_max_kernel_ms_per_call": round(ks["ms"], 3), "ns_per_request_iteration": round(ks["ms"] * 1e6 / max(1.0, float(it.sum())), 2),
           "mean_iterations": round(float(it.mean()), 2), "share_converged": round(float((res <= TOL).mean()), 4),
           "mean_best_iteration": round(float(info[:, 0].mean()), 2), "mean_sweeps": round(float(info[:, 1].mean()), 2),
           "mean_moves": round(float(info[:, 2].mean()), 2), "mean_log_p": round(float(log_p.mean()), 3),
           "last_call_total_ms": round(st["total_ms"], 2)}
    print(json.dumps(out), flush=True)
    return out, codes, log_p


def sum_row(eng, name, evars, ecodes, iterations, seconds):
    n, dt, (bel, it, res) = timed(lambda: eng.bp(evars, ecodes, iterations, TOL, DAMPING), seconds, eng.synchronize)
    ks = kernel_row(eng, "bp_kernel")
    out = {"row": name, "requests_per_s": round(n * len(evars) / dt, 1), "bp_kernel_ms_per_call": round(ks["ms"], 3),
           "ns_per_request_iteration": round(ks["ms"] * 1e6 / max(1.0, float(it.sum())), 2), "mean_iterations": round(float(it.mean()), 2)}
    print(json.dumps(out), flush=True)
    return out, bel


def gaps(name, exact_lp, lp):
    gap = exact_lp - lp
    print(json.dumps({"row": name, "requests": len(lp), "share_exact": round(float((gap <= 1e-9).mean()), 4), "mean_gap": round(float(gap.mean()), 4),
                      "max_gap": round(float(gap.max()), 4), "mean_log_p": round(float(lp.mean()), 3), "mean_log_p_exact": round(float(exact_lp.mean()), 3)}),
          flush=True)


def grid_rows(R, K, requests, iterations, seconds, seed):
    bn = netspec.build(netspec.grid_spec(R, R, K, seed=3), sorobn_amd.BayesNet).use_device(0)
    eng = bn.backend.engine
    ids = np.array([bn.backend.var_id(f"{i:03d}") for i in range(R * R)], np.int32)
    _, ev, ec = netspec.c3_requests(R * R, K, requests, 4, seed=seed)
    a, _, _ = mpe_row(eng, f"grid {R}x{R}", ids[ev], ec, iterations, seconds)
    mpe_row(eng, f"grid {R}x{R} polish=0", ids[ev], ec, iterations, seconds, polish=0)
    s, _ = sum_row(eng, f"grid {R}x{R} sum", ids[ev], ec, iterations, seconds)
    print(json.dumps({"row": f"grid {R}x{R} max / sum", "ns_per_request_iteration_ratio": round(a["ns_per_request_iteration"] / s["ns_per_request_iteration"], 3)}), flush=True)
    if a["form"] == "MsgLds":
        eng.set_option("bp_lds", 0)
        b, _, _ = mpe_row(eng, f"grid {R}x{R} bp_lds=0", ids[ev], ec, iterations, seconds)
        eng.set_option("bp_lds", 1)
        print(json.dumps({"row": f"grid {R}x{R} MsgGlobal / MsgLds", "kernel_time_ratio": round(b["bp_max_kernel_ms_per_call"] / a["bp_max_kernel_ms_per_call"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32768)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--big", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=40)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    be = bn.backend
    eng = be.engine
    _, ev, ec = netspec.c3_requests(100, 4, a.requests, 4, seed=a.seed)
    ids = np.array([be.var_id(f"{i:03d}") for i in range(100)], np.int32)
    evars = ids[ev]
    c3, codes, log_p = mpe_row(eng, "c3", evars, ec, a.iterations, a.seconds)
    s, bel = sum_row(eng, "c3 sum", evars, ec, a.iterations, a.seconds)
    print(json.dumps({"row": "c3 max / sum", "ns_per_request_iteration_ratio": round(c3["ns_per_request_iteration"] / s["ns_per_request_iteration"], 3)}), flush=True)
    # ---- quality on the first 256 requests, against the exact MPE
    n_q = min(256, a.requests)
    _, exact_lp = eng.mpe(evars[:n_q], ec[:n_q])
    gaps("c3 quality", exact_lp, log_p[:n_q])
    gaps("c3 quality polish=0", exact_lp, eng.bp_mpe(evars[:n_q], ec[:n_q], a.iterations, TOL, DAMPING, 0)[1])
    gaps("c3 quality damping=0 polish=0", exact_lp, eng.bp_mpe(evars[:n_q], ec[:n_q], a.iterations, TOL, 0.0, 0)[1])
    # the argmax of the sum-product marginals: observe every variable at it, one step - log_p is that assignment's log-probability
    card = eng.card
    off = np.concatenate([[0], np.cumsum(card, dtype=np.int64)])
    arg = np.stack([bel[:n_q, off[v]:off[v + 1]].argmax(axis=1) for v in range(len(card))], axis=1).astype(np.int32)
    every = np.tile(np.arange(len(card), dtype=np.int32), (n_q, 1))
    gaps("c3 quality argmax of sum-product marginals", exact_lp, eng.bp_mpe(every, arg, 1, TOL, 0.0, 0)[1])
    # ---- beyond the reach of the exact call
    for R in (20, 30):
        grid_rows(R, 4, a.big, a.iterations, a.seconds / 2, a.seed)


if __name__ == "__main__":
    main()
