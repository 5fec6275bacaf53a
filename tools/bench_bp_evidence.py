"""What the Bethe log P(e) and the family beliefs of loopy belief propagation (mibn_bp_evidence_batch) cost beside mibn_bp_batch, and how
far log_z is from the exact log P(e).

    python tools/bench_bp_evidence.py [--requests 32768] [--seconds 2] [--seed 1] [--big 1024] [--iterations 40] [--log profiles/bp_evidence_bench.log]

One JSON line per row, printed and written to --log:

  c3              the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), the evidence of netspec.c3_requests (4 evidence
                  variables), calls of the whole batch at --iterations, tol 1e-9, damping 0, log_z alone: requests/s, bp_evidence_kernel's
                  time a call and per executed request-iteration, mean iterations, share converged.
  c3 sum          mibn_bp_batch on the same batch with the same arguments in the same session - the yardstick: bp_kernel's time per
                  request-iteration -, and the ratio of the two.
  c3 quality      on the first 256 requests: log_z against the exact log P(e) - mean and maximum absolute error, mean signed error, the
                  share converged.
  c3 e-step       a quarter of the 100 cells of every row missing, one call as fit_em(algorithm="lbp") makes it: with `acc` (the
                  family-belief buffer and bp_accumulate_kernel) and without, kernel times and wall time of a call.
  grid NxN        20 x 20 and 30 x 30 four-state grids, --big requests: requests/s, the form, time per request-iteration beside
                  bp_kernel's and their ratio; for a grid in MsgLds also under bp_lds = 0.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import golden_util as gu  # noqa: E402
import netspec  # noqa: E402
import sorobn_amd  # noqa: E402
from bench_bp import timed  # noqa: E402
from sorobn_amd import _capi  # noqa: E402
from sorobn_amd.events import csr_rows  # noqa: E402

TOL, DAMPING = 1e-9, 0.0
LOG = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if LOG:
        LOG.write(line + "\n")
        LOG.flush()


def kernel_row(eng, name):
    return {k["name"]: k for k in eng.kernel_stats()}.get(name, {"ms": 0.0, "launches": 0.0})


def ev_row(eng, name, evars, ecodes, iterations, seconds):
    requests = len(evars)
    n, dt, (log_z, _, _, it, res) = timed(lambda: eng.bp_evidence(evars, ecodes, iterations, TOL, DAMPING), seconds, eng.synchronize)
    st, ks = eng.stats(), kernel_row(eng, "bp_evidence_kernel")
    out = {"row": name, "requests": requests, "requests_per_s": round(n * requests / dt, 1), "calls": n, "window_s": round(dt, 3),
           "form": "MsgGlobal" if st["arena_bytes"] > 0 else "MsgLds", "bp_evidence_kernel_launches": ks["launches"],
           "bp_evidence_kernel_ms_per_call": round(ks["ms"], 3), "ns_per_request_iteration": round(ks["ms"] * 1e6 / max(1.0, float(it.sum())), 2),
           "mean_iterations": round(float(it.mean()), 2), "share_converged": round(float((res <= TOL).mean()), 4),
           "mean_log_z": round(float(log_z[np.isfinite(log_z)].mean()), 4), "last_call_total_ms": round(st["total_ms"], 2)}
    emit(out)
    return out, log_z, res


def sum_row(eng, name, evars, ecodes, iterations, seconds):
    n, dt, (_, it, _) = timed(lambda: eng.bp(evars, ecodes, iterations, TOL, DAMPING), seconds, eng.synchronize)
    ks = kernel_row(eng, "bp_kernel")
    out = {"row": name, "requests_per_s": round(n * len(evars) / dt, 1), "bp_kernel_ms_per_call": round(ks["ms"], 3),
           "ns_per_request_iteration": round(ks["ms"] * 1e6 / max(1.0, float(it.sum())), 2), "mean_iterations": round(float(it.mean()), 2)}
    emit(out)
    return out


def ratio(name, a, s):
    emit({"row": name, "ns_per_request_iteration_ratio": round(a["ns_per_request_iteration"] / s["ns_per_request_iteration"], 3)})


def grid_rows(R, K, requests, iterations, seconds, seed):
    bn = netspec.build(netspec.grid_spec(R, R, K, seed=3), sorobn_amd.BayesNet).use_device(0)
    eng = bn.backend.engine
    ids = np.array([bn.backend.var_id(f"{i:03d}") for i in range(R * R)], np.int32)
    _, ev, ec = netspec.c3_requests(R * R, K, requests, 4, seed=seed)
    a, _, _ = ev_row(eng, f"grid {R}x{R}", ids[ev], ec, iterations, seconds)
    s = sum_row(eng, f"grid {R}x{R} sum", ids[ev], ec, iterations, seconds)
    ratio(f"grid {R}x{R} evidence / sum", a, s)
    if a["form"] == "MsgLds":
        eng.set_option("bp_lds", 0)
        b, _, _ = ev_row(eng, f"grid {R}x{R} bp_lds=0", ids[ev], ec, iterations, seconds)
        s0 = sum_row(eng, f"grid {R}x{R} sum bp_lds=0", ids[ev], ec, iterations, seconds)
        eng.set_option("bp_lds", 1)
        ratio(f"grid {R}x{R} evidence / sum bp_lds=0", b, s0)


def e_step_rows(eng, ids, requests, iterations, seconds, seed):
    """Rows of the C3 grid with a quarter of the cells missing, as fit_em(algorithm="lbp") sends them: one request per row."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(requests, 100)).astype(np.int32)
    seen = rng.random((requests, 100)) >= 0.25
    args = csr_rows(ids, codes, seen)
    acc = np.zeros(int(eng.family_off[-1]), np.float64)
    for name, more in (("c3 e-step log_z alone", {}), ("c3 e-step with acc", {"acc": acc})):
        n, dt, (log_z, _, _, it, _) = timed(lambda: eng.bp_evidence_batch(*args, iterations, TOL, DAMPING, **more), seconds, eng.synchronize)
        st, ke, ka = eng.stats(), kernel_row(eng, "bp_evidence_kernel"), kernel_row(eng, "bp_accumulate_kernel")
        emit({"row": name, "requests": requests, "requests_per_s": round(n * requests / dt, 1), "calls": n,
              "bp_evidence_kernel_ms_per_call": round(ke["ms"], 3), "bp_accumulate_kernel_ms_per_call": round(ka["ms"], 3),
              "launches": [ke["launches"], ka["launches"]], "family_belief_buffer_mb": round(8e-6 * len(acc) * requests if more else 0.0, 1),
              "ns_per_request_iteration": round(ke["ms"] * 1e6 / max(1.0, float(it.sum())), 2), "mean_iterations": round(float(it.mean()), 2),
              "h2d_ms": round(st["h2d_ms"], 2), "d2h_ms": round(st["d2h_ms"], 2), "last_call_total_ms": round(st["total_ms"], 2),
              "share_finite": round(float(np.isfinite(log_z).mean()), 4)})


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32768)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--big", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "bp_evidence_bench.log"))
    a = ap.parse_args()
    LOG = open(a.log, "w") if a.log else None
    emit({"row": "arguments", **{k: v for k, v in vars(a).items() if k != "log"}, "tol": TOL, "damping": DAMPING})
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    be = bn.backend
    eng = be.engine
    _, ev, ec = netspec.c3_requests(100, 4, a.requests, 4, seed=a.seed)
    ids = np.array([be.var_id(f"{i:03d}") for i in range(100)], np.int32)
    evars = ids[ev]
    c3, log_z, res = ev_row(eng, "c3", evars, ec, a.iterations, a.seconds)
    s = sum_row(eng, "c3 sum", evars, ec, a.iterations, a.seconds)
    ratio("c3 evidence / sum", c3, s)
    # ---- quality on the first 256 requests, against the exact P(e)
    n_q = min(256, a.requests)
    p = eng.query_fixed(np.zeros((n_q, 0), np.int32), evars[:n_q], ec[:n_q], flags=_capi.Q_UNNORMALISED)[:, 0]
    err = log_z[:n_q] - np.log(p)
    emit({"row": "c3 quality", "requests": n_q, "mean_abs_error": float(np.abs(err).mean()), "max_abs_error": float(np.abs(err).max()),
          "mean_signed_error": float(err.mean()), "share_converged": round(float((res[:n_q] <= TOL).mean()), 4),
          "mean_log_p_exact": round(float(np.log(p).mean()), 4)})
    e_step_rows(eng, ids, a.requests, a.iterations, a.seconds / 2, a.seed)
    # ---- beyond the reach of the exact call
    for R in (20, 30):
        grid_rows(R, 4, a.big, a.iterations, a.seconds / 2, a.seed)


if __name__ == "__main__":
    main()
