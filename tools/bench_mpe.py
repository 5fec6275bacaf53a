"""Throughput of the most-probable-explanation path (mibn_mpe_batch) on the C3 workload, beside the sum path on the same evidence.

    python tools/bench_mpe.py [--requests 32768] [--evidence 4] [--seconds 2] [--seed 1]

Workload: the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), evidence sets of netspec.c3_requests (seeded,
4 evidence variables).  One warm-up call, then calls of the whole batch until at least --seconds have passed, the window ended
by a device synchronise.  Prints one JSON line: MPE/s, bytes per request (tables + argmax), ve_max_kernel's GB/s and its share
of the 8 TB/s HBM peak, and the sum path's queries/s for the same evidence sets (query = each request's C3 query variable).
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

HBM_PEAK = 8.0e12


def timed(fn, seconds, sync):
    fn()  # warm-up
    sync()
    n = 0
    t0 = time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    sync()
    return n, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32768)
    ap.add_argument("--evidence", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    be = bn.backend
    eng = be.engine
    q, ev, ec = netspec.c3_requests(100, 4, a.requests, a.evidence, seed=a.seed)
    ids = np.array([be.var_id(f"{i:03d}") for i in range(100)], np.int32)
    evars, qvars = ids[ev], ids[q].reshape(-1, 1)

    n, dt = timed(lambda: eng.mpe(evars, ec), a.seconds, eng.synchronize)
    st = eng.stats()
    ks = {k["name"]: k for k in eng.kernel_stats()}
    mk = ks.get("ve_max_kernel", {"ms": 0.0, "alg_bytes": 0.0})
    tb = ks.get("mpe_traceback_kernel", {"ms": 0.0})
    mpe_rate = n * a.requests / dt
    gbs = mk["alg_bytes"] / (mk["ms"] * 1e-3) / 1e9 if mk["ms"] else 0.0

    nq, dtq = timed(lambda: eng.query_fixed(qvars, evars, ec), a.seconds, eng.synchronize)
    out = {
        "workload": f"C3 10x10 K=4, {a.evidence} evidence, {a.requests} requests per call",
        "mpe_per_s": round(mpe_rate, 1),
        "mpe_calls": n,
        "mpe_window_s": round(dt, 3),
        "bytes_per_request": round(st["alg_bytes"] / a.requests, 1),
        "ve_max_kernel_ms": round(mk["ms"], 3),
        "ve_max_kernel_GBps": round(gbs, 1),
        "ve_max_kernel_share_of_hbm_peak": round(gbs * 1e9 / HBM_PEAK, 4),
        "mpe_traceback_kernel_ms": round(tb["ms"], 3),
        "last_call_total_ms": round(st["total_ms"], 2),
        "last_call_plan_ms": round(st["plan_ms"], 2),
        "last_call_kernel_ms": round(st["kernel_ms"], 2),
        "sum_queries_per_s": round(nq * a.requests / dtq, 1),
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
