"""Throughput of the evidence-likelihood path (P(e): mibn_query_batch_ex with MIBN_Q_UNNORMALISED and no query variable) on the C3
workload, beside the sum path's posterior queries on the same evidence.

    python tools/bench_evidence.py [--requests 32768] [--evidence 4,8,16] [--seconds 2] [--seed 1]

Workload: the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), evidence sets of netspec.c3_requests (seeded) with
4, 8 and 16 observed values.  Per evidence count: one warm-up call, then calls of the whole batch until at least --seconds have
passed, the window ended by a device synchronise - first P(e) of every request, then the posterior of each request's C3 query
variable given the same evidence (the sum path).  Prints one JSON line: per evidence count, P(e)/s, the section-8(d) algorithmic
bytes per request, the all-kernel GB/s of the last P(e) call (its bytes over the summed HIP-event time of its launches) and its
share of the 8 TB/s HBM peak, and the sum path's queries/s.
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
from sorobn_amd import _capi  # noqa: E402

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
    ap.add_argument("--evidence", default="4,8,16")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    be = bn.backend
    eng = be.engine
    ids = np.array([be.var_id(f"{i:03d}") for i in range(100)], np.int32)
    none = np.zeros((a.requests, 0), np.int32)
    out = {"workload": f"C3 10x10 K=4, {a.requests} requests per call", "hbm_peak_TBps": HBM_PEAK / 1e12}
    for ne in [int(x) for x in a.evidence.split(",")]:
        q, ev, ec = netspec.c3_requests(100, 4, a.requests, ne, seed=a.seed)
        evars, qvars = ids[ev], ids[q].reshape(-1, 1)
        n, dt = timed(lambda: eng.query_fixed(none, evars, ec, flags=_capi.Q_UNNORMALISED), a.seconds, eng.synchronize)
        st = eng.stats()
        gbs = st["alg_bytes"] / (st["kernel_ms"] * 1e-3) / 1e9 if st["kernel_ms"] else 0.0
        nq, dtq = timed(lambda: eng.query_fixed(qvars, evars, ec), a.seconds, eng.synchronize)
        stq = eng.stats()
        out[f"evidence_{ne}"] = {
            "pe_per_s": round(n * a.requests / dt, 1),
            "pe_calls": n,
            "bytes_per_request": round(st["alg_bytes"] / a.requests, 1),
            "all_kernel_GBps": round(gbs, 1),
            "all_kernel_share_of_hbm_peak": round(gbs * 1e9 / HBM_PEAK, 4),
            "last_call_total_ms": round(st["total_ms"], 2),
            "last_call_plan_ms": round(st["plan_ms"], 2),
            "last_call_kernel_ms": round(st["kernel_ms"], 2),
            "sum_queries_per_s": round(nq * a.requests / dtq, 1),
            "sum_bytes_per_request": round(stq["alg_bytes"] / a.requests, 1),
        }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
