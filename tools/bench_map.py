"""Throughput of the marginal MAP path (mibn_map_batch) on the C3 workload, beside the sum path's `query` over the same M.

    python tools/bench_map.py [--requests 32768] [--evidence 4] [--map-vars 4,8] [--seconds 2] [--seed 1]

Workload: the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), evidence sets of netspec.c3_requests (seeded,
4 evidence variables), and per request |M| MAP variables drawn uniformly from the others (default_rng(seed + |M|)).  A request
whose max phase would need a table of 2^31 cells - the planner's limit, inherent to marginal MAP - is redrawn until it plans
(counted in "redrawn").  Per |M|: one warm-up call, then calls of the whole batch until at least --seconds have passed, the
window ended by a device synchronise; then the sum path (query_fixed, the dense posterior over the same M - the argmax of it
would be taken on the host) in the same process.  Prints one JSON line per |M|: MAP/s, bytes per request (tables + argmax),
ve_map_kernel's GB/s and its share of the 8 TB/s HBM peak, the planning ms of the last call, and the sum path's queries/s.
The sum phase of a map program uses the GENERIC step form only; a grid request with scattered M carries M through its frontier
tables, so --requests well below the default keeps a run short.
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


def draw_map_vars(planner, ids, ev, nm, seed):
    """[B, nm] MAP variables (network ids), none of them evidence; a request the planner refuses (cell limit) is redrawn."""
    rng = np.random.default_rng(seed)
    out = np.empty((len(ev), nm), np.int32)
    redrawn = 0
    for r in range(len(ev)):
        free = np.setdiff1d(np.arange(100), ev[r])
        while True:
            out[r] = ids[rng.choice(free, size=nm, replace=False)]
            try:  # (the sum program over the same variables hits the same frontier tables: a cheap host-only probe)
                planner.plan_stats(out[r], ids[ev[r]])
                break
            except _capi.MibnError:
                redrawn += 1
    return out, redrawn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32768)
    ap.add_argument("--evidence", type=int, default=4)
    ap.add_argument("--map-vars", default="4,8")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    be = bn.backend
    eng = be.engine
    q, ev, ec = netspec.c3_requests(100, 4, a.requests, a.evidence, seed=a.seed)
    ids = np.array([be.var_id(f"{i:03d}") for i in range(100)], np.int32)
    evars = ids[ev]
    for nm in (int(x) for x in a.map_vars.split(",")):
        mvars, redrawn = draw_map_vars(eng, ids, ev, nm, a.seed + nm)
        try:
            n, dt = timed(lambda: eng.map(mvars, evars, ec, flags=_capi.MAP_PRUNE), a.seconds, eng.synchronize)
        except _capi.MibnError as e:  # (a request past the probe whose map program still meets the cell limit)
            print(json.dumps({"workload": f"|M| = {nm}", "error": e.msg}), flush=True)
            continue
        st = eng.stats()
        ks = {k["name"]: k for k in eng.kernel_stats()}
        mk = ks.get("ve_map_kernel", {"ms": 0.0, "alg_bytes": 0.0})
        tb = ks.get("map_traceback_kernel", {"ms": 0.0})
        gbs = mk["alg_bytes"] / (mk["ms"] * 1e-3) / 1e9 if mk["ms"] else 0.0
        nq, dtq = timed(lambda: eng.query_fixed(mvars, evars, ec), a.seconds, eng.synchronize)
        out = {
            "workload": f"C3 10x10 K=4, {a.evidence} evidence, |M| = {nm}, {a.requests} requests per call",
            "map_per_s": round(n * a.requests / dt, 2),
            "map_calls": n,
            "map_window_s": round(dt, 3),
            "redrawn": redrawn,
            "bytes_per_request": round(st["alg_bytes"] / a.requests, 1),
            "ve_map_kernel_ms": round(mk["ms"], 3),
            "ve_map_kernel_GBps": round(gbs, 1),
            "ve_map_kernel_share_of_hbm_peak": round(gbs * 1e9 / HBM_PEAK, 4),
            "sum_tiles": ks.get("ve_map_kernel:sum tiles", {"launches": 0})["launches"],
            "max_tiles": ks.get("ve_map_kernel:max tiles", {"launches": 0})["launches"],
            "map_traceback_kernel_ms": round(tb["ms"], 3),
            "last_call_total_ms": round(st["total_ms"], 2),
            "last_call_plan_ms": round(st["plan_ms"], 2),
            "last_call_kernel_ms": round(st["kernel_ms"], 2),
            "sum_queries_per_s": round(nq * a.requests / dtq, 2),
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
