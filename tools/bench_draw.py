"""Throughput of exact posterior sampling (mibn_posterior_sample_batch) on the C3 workload, beside forward sampling (mibn_sample,
same number of rows) and the MPE path (mibn_mpe_batch, same requests) in the same process.

    python tools/bench_draw.py [--evidence 4] [--seconds 2] [--seed 1] [--no-prune]

Workload: the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), evidence sets of netspec.c3_requests (seeded,
4 evidence variables).  Two shapes: (a) one request x 1 M samples, (b) 1 024 requests x 1 024 samples.  Per shape one warm-up
call, then calls until at least --seconds have passed.  Prints one JSON line per shape: elimination ms (ve_sum_kernel), draw ms
(posterior_draw_kernel), samples/s end to end and of the draw kernel alone, table bytes gathered per sample, and the draw
kernel's share of its latency bound:

    bound = rows / resident lanes x draws per row x (one LDS round trip + one L2-hit global load), on 256 CUs at 2.4 GHz,

resident lanes = 64 x waves per CU that the kernel's LDS state and its 70 VGPRs allow - the time the chain of dependent gathers
takes when nothing but occupancy hides it and every table read hits the L2.
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

CLOCK_HZ, N_CU, LDS_PER_CU = 2.4e9, 256, 160 * 1024
L2_HIT_CYC, LDS_CYC = 200.0, 50.0  # global_load_dword L2-hit latency, ds_read latency (one lane, idle chip)
DRAW_WG, VGPR_WAVES_PER_SIMD = 256, 7


def timed(fn, seconds):
    fn()  # warm-up
    n = 0
    t0 = time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    return n, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evidence", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-prune", action="store_true", help="every CPT takes part (the path of sparse CPTs)")
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    be = bn.backend
    eng = be.engine
    ids = np.array([be.var_id(f"{i:03d}") for i in range(100)], np.int32)
    flags = 0 if a.no_prune else _capi.DRAW_PRUNE
    n_vars = 100
    lds = n_vars * DRAW_WG + DRAW_WG
    waves_per_cu = min(LDS_PER_CU // lds, VGPR_WAVES_PER_SIMD) * (DRAW_WG // 64)
    for tag, n_req, n_samples in (("a", 1, 1 << 20), ("b", 1024, 1024)):
        _, ev, ec = netspec.c3_requests(100, 4, n_req, a.evidence, seed=a.seed)
        evars = ids[ev]
        rows = n_req * n_samples
        n, dt = timed(lambda: eng.posterior_sample(evars, ec, n_samples, seed=a.seed, flags=flags), a.seconds)
        st = eng.stats()
        ks = {k["name"]: k for k in eng.kernel_stats()}
        el = ks.get("ve_sum_kernel", {"ms": 0.0, "alg_bytes": 0.0, "launches": 0})
        dr = ks.get("posterior_draw_kernel", {"ms": 0.0, "alg_bytes": 0.0, "launches": 0})
        draws_per_row = n_vars - a.evidence
        bound_ms = rows / (N_CU * waves_per_cu * 64) * draws_per_row * (L2_HIT_CYC + LDS_CYC) / CLOCK_HZ * 1e3
        nf, dtf = timed(lambda: eng.sample(rows, [], [], seed=a.seed), a.seconds)
        nm, dtm = timed(lambda: eng.mpe(evars, ec), a.seconds)
        out = {
            "shape": tag,
            "workload": f"C3 10x10 K=4, {a.evidence} evidence, {n_req} requests x {n_samples} samples, prune={int(bool(flags))}",
            "samples_per_s": round(n * rows / dt, 1),
            "calls": n,
            "window_s": round(dt, 3),
            "elimination_ms": round(el["ms"], 3),
            "elimination_launches": int(el["launches"]),
            "draw_ms": round(dr["ms"], 3),
            "draw_launches": int(dr["launches"]),
            "draw_kernel_samples_per_s": round(rows / (dr["ms"] * 1e-3), 1) if dr["ms"] else 0.0,
            "gathered_bytes_per_sample": round(dr["alg_bytes"] / rows, 1),
            "draw_gather_GBps": round(dr["alg_bytes"] / (dr["ms"] * 1e-3) / 1e9, 1) if dr["ms"] else 0.0,
            "draw_resident_waves_per_cu": int(waves_per_cu),
            "draw_latency_bound_ms": round(bound_ms, 3),
            "draw_share_of_latency_bound": round(bound_ms / dr["ms"], 4) if dr["ms"] else 0.0,
            "last_call_total_ms": round(st["total_ms"], 2),
            "last_call_plan_ms": round(st["plan_ms"], 2),
            "last_call_d2h_ms": round(st["d2h_ms"], 2),
            "arena_MB": round(st["arena_bytes"] / 1e6, 1),
            "forward_samples_per_s": round(nf * rows / dtf, 1),
            "mpe_per_s": round(nm * n_req / dtm, 1),
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
