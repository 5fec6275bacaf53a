"""Throughput of the E-step of BayesNet.fit_em (mibn_expect_batch: planned queries + expect_kernel) on the C3 grid, beside the same
E-step done the naive way - every posterior downloaded (mibn_query_batch_ex with MIBN_Q_UNNORMALISED) and scattered into the family
tables with np.add.at - in the same process.

    python tools/bench_em.py [--rows 2000] [--missing 0.05,0.15,0.30] [--repeats 3] [--sub-batch 32768] [--seed 1]

Workload: the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), rows drawn with bn.sample, cells knocked out
independently.  Per setting one JSON line: rows/s and requests/s of an E-step (best of --repeats after one warm-up, host clock around
blocking calls), planning / kernel / expect_kernel ms of the last expect call, the naive E-step's time and its numpy share, and the
largest difference between the two accumulation buffers.  The requests are built once, outside the timed region (fit_em does the
same: they do not change between iterations).
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
from sorobn_amd import _capi, learning  # noqa: E402


def naive_e_step(eng, card, batches, n_acc):
    """query_batch download + np.add.at: -> (acc, seconds spent in numpy)."""
    acc = np.zeros(n_acc)
    host = 0.0
    for rq in batches:
        out, out_off = eng.query_batch(rq["q_off"], rq["q_vars"], rq["e_off"], rq["e_vars"], rq["e_codes"], out_off=rq["out_off"],
                                       flags=_capi.Q_UNNORMALISED)
        t0 = time.perf_counter()
        cells = np.diff(out_off)
        s = np.add.reduceat(out, out_off[:-1])
        req = np.repeat(np.arange(len(cells)), cells)
        idx = np.arange(len(out)) - out_off[:-1][req]
        nq = np.diff(rq["q_off"])
        target = rq["acc_base"][req].copy()
        # mixed-radix decode of the slice index, last query variable fastest
        for k in range(int(nq.max()) if len(nq) else 0):
            has = nq > k
            pos = np.where(has, rq["q_off"][1:] - 1 - k, 0)
            c = np.where(has, card[rq["q_vars"][pos]], 1)[req]
            st = np.where(has, rq["acc_stride"][pos], 0)[req]
            target += (idx % c) * st
            idx //= c
        keep = (nq[req] > 0) & (s[req] > 0)
        np.add.at(acc, target[keep], out[keep] / s[req][keep])
        host += time.perf_counter() - t0
    return acc, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--missing", default="0.05,0.15,0.30")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sub-batch", type=int, default=32768)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    bn.seed = a.seed
    be = bn.backend
    eng = be.engine
    f = be.flat
    card = np.asarray(f.card)
    scopes = [list(map(int, sc)) for sc in f.scope]
    fam_off, strides = learning.em_family_layout(scopes, card)
    n_acc = int(fam_off[-1])
    full = bn.sample(a.rows)[list(f.names)].to_numpy().astype(np.int32)  # (grid labels are their own codes)
    rng = np.random.default_rng(a.seed)
    for frac in [float(x) for x in a.missing.split(",")]:
        codes = np.where(rng.random(full.shape) < frac, -1, full).astype(np.int32)
        batches = [learning.em_requests(codes, rows, scopes, strides, fam_off) for rows in learning.em_sub_batches(codes, scopes, a.sub_batch)]
        n_req = sum(len(rq["acc_base"]) for rq in batches)
        for rq in batches:  # the naive path's result offsets, outside the timed region like the requests themselves
            cells = np.multiply.reduceat(np.append(card[rq["q_vars"]], 1).astype(np.int64), np.minimum(rq["q_off"][:-1], len(rq["q_vars"])))
            rq["out_off"] = np.concatenate([[0], np.cumsum(np.where(np.diff(rq["q_off"]) > 0, cells, 1))]).astype(np.int64)

        def device():
            acc = np.zeros(n_acc)
            for rq in batches:
                eng.expect_batch(rq["q_off"], rq["q_vars"], rq["e_off"], rq["e_vars"], rq["e_codes"], rq["acc_base"], rq["acc_stride"], acc)
            return acc
        device()  # warm-up
        best, acc = 1e30, None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            acc = device()
            best = min(best, time.perf_counter() - t0)
        st = eng.stats()
        ek = [k for k in eng.kernel_stats() if k["name"] == "expect_kernel"]
        naive_e_step(eng, card, batches, n_acc)  # warm-up
        nbest, nhost, nacc = 1e30, 0.0, None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            nacc, host = naive_e_step(eng, card, batches, n_acc)
            dt = time.perf_counter() - t0
            if dt < nbest:
                nbest, nhost = dt, host
        print(json.dumps({
            "workload": f"C3 10x10 K=4, {a.rows} rows, {frac:.0%} of the cells missing", "requests": n_req, "calls": len(batches),
            "query_vars_per_request": round(float(np.mean(np.concatenate([np.diff(rq['q_off']) for rq in batches]))), 2),
            "evidence_per_request": round(float(np.mean(np.concatenate([np.diff(rq['e_off']) for rq in batches]))), 1),
            "e_step_s": round(best, 4), "rows_per_s": round(a.rows / best, 1), "requests_per_s": round(n_req / best, 1),
            "last_call_total_ms": round(st["total_ms"], 2), "last_call_plan_ms": round(st["plan_ms"], 2),
            "last_call_kernel_ms": round(st["kernel_ms"], 2), "last_call_expect_kernel_ms": round(ek[0]["ms"], 3) if ek else None,
            "naive_e_step_s": round(nbest, 4), "naive_numpy_s": round(nhost, 4), "naive_requests_per_s": round(n_req / nbest, 1),
            "max_abs_diff_device_vs_naive": float(np.max(np.abs(acc - nacc))),
        }), flush=True)


if __name__ == "__main__":
    main()
