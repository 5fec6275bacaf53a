"""Throughput of constraint-based structure learning (structure.pc: mibn_ci_tests = count_kernel + the kernels of
csrc/citest_kernel.hip.h) on rows sampled from the C3 grid, beside the same batches of tests done the way the library allowed before
mibn_ci_tests - every table counted by Engine.count_tables, downloaded, and the statistic computed in numpy - in the same process.

    python tools/bench_citest.py [--rows 100000,1000000] [--max-cond 3] [--alpha 0.01] [--seed 1] [--baseline-cap 20000]

Workload: the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe, 100 columns, 180 edges), rows drawn with bn.sample,
PC-stable with G2 and the classic degrees of freedom.  Per row count one JSON line: the tests of every level, the device's ms per level
split into count_kernel and citest_kernel (last-call statistics of the level's one call), the wall time of the call and of the host's
p-values, tests/s over the whole search (wall clock of the calls, the p-values and the search itself), the edges of the skeleton
that are edges of the grid out of 180, and the baseline's wall time and tests/s on the same recorded batches (a level above
--baseline-cap tests is measured on its first --baseline-cap tests and scaled), with the largest difference between the statistics.
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
from sorobn_amd import learning  # noqa: E402


def numpy_g2(tables, shapes):
    """G2 of dense tables [(q, rx, ry)], strata by strata in numpy."""
    out = np.zeros(len(tables))
    for i, (t, (q, rx, ry)) in enumerate(zip(tables, shapes)):
        t = t.reshape(q, rx, ry).astype(np.float64)
        nz = t.sum(axis=(1, 2), keepdims=True)
        nx = t.sum(axis=2, keepdims=True)
        ny = t.sum(axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = t * np.log((t * nz) / (nx * ny))
        out[i] = 2.0 * float(term[t > 0].sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--max-cond", type=int, default=3)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--baseline-cap", type=int, default=20000)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    spec = gu.grid_spec_from_recipe(entry)
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    bn.seed = a.seed
    names = list(spec["nodes"])
    truth = {frozenset((names.index(p), v)) for v, nm in enumerate(names) for p in spec["cpts"][nm]["names"][:-1]}
    eng = learning.counting_engine(0)
    for n_rows in [int(x) for x in a.rows.split(",")]:
        X = bn.sample(n_rows)[names]
        codes, _, cards = learning.encode_complete(X, names)
        levels, batches = [], []
        with eng.dataset(codes, cards) as ds:
            def tester(batch):
                t0 = time.perf_counter()
                stat, adj = ds.ci_tests([(*S, x, y) for x, y, S in batch], "g2")
                t1 = time.perf_counter()
                ks = {k["name"]: k for k in eng.kernel_stats()}
                dof = [int(np.prod([cards[z] for z in S], dtype=np.int64)) * (cards[x] - 1) * (cards[y] - 1) for x, y, S in batch]
                p = [learning.chi2_sf(s, d) for s, d in zip(stat.tolist(), dof)]
                t2 = time.perf_counter()
                levels.append({"tests": len(batch), "call_ms": round(1e3 * (t1 - t0), 2), "count_kernel_ms": round(ks["count_kernel"]["ms"], 3),
                               "citest_kernel_ms": round(ks["citest_kernel"]["ms"], 3), "launches": int(ks["count_kernel"]["launches"] + ks["citest_kernel"]["launches"]),
                               "p_value_ms": round(1e3 * (t2 - t1), 2)})
                batches.append((list(batch), stat))
                return p

            learning._pc_search(len(names), lambda b: [1.0] * len(b), a.alpha, 0)  # (imports, allocator)
            ds.ci_tests([(0, 1)], "g2")  # warm-up: module load, buffers
            t0 = time.perf_counter()
            found = learning._pc_search(len(names), tester, a.alpha, a.max_cond)
            wall = time.perf_counter() - t0
        n_tests = sum(lv["tests"] for lv in levels)
        skeleton = {frozenset((u, v)) for u in range(len(names)) for v in found["adj"][u]}
        # the same batches without mibn_ci_tests: count_tables (uploads the rows per call, downloads every table) + numpy
        base_s, worst = 0.0, 0.0
        for batch, stat in batches:
            part = batch[:a.baseline_cap]
            t0 = time.perf_counter()
            tables = eng.count_tables(codes, cards, [(*S, x, y) for x, y, S in part])
            shapes = [(int(np.prod([cards[z] for z in S], dtype=np.int64)), cards[x], cards[y]) for x, y, S in part]
            got = numpy_g2(tables, shapes)
            base_s += (time.perf_counter() - t0) * len(batch) / len(part)
            worst = max(worst, float(np.max(np.abs(got - stat[:len(part)]) / np.maximum(1.0, np.abs(got)))))
        print(json.dumps({
            "workload": f"C3 10x10 K=4, {n_rows} rows, pc max_cond={a.max_cond} alpha={a.alpha} g2", "levels": levels, "tests": n_tests,
            "search_s": round(wall, 4), "tests_per_s": round(n_tests / wall, 1),
            "device_ms": round(sum(lv["count_kernel_ms"] + lv["citest_kernel_ms"] for lv in levels), 3),
            "count_share_of_device": round(sum(lv["count_kernel_ms"] for lv in levels) / max(1e-9, sum(lv["count_kernel_ms"] + lv["citest_kernel_ms"] for lv in levels)), 4),
            "skeleton_edges": len(skeleton), "true_edges_recovered": len(skeleton & truth), "true_edges": len(truth),
            "baseline_s": round(base_s, 4), "baseline_tests_per_s": round(n_tests / base_s, 1), "max_rel_diff_vs_numpy": worst,
        }), flush=True)


if __name__ == "__main__":
    main()
