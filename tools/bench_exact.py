"""Exact structure learning on the first 16 and 20 columns of the C3 grid (10 x 10, K = 4): what DESIGN section 25 records.

    python tools/bench_exact.py [--columns 16 20] [--rows 10000 1000000] [--repeat 5] [--seed 1] [--sim PATH]

Rows are drawn with bn.sample from the BASELINE grid (tests/golden/grid10x10.json recipe), as tools/bench_bootstrap.py draws them.
BIC, max_parents 3.  One JSON line per (columns, rows), all in one process after a warm-up; kernel times are the engine's own
event times (last-call kernel statistics), medians of --repeat calls with [min, max]; calls that are compared alternate:

  scoring    the ONE mibn_score_families call over every candidate family: its kernels and its wall time;
  dp         mibn_best_dag on those scores under the default passes and with dag_tile_bits = dag_group_bits = 1 (one index bit per
             pass over the whole table - what the tiling replaces): the rows dag_subset_kernel and dag_sink_kernel, the wall time;
  cpu        tools/dag_plan_sim (the same schedule on one CPU core) on the same candidates: its phases A + B, and the wall time of
             the process (which includes reading the candidates as text);
  end to end structure.exact_search(X), encoding included; hill_climb's total beside the exact total.
--sim: a dag_plan_sim built beforehand (default: built here with g++ into a temporary directory)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import golden_util as gu  # noqa: E402
import netspec  # noqa: E402
import sorobn_amd  # noqa: E402
from sorobn_amd import learning, structure  # noqa: E402


def rows_ms(engine):
    return {k["name"]: k for k in engine.kernel_stats()}


def span(v):
    return [round(float(min(v)), 3), round(float(max(v)), 3)]


def med(v):
    return round(float(np.median(v)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--rows", type=int, nargs="+", default=[10_000, 1_000_000])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sim", default=None)
    a = ap.parse_args()
    sim = a.sim
    if sim is None:
        sim = os.path.join(tempfile.mkdtemp(), "dag_plan_sim")
        subprocess.check_call(["g++", "-O2", "-mpopcnt", "-std=c++17", os.path.join(ROOT, "tools", "dag_plan_sim.cpp"), "-o", sim])
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    bn.seed = a.seed
    X_all = bn.sample(max(a.rows))
    engine = learning.counting_engine()
    structure.exact_search(X_all[list(X_all.columns)[:6]].iloc[:2000])  # warm-up: library, kernels, buffers
    for n in a.columns:
        for n_rows in a.rows:
            X = X_all[list(X_all.columns)[:n]].iloc[:n_rows].reset_index(drop=True)
            cols = list(X.columns)
            codes, _, cards = learning.encode_complete(X, cols)
            _, cand = learning._exact_plan(X, "bic", 1.0, 3, (), (), 2_000_000, lambda: cards)
            scopes = [learning._mask_scope(v, pm) for v, pm in cand]
            children, masks = [v for v, _ in cand], [pm for _, pm in cand]
            out = {"columns": n, "rows": n_rows, "families": len(cand), "score": "bic", "max_parents": 3}
            # ---- scoring
            with engine.dataset(codes, cards) as ds:
                wall, count, reduce = [], [], []
                for _ in range(a.repeat + 1):  # (the first call is the warm-up)
                    t0 = time.perf_counter()
                    scores = ds.score_families(scopes, "bic")
                    wall.append(1e3 * (time.perf_counter() - t0))
                    k = rows_ms(engine)
                    count.append(k["count_kernel"]["ms"])
                    reduce.append(k["score_kernel"]["ms"])
            out["scoring"] = {"wall_ms": med(wall[1:]), "wall_min_max": span(wall[1:]), "count_kernel_ms": med(count[1:]), "count_min_max": span(count[1:]),
                              "score_kernel_ms": med(reduce[1:]), "score_min_max": span(reduce[1:])}
            # ---- the DP: default passes and one bit per pass, alternating
            runs = {"default": {"wall": [], "subset": [], "sink": []}, "one_bit": {"wall": [], "subset": [], "sink": []}}
            launches, results = {}, {}
            for i in range(a.repeat + 1):
                for name, (t, g) in (("default", (12, 6)), ("one_bit", (1, 1))):
                    engine.set_option("dag_tile_bits", t)
                    engine.set_option("dag_group_bits", g)
                    t0 = time.perf_counter()
                    res = engine.best_dag(n, children, masks, scores)
                    w = 1e3 * (time.perf_counter() - t0)
                    k = rows_ms(engine)
                    launches[name] = int(k["dag_subset_kernel"]["launches"])
                    results[name] = res
                    if i:
                        runs[name]["wall"].append(w)
                        runs[name]["subset"].append(k["dag_subset_kernel"]["ms"])
                        runs[name]["sink"].append(k["dag_sink_kernel"]["ms"])
            engine.set_option("dag_tile_bits", 12)
            engine.set_option("dag_group_bits", 6)
            for name, r in runs.items():
                out["dp_" + name] = {"subset_launches": launches[name], "dag_subset_kernel_ms": med(r["subset"]), "subset_min_max": span(r["subset"]),
                                     "dag_sink_kernel_ms": med(r["sink"]), "sink_min_max": span(r["sink"]), "wall_ms": med(r["wall"]), "wall_min_max": span(r["wall"])}
            d, o = results["default"], results["one_bit"]
            out["same_bits_either_way"] = bool(np.array_equal(d[0], o[0]) and np.array_equal(d[1], o[1]) and d[2] == o[2])
            # ---- the same schedule on a CPU core
            text = f"{n} 0 0 0 {len(cand)}\n" + "\n".join(f"{v} {pm} {float(s)!r}" for (v, pm), s in zip(cand, scores)) + "\n"
            t0 = time.perf_counter()
            got = json.loads(subprocess.run([sim], input=text, capture_output=True, text=True, check=True).stdout)
            out["cpu_sim"] = {"phases_ms": round(1e3 * got["seconds"], 1), "process_wall_ms": round(1e3 * (time.perf_counter() - t0), 1),
                              "same_result": got["parents"] == d[0].tolist() and got["order"] == d[1].tolist() and got["total"] == d[2]}
            # ---- end to end, and hill climbing beside it
            e2e = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                result, info = structure.exact_search(X, return_info=True)
                e2e.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            _, _, hc_total = structure.hill_climb(X, return_trace=True)
            hc_ms = 1e3 * (time.perf_counter() - t0)
            out["end_to_end"] = {"exact_search_ms": med(e2e), "min_max": span(e2e), "edges": sum(isinstance(e, tuple) for e in result),
                                 "exact_total": info["total"], "hill_climb_total": hc_total, "exact_minus_hill_climb": info["total"] - hc_total,
                                 "hill_climb_ms": round(hc_ms, 1)}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
