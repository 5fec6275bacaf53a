"""Exact arc posteriors on the first 16, 20 and 24 columns of the C3 grid (10 x 10, K = 4): what DESIGN section 26 records.

    python tools/bench_arc_posterior.py [--columns 16 20] [--once 24] [--rows 10000] [--repeat 5] [--n-boot 100] [--seed 1] [--sim PATH]

Rows are drawn with bn.sample from the BASELINE grid (tests/golden/grid10x10.json recipe), as tools/bench_exact.py draws them.
BDeu (ess 1), max_parents 3.  One JSON line per size, all in one process after a warm-up; kernel times are the engine's own event
times (last-call kernel statistics), medians of --repeat calls with [min, max]; the two device calls alternate:

  posterior  mibn_arc_posteriors on the scores of ONE mibn_score_families call: its four statistics rows and its wall time;
  best_dag   mibn_best_dag on the same candidates: dag_subset_kernel and dag_sink_kernel, the wall time;
  cpu        tools/dag_post_sim (the same schedule on one CPU core) on the same candidates: the time between its check and its
             outputs, the wall time of the process (reading the candidates as text included), its largest deviation from the device;
  bootstrap  structure.bootstrap(n_boot) of hill_climb on the same frame, once: the frequentist answer to the same question;
  end to end structure.arc_posteriors(X), encoding and scoring included.
Sizes under --once (default 24: 1.9 GB of tables) make one timed call of each device entry point after one warm-up call, and skip
the bootstrap.  --sim: a dag_post_sim built beforehand (default: built here with g++ into a temporary directory)."""
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

POST_ROWS = ("dag_post_subset_kernel", "dag_post_level_kernel", "dag_post_superset_kernel", "dag_post_arc_kernel")
BEST_ROWS = ("dag_subset_kernel", "dag_sink_kernel")


def rows_ms(engine):
    return {k["name"]: k["ms"] for k in engine.kernel_stats()}


def span(v):
    return [round(float(min(v)), 3), round(float(max(v)), 3)]


def med(v):
    return round(float(np.median(v)), 3)


def summary(runs, names):
    out = {"wall_ms": med(runs["wall"]), "wall_min_max": span(runs["wall"])}
    for k in names:
        out[k + "_ms"] = med(runs[k])
        out[k + "_min_max"] = span(runs[k])
    out["kernels_ms"] = med([sum(r) for r in zip(*[runs[k] for k in names])])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--once", type=int, nargs="*", default=[24])
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--n-boot", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sim", default=None)
    a = ap.parse_args()
    sim = a.sim
    if sim is None:
        sim = os.path.join(tempfile.mkdtemp(), "dag_post_sim")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "dag_post_sim.cpp"), "-o", sim])
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    bn.seed = a.seed
    X_all = bn.sample(a.rows)
    engine = learning.counting_engine()
    structure.arc_posteriors(X_all[list(X_all.columns)[:6]].iloc[:2000])  # warm-up: library, kernels, buffers
    for n in list(a.columns) + list(a.once):
        once = n not in a.columns
        repeat = 1 if once else a.repeat
        X = X_all[list(X_all.columns)[:n]].reset_index(drop=True)
        cols = list(X.columns)
        codes, _, cards = learning.encode_complete(X, cols)
        _, cand = learning._exact_plan(X, "bdeu", 1.0, 3, (), (), 2_000_000, lambda: cards)
        children, masks = [v for v, _ in cand], [pm for _, pm in cand]
        with engine.dataset(codes, cards) as ds:
            scores = ds.score_families([learning._mask_scope(v, pm) for v, pm in cand], "bdeu", 1.0)
        out = {"columns": n, "rows": a.rows, "families": len(cand), "score": "bdeu", "max_parents": 3, "timed_calls": repeat}
        post = {k: [] for k in ("wall",) + POST_ROWS}
        best = {k: [] for k in ("wall",) + BEST_ROWS}
        res = None
        for i in range(repeat + 1):  # (the first round is the warm-up)
            t0 = time.perf_counter()
            res = engine.arc_posteriors(n, children, masks, scores)
            w = 1e3 * (time.perf_counter() - t0)
            k = rows_ms(engine)
            if i:
                post["wall"].append(w)
                for name in POST_ROWS:
                    post[name].append(k[name])
            t0 = time.perf_counter()
            engine.best_dag(n, children, masks, scores)
            w = 1e3 * (time.perf_counter() - t0)
            k = rows_ms(engine)
            if i:
                best["wall"].append(w)
                for name in BEST_ROWS:
                    best[name].append(k[name])
        out["posterior"] = summary(post, POST_ROWS)
        out["best_dag"] = summary(best, BEST_ROWS)
        out["posterior_over_best_dag_kernels"] = round(out["posterior"]["kernels_ms"] / out["best_dag"]["kernels_ms"], 2)
        out["log_evidence"] = res[2]
        # ---- the same schedule on a CPU core
        text = f"{n} 0 0 0 {len(cand)}\n" + "\n".join(f"{v} {pm} {float(s)!r}" for (v, pm), s in zip(cand, scores)) + "\n"
        t0 = time.perf_counter()
        got = json.loads(subprocess.run([sim], input=text, capture_output=True, text=True, check=True).stdout)
        wall = 1e3 * (time.perf_counter() - t0)
        as_f64 = lambda key: np.array(got[key], np.uint64).view(np.float64)  # noqa: E731
        out["cpu_sim"] = {"one_core_ms": round(1e3 * got["seconds"], 1), "process_wall_ms": round(wall, 1),
                          "max_dev_log_post": float(np.abs(as_f64("log_post_bits") - res[0]).max()),
                          "max_dev_arc": float(np.abs(as_f64("arc_bits").reshape(n, n) - res[1]).max()),
                          "dev_log_evidence": float(abs(as_f64("log_evidence_bits")[0] - res[2]))}
        # ---- end to end, and the bootstrap beside it
        e2e = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            ap_ = structure.arc_posteriors(X)
            e2e.append(1e3 * (time.perf_counter() - t0))
        out["end_to_end"] = {"arc_posteriors_ms": med(e2e), "min_max": span(e2e), "pairs_with_strength_over_half": int((ap_.frame["strength"] >= 0.5).sum())}
        if not once:
            t0 = time.perf_counter()
            bs = structure.bootstrap(X, n_boot=a.n_boot, seed=a.seed)
            ms = 1e3 * (time.perf_counter() - t0)
            out["bootstrap"] = {"n_boot": a.n_boot, "learner": "hill_climb", "ms": round(ms, 1), "pairs_with_strength_over_half": int((bs.frame["strength"] >= 0.5).sum()),
                                "over_arc_posteriors": round(ms / out["end_to_end"]["arc_posteriors_ms"], 1)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
