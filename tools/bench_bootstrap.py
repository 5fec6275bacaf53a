"""Row weights and bootstrap arc strengths on the first 20 columns of the C3 grid (10 x 10, K = 4): what DESIGN section 24 records.

    python tools/bench_bootstrap.py [--rows 1000000] [--boot-rows 1000000] [--n-boot 100] [--loop-replicates 100] [--repeat 5] [--seed 1]

Rows are drawn with bn.sample from the BASELINE grid (tests/golden/grid10x10.json recipe).  One JSON line per measurement, all in one
process after a warm-up; kernel times are the engine's own event times (last-call kernel statistics), medians of --repeat calls
with their smallest and largest value; calls that are compared alternate:

  counting   the first hill-climb sweep (n + n (n - 1) families) over --rows rows: count_kernel (unweighted call) beside
             count_weighted_kernel under an all-ones set and under a bootstrap set, each with its ratio to count_kernel;
  packing    the same sweep under 4 bootstrap sets in one call, tables of one scope next to each other, with the cell index kept
             across them (option weighted_share = 1) and recomputed per table (0), and set-major (no neighbours to share with);
  draw       mibn_dataset_bootstrap of --n-boot sets over --rows rows, wall time of the blocking call (allocation, zeroing, kernel);
  bootstrap  structure.bootstrap(n_boot, hill_climb) over --boot-rows rows end to end beside the loop the parent commit allows:
             hill_climb(X.iloc[the rows the same weight sets stand for]) per replicate (--loop-replicates of them, scaled to n_boot),
             and whether both give the same edges.
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
from sorobn_amd import learning, structure  # noqa: E402


def kernel_ms(engine, name):
    return next((k["ms"] for k in engine.kernel_stats() if k["name"] == name), 0.0)


def spread_ms(engine, name, call, repeat):
    out = []
    for _ in range(repeat):
        call()
        out.append(kernel_ms(engine, name))
    return out


def span(v):
    return [round(float(min(v)), 3), round(float(max(v)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--boot-rows", type=int, default=1_000_000)
    ap.add_argument("--n-boot", type=int, default=100)
    ap.add_argument("--loop-replicates", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    bn.seed = a.seed
    X = bn.sample(max(a.rows, a.boot_rows))
    X = X[list(X.columns)[:20]]
    cols = list(X.columns)
    n = len(cols)
    engine = learning.counting_engine()
    structure.bootstrap(X.iloc[:2000], n_boot=3, max_iter=2)  # warm-up: library, kernels, buffers
    structure.hill_climb(X.iloc[:2000], max_iter=2)

    # ---- counting and packing
    codes, _, cards = learning.encode_complete(X.iloc[:a.rows], cols)
    sweep = [(v,) for v in range(n)] + [(u, v) for v in range(n) for u in range(n) if u != v]
    with engine.dataset(codes, cards) as ds:
        draws = []
        for _ in range(a.repeat + 1):  # (the first call is the warm-up)
            t0 = time.perf_counter()
            ds.bootstrap(a.n_boot, a.seed)
            draws.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"measurement": "draw", "rows": a.rows, "sets": a.n_boot, "draws": a.rows * a.n_boot,
                          "mibn_dataset_bootstrap_wall_ms": round(float(np.median(draws[1:])), 2), "min_max_ms": span(draws[1:])}), flush=True)
        boot = ds.bootstrap(4, a.seed, return_weights=True)
        zero_share = float((boot[0] == 0).mean())
        ds.set_weights(np.concatenate([boot, np.ones((1, a.rows), np.uint32)]))
        ones = np.full(len(sweep), 4, np.int32)
        r_base, r_ones, r_boot = [], [], []
        for _ in range(a.repeat):  # alternating, as above
            r_base += spread_ms(engine, "count_kernel", lambda: ds.score_families(sweep, "bic"), 1)
            r_ones += spread_ms(engine, "count_weighted_kernel", lambda: ds.score_families(sweep, "bic", wset=ones), 1)
            r_boot += spread_ms(engine, "count_weighted_kernel", lambda: ds.score_families(sweep, "bic", wset=np.zeros(len(sweep), np.int32)), 1)
        base, w_ones, w_boot = (float(np.median(v)) for v in (r_base, r_ones, r_boot))
        print(json.dumps({"measurement": "counting", "rows": a.rows, "tables": len(sweep), "zero_weight_share_of_a_bootstrap_set": round(zero_share, 4),
                          "count_kernel_ms": round(base, 3), "count_weighted_kernel_all_ones_ms": round(w_ones, 3),
                          "all_ones_over_count_kernel": round(w_ones / base, 3), "count_weighted_kernel_bootstrap_set_ms": round(w_boot, 3),
                          "bootstrap_set_over_count_kernel": round(w_boot / base, 3),
                          "min_max_ms": {"count_kernel": span(r_base), "all_ones": span(r_ones), "bootstrap_set": span(r_boot)}}), flush=True)
        by_scope = [f for f in sweep for _ in range(4)]
        by_scope_sets = np.tile(np.arange(4, dtype=np.int32), len(sweep))
        by_set = sweep * 4
        by_set_sets = np.repeat(np.arange(4, dtype=np.int32), len(sweep))
        runs = {1: [], 0: [], "set": []}
        for _ in range(a.repeat):  # the three alternate, so that a drift of the machine meets all of them
            for share in (1, 0):
                engine.set_option("weighted_share", share)
                runs[share] += spread_ms(engine, "count_weighted_kernel", lambda: ds.score_families(by_scope, "bic", wset=by_scope_sets), 1)
            engine.set_option("weighted_share", 1)
            runs["set"] += spread_ms(engine, "count_weighted_kernel", lambda: ds.score_families(by_set, "bic", wset=by_set_sets), 1)
        times = {k: float(np.median(v)) for k, v in runs.items()}
        set_major = times["set"]
        same = np.array_equal(ds.score_families(by_scope, "bic", wset=by_scope_sets).reshape(len(sweep), 4).T.reshape(-1),
                              ds.score_families(by_set, "bic", wset=by_set_sets))
        print(json.dumps({"measurement": "packing", "rows": a.rows, "tables": 4 * len(sweep), "sets": 4,
                          "scope_major_shared_index_ms": round(times[1], 3), "scope_major_index_per_table_ms": round(times[0], 3),
                          "set_major_ms": round(set_major, 3), "per_set_shared_over_count_kernel": round(times[1] / 4 / base, 3),
                          "min_max_ms": {"shared": span(runs[1]), "per_table": span(runs[0]), "set_major": span(runs["set"])},
                          "same_scores_either_way": bool(same)}), flush=True)

    # ---- bootstrap against the loop
    Xb = X.iloc[:a.boot_rows].reset_index(drop=True)
    lock = []
    for _ in range(2):
        t0 = time.perf_counter()
        strength, reps = structure.bootstrap(Xb, n_boot=a.n_boot, seed=a.seed, return_replicates=True)
        lock.append(time.perf_counter() - t0)
    lock_s = min(lock)
    with engine.dataset(learning.encode_complete(Xb, cols)[0], cards) as ds:
        sets = ds.bootstrap(a.n_boot, a.seed, return_weights=True)
    k = min(a.loop_replicates, a.n_boot)
    t0 = time.perf_counter()
    loop = [structure.hill_climb(Xb.iloc[np.repeat(np.arange(len(Xb)), sets[r])]) for r in range(k)]
    loop_s = time.perf_counter() - t0
    print(json.dumps({"measurement": "bootstrap", "rows": a.boot_rows, "columns": n, "n_boot": a.n_boot, "learner": "hill_climb, bic, max_parents 3",
                      "lockstep_s": round(lock_s, 3), "lockstep_s_both_runs": [round(x, 3) for x in lock], "loop_replicates_measured": k, "loop_s_measured": round(loop_s, 3),
                      "loop_s_for_n_boot": round(loop_s * a.n_boot / k, 3), "loop_over_lockstep": round(loop_s * a.n_boot / k / lock_s, 2),
                      "same_edges": all(set(map(str, x)) == set(map(str, y)) for x, y in zip(reps[:k], loop)),
                      "arcs_with_strength_above_half": int((strength.frame["strength"] >= 0.5).sum()), "pairs_seen": len(strength.frame)}), flush=True)


if __name__ == "__main__":
    main()
