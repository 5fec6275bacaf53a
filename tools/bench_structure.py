"""Hill climbing on the C3 grid (100 four-state columns): the resident data set and the device reduction (mibn_dataset_create /
mibn_score_families) beside the same family batches done the way the parent commit allows - `Engine.count_tables` (rows uploaded and
tables downloaded on every call) scored by vectorised numpy - in the same process.

    python tools/bench_structure.py [--rows 100000,1000000] [--max-parents 3] [--baseline-iterations 15] [--seed 1]

Rows are drawn with bn.sample from the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe); score "bic", start empty.
After a warm-up call, per row count one JSON line: the upload, the first sweep (n + n (n - 1) families) in ms and families/s, the
median iteration (one scoring call) and its split into device call and host search, the whole search, iterations and families, the
share of count_kernel / score_kernel in the GPU time (last-call kernel statistics summed over the calls), and for the baseline the
first sweep and the median of the first --baseline-iterations later batches (every batch would take as long as the search has
iterations; the batches are the recorded ones of the device run) with its numpy share, plus the largest difference of the scores.
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


class Recorder:
    """The counting engine with a stop-watch: every scoring call's families, host time and kernel statistics."""

    def __init__(self, engine):
        self.engine, self.calls, self.upload_s = engine, [], 0.0

    def dataset(self, codes, card):
        t0 = time.perf_counter()
        ds = self.engine.dataset(codes, card)
        self.upload_s = time.perf_counter() - t0
        self.codes, self.card = codes, card
        return RecordingDataset(self, ds)


class RecordingDataset:
    def __init__(self, rec, ds):
        self.rec, self.ds = rec, ds

    def score_families(self, families, kind="bic", ess=1.0):
        t0 = time.perf_counter()
        out = self.ds.score_families(families, kind, ess)
        dt = time.perf_counter() - t0
        ks = {k["name"]: k["ms"] for k in self.rec.engine.kernel_stats()}
        self.rec.calls.append({"families": families, "t0": t0, "s": dt, "count_ms": ks.get("count_kernel", 0.0),
                               "score_ms": ks.get("score_kernel", 0.0), "scores": out})
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ds.close()


def numpy_bic(tables, n_rows):
    """BIC of dense family tables (child last), same-shaped tables stacked: the arithmetic of the score table in include/mibn.h."""
    out = np.empty(len(tables))
    by_shape = {}
    for k, t in enumerate(tables):
        by_shape.setdefault((t.size // t.shape[-1], t.shape[-1]), []).append(k)
    for (q, r), ks in by_shape.items():
        c = np.stack([tables[k].reshape(q, r) for k in ks]).astype(np.float64)
        nj = c.sum(axis=2, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(c > 0, c * (np.log(c) - np.log(nj)), 0.0)
        out[ks] = term.reshape(len(ks), -1).sum(axis=1) - 0.5 * np.log(max(n_rows, 1)) * q * (r - 1)
    return out


def baseline_call(engine, codes, card, families, n_rows):
    t0 = time.perf_counter()
    tables = engine.count_tables(codes, card, families)
    t1 = time.perf_counter()
    scores = numpy_bic(tables, n_rows)
    return scores, time.perf_counter() - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="100000,1000000")
    ap.add_argument("--max-parents", type=int, default=3)
    ap.add_argument("--baseline-iterations", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    bn.seed = a.seed
    true_edges = {(p, c) for c, ps in bn.parents.items() for p in ps}
    engine = learning.counting_engine()
    real = learning.counting_engine
    for n_rows in [int(x) for x in a.rows.split(",")]:
        X = bn.sample(n_rows)
        warm = X.iloc[:2000]
        structure.hill_climb(warm, max_parents=a.max_parents, max_iter=2)  # warm-up: library, kernels, buffers
        rec = Recorder(engine)
        learning.counting_engine = lambda device=None: rec
        try:
            t0 = time.perf_counter()
            result, trace, total = structure.hill_climb(X, max_parents=a.max_parents, return_trace=True)
            search_s = time.perf_counter() - t0
        finally:
            learning.counting_engine = real
        calls = rec.calls
        later = calls[1:]
        gaps = [b["t0"] - (p["t0"] + p["s"]) for p, b in zip(calls[:-1], later)]  # host search between two scoring calls
        found = {e for e in result if isinstance(e, tuple)}
        skeleton = lambda es: {frozenset(e) for e in es}
        count_ms = sum(c["count_ms"] for c in calls)
        score_ms = sum(c["score_ms"] for c in calls)
        # the baseline: the recorded batches through count_tables + numpy
        baseline_call(engine, rec.codes, rec.card, calls[0]["families"][:100], n_rows)  # warm-up
        b_scores, b_first_s, b_first_np = baseline_call(engine, rec.codes, rec.card, calls[0]["families"], n_rows)
        diff = float(np.max(np.abs(b_scores - calls[0]["scores"])))
        b_later = []
        for c in later[:a.baseline_iterations]:
            s, dt, dnp = baseline_call(engine, rec.codes, rec.card, c["families"], n_rows)
            diff = max(diff, float(np.max(np.abs(s - c["scores"]))))
            b_later.append((dt, dnp))
        med = lambda v: float(np.median(v)) if len(v) else None
        print(json.dumps({
            "workload": f"hill_climb, C3 10x10 K=4 grid, {n_rows} rows, bic, max_parents {a.max_parents}, start empty",
            "encode_and_search_s": round(search_s, 3), "upload_ms": round(rec.upload_s * 1e3, 2),
            "iterations": len(trace), "scoring_calls": len(calls), "families": sum(len(c["families"]) for c in calls),
            "first_sweep_families": len(calls[0]["families"]), "first_sweep_ms": round(calls[0]["s"] * 1e3, 2),
            "first_sweep_families_per_s": round(len(calls[0]["families"]) / calls[0]["s"], 1),
            "first_sweep_count_kernel_ms": round(calls[0]["count_ms"], 3), "first_sweep_score_kernel_ms": round(calls[0]["score_ms"], 3),
            "median_iteration_ms": round(1e3 * med([c["s"] + g for c, g in zip(later, gaps)]), 3) if later else None,
            "median_iteration_device_call_ms": round(1e3 * med([c["s"] for c in later]), 3) if later else None,
            "median_iteration_host_search_ms": round(1e3 * med(gaps), 3) if gaps else None,
            "median_iteration_families": med([len(c["families"]) for c in later]),
            "scoring_calls_total_s": round(sum(c["s"] for c in calls), 3),
            "gpu_ms_count_kernel": round(count_ms, 2), "gpu_ms_score_kernel": round(score_ms, 2),
            "count_kernel_share": round(count_ms / max(count_ms + score_ms, 1e-12), 4),
            "final_bic": total, "edges_found": len(found), "true_edges": len(true_edges),
            "true_skeleton_recovered": len(skeleton(found) & skeleton(true_edges)),
            "baseline_first_sweep_ms": round(b_first_s * 1e3, 2), "baseline_first_sweep_numpy_ms": round(b_first_np * 1e3, 2),
            "baseline_median_iteration_call_ms": round(1e3 * med([x[0] for x in b_later]), 3) if b_later else None,
            "baseline_median_iteration_numpy_ms": round(1e3 * med([x[1] for x in b_later]), 3) if b_later else None,
            "baseline_iterations_measured": len(b_later),
            "max_abs_diff_device_vs_baseline": diff,
        }), flush=True)


if __name__ == "__main__":
    main()
