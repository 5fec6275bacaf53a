"""What likelihood findings cost on the C3 workload, beside the same stream with hard evidence.

    python tools/bench_likelihood.py [--requests 32768] [--evidence 4] [--seconds 2] [--seed 1]

Workload: the BASELINE 10 x 10 K = 4 grid (tests/golden/grid10x10.json recipe), the requests of netspec.c3_requests (seeded, one query
variable, 4 evidence variables), calls of the whole batch.  One warm-up call per row, then calls until at least --seconds have
passed, the window ended by a device synchronise.  One JSON line per row:

  a        the stream as it is (hard evidence only);
  b k=1|2|4  the first k evidence variables of every request turned into one-hot findings - the same answers at a different cost: a
           finding slices no table, its variable stays an axis until it is eliminated;
  c k=1|2|4  those k variables simply left unobserved - the floor of b: b multiplies one more factor into the programs of c;
  asia     10 000 Asia requests through tiny_kernel, and the same with one finding each through tiny_lh_kernel.

Every row: queries/s, algorithmic MB per query (section-8(d) bytes of the programs), the call's planning and kernel time; the b rows
also likelihood_seed_kernel's launches and milliseconds per call.  Rows a and the b / c rows differ in who plans: a call with findings
is planned by the host's workers only (no plan templates, no device planner), which the plan_ms column shows.
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


def one_hot_block(fvars, fcodes, card):
    """findings [B, k] as one-hot weight vectors -> the CSR block of Engine.*(likelihoods=...)."""
    B, k = fvars.shape
    l_off = np.arange(B + 1, dtype=np.int64) * k
    l_vars = fvars.reshape(-1).astype(np.int32)
    cards = card[l_vars].astype(np.int64)
    v_off = np.concatenate([[0], np.cumsum(cards)]).astype(np.int64)
    values = np.zeros(int(v_off[-1]), np.float64)
    values[v_off[:-1] + fcodes.reshape(-1)] = 1.0
    return l_off, l_vars, v_off, values


def row(eng, name, fn, requests, seconds):
    n, dt = timed(fn, seconds, eng.synchronize)
    st = eng.stats()
    ks = {k["name"]: k for k in eng.kernel_stats()}
    seed = ks.get("likelihood_seed_kernel", {"launches": 0.0, "ms": 0.0})
    out = {"row": name, "queries_per_s": round(n * requests / dt, 1), "calls": n, "window_s": round(dt, 3),
           "alg_MB_per_query": round(st["alg_bytes"] / requests / 1e6, 4), "last_call_plan_ms": round(st["plan_ms"], 2),
           "last_call_kernel_ms": round(st["kernel_ms"], 3), "last_call_total_ms": round(st["total_ms"], 2),
           "seed_kernel_launches": seed["launches"], "seed_kernel_ms": round(seed["ms"], 4),
           "kernels": sorted(k for k, v in ks.items() if v["launches"] > 0 and not k.startswith("level:"))}
    print(json.dumps(out), flush=True)
    return out


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
    base = eng.query_fixed(qvars, evars, ec)
    row(eng, "a", lambda: eng.query_fixed(qvars, evars, ec), a.requests, a.seconds)
    for k in (1, 2, 4):
        if k > a.evidence:
            continue
        block = one_hot_block(evars[:, :k], ec[:, :k], eng.card)
        got = eng.query_fixed(qvars, evars[:, k:], ec[:, k:], likelihoods=block)
        print(json.dumps({"row": f"b k={k}", "max_abs_diff_to_a": float(np.max(np.abs(got - base)))}), flush=True)
        row(eng, f"b k={k}", lambda: eng.query_fixed(qvars, evars[:, k:], ec[:, k:], likelihoods=block), a.requests, a.seconds)
        row(eng, f"c k={k}", lambda: eng.query_fixed(qvars, evars[:, k:], ec[:, k:]), a.requests, a.seconds)
    # Asia: the tiny kernel and its twin
    asia = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "asia")
    bn2 = netspec.build(asia, sorobn_amd.BayesNet).use_device(0)
    eng2 = bn2.backend.engine
    n = 10000
    rng = np.random.default_rng(a.seed)
    perm = np.argsort(rng.random((n, 8)), axis=1).astype(np.int32)
    q2, e2, l2 = perm[:, :1], perm[:, 1:3], perm[:, 3:4]
    c2 = rng.integers(0, 2, size=(n, 2)).astype(np.int32)
    block2 = (np.arange(n + 1, dtype=np.int64), l2.reshape(-1), np.arange(n + 1, dtype=np.int64) * 2, rng.uniform(0.1, 1.0, 2 * n))
    row(eng2, "asia plain (tiny_kernel)", lambda: eng2.query_fixed(q2, e2, c2), n, a.seconds / 2)
    row(eng2, "asia one finding (tiny_lh_kernel)", lambda: eng2.query_fixed(q2, e2, c2, likelihoods=block2), n, a.seconds / 2)


if __name__ == "__main__":
    main()
