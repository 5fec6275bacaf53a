"""Plain numpy checkers of the evidence likelihood P(e) (tests/test_evidence.py, tests/test_evidence_host.py): P(q, e) of a small
network by enumeration of its dense joint, and the host interpreter of MIBN_Q_UNNORMALISED programs (tools/prog_sim.cpp ev) - all over
the flattened network (sorobn_amd.flatten), i.e. the tables the engine itself is given."""
import os
import subprocess

import numpy as np

import golden_util as gu
import mpe_check as mc
import netspec
import sim_tools
import sorobn_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def joint(f):
    """Dense product of every CPT: (variable ids in axis order = 0..n-1, table)."""
    vs, a = mc._mul(mc.cpts(f))
    assert vs == list(range(len(f.card)))
    return a


def brute(f, q, ev, no_prune=False, normalise=True, table=None):
    """P(q, e) [C-order over q] of the product of every CPT, by enumeration; normalise: divided by its total mass Z (the
    semantics of predict_proba); else the raw sum - with pruning the relevant CPTs only, which equals the NOPRUNE sum when every
    CPT is a distribution.  A code of -1 gives zeros."""
    a = joint(f) if table is None else table
    if any(c < 0 or c >= f.card[v] for v, c in ev.items()):
        return np.zeros([int(f.card[v]) for v in q]).reshape(-1)
    if not no_prune and not normalise:
        rel = set(q) | set(ev)
        for v in list(rel):
            rel |= _ancestors(f, v)
        fs = [(sc, t) for (sc, t), v in zip(mc.cpts(f), range(len(f.card))) if v in rel]
        vs, a = mc._mul(fs) if fs else ([], np.ones(()))
    else:
        vs = list(range(len(f.card)))
    z = a.sum() if normalise else 1.0
    idx = tuple(ev.get(v, slice(None)) for v in vs)
    kept = [v for v in vs if v not in ev]
    s = a[idx]
    s = s.sum(axis=tuple(i for i, v in enumerate(kept) if v not in q)) if kept else s
    rest = [v for v in kept if v in q]
    s = np.transpose(s, [rest.index(v) for v in q]) if q else s
    return (np.asarray(s, np.float64) / z).reshape(-1)


def _ancestors(f, v):
    out, stack = set(), [v]
    while stack:
        for p in f.parents[stack.pop()]:
            if p not in out:
                out.add(p)
                stack.append(p)
    return out


def small_specs(max_states=2 ** 16):
    """(name, spec) of every examples.json / random_dags.json network without a missing CPT whose joint fits."""
    for fname in ("examples.json", "random_dags.json"):
        for entry in gu.load(fname):
            spec = entry["spec"]
            f = mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))
            if f.missing or np.prod([float(c) for c in f.card]) > max_states:
                continue
            yield spec["name"], spec


def evidence_sets(f, rng, n_random=3):
    """Partial evidence of every kind: empty, single, half the variables, all, out of domain, zero probability (where the joint
    has a zero cell) and a few random ones - [(tag, {id: code})]."""
    n = len(f.card)
    sets = [("empty", {}), ("single", {0: int(rng.integers(0, f.card[0]))})]
    half = rng.choice(n, size=max(1, n // 2), replace=False).tolist()
    sets.append(("half", {int(v): int(rng.integers(0, f.card[v])) for v in half}))
    sets.append(("all", {v: int(rng.integers(0, f.card[v])) for v in range(n)}))
    sets.append(("out_of_domain", {0: -1, n - 1: 0} if n > 1 else {0: -1}))
    a = joint(f)
    zeros = np.flatnonzero(a.reshape(-1) == 0)
    if len(zeros):
        cell = np.unravel_index(int(zeros[0]), a.shape)
        sets.append(("zero", {v: int(c) for v, c in enumerate(cell)}))
    for k in range(n_random):
        vs = rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False).tolist()
        sets.append((f"random{k}", {int(v): int(rng.integers(0, f.card[v])) for v in vs}))
    return sets


def net_text(f, requests):
    """Input of tools/prog_sim.cpp ev: the network, then the requests [(no_prune, qvars, evars, ecodes)]."""
    parts = sim_tools.network_prefix(f) + [str(len(requests))]
    for no_prune, qs, evs, ecs in requests:
        parts.append(f"{int(no_prune)} {len(qs)} {' '.join(map(str, qs))} {len(evs)} {' '.join(map(str, evs))} {' '.join(map(str, ecs))}")
    return "\n".join(parts) + "\n"


def build_ev_sim(tmp_path):
    return sim_tools.build_prog_sim()


def run_ev_sim(exe, tmp_path, f, requests, mode="run"):
    """-> the output lines of tools/prog_sim.cpp ev: "run" - a float64 array per request; else the lines as strings."""
    path = os.path.join(str(tmp_path), "net.txt")
    with open(path, "w") as fh:
        fh.write(net_text(f, requests))
    r = subprocess.run([exe, "ev", mode, path], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests)
    if mode != "run":
        return lines
    return [np.array([float.fromhex(t) for t in line.split()]) for line in lines]
