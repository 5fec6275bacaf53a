"""Plain numpy checkers of the most probable explanation (tests/test_mpe.py, tests/test_mpe_host.py): the dense joint of a small
network, max-product variable elimination in a given order, and the log joint probability of an assignment - all over the
flattened network (sorobn_amd.flatten), i.e. the tables the engine itself is given."""
import os
import subprocess

import numpy as np

import sim_tools
from sorobn_amd.flatten import flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpts(f):
    """[(scope ids, dense table)] of every variable: table axes in scope order (parents, then the variable)."""
    out = []
    for v in range(len(f.card)):
        sc = [int(u) for u in f.scope_vars[f.scope_off[v]:f.scope_off[v + 1]]]
        a = np.asarray(f.values[f.value_off[v]:f.value_off[v + 1]], np.float64).reshape([int(f.card[u]) for u in sc])
        out.append((sc, a))
    return out


def _sliced(f, ev):
    fs = []
    for sc, a in cpts(f):
        idx = tuple(ev.get(u, slice(None)) for u in sc)
        fs.append(([u for u in sc if u not in ev], a[idx]))
    return fs


def _mul(fs):
    vs = sorted(set().union(*[set(v) for v, _ in fs])) if fs else []
    out = np.ones([1] * len(vs))
    for v, a in fs:
        perm = sorted(range(len(v)), key=lambda i: vs.index(v[i]))
        shape = [1] * len(vs)
        for i in perm:
            shape[vs.index(v[i])] = a.shape[i]
        out = out * np.transpose(a, perm).reshape(shape)
    return vs, out


def brute(f, ev):
    """Dense joint over the non-evidence variables: (log of the best probability, the best codes [n] (evidence: their codes),
    the best and the runner-up probability)."""
    n = len(f.card)
    vs, joint = _mul(_sliced(f, ev))
    flat = joint.reshape(-1)
    order = np.argsort(-flat, kind="stable")
    p1 = float(flat[order[0]])
    p2 = float(flat[order[1]]) if flat.size > 1 else 0.0
    codes = np.zeros(n, np.int64)
    for u, c in ev.items():
        codes[u] = c
    best = np.unravel_index(int(np.flatnonzero(flat == p1)[0]), joint.shape) if joint.ndim else ()
    for u, c in zip(vs, best):
        codes[u] = c
    return (np.log(p1) if p1 > 0 else -np.inf), codes, p1, p2


def ve_max(f, ev, order):
    """max_x P(x, e) by max-product elimination of the non-evidence variables in `order` (log)."""
    fs = _sliced(f, ev)
    for x in order:
        if x in ev:
            continue
        mine = [t for t in fs if x in t[0]]
        fs = [t for t in fs if x not in t[0]]
        vs, a = _mul(mine)
        fs.append(([u for u in vs if u != x], a.max(axis=vs.index(x))))
    _, a = _mul(fs)
    m = float(a.reshape(-1)[0])
    return np.log(m) if m > 0 else -np.inf


def log_joint(f, codes):
    """sum_v log CPT_v[codes] (-inf where a factor is 0)."""
    s = 0.0
    for sc, a in cpts(f):
        p = float(a[tuple(int(codes[u]) for u in sc)])
        s += np.log(p) if p > 0 else -np.inf
    return s


def flat_of(bn):
    return flatten(bn)


def net_text(f, requests):
    """Input of tools/prog_sim.cpp max: the network, then the requests [(evars, ecodes)]."""
    parts = sim_tools.network_prefix(f) + [str(len(requests))]
    for evs, ecs in requests:
        parts.append(f"{len(evs)} {' '.join(map(str, evs))} {' '.join(map(str, ecs))}")
    return "\n".join(parts) + "\n"


def build_max_sim(tmp_path):
    return sim_tools.build_prog_sim()


def run_max_sim(exe, tmp_path, f, requests, options=None, ties=False):
    """-> (log_p [B], codes [B, n]) as tools/prog_sim.cpp max computes them from the max programs - planned by a bare Network, or
    with `options` as an engine with these set_option values plans them (sim_tools.sim_args).  ties: a third result, sim_tools.parse_ties."""
    path = os.path.join(str(tmp_path), "net.txt")
    with open(path, "w") as fh:
        fh.write(net_text(f, requests))
    r = subprocess.run([exe, "max", path] + sim_tools.sim_args(f, tmp_path, options, ties), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lp, codes = [], []
    for line in r.stdout.splitlines():
        t = line.split()
        lp.append(-np.inf if t[0] == "-inf" else float.fromhex(t[0]))
        codes.append([int(x) for x in t[1:]])
    out = np.array(lp), np.array(codes, np.int64).reshape(len(requests), len(f.card))
    return out + (sim_tools.parse_ties(r.stderr),) if ties else out


def check_against_brute(f, ev, log_p, codes, ctx=""):
    """The acceptance rule of the brute-force cases: log_p within 1e-12; the assignment equal where the best state beats the
    runner-up by more than 1e-9 relative, elsewhere of the same probability."""
    lp_star, best, p1, p2 = brute(f, ev)
    if p1 <= 0:
        assert log_p == -np.inf, ctx
        assert all(codes[v] == -1 for v in range(len(f.card)) if v not in ev), ctx
        return
    assert abs(log_p - lp_star) <= 1e-12, (ctx, log_p, lp_star)
    if p1 - p2 > 1e-9 * p1:
        assert np.array_equal(np.asarray(codes), best), (ctx, codes, best)
    else:
        assert abs(log_joint(f, codes) - lp_star) <= 1e-12, (ctx, codes, best)
