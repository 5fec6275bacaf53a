"""Plain numpy twin of marginal MAP (tests/test_map.py, tests/test_map_host.py): the dense joint of a small network, sliced by the
evidence and summed over every axis that is not a MAP variable - over the flattened network (sorobn_amd.flatten), i.e. the tables
the engine itself is given - plus the runner of the host interpreter tools/prog_sim.cpp map."""
import os
import subprocess

import numpy as np

import mpe_check as mc
import sim_tools

ROOT = mc.ROOT
_joints = {}


def relevant(f, variables):
    """`variables` and their ancestors (ids)."""
    rel, todo = set(), [int(v) for v in variables]
    while todo:
        v = todo.pop()
        if v in rel:
            continue
        rel.add(v)
        todo.extend(int(u) for u in f.scope_vars[f.scope_off[v]:f.scope_off[v + 1] - 1])
    return rel


def marginal(f, mvars, ev, prune=False):
    """-> (table, axes): sum_h P(m, h, e) as a dense table whose axes are `axes` = sorted(mvars).  prune: only the CPTs of the MAP
    variables, the evidence and their ancestors take part (a barren summed variable sums to 1 where the CPTs are distributions -
    and is left out where they are not: the rule of MIBN_MAP_PRUNE)."""
    rel = frozenset(relevant(f, list(mvars) + list(ev))) if prune else frozenset(range(len(f.card)))
    key = (id(f), tuple(sorted(ev.items())), rel)
    if key not in _joints:  # (the dense joint of a factor set and an event is shared by every M that asks for it, never modified)
        if len(_joints) >= 8:
            _joints.pop(next(iter(_joints)))
        # (the entry holds f itself: while it is cached no other network can take its id)
        _joints[key] = (f, mc._mul([t for v, t in enumerate(mc._sliced(f, ev)) if v in rel]))
    assert _joints[key][0] is f
    vs, joint = _joints[key][1]
    ms = set(int(v) for v in mvars)
    drop = tuple(i for i, v in enumerate(vs) if v not in ms)
    table = joint.sum(axis=drop) if drop else joint
    axes = [v for v in vs if v in ms]
    # a MAP variable no factor mentions cannot happen (its own CPT does); a single-state one is an axis of extent 1
    return np.asarray(table, np.float64), axes


def brute(f, mvars, ev, prune=False):
    """-> (p1, p2, codes, table, axes): the best and the runner-up marginal probability, the best codes in the order of `mvars`
    (the first maximum in C order of the sorted axes: ties go to the lowest codes), and the table for prob_of."""
    table, axes = marginal(f, mvars, ev, prune)
    flat = table.reshape(-1)
    order = np.argsort(-flat, kind="stable")
    p1 = float(flat[order[0]])
    p2 = float(flat[order[1]]) if flat.size > 1 else 0.0
    best = np.unravel_index(int(order[0]), table.shape) if table.ndim else ()
    at = dict(zip(axes, (int(c) for c in best)))
    return p1, p2, [at[int(v)] for v in mvars], table, axes


def prob_of(table, axes, mvars, codes):
    """The marginal probability of the assignment mvars = codes, read from the twin's table."""
    at = dict(zip((int(v) for v in mvars), (int(c) for c in codes)))
    return float(table[tuple(at[a] for a in axes)]) if axes else float(table.reshape(-1)[0])


def check(f, mvars, ev, log_p, codes, prune=False, ctx="", tol=1e-12):
    """The acceptance rule of an answer against the twin: log_p within tol; the codes equal where the best marginal beats the
    runner-up by more than 1e-9 relative; elsewhere the returned assignment's own marginal within 1e-9 relative of the best.
    -> "zero" | "strict" | "tie": the branch taken."""
    p1, p2, best, table, axes = brute(f, mvars, ev, prune)
    if p1 <= 0:
        assert log_p == -np.inf, (ctx, log_p)
        assert all(int(c) == -1 for c in codes), (ctx, codes)
        return "zero"
    assert abs(log_p - np.log(p1)) <= tol, (ctx, log_p, np.log(p1))
    if p1 - p2 > 1e-9 * p1:
        assert [int(c) for c in codes] == best, (ctx, list(codes), best)
        return "strict"
    assert all(0 <= int(c) < f.card[int(v)] for v, c in zip(mvars, codes)), (ctx, codes)
    assert abs(prob_of(table, axes, mvars, codes) - p1) <= 1e-9 * p1, (ctx, list(codes), best)
    return "tie"


def net_text(f, requests):
    """Input of tools/prog_sim.cpp map: the network, then the requests [(no_prune, mvars, evars, ecodes)]."""
    parts = sim_tools.network_prefix(f) + [str(len(requests))]
    for no_prune, ms, evs, ecs in requests:
        parts.append(f"{int(no_prune)} {len(ms)} {' '.join(map(str, ms))} {len(evs)} {' '.join(map(str, evs))} {' '.join(map(str, ecs))}")
    return "\n".join(parts) + "\n"


def build_map_sim(tmp_path):
    return sim_tools.build_prog_sim()


def run_map_sim(exe, tmp_path, f, requests, expect_fail=False, options=None, ties=False):
    """-> (log_p [B], [codes of request b, in the order of its mvars]) as tools/prog_sim.cpp map computes them from the map programs -
    planned by a bare Network, or with `options` as an engine with these set_option values plans them (sim_tools.sim_args).  ties: a
    third result, sim_tools.parse_ties."""
    path = os.path.join(str(tmp_path), "map_net.txt")
    with open(path, "w") as fh:
        fh.write(net_text(f, requests))
    r = subprocess.run([exe, "map", path] + sim_tools.sim_args(f, tmp_path, options, ties), capture_output=True, text=True, timeout=900)
    if expect_fail:
        return r
    assert r.returncode == 0, r.stderr[-2000:]
    lp, codes = [], []
    for line in r.stdout.splitlines():
        t = line.split()
        lp.append(-np.inf if t[0] == "-inf" else float.fromhex(t[0]))
        codes.append([int(x) for x in t[1:]])
    assert len(lp) == len(requests)
    return (np.array(lp), codes, sim_tools.parse_ties(r.stderr)) if ties else (np.array(lp), codes)
