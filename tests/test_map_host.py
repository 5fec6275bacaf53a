"""Marginal MAP on the CPU: the map programs, traceback records and gather lists the planner emits for mibn_map_batch, run by a
host interpreter (tools/prog_sim.cpp map, linked against planner.cpp - it also checks the structure of every program it runs) and
checked against a plain numpy twin (tests/map_check.py); plus the argument errors of BayesNet.map_query / map_frame, raised before
any engine exists, and the C-ABI bookkeeping."""
import os
import re
import shutil

import numpy as np
import pandas as pd
import pytest

import evidence_check as ec
import golden_util as gu
import map_check as mp
import mpe_check as mc
import netspec
import sorobn_amd
from sorobn_amd import _capi

ROOT = mc.ROOT
needs_gxx = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")


@pytest.fixture(scope="module")
def map_sim(tmp_path_factory):
    return mp.build_map_sim(tmp_path_factory.mktemp("map_sim"))


def _small_nets():
    """The small networks of the MPE host test: examples, small grids and random DAGs (mixed cardinalities, zeros) whose joint
    fits 2^20 cells."""
    for fname in ("examples.json", "random_dags.json"):
        for entry in gu.load(fname):
            spec = entry["spec"]
            f = mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))
            if f.missing or np.prod([float(c) for c in f.card]) > 2 ** 20:
                continue
            yield spec["name"], f
    for r, c, k in ((2, 3, 3), (3, 3, 2)):
        spec = netspec.grid_spec(r, c, k)
        yield spec["name"], mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))


def _evidence_sets(f, rng, n_sets=5):
    """The empty event and n_sets - 1 random ones of up to half the variables."""
    n = len(f.card)
    sets = [{}]
    for _ in range(n_sets - 1):
        m = int(rng.integers(1, max(2, n // 2) + 1))
        vs = sorted(rng.choice(n, size=min(m, n), replace=False).tolist())
        sets.append({int(v): int(rng.integers(0, f.card[v])) for v in vs})
    return sets


def _map_sets(f, ev, rng):
    """M = nothing, one variable, about half of the non-evidence variables, all of them (in a shuffled order: the caller's)."""
    free = [v for v in range(len(f.card)) if v not in ev]
    out = [[]]
    if free:
        out.append([int(rng.choice(free))])
        out.append([int(v) for v in rng.permutation(free)[:max(1, len(free) // 2)]])
        out.append([int(v) for v in rng.permutation(free)])
    return out


@needs_gxx
def test_map_programs_match_brute_force(map_sim, tmp_path):
    """Every small network x 5 evidence sets x M in {nothing, one, half, all} x pruned / unpruned against the dense twin: log_p
    within 1e-12, the codes equal where the best marginal is unique (map_sim itself checks the structure of every program)."""
    rng = np.random.default_rng(11)
    n_nets, taken = 0, {"zero": 0, "strict": 0, "tie": 0}
    for name, f in _small_nets():
        cases = [(no_prune, ms, ev) for ev in _evidence_sets(f, rng) for ms in _map_sets(f, ev, rng) for no_prune in (0, 1)]
        lp, codes = mp.run_map_sim(map_sim, tmp_path, f, [(np_, ms, list(ev), list(ev.values())) for np_, ms, ev in cases])
        for (no_prune, ms, ev), l, c in zip(cases, lp, codes):
            taken[mp.check(f, ms, ev, l, c, prune=not no_prune, ctx=f"{name} M={ms} e={ev} no_prune={no_prune}")] += 1
        n_nets += 1
    assert n_nets >= 7
    assert taken["strict"] >= 0.9 * (taken["strict"] + taken["tie"]), taken
    assert taken["strict"] >= 200, taken


@needs_gxx
def test_map_of_everything_is_mpe_and_of_nothing_is_p_e(map_sim, tmp_path):
    """M = every non-evidence variable: log_p equals max_sim's (the max program of the same evidence); M empty: the value equals
    ev_sim's P(e) - both within 1e-12."""
    max_sim = mc.build_max_sim(tmp_path)
    ev_sim = ec.build_ev_sim(tmp_path)
    rng = np.random.default_rng(12)
    n_cmp = 0
    for name, f in _small_nets():
        sets = _evidence_sets(f, rng, 4)
        n = len(f.card)
        all_reqs = [(1, [v for v in range(n) if v not in ev], list(ev), list(ev.values())) for ev in sets]
        lp_all, codes_all = mp.run_map_sim(map_sim, tmp_path, f, all_reqs)
        lp_mpe, codes_mpe = mc.run_max_sim(max_sim, tmp_path, f, [(list(ev), list(ev.values())) for ev in sets])
        for ev, a, b in zip(sets, lp_all, lp_mpe):
            assert (a == b == -np.inf) or abs(a - b) <= 1e-12, (name, ev, a, b)
        for no_prune in (0, 1):
            none_reqs = [(no_prune, [], list(ev), list(ev.values())) for ev in sets]
            lp_none, codes_none = mp.run_map_sim(map_sim, tmp_path, f, none_reqs)
            p_e = ec.run_ev_sim(ev_sim, tmp_path, f, none_reqs)
            for ev, a, p, c in zip(sets, lp_none, p_e, codes_none):
                assert c == []
                want = np.log(p[0]) if p[0] > 0 else -np.inf
                assert (a == want == -np.inf) or abs(a - want) <= 1e-12, (name, ev, a, want)
                n_cmp += 1
    assert n_cmp >= 50


@needs_gxx
def test_map_program_structure_on_a_grid(map_sim, tmp_path):
    """A 6 x 6 K = 4 grid with a column as M: too big for the dense twin, but map_sim's structural checks (GENERIC only, no sum
    after the first max step, every max step over a variable of M, argmax tables clear of each other and of live intermediates,
    traceback axes decoded before use, the gather list in the caller's order) run on programs with pre-multiplied products and
    dozens of steps; M = nothing gives the same mass pruned and unpruned (the CPTs are distributions)."""
    f = mc.flat_of(netspec.build(netspec.grid_spec(6, 6, 4), sorobn_amd.BayesNet))
    col = [f.id[f"{6 * r + 2:03d}"] for r in range(6)]
    ev = {f.id["000"]: 1, f.id["035"]: 2, f.id["017"]: 0}
    reqs = [(np_, ms, list(ev), list(ev.values())) for np_ in (0, 1) for ms in ([], col, col[::-1], [col[0]])]
    lp, codes = mp.run_map_sim(map_sim, tmp_path, f, reqs)
    assert np.isfinite(lp).all() and abs(lp[0] - lp[4]) <= 1e-12 and abs(lp[1] - lp[5]) <= 1e-12
    assert codes[1] == codes[2][::-1] and lp[1] == lp[2]  # (the caller's order changes the gather list alone)
    assert lp[1] < lp[3] < lp[0]  # (max over more variables of a sum: a smaller mass)
    assert all(0 <= c < 4 for c in codes[1])


@needs_gxx
def test_map_zero_probability_and_out_of_domain(map_sim, tmp_path):
    rng = np.random.default_rng(13)
    n_zero = 0
    for name, f in _small_nets():
        n = len(f.card)
        reqs = [(0, [n - 1], [0], [-1]), (1, [], [0], [int(f.card[0])])]
        joint = ec.joint(f)
        zeros = np.flatnonzero(joint.reshape(-1) == 0)
        if len(zeros):  # a full assignment of probability zero, its first variables as evidence cut down until ... still zero mass
            cell = [int(c) for c in np.unravel_index(int(zeros[0]), joint.shape)]
            ev = {v: c for v, c in enumerate(cell)}
            while len(ev) > 1:
                trial = dict(list(ev.items())[:-1])
                if mp.brute(f, [], trial, prune=False)[0] > 0:
                    break
                ev = trial
            ms = [v for v in range(n) if v not in ev][:2]
            for no_prune in (0, 1):
                reqs.append((no_prune, ms, list(ev), list(ev.values())))
        lp, codes = mp.run_map_sim(map_sim, tmp_path, f, reqs)
        for (np_, ms, evs, ecs), l, c in zip(reqs, lp, codes):
            assert l == -np.inf and c == [-1] * len(ms), (name, ms, evs, ecs, l, c)
            n_zero += 1
    assert n_zero >= 16


def test_map_argument_errors_before_any_engine(monkeypatch):
    """Unknown names, a node without a CPT and a variable both queried and observed raise the exceptions of `query` before an
    engine is created - in map_query and in map_frame."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    bn = netspec.build(spec, sorobn_amd.BayesNet)

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", no_engine)
    with pytest.raises(KeyError):
        bn.map_query("Nope", event={"Burglary": True})
    with pytest.raises(KeyError):
        bn.map_query("Alarm", event={"Nope": True})
    with pytest.raises(ValueError, match="cannot be part of the event"):
        bn.map_query("Alarm", "Burglary", event={"Burglary": True})
    with pytest.raises(ValueError):
        bn.map_query("Alarm", "Alarm")
    with pytest.raises(KeyError):
        bn.map_frame("Alarm", events=pd.DataFrame({"Burglary": [True], "Not a variable": [1]}))
    with pytest.raises(KeyError):
        bn.map_frame("Nope", events=pd.DataFrame({"Burglary": [True]}))
    with pytest.raises(ValueError, match="cannot be part of the event"):
        bn.map_frame("Alarm", "Burglary", events=pd.DataFrame({"Burglary": [True, None], "Mary calls": [True, True]}))
    # a node without a CPT
    bare = sorobn_amd.BayesNet(("A", "B"))
    bare.P["A"] = pd.Series({True: 0.5, False: 0.5})
    bare.P["A"].index.names = ["A"]
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", no_engine)
    with pytest.raises(KeyError):
        bare.map_query("A", event={})


def test_map_symbol_is_declared_and_bound():
    """mibn_map_batch is in the public header, with its flag, and in the list of symbols build() checks the library for; the
    ctypes wrapper exists."""
    with open(os.path.join(ROOT, "include", "mibn.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint\s+mibn_map_batch\s*\(\s*mibn_t\s*\*\s*h\s*,\s*uint32_t\s+flags\s*,\s*int64_t\s+B\s*,", header)
    assert re.search(r"#define\s+MIBN_MAP_PRUNE\s+1u", header)
    assert "mibn_map_batch" in _capi.SYMBOLS
    assert _capi.MAP_PRUNE == 1
    assert callable(getattr(_capi.Engine, "map_batch", None)) and callable(getattr(_capi.Engine, "map", None))
    lib_path = os.path.join(ROOT, "sorobn_amd", "libmibn.so")
    if os.path.exists(lib_path):
        assert hasattr(_capi.lib(), "mibn_map_batch")
