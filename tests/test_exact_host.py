"""Exact structure learning, host side (no GPU): the numpy twin of mibn_best_dag (tests/dag_check.py) against an enumeration of
every DAG, the CPU twin of the device's pass schedule (tools/dag_plan_sim.cpp running sorobn_amd/csrc/dag_plan.h) against the
numpy twin bit for bit, `learning.exact_search` / `learning.best_dag` over test doubles of the engine, and every argument error
with the engine patched to fail."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import dag_check as dc
import structure_check as sc
import weights_check as wc
from sorobn_amd import _capi, learning, structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12  # the structure tests' relative tolerance; the DP total is n - 1 <= 4 additions of <= 1.1e-16 relative each
OPTION_PAIRS = [(0, 0), (3, 2), (3, 3), (1, 1), (2, 5)]  # (dag_tile_bits, dag_group_bits); 0 = the default
needs_gxx = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")


def planted(n, seed, n_rows=300):
    """Random rows with cardinalities 2 to 3 and two planted dependencies: column 1 copies column 0 (mod its card) four times
    out of five; the last column is the parity of columns 0 and 2 (all three binary) nine times out of ten - a dependence no
    single edge reveals, so a greedy search that adds one edge at a time has no first step towards it."""
    rng = np.random.default_rng(seed)
    card = [int(c) for c in rng.integers(2, 4, n)]
    card[0] = card[2] = card[n - 1] = 2
    codes = np.stack([rng.integers(0, c, n_rows) for c in card], axis=1)
    keep = rng.random(n_rows) < 0.8
    codes[keep, 1] = codes[keep, 0] % card[1]
    keep = rng.random(n_rows) < 0.9
    codes[keep, n - 1] = (codes[keep, 0] + codes[keep, 2]) % 2
    return codes, card


def scored(codes, card, cand, kind, ess=1.0):
    score = sc.scorer(codes, card, kind, ess)
    return np.array([score(v, [u for u in range(len(card)) if (pm >> u) & 1]) for v, pm in cand])


def cached_scorer(codes, card, kind, ess=1.0):
    score, memo = sc.scorer(codes, card, kind, ess), {}

    def get(v, parents):
        key = (v, frozenset(parents))
        if key not in memo:
            memo[key] = score(v, parents)
        return memo[key]
    return get


CASES = [  # (n, max_parents, kind, seed, required, forbidden)
    (4, 3, "bic", 0, (), ()),
    (4, 3, "bdeu", 1, (), ()),
    (5, 2, "bic", 2, (), ()),
    (5, 2, "bdeu", 3, (), ()),
    (4, 3, "bic", 4, ((3, 1),), ((0, 1),)),
]


@pytest.fixture(scope="module")
def solved():
    """Every case once: candidates, scores, the twin's answer, the enumeration's and the brute-force hill climb's."""
    out = []
    for n, k, kind, seed, req, forb in CASES:
        codes, card = planted(n, seed)
        cand = dc.bounded_candidates(n, k, req, forb)
        children, masks = [v for v, _ in cand], [pm for _, pm in cand]
        scores = scored(codes, card, cand, kind)
        parents, order, total = dc.best_dag(n, children, masks, scores)
        enum_total, enum_pms = dc.all_dags_best(n, children, masks, scores)
        _, _, hc_total, _ = sc.hill_climb(cached_scorer(codes, card, kind), n, max_parents=k, required=req, forbidden=forb)
        out.append(dict(n=n, cand=cand, scores=scores, parents=parents, order=order, total=total, enum_total=enum_total, enum_pms=enum_pms,
                        hc_total=hc_total, req=req, forb=forb))
    return out


def test_twin_equals_the_enumeration_of_every_dag(solved):
    for c in solved:
        n, at = c["n"], {k: i for i, k in enumerate(c["cand"])}
        chosen = [c["scores"][at[(v, int(c["parents"][v]))]] for v in range(n)]  # (KeyError: not a candidate)
        bound = TOL * math.fsum(abs(s) for s in chosen)
        print(f"n={n} dp_total={c['total']!r} enumerated={c['enum_total']!r} hill_climb={c['hc_total']!r} bound={bound:.3e}")
        assert abs(c["total"] - c["enum_total"]) <= bound
        assert abs(math.fsum(chosen) - c["total"]) <= bound
        pa = [[u for u in range(n) if (int(pm) >> u) & 1] for pm in c["parents"]]
        assert not sc.has_cycle(n, pa)
        where = {int(v): k for k, v in enumerate(c["order"])}
        assert sorted(where) == list(range(n)) and all(where[u] < where[v] for v in range(n) for u in pa[v])
        for u, v in c["req"]:
            assert u in pa[v]
        for u, v in c["forb"]:
            assert u not in pa[v]
        assert c["total"] >= c["hc_total"] - bound


def test_exact_beats_hill_climbing_somewhere(solved):
    """Hill climbing stops at local optima: on at least one of these cases the exact total is strictly better."""
    gaps = [c["total"] - c["hc_total"] for c in solved]
    print("exact - hill_climb:", gaps)
    assert max(gaps) > 1e-6


def test_twin_by_hand():
    """Three columns, hand-made scores: 0 <- {} 0, 1 <- {0} 1, 1 <- {} 0, 2 <- {1} 1, 2 <- {} 0 and 0 <- {2} 1.5 (closing the
    cycle 0 -> 1 -> 2 -> 0): the best DAG drops the cheapest edge of the cycle - a tie between 0 -> 1 and 1 -> 2 at total 2.5."""
    children, masks, scores = [0, 1, 1, 2, 2, 0], [0, 1, 0, 2, 0, 4], [0.0, 1.0, 0.0, 1.0, 0.0, 1.5]
    parents, order, total = dc.best_dag(3, children, masks, scores)
    assert total == 2.5 == dc.all_dags_best(3, children, masks, scores)[0]
    # best[V]: sink 0 gives best[{1,2}] + 1.5 = 1 + 1.5, sink 1 gives best[{0,2}] + 1 = 1.5 + 1, sink 2 the same: ties -> sink 0
    assert order.tolist() == [1, 2, 0] and parents.tolist() == [4, 0, 2]
    # an equal score inside phase A: the smaller mask wins
    score, mask = dc.bps_tables(3, [0, 1, 2, 2, 2], [0, 0, 1, 2, 0], [0.0, 0.0, 1.0, 1.0, 0.0])
    assert score[2].tolist() == [0.0, 1.0, 1.0, 1.0] and mask[2].tolist() == [0, 1, 2, 1]
    # no DAG
    parents, order, total = dc.best_dag(2, [0, 1], [2, 1], [0.0, 0.0])
    assert total == -math.inf and parents.tolist() == [dc.NO_MASK] * 2 and order.tolist() == [-1, -1]
    # the chain of the device test: total n - 1
    for n in (12, 16):
        ch, ms, ss = chain_candidates(n)
        parents, order, total = dc.best_dag(n, ch, ms, ss)
        assert total == n - 1 and order.tolist() == list(range(n)) and parents.tolist() == [0] + [1 << (v - 1) for v in range(1, n)]


def chain_candidates(n):
    """{} at 0 for every child, {v - 1} at 1 for v >= 1, {n - 1} at 0.5 for child 0 (would close the cycle)."""
    children = list(range(n)) + list(range(1, n)) + [0]
    masks = [0] * n + [1 << (v - 1) for v in range(1, n)] + [1 << (n - 1)]
    return children, masks, [0.0] * n + [1.0] * (n - 1) + [0.5]


# ------------------------------------------------------------------------------------------- tools/dag_plan_sim against the twin
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dag") / "dag_plan_sim")
    r = subprocess.run(["g++", "-O2", "-mpopcnt", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "dag_plan_sim.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(n, children, masks, scores, tile_bits=0, group_bits=0, tables=True):
        lines = [f"{n} {tile_bits} {group_bits} {int(tables)} {len(children)}"]
        lines += [f"{int(v)} {int(pm)} {float(s)!r}" for v, pm, s in zip(children, masks, scores)]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout)
    return run


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64).reshape(-1)


@needs_gxx
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 13])
def test_sim_equals_the_twin_bit_for_bit(sim, n):
    children, masks, scores = dc.tie_candidates(n, seed=100 + n)
    parents, order, total, score, mask, best, sink = dc.best_dag(n, children, masks, scores, tables=True)
    for tile_bits, group_bits in OPTION_PAIRS:
        got = sim(n, children, masks, scores, tile_bits, group_bits)
        ctx = f"n={n} options={(tile_bits, group_bits)}"
        assert got["parents"] == parents.tolist() and got["order"] == order.tolist(), ctx
        assert got["total_bits"] == int(bits([total])[0]), ctx
        assert np.array_equal(np.array(got["bps_score_bits"], np.uint64), bits(score)), ctx
        assert np.array_equal(np.array(got["bps_mask"], np.uint32), mask.reshape(-1)), ctx
        assert np.array_equal(np.array(got["best_bits"], np.uint64), bits(best)), ctx
        assert np.array_equal(np.array(got["sink"], np.uint8), sink), ctx
        # the printed schedule: every one of the n - 1 index bits at least once, tiles that fit the kernel's LDS arrays and tile
        # the child's table exactly
        T, G = tile_bits or 12, group_bits or 6
        covered = set()
        for k, p in enumerate(got["schedule"]):
            covered |= set(range(p["b0"], p["b0"] + p["g"]))
            assert 0 <= p["c"] <= p["b0"] and p["g"] >= 1 and p["g"] + p["c"] <= 12 and p["b0"] + p["g"] <= n - 1, ctx
            assert p["g"] <= (T if k == 0 else G), ctx
            assert p["tiles_per_child"] << (p["g"] + p["c"]) == 1 << (n - 1) and p["grid"] == n * p["tiles_per_child"], ctx
        assert covered == set(range(n - 1)), ctx


@needs_gxx
def test_sim_schedules_by_hand(sim):
    """n = 9 (8 index bits): (3, 2) ends in a ragged group of one bit, (2, 5) in a group wider than the bit left; the defaults
    are one pass up to n = 13 and split above."""
    ch, ms, ss = chain_candidates(9)
    shape = lambda got: [(p["b0"], p["g"], p["c"]) for p in got["schedule"]]  # noqa: E731
    assert shape(sim(9, ch, ms, ss, 3, 2, tables=False)) == [(0, 3, 0), (3, 2, 1), (5, 2, 1), (7, 1, 2)]
    assert shape(sim(9, ch, ms, ss, 3, 3, tables=False)) == [(0, 3, 0), (3, 3, 0), (6, 2, 1)]
    assert shape(sim(9, ch, ms, ss, 1, 1, tables=False)) == [(b, 1, 0) for b in range(8)]
    assert shape(sim(9, ch, ms, ss, 2, 5, tables=False)) == [(0, 2, 0), (2, 5, 0), (7, 1, 1)]
    assert shape(sim(9, ch, ms, ss, tables=False)) == [(0, 8, 0)]
    ch, ms, ss = chain_candidates(16)
    got = sim(16, ch, ms, ss, tables=False)
    assert shape(got) == [(0, 12, 0), (12, 3, 9)] and got["total"] == 15.0 and got["order"] == list(range(16))


@needs_gxx
def test_sim_refuses_what_the_call_refuses(sim):
    bad = [(0, [], [], []), (2, [2], [0], [0.0]), (2, [0], [1], [0.0]), (2, [0], [4], [0.0]), (2, [0], [0], [math.nan]), (2, [0], [0], [math.inf]),
           (2, [0, 1, 0], [0, 0, 0], [0.0, 0.0, 1.0])]
    for n, ch, ms, ss in bad:
        got = sim(n, ch, ms, ss)
        assert got["error"] == _capi.E_ARG, (n, ch, ms, got)
    assert sim(25, [0], [0], [0.0])["error"] == _capi.E_LIMIT
    got = sim(2, [0, 1], [2, 1], [0.0, 0.0])  # no DAG
    assert got["total"] == "-inf" and got["parents"] == [dc.NO_MASK] * 2 and got["order"] == [-1, -1]


# --------------------------------------------------------------------------------------------- exact_search over test doubles
class DagTwinEngine(wc.WeightedTwinEngine):
    """TEST DOUBLE for the counting engine (never on the product path): weighted family scores by the twins, `best_dag` by
    tests/dag_check.py; `dag_calls` keeps the arguments of every best_dag call."""

    def __init__(self):
        super().__init__()
        self.dag_calls = []

    def best_dag(self, n_vars, children, parent_masks, scores):
        self.dag_calls.append((n_vars, list(children), list(parent_masks), np.array(scores)))
        return dc.best_dag(n_vars, children, parent_masks, scores)


@pytest.fixture
def twin_engine(monkeypatch):
    eng = DagTwinEngine()
    monkeypatch.setattr(learning, "counting_engine", lambda device=None: eng)
    return eng


@pytest.fixture
def no_engine(monkeypatch):
    def fail(device=None):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(learning, "counting_engine", fail)


def frame(codes, names=None):
    return pd.DataFrame(np.asarray(codes).astype(np.int64), columns=names or [f"c{j}" for j in range(codes.shape[1])])


def recode(codes):
    cols = [np.unique(codes[:, j], return_inverse=True) for j in range(codes.shape[1])]
    return np.stack([np.asarray(inv).reshape(-1) for _, inv in cols], axis=1), [len(u) for u, _ in cols]


def test_exact_search_candidates_scores_and_result(twin_engine):
    codes, _ = planted(5, 7)
    codes, card = recode(codes)
    X = frame(codes)
    names = list(X.columns)
    for k, req, forb in [(2, (), ()), (1, (), ()), (0, (), ()), (3, (("c3", "c1"),), (("c0", "c1"), ("c4", "c2"))), (4, (), ())]:
        twin_engine.calls.clear()
        twin_engine.dag_calls.clear()
        result, info = learning.exact_search(X, "bic", max_parents=k, required=req, forbidden=forb, return_info=True)
        ireq = [(names.index(u), names.index(v)) for u, v in req]
        iforb = [(names.index(u), names.index(v)) for u, v in forb]
        want = dc.bounded_candidates(5, k, ireq, iforb)
        # one score_families call, no family asked twice, in the pinned order, parents ascending and the child last
        assert len(twin_engine.calls) == 1 and twin_engine.calls[0][0] == "score"
        asked = [scope for scope, s in twin_engine.calls[0][1]]
        assert all(s == -1 for _, s in twin_engine.calls[0][1])
        assert len(set(asked)) == len(asked) == len(want) == info["n_families"]
        assert asked == [tuple(u for u in range(5) if (pm >> u) & 1) + (v,) for v, pm in want]
        if not req and not forb:
            assert len(want) == 5 * sum(math.comb(4, j) for j in range(k + 1))
        # the same candidates reach best_dag with those scores
        (n_vars, children, masks, scores), = twin_engine.dag_calls
        assert n_vars == 5 and list(zip(children, masks)) == want
        assert np.array_equal(scores, scored(codes, card, want, "bic"))
        # the result: what the twin finds, in hill_climb's form
        parents, order, total = dc.best_dag(5, children, masks, scores)
        edges = [(names[u], names[v]) for v in range(5) for u in range(5) if (int(parents[v]) >> u) & 1]
        linked = {c for e in edges for c in e}
        assert result == edges + [c for c in names if c not in linked]
        assert learning.exact_search(X, "bic", max_parents=k, required=req, forbidden=forb) == result
        at = dict(zip(want, scores.tolist()))
        assert info["total"] == math.fsum(at[(v, int(parents[v]))] for v in range(5))
        assert info["dp_total"] == total and info["order"] == [names[v] for v in order]
        for u, v in req:
            assert (u, v) in result
        for u, v in forb:
            assert (u, v) not in result
        # never worse than hill climbing on the same scores
        _, _, hc_total = learning.hill_climb(X, "bic", max_parents=k, required=req, forbidden=forb, return_trace=True)
        assert info["total"] >= hc_total - TOL * abs(hc_total)
    assert structure.exact_search is learning.exact_search and structure.best_dag is learning.best_dag
    assert {"exact_search", "best_dag"} <= set(structure.__all__)


def test_exact_search_weights_equal_the_expanded_frame(twin_engine):
    codes, _ = planted(4, 11, n_rows=120)
    codes, _ = recode(codes)
    rng = np.random.default_rng(5)
    w = rng.integers(0, 4, len(codes))
    w[:8] = 1  # (every label occurs in the expanded frame too: the domains are those of all rows)
    X = frame(codes)
    a, ia = learning.exact_search(X, "bdeu", ess=2.0, max_parents=2, weights=w, return_info=True)
    assert all(s == 0 for _, s in twin_engine.calls[-1][1])  # every family under weight set 0, as hill_climb asks
    b, ib = learning.exact_search(frame(wc.expand(codes, w)), "bdeu", ess=2.0, max_parents=2, return_info=True)
    assert a == b and ia == ib
    Xw = X.assign(freq=w)
    assert learning.exact_search(Xw, "bdeu", ess=2.0, max_parents=2, weights="freq", return_info=True) == (a, ia)


def test_best_dag_of_own_scores(twin_engine):
    cols = ["a", "b", "c"]
    cand = [("a", []), ("b", ["a"]), ("b", []), ("c", "b"), ("c", []), ("a", ["c"])]
    assert learning.best_dag(cols, cand, [0.0, 1.0, 0.0, 1.0, 0.0, 1.5]) == [("c", "a"), ("b", "c")]
    assert learning.best_dag(cols, [("a", []), ("b", []), ("c", [])], [1.0, 2.0, 3.0]) == ["a", "b", "c"]
    with pytest.raises(ValueError, match="no DAG"):
        learning.best_dag(cols, [("a", []), ("b", ["a"])], [0.0, 0.0])  # c has no candidate
    with pytest.raises(ValueError, match="no DAG"):
        learning.best_dag(["a", "b"], [("a", ["b"]), ("b", ["a"])], [0.0, 0.0])


def test_best_dag_argument_errors(no_engine):
    for cols, cand, scores, msg in [(["a", "a"], [], [], "duplicate"), ([], [], [], "columns"), ([f"c{j}" for j in range(25)], [], [], "columns"),
                                    (["a"], [("a", [])], [], "one entry"), (["a"], [("a", [])], [math.nan], "finite"), (["a"], [("b", [])], [0.0], "unknown"),
                                    (["a", "b"], [("a", ["z"])], [0.0], "unknown"), (["a", "b"], [("a", ["a"])], [0.0], "twice"),
                                    (["a", "b"], [("a", ["b"]), ("a", ["b"])], [0.0, 1.0], "listed twice")]:
        with pytest.raises(ValueError, match=msg):
            learning.best_dag(cols, cand, scores)


def test_exact_search_argument_errors(no_engine):
    codes, _ = planted(4, 3, n_rows=40)
    X = frame(codes)
    bad = [
        (dict(X=pd.DataFrame(codes[:, [0, 1]], columns=["a", "a"])), "duplicate column"),
        (dict(X=frame(np.zeros((3, 25), np.int64))), "hill_climb or pc"),
        (dict(max_parents=-1), "max_parents"),
        (dict(required=[("c0", "c1")], forbidden=[("c0", "c1")]), "both required and forbidden"),
        (dict(required=[("c0", "c1"), ("c1", "c2"), ("c2", "c0")]), "cycle"),
        (dict(required=[("c0", "c3"), ("c1", "c3")], max_parents=1), "2 required parents"),
        (dict(max_families=31), "32 candidate families"),
        (dict(X=frame(np.tile(np.arange(200)[:, None], (1, 5))), max_parents=4), "cells"),
        (dict(X=X.astype(float).mask(X == X.iloc[0, 0])), "missing values"),
        (dict(score="nope"), "score must be"),
        (dict(score="bdeu", ess=0.0), "ess"),
        (dict(required=[("c0", "zz")]), "unknown column"),
        (dict(weights=np.ones(3)), "weights"),
    ]
    for kw, msg in bad:
        args = dict(X=X, max_parents=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            learning.exact_search(**args)


def test_binding_declares_mibn_best_dag():
    assert "mibn_best_dag" in _capi.SYMBOLS and _capi.BEST_DAG_MAX_VARS == 24
    with open(os.path.join(ROOT, "include", "mibn.h")) as fh:
        header = fh.read()
    assert "int mibn_best_dag(mibn_t *h, int32_t n_vars, int64_t n_fam," in header and "#define MIBN_BEST_DAG_MAX_VARS 24" in header
    L = _capi.lib()
    assert hasattr(L, "mibn_best_dag") and len(L.mibn_best_dag.argtypes) == 9
    assert callable(_capi.Engine.best_dag)
