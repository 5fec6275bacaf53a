"""Exact arc posteriors, host side (no GPU): the numpy twin of mibn_arc_posteriors (tests/arc_check.py) against an enumeration
of every (order, consistent parent sets) pair and against closed forms, the CPU twin of the device's schedule
(tools/dag_post_sim.cpp running sorobn_amd/csrc/dag_plan.h) against the numpy twin within the derived tolerance,
`learning.arc_posteriors` / `learning.arc_posteriors_from_scores` over test doubles of the engine, and every argument error with
the engine patched to fail.

Tolerance (derived, include/mibn.h): the operands are positive in the linear domain, so nothing cancels; a result sits at most
D = n^2 + 2 n + ceil(log2(n_fam + 1)) roundings deep, each within a few ulp of the magnitude M of the log values involved:
tol = 8 D 2^-53 (1 + M), M = the largest finite |value| among the twin's L, R and centred scores (arc_check.tolerance)."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest

import arc_check as ac
import dag_check as dc
import structure_check as sc
import weights_check as wc
from sorobn_amd import _capi, learning, structure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_PAIRS = [(0, 0), (3, 2), (3, 3), (1, 1), (2, 5)]  # (dag_tile_bits, dag_group_bits); 0 = the default
needs_gxx = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")

ENUMERATED = [  # (n, max_parents, seed, required, forbidden, drop): drop = candidates taken away (index in the bounded list)
    (4, 3, 0, (), (), ()),
    (5, 2, 1, (), (), ()),
    (4, 3, 2, ((3, 1),), ((0, 1),), ()),
    (5, 2, 3, ((0, 4),), ((2, 3),), ()),
    (4, 3, 4, (), (), "all but {} of child 2"),
]


def enumerated_case(n, k, seed, req, forb, drop):
    ch, ms, ss = ac.random_candidates(n, k, seed, req, forb)
    if drop:  # one child with a single candidate
        keep = [f for f in range(len(ch)) if ch[f] != 2 or ms[f] == 0]
        ch, ms, ss = [ch[f] for f in keep], [ms[f] for f in keep], ss[keep]
        assert sum(1 for v in ch if v == 2) == 1
    return ch, ms, ss


@pytest.mark.parametrize("case", ENUMERATED, ids=lambda c: f"n{c[0]}k{c[1]}s{c[2]}")
def test_twin_equals_the_enumeration_of_every_order(case):
    n, _, _, req, forb, _ = case
    ch, ms, ss = enumerated_case(*case)
    log_post, arc, log_evidence = ac.arc_posteriors(n, ch, ms, ss)
    post, want_arc, want_evidence = ac.all_orders_posterior(n, ch, ms, ss)
    worst = (float(np.abs(np.exp(log_post) - post).max()), float(np.abs(arc - want_arc).max()), abs(log_evidence - want_evidence))
    print(f"n={n} families={len(ch)} max|post - enum| {worst[0]:.2e} max|arc - enum| {worst[1]:.2e} |log_evidence - enum| {worst[2]:.2e}")
    assert max(worst) <= 1e-9
    for u, v in req:
        assert abs(arc[u, v] - 1.0) <= 1e-9
    for u, v in forb:
        assert arc[u, v] == 0.0


def test_two_columns_closed_form():
    """0 <- {} a, 0 <- {1} b, 1 <- {} c, 1 <- {0} d: the orders (0, 1) and (1, 0) give Z = 2 e^(a+c) + e^(a+d) + e^(b+c) - the empty
    graph counts twice: the prior is order-modular, not uniform."""
    a, b, c, d = 0.3, -1.1, 0.7, 0.2
    log_post, arc, log_evidence = ac.arc_posteriors(2, [0, 0, 1, 1], [0, 2, 0, 1], [a, b, c, d])
    Z = 2 * math.exp(a + c) + math.exp(a + d) + math.exp(b + c)
    assert abs(log_evidence - math.log(Z)) <= 1e-14
    assert abs(arc[0, 1] - math.exp(a + d) / Z) <= 1e-15 and abs(arc[1, 0] - math.exp(b + c) / Z) <= 1e-15
    assert arc[0, 0] == arc[1, 1] == 0.0
    want = [(2 * math.exp(a + c) + math.exp(a + d)) / Z, math.exp(b + c) / Z, (2 * math.exp(a + c) + math.exp(b + c)) / Z, math.exp(a + d) / Z]
    assert np.abs(np.exp(log_post) - want).max() <= 1e-15
    # all four scores equal: the empty graph has half the mass, each arc a quarter
    _, arc, log_evidence = ac.arc_posteriors(2, [0, 0, 1, 1], [0, 2, 0, 1], [0.0] * 4)
    assert abs(arc[0, 1] - 0.25) <= 1e-15 and abs(arc[1, 0] - 0.25) <= 1e-15 and abs(log_evidence - math.log(4.0)) <= 1e-15


def test_posteriors_are_distributions():
    for n, seed in [(6, 0), (7, 1), (8, 2)]:
        ch, ms, ss = ac.dense_candidates(n, seed, scale=6.0)
        log_post, arc, _, L, R, _, M = ac.arc_posteriors(n, ch, ms, ss, tables=True)
        tol = ac.tolerance(n, len(ch), M)
        for v in range(n):
            own = np.asarray(ch) == v
            assert abs(np.exp(log_post[own]).sum() - 1.0) <= tol * own.sum(), (n, v)
        assert (arc + arc.T <= 1.0 + tol).all() and (arc >= 0.0).all() and (np.diag(arc) == 0.0).all()
        assert abs(L[-1] - R[-1]) <= tol  # L(V) = R(V) up to rounding


def test_empty_parent_sets_only():
    n = 6
    s = np.array([-3.5, 2.0, 0.25, -7.0, 1.0, 4.0])
    log_post, arc, log_evidence = ac.arc_posteriors(n, list(range(n)), [0] * n, s)
    assert abs(log_evidence - (math.log(math.factorial(n)) + s.sum())) <= 1e-12
    assert (arc == 0.0).all() and np.abs(log_post).max() <= 1e-12


@pytest.mark.parametrize("n", [2, 5, 9, 12])
def test_forced_chain_is_exact(n):
    ch, ms, ss = ac.forced_chain(n, seed=n)
    log_post, arc, log_evidence = ac.arc_posteriors(n, ch, ms, ss)
    assert log_evidence == float(ss.sum())
    assert (log_post == 0.0).all()
    want = np.zeros((n, n))
    want[np.arange(n - 1), np.arange(1, n)] = 1.0
    assert np.array_equal(arc, want)


def test_large_negative_scores_stay_finite():
    """Scores near -1e6 with gaps of 1e4: exp of any of them, or of a gap, is 0 in fp64 - a linear-domain DP would return 0 / 0."""
    n = 5
    cand = dc.bounded_candidates(n, 2)
    ch, ms = [v for v, _ in cand], [pm for _, pm in cand]
    rng = np.random.default_rng(0)
    ss = -1e6 - 1e4 * rng.integers(0, 6, len(cand)).astype(np.float64)
    assert math.exp(ss.max()) == 0.0 and math.exp(-1e4) == 0.0
    with np.errstate(all="raise", under="ignore"):
        log_post, arc, log_evidence = ac.arc_posteriors(n, ch, ms, ss)
    assert np.isfinite(log_evidence) and not np.isnan(log_post).any() and np.isfinite(arc).all()
    assert -5.1e6 - 1e5 < log_evidence < -4.9e6
    for v in range(n):
        assert abs(np.exp(log_post[np.asarray(ch) == v]).sum() - 1.0) <= 1e-9


def test_no_dag_gives_the_pinned_outputs():
    for n, ch, ms, ss in [(2, [0, 1], [2, 1], [0.0, 0.0]), (3, [0, 1], [0, 1], [0.5, 0.25]), (2, [], [], [])]:
        log_post, arc, log_evidence = ac.arc_posteriors(n, ch, ms, np.array(ss))
        assert log_evidence == -math.inf and (log_post == -math.inf).all() and len(log_post) == len(ch)
        assert np.array_equal(arc, np.zeros((n, n)))


def test_logaddexp_as_pinned():
    inf = math.inf
    assert ac.logaddexp(-inf, -inf) == -inf and ac.logaddexp(-inf, 1.5) == 1.5 and ac.logaddexp(-2.25, -inf) == -2.25
    assert ac.logaddexp(0.0, 0.0) == math.log(2.0) and ac.logaddexp(3.0, -800.0) == 3.0
    x = np.array([-inf, 0.1, -5.0])
    assert np.array_equal(ac.logaddexp(x, np.array([-inf, -inf, -5.0])), np.array([-inf, 0.1, -5.0 + math.log1p(1.0)]))


# ------------------------------------------------------------------------------------------- tools/dag_post_sim against the twin
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dagpost") / "dag_post_sim")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "dag_post_sim.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(n, children, masks, scores, tile_bits=0, group_bits=0, tables=True):
        lines = [f"{n} {tile_bits} {group_bits} {int(tables)} {len(children)}"]
        lines += [f"{int(v)} {int(pm)} {float(s)!r}" for v, pm, s in zip(children, masks, scores)]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout)
    return run


def floats(bits):
    return np.array(bits, np.uint64).view(np.float64)


def deviation(got, want):
    """max |got - want| where both are finite; -inf must stand in the same places."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and not np.isnan(got).any()
    assert np.array_equal(got[~np.isfinite(got)], want[~np.isfinite(want)])
    both = np.isfinite(got)
    return float(np.abs(got[both] - want[both]).max()) if both.any() else 0.0


@needs_gxx
@pytest.mark.parametrize("n,scale", [(1, 8.0), (2, 8.0), (3, 8.0), (8, 8.0), (9, 8.0), (9, 1000.0), (13, 8.0)])
def test_sim_equals_the_twin_within_the_bound(sim, n, scale):
    ch, ms, ss = ac.dense_candidates(n, seed=100 + n, scale=scale)
    log_post, arc, log_evidence, L, R, _, M = ac.arc_posteriors(n, ch, ms, ss, tables=True)
    tol = ac.tolerance(n, len(ch), M)
    assert tol < 1e-9
    for tile_bits, group_bits in OPTION_PAIRS:
        got = sim(n, ch, ms, ss, tile_bits, group_bits)
        ctx = f"n={n} scale={scale} options={(tile_bits, group_bits)}"
        worst = (deviation(floats(got["log_post_bits"]), log_post), deviation(floats(got["arc_bits"]), arc),
                 deviation(floats(got["log_evidence_bits"]), [log_evidence]), deviation(floats(got["L_bits"]), L), deviation(floats(got["R_bits"]), R))
        print(f"{ctx}: families={len(ch)} M={M:.1f} tol={tol:.2e} max deviation log_post {worst[0]:.2e} arc {worst[1]:.2e} "
              f"log_evidence {worst[2]:.2e} L {worst[3]:.2e} R {worst[4]:.2e}")
        assert max(worst) <= tol, ctx
        T, G = tile_bits or 12, group_bits or 6
        covered = set()
        for k, p in enumerate(got["schedule"]):
            covered |= set(range(p["b0"], p["b0"] + p["g"]))
            assert p["g"] <= (T if k == 0 else G) and p["g"] + p["c"] <= 12, ctx
        assert covered == set(range(n - 1)), ctx


@needs_gxx
def test_sim_exact_cases_and_refusals(sim):
    ch, ms, ss = ac.forced_chain(9, seed=9)
    for tile_bits, group_bits in OPTION_PAIRS:
        got = sim(9, ch, ms, ss, tile_bits, group_bits, tables=False)
        assert floats(got["log_evidence_bits"])[0] == float(ss.sum()) and (floats(got["log_post_bits"]) == 0.0).all()
        arc = floats(got["arc_bits"]).reshape(9, 9)
        assert all(arc[v - 1, v] == 1.0 for v in range(1, 9)) and arc.sum() == 8.0
    got = sim(2, [0, 1], [2, 1], [0.0, 0.0])  # no DAG
    assert floats(got["log_evidence_bits"])[0] == -math.inf and (floats(got["log_post_bits"]) == -math.inf).all()
    assert (floats(got["arc_bits"]) == 0.0).all()
    for n, c, m, s in [(0, [], [], []), (2, [2], [0], [0.0]), (2, [0], [1], [0.0]), (2, [0], [0], [math.nan]), (2, [0, 0], [0, 0], [0.0, 1.0])]:
        assert sim(n, c, m, s)["error"] == _capi.E_ARG
    assert sim(25, [0], [0], [0.0])["error"] == _capi.E_LIMIT


# --------------------------------------------------------------------------------------------- arc_posteriors over test doubles
class ArcTwinEngine(wc.WeightedTwinEngine):
    """TEST DOUBLE for the counting engine (never on the product path): weighted family scores by the twins, `arc_posteriors` by
    tests/arc_check.py; `arc_calls` keeps the arguments of every arc_posteriors call."""

    def __init__(self):
        super().__init__()
        self.arc_calls = []

    def arc_posteriors(self, n_vars, children, parent_masks, scores):
        self.arc_calls.append((n_vars, list(children), list(parent_masks), np.array(scores)))
        return ac.arc_posteriors(n_vars, children, parent_masks, scores)


@pytest.fixture
def twin_engine(monkeypatch):
    eng = ArcTwinEngine()
    monkeypatch.setattr(learning, "counting_engine", lambda device=None: eng)
    return eng


@pytest.fixture
def no_engine(monkeypatch):
    def fail(device=None):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(learning, "counting_engine", fail)


def planted(n, seed, n_rows=300):
    """Random rows with cardinalities 2 to 3; column 1 copies column 0 (mod its card) four times out of five."""
    rng = np.random.default_rng(seed)
    card = [int(c) for c in rng.integers(2, 4, n)]
    codes = np.stack([rng.integers(0, c, n_rows) for c in card], axis=1)
    keep = rng.random(n_rows) < 0.8
    codes[keep, 1] = codes[keep, 0] % card[1]
    cols = [np.unique(codes[:, j], return_inverse=True) for j in range(n)]
    return np.stack([np.asarray(inv).reshape(-1) for _, inv in cols], axis=1), [len(u) for u, _ in cols]


def frame(codes, names=None):
    return pd.DataFrame(np.asarray(codes).astype(np.int64), columns=names or [f"c{j}" for j in range(codes.shape[1])])


def scored(codes, card, cand, kind, ess=1.0):
    score = sc.scorer(codes, card, kind, ess)
    return np.array([score(v, [u for u in range(len(card)) if (pm >> u) & 1]) for v, pm in cand])


def test_arc_posteriors_candidates_scores_and_result(twin_engine):
    codes, card = planted(5, 7)
    X = frame(codes)
    names = list(X.columns)
    for k, req, forb, prior in [(2, (), (), "uniform"), (1, (), (), "size"), (0, (), (), "uniform"),
                                (3, (("c3", "c1"),), (("c0", "c1"), ("c4", "c2")), "size")]:
        twin_engine.calls.clear()
        twin_engine.arc_calls.clear()
        got = learning.arc_posteriors(X, "bdeu", max_parents=k, required=req, forbidden=forb, parent_prior=prior)
        ireq = [(names.index(u), names.index(v)) for u, v in req]
        iforb = [(names.index(u), names.index(v)) for u, v in forb]
        want = dc.bounded_candidates(5, k, ireq, iforb)
        # one score_families call, in exact_search's pinned order, parents ascending and the child last
        assert len(twin_engine.calls) == 1 and twin_engine.calls[0][0] == "score"
        asked = [scope for scope, s in twin_engine.calls[0][1]]
        assert all(s == -1 for _, s in twin_engine.calls[0][1])
        assert asked == [tuple(u for u in range(5) if (pm >> u) & 1) + (v,) for v, pm in want]
        assert got.n_families == len(want) == len(set(asked))
        (n_vars, children, masks, scores), = twin_engine.arc_calls
        assert n_vars == 5 and list(zip(children, masks)) == want
        base = scored(codes, card, want, "bdeu")
        if prior == "size":
            base = base - np.array([math.log(math.comb(4, bin(pm).count("1"))) for _, pm in want])
        assert np.array_equal(scores, base)
        # the result object
        log_post, arc, log_evidence = ac.arc_posteriors(5, children, masks, scores)
        assert isinstance(got, learning.ArcPosterior) and got.columns == names and got.log_evidence == log_evidence
        assert list(got.matrix.index) == list(got.matrix.columns) == names and np.array_equal(got.matrix.to_numpy(), arc)
        pairs = [(i, j) for i in range(5) for j in range(i + 1, 5) if arc[i, j] + arc[j, i] > 0.0]
        assert list(got.frame.columns) == ["from", "to", "strength", "direction"]
        assert list(zip(got.frame["from"], got.frame["to"])) == [(names[i], names[j]) for i, j in pairs]
        assert np.array_equal(got.frame["strength"].to_numpy(), np.array([arc[i, j] + arc[j, i] for i, j in pairs]))
        assert np.array_equal(got.frame["direction"].to_numpy(), np.array([arc[i, j] / (arc[i, j] + arc[j, i]) for i, j in pairs]))
        if k == 0:
            assert len(got.frame) == 0 and got.edges() == names
        for u, v in req:
            assert abs(got.matrix.loc[u, v] - 1.0) <= 1e-12 and (u, v) in got.edges()
        for u, v in forb:
            assert got.matrix.loc[u, v] == 0.0
        # parent_sets: the child's candidates, descending, summing to 1
        for v, name in enumerate(names):
            ps = got.parent_sets(name)
            own = [f for f, (c, _) in enumerate(want) if c == v]
            assert len(ps) == len(own) and abs(ps.sum() - 1.0) <= 1e-12 and (np.diff(ps.to_numpy()) <= 0.0).all()
            at = {tuple(names[u] for u in range(5) if (want[f][1] >> u) & 1): float(np.exp(log_post[f])) for f in own}
            assert {k_: float(p) for k_, p in ps.items()} == pytest.approx(at, rel=1e-14, abs=0.0)  # (exp of a scalar and of an array may differ by an ulp)
        with pytest.raises(ValueError, match="unknown column"):
            got.parent_sets("zz")
    assert structure.arc_posteriors is learning.arc_posteriors and structure.ArcPosterior is learning.ArcPosterior
    assert structure.arc_posteriors_from_scores is learning.arc_posteriors_from_scores
    assert {"arc_posteriors", "arc_posteriors_from_scores", "ArcPosterior"} <= set(structure.__all__)


def test_arc_posteriors_weights_equal_the_expanded_frame(twin_engine):
    codes, _ = planted(4, 11, n_rows=120)
    rng = np.random.default_rng(5)
    w = rng.integers(0, 4, len(codes))
    w[:8] = 1  # (every label occurs in the expanded frame too: the domains are those of all rows)
    X = frame(codes)
    a = learning.arc_posteriors(X, "bdeu", ess=2.0, max_parents=2, weights=w)
    assert all(s == 0 for _, s in twin_engine.calls[-1][1])  # every family under weight set 0, as exact_search asks
    b = learning.arc_posteriors(frame(wc.expand(codes, w)), "bdeu", ess=2.0, max_parents=2)
    assert a.matrix.equals(b.matrix) and a.frame.equals(b.frame) and a.log_evidence == b.log_evidence
    c = learning.arc_posteriors(X.assign(freq=w), "bdeu", ess=2.0, max_parents=2, weights="freq")
    assert a.matrix.equals(c.matrix) and a.log_evidence == c.log_evidence


def test_edges_rule_is_arc_strengths(twin_engine):
    """`ArcPosterior.edges` and `ArcStrength.edges` share one body: the same frame gives the same list."""
    cols = ["a", "b", "c"]
    cand = [("a", []), ("a", ["c"]), ("b", []), ("b", ["a"]), ("c", []), ("c", ["b"])]
    got = learning.arc_posteriors_from_scores(cols, cand, [0.0, 1.0, 0.0, 3.0, 0.0, 2.0])
    strength = learning.ArcStrength(cols, [])
    strength.frame = got.frame
    for t in (0.0, 0.3, 0.5, 0.9):
        assert got.edges(t) == strength.edges(t)
    assert got.edges(0.0)[:2] == [("a", "b"), ("b", "c")] and ("c", "a") not in got.edges(0.0)  # the weakest arc would close the cycle
    # ArcStrength itself is unchanged: replicates -> the frame and the edges it always gave
    reps = [[("a", "b"), "c"], [("b", "a"), ("b", "c")], [("a", "b"), ("b", "c")]]
    s = learning.ArcStrength(cols, reps)
    assert s.frame["strength"].tolist() == [1.0, 2 / 3] and s.frame["direction"].tolist() == [2 / 3, 1.0]
    assert s.edges() == [("a", "b"), ("b", "c")] and s.edges(0.9) == [("a", "b"), "c"]


def test_arc_posteriors_from_scores(twin_engine):
    a, b, c, d = 0.3, -1.1, 0.7, 0.2
    got = learning.arc_posteriors_from_scores(["x", "y"], [("x", []), ("x", ["y"]), ("y", []), ("y", "x")], [a, b, c, d])
    Z = 2 * math.exp(a + c) + math.exp(a + d) + math.exp(b + c)
    assert abs(got.matrix.loc["x", "y"] - math.exp(a + d) / Z) <= 1e-15 and abs(got.log_evidence - math.log(Z)) <= 1e-14
    assert got.n_families == 4 and got.parent_sets("y").index.tolist() == [(), ("x",)]
    with pytest.raises(ValueError, match="no DAG"):
        learning.arc_posteriors_from_scores(["a", "b"], [("a", ["b"]), ("b", ["a"])], [0.0, 0.0])
    with pytest.raises(ValueError, match="no DAG"):
        learning.arc_posteriors_from_scores(["a", "b", "c"], [("a", []), ("b", ["a"])], [0.0, 0.0])


def test_from_scores_argument_errors(no_engine):
    for cols, cand, scores, msg in [(["a", "a"], [], [], "duplicate"), ([], [], [], "columns"), ([f"c{j}" for j in range(25)], [], [], "columns"),
                                    (["a"], [("a", [])], [], "one entry"), (["a"], [("a", [])], [math.nan], "finite"), (["a"], [("b", [])], [0.0], "unknown"),
                                    (["a", "b"], [("a", ["z"])], [0.0], "unknown"), (["a", "b"], [("a", ["a"])], [0.0], "twice"),
                                    (["a", "b"], [("a", ["b"]), ("a", ["b"])], [0.0, 1.0], "listed twice")]:
        with pytest.raises(ValueError, match=msg):
            learning.arc_posteriors_from_scores(cols, cand, scores)


def test_arc_posteriors_argument_errors(no_engine):
    codes, _ = planted(4, 3, n_rows=40)
    X = frame(codes)
    bad = [
        (dict(X=pd.DataFrame(codes[:, [0, 1]], columns=["a", "a"])), "duplicate column"),
        (dict(X=frame(np.zeros((3, 25), np.int64))), "arc_posteriors handles at most 24 columns.*use bootstrap"),
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
        (dict(parent_prior="flat"), "parent_prior"),
    ]
    for kw, msg in bad:
        args = dict(X=X, max_parents=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            learning.arc_posteriors(**args)


def test_binding_declares_mibn_arc_posteriors():
    assert "mibn_arc_posteriors" in _capi.SYMBOLS and _capi.ARC_POSTERIOR_MAX_VARS == 24
    with open(os.path.join(ROOT, "include", "mibn.h")) as fh:
        header = fh.read()
    assert "int mibn_arc_posteriors(mibn_t *h, int32_t n_vars, int64_t n_fam," in header and "#define MIBN_ARC_POSTERIOR_MAX_VARS 24" in header
    assert "ORDER-MODULAR" in header
    L = _capi.lib()
    assert hasattr(L, "mibn_arc_posteriors") and len(L.mibn_arc_posteriors.argtypes) == 9
    assert callable(_capi.Engine.arc_posteriors)
