"""Exact arc posteriors on the GPU: `mibn_arc_posteriors` (csrc/dag_post_kernel.hip.h under the schedule of csrc/dag_plan.h)
against the numpy twin of tests/arc_check.py within the derived tolerance - under the default passes and under the test-hook
options that force multi-pass schedules at small n -, exact answers on a forced chain, repeatability, the error paths, the
statistics rows, and `structure.arc_posteriors` end to end against the twin fed with twin-scored candidates.

Tolerance (include/mibn.h, derived in tests/test_arc_posterior_host.py): tol = 8 D 2^-53 (1 + M), D = n^2 + 2 n +
ceil(log2(n_fam + 1)), M = the largest finite |value| among the twin's L, R and centred scores; absolute on log_post and
log_evidence, and on the arcs as probabilities."""
import math
import os

import numpy as np
import pandas as pd
import pytest

import arc_check as ac
import dag_check as dc
import netspec
import structure_check as sc
from sorobn_amd import _capi, learning, structure

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DAG_TILE_BITS, DAG_GROUP_BITS = 12, 6  # kDagTileBits / kDagGroupBits of csrc/dag_plan.h
OPTION_PAIRS = [(3, 2), (3, 3), (1, 1), (2, 5)]  # (dag_tile_bits, dag_group_bits) beside the defaults
SIZES = [1, 2, 3, 5, 8, 9, 13, 16]
SCALE = 8.0  # scores uniform in [-8, 0]: neighbouring terms of a sum are of comparable size, so every (+) rounds
SCORE_TOL = 1e-12  # the structure tests' relative tolerance between the device's family scores and structure_check's


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _deviation(got, want):
    """max |got - want| over log_post, the arcs and log_evidence; -inf must stand in the same places."""
    worst = 0.0
    for g, w in zip(got, want):
        g, w = np.asarray(g, np.float64).reshape(-1), np.asarray(w, np.float64).reshape(-1)
        assert g.shape == w.shape and not np.isnan(g).any()
        assert np.array_equal(np.isfinite(g), np.isfinite(w)) and np.array_equal(g[~np.isfinite(g)], w[~np.isfinite(w)])
        both = np.isfinite(g)
        if both.any():
            worst = max(worst, float(np.abs(g[both] - w[both]).max()))
    return worst


@pytest.fixture(scope="module")
def engine():
    assert _capi.device_count() > 0, "no HIP device visible"
    return learning.counting_engine()


@pytest.fixture(scope="module")
def hooked():
    """One engine per option pair."""
    made = []
    for t, g in OPTION_PAIRS:
        e = _capi.Engine(0)
        e.set_option("dag_tile_bits", t)
        e.set_option("dag_group_bits", g)
        made.append(e)
    yield made
    for e in made:
        e.close()


@pytest.fixture(scope="module")
def dense_cases():
    """The score sets of the host test with the twin's answer and its tolerance, computed once."""
    out = {}
    for n in SIZES:
        cand = ac.dense_candidates(n, seed=100 + n, scale=SCALE)
        log_post, arc, log_evidence, _, _, _, M = ac.arc_posteriors(n, *cand, tables=True)
        out[n] = (cand, (log_post, arc, log_evidence), ac.tolerance(n, len(cand[0]), M))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_twin_within_the_bound(engine, hooked, dense_cases, n):
    # both sides of every boundary of the schedule, as tests/test_exact.py: n = 13 is the first size with a second pass under the
    # defaults, n = 9 under (3, 2) has the ragged last group, n <= 6 has fewer entries per child than one wave
    assert DAG_TILE_BITS + 1 in SIZES and any(s - 1 > DAG_TILE_BITS for s in SIZES) and (9 - 1 - 3) % 2 == 1
    cand, want, tol = dense_cases[n]
    assert tol < 1e-9
    got = engine.arc_posteriors(n, *cand)
    assert got[0].shape == (len(cand[0]),) and got[1].shape == (n, n)
    worst = _deviation(got, want)
    print(f"n={n} families={len(cand[0])} tol={tol:.2e} defaults: max deviation {worst:.2e}")
    assert worst <= tol, (n, worst, tol)
    for e, pair in zip(hooked, OPTION_PAIRS):
        worst = _deviation(e.arc_posteriors(n, *cand), want)
        print(f"n={n} options={pair}: max deviation {worst:.2e}")
        assert worst <= tol, (n, pair, worst, tol)
    if n > 1:
        for v in range(n):
            own = cand[0] == v
            assert abs(np.exp(got[0][own]).sum() - 1.0) <= tol * max(1, int(own.sum())), (n, v)
        assert (got[1] + got[1].T <= 1.0 + tol).all() and (np.diag(got[1]) == 0.0).all()


def test_magnitudes_of_a_thousand(engine, hooked):
    """Scores uniform in [-1000, 0] at n = 9: M in the thousands, most sums have one term that counts."""
    cand = ac.dense_candidates(9, seed=109, scale=1000.0)
    log_post, arc, log_evidence, _, _, _, M = ac.arc_posteriors(9, *cand, tables=True)
    tol = ac.tolerance(9, len(cand[0]), M)
    assert M > 1000.0 and tol < 1e-9
    for e in [engine, *hooked]:
        worst = _deviation(e.arc_posteriors(9, *cand), (log_post, arc, log_evidence))
        print(f"M={M:.1f} tol={tol:.2e} max deviation {worst:.2e}")
        assert worst <= tol


def test_a_full_later_group_of_the_default_schedule(engine, hooked):
    """n = 19: the defaults take 12 + 6 bits.  The twin needs seconds here, so the yardstick is the device under the option pairs,
    whose schedules the twin pins at the smaller sizes above.  M is not at hand without the twin; the centred scores alone bound it
    from below (M >= max |s'|), and a smaller M only makes the tolerance stricter."""
    n = DAG_TILE_BITS + DAG_GROUP_BITS + 1
    children, masks, scores = ac.dense_candidates(n, seed=100 + n, keep=0.05, scale=SCALE)
    c = ac.centres(n, children, scores)
    tol = ac.tolerance(n, len(children), float(np.abs(scores - c[children]).max()))
    got = engine.arc_posteriors(n, children, masks, scores)
    assert np.isfinite(got[2]) and (got[1] >= 0.0).all()
    for e, pair in zip(hooked, OPTION_PAIRS):
        if pair != (1, 1):  # (one bit per pass at this size is 18 passes of 2-entry tiles: covered at n <= 16)
            worst = _deviation(e.arc_posteriors(n, children, masks, scores), got)
            print(f"n={n} families={len(children)} options={pair} tol={tol:.2e}: max deviation from the defaults {worst:.2e}")
            assert worst <= tol, (pair, worst, tol)


@pytest.mark.parametrize("n", [17, 20])
def test_forced_chain_is_exact(engine, n):
    """One DAG, one order, integer scores: every sum has a single finite term, which passes through bit for bit."""
    children, masks, scores = ac.forced_chain(n, seed=n)
    log_post, arc, log_evidence = engine.arc_posteriors(n, children, masks, scores)
    assert log_evidence == float(scores.sum())
    assert (log_post == 0.0).all()
    want = np.zeros((n, n))
    want[np.arange(n - 1), np.arange(1, n)] = 1.0
    assert np.array_equal(arc, want)


def test_repeatable_in_any_call_and_through_any_handle(engine, dense_cases):
    cand, _, _ = dense_cases[13]
    first = engine.arc_posteriors(13, *cand)
    for _ in range(2):
        assert _same(engine.arc_posteriors(13, *cand), first)
    other = _capi.Engine(0)
    try:
        assert _same(other.arc_posteriors(13, *cand), first)
    finally:
        other.close()
    engine.best_dag(9, *dc.tie_candidates(9, seed=109))  # (shares the tables' buffers)
    assert _same(engine.arc_posteriors(13, *cand), first)


def test_error_paths_leave_the_engine_usable(engine):
    tie = dc.tie_candidates(8, seed=108)
    want = dc.best_dag(8, *tie)

    def still_answers():
        got = engine.best_dag(8, *tie)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits([got[2]]), _bits([want[2]]))

    nan, inf = float("nan"), float("inf")
    bad = [(0, [], [], [], _capi.E_ARG), (25, [0], [0], [0.0], _capi.E_LIMIT), (3, [3], [0], [0.0], _capi.E_ARG), (3, [-1], [0], [0.0], _capi.E_ARG),
           (3, [1], [2], [0.0], _capi.E_ARG), (3, [0], [8], [0.0], _capi.E_ARG), (3, [0], [0], [nan], _capi.E_ARG), (3, [0], [0], [inf], _capi.E_ARG),
           (3, [0], [0], [-inf], _capi.E_ARG), (3, [0, 1, 0], [6, 0, 6], [0.0, 0.0, 1.0], _capi.E_ARG)]
    for n, ch, ms, ss, code in bad:
        with pytest.raises(_capi.MibnError) as e:
            engine.arc_posteriors(n, ch, ms, ss)
        assert e.value.code == code, (n, ch, ms, ss, e.value)
        assert "arc_posteriors" in str(e.value)
        still_answers()
    # candidates without a DAG (0 <- 1 and 1 <- 0 only), a child without any candidate, no candidate at all: the pinned outputs
    for n, ch, ms, ss in [(2, [0, 1], [2, 1], [0.0, 0.0]), (3, [0, 1], [0, 1], [0.0, 0.0]), (2, [], [], [])]:
        log_post, arc, log_evidence = engine.arc_posteriors(n, ch, ms, ss)
        assert log_evidence == -math.inf and len(log_post) == len(ch) and (log_post == -math.inf).all()
        assert np.array_equal(arc, np.zeros((n, n)))
        still_answers()
    with pytest.raises(ValueError, match="no DAG"):
        structure.arc_posteriors_from_scores(["a", "b"], [("a", ["b"]), ("b", ["a"])], [0.0, 0.0])
    got = structure.arc_posteriors_from_scores(["a", "b"], [("a", []), ("b", []), ("b", ["a"])], [0.0, 0.0, 0.0])
    assert abs(got.matrix.loc["a", "b"] - 1.0 / 3.0) <= 1e-15 and got.matrix.loc["b", "a"] == 0.0  # orders (a, b): 2 graphs, (b, a): 1


def test_statistics_rows(engine, dense_cases):
    cand, _, _ = dense_cases[9]
    engine.arc_posteriors(9, *cand)
    rows = {k["name"]: k for k in engine.kernel_stats()}
    assert set(rows) == {"dag_post_subset_kernel", "dag_post_level_kernel", "dag_post_superset_kernel", "dag_post_arc_kernel"}
    assert rows["dag_post_subset_kernel"]["launches"] == 3 and rows["dag_post_level_kernel"]["launches"] == 10  # fill, scatter, one pass; levels 0 .. 9
    assert rows["dag_post_superset_kernel"]["launches"] == 1 and rows["dag_post_arc_kernel"]["launches"] == 3
    assert all(r["alg_bytes"] > 0 for r in rows.values())
    assert rows["dag_post_subset_kernel"]["items"] == len(cand[0]) == rows["dag_post_arc_kernel"]["items"]
    total_before = engine.total_kernel_stats()
    engine.arc_posteriors(9, *cand)
    assert engine.total_kernel_stats() == total_before, "arc_posteriors books last-call statistics only"


def _example(name):
    return next(n for n in netspec.load(os.path.join(GOLDEN, "examples.json")) if n["spec"]["name"] == name)["spec"]


@pytest.mark.parametrize("name", ["sprinkler", "asia"])
def test_arc_posteriors_end_to_end(engine, name):
    """The device scores the candidates itself; the twin is fed with structure_check's scores.  A result is a log ratio of sums of
    products of n weights, so scores that differ by at most d move a log_post by at most 2 n d; d <= SCORE_TOL * max |score|."""
    names, raw, _ = sc.forward_sample(_example(name), 2000, seed=3)
    X = pd.DataFrame(raw.astype(np.int64), columns=names)
    cols = [np.unique(raw[:, j], return_inverse=True) for j in range(raw.shape[1])]
    codes = np.stack([np.asarray(inv).reshape(-1) for _, inv in cols], axis=1)
    card = [len(u) for u, _ in cols]
    n = len(names)
    cand = dc.bounded_candidates(n, 3)
    children, masks = [v for v, _ in cand], [pm for _, pm in cand]
    score = sc.scorer(codes, card, "bdeu")
    base = np.array([score(v, [u for u in range(n) if (pm >> u) & 1]) for v, pm in cand])
    for prior in ("uniform", "size"):
        scores = base if prior == "uniform" else base - np.array([math.log(math.comb(n - 1, bin(pm).count("1"))) for pm in masks])
        log_post, arc, log_evidence, _, _, _, M = ac.arc_posteriors(n, children, masks, scores, tables=True)
        bound = ac.tolerance(n, len(cand), M) + 2 * n * SCORE_TOL * float(np.abs(scores).max())
        got = structure.arc_posteriors(X, "bdeu", parent_prior=prior)
        assert got.n_families == len(cand) and got.columns == names
        worst = (float(np.abs(got.matrix.to_numpy() - arc).max()), abs(got.log_evidence - log_evidence))
        print(f"{name} {prior}: families={len(cand)} M={M:.1f} bound={bound:.2e} max|arc - twin| {worst[0]:.2e} |log_evidence - twin| {worst[1]:.2e}")
        assert max(worst) <= bound
        for v, child in enumerate(names):
            ps = got.parent_sets(child)
            own = [f for f in range(len(cand)) if children[f] == v]
            at = {tuple(names[u] for u in range(n) if (masks[f] >> u) & 1): float(np.exp(log_post[f])) for f in own}
            assert abs(ps.sum() - 1.0) <= bound * len(own) and set(ps.index) == set(at)
            assert max(abs(float(p) - at[k]) for k, p in ps.items()) <= bound
        strength = got.frame["strength"].to_numpy()
        assert ((strength > 0.0) & (strength <= 1.0 + bound)).all()
        edges = [e for e in got.edges() if isinstance(e, tuple)]
        pos = {c: j for j, c in enumerate(names)}
        parents = [set() for _ in names]
        for u, v in edges:
            parents[pos[v]].add(pos[u])
        assert not sc.has_cycle(n, parents)
    # all rows twice by weight = the rows written out twice
    a = structure.arc_posteriors(X, "bdeu", weights=np.full(len(X), 2))
    b = structure.arc_posteriors(pd.concat([X, X], ignore_index=True), "bdeu")
    assert a.matrix.equals(b.matrix) and a.log_evidence == b.log_evidence
