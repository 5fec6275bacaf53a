"""Row weights and bootstrap arc strengths, host logic (no GPU): the twin of tests/weights_check.py against the rows written out,
and the Python surface (`weights=` on the learning calls, `structure.bootstrap`, `ArcStrength`) over its weighted test double."""
import numpy as np
import pandas as pd
import pytest

import netspec
import structure_check as sc
import weights_check as wc
import sorobn_amd
from sorobn_amd import _capi, learning, structure


def _frame(n_rows=400, seed=3, spec=None):
    """(frame of integer codes, codes, cards) of forward samples of a small grid; every label of every column occurs."""
    names, codes, card = sc.forward_sample(spec or netspec.grid_spec(2, 3, 3, seed=4), n_rows, seed)
    assert all(len(np.unique(codes[:, j])) == card[j] for j in range(len(card)))
    return pd.DataFrame(codes.astype(np.int64), columns=names), codes, card


def _weights(codes, card, seed, top=3):
    """Random weights 0 .. top under which EVERY LABEL OF EVERY COLUMN SURVIVES the expansion: a label that only zero-weight rows
    carry is still in the weighted call's domain but not in the expanded frame's, so the cardinalities - and with them BIC,
    AIC, BDeu and the CPT index - would differ.  The comparison with the expanded frame is only defined where they do not."""
    w = np.random.default_rng(seed).integers(0, top + 1, len(codes))
    for j in range(codes.shape[1]):
        for lab in range(card[j]):
            w[np.flatnonzero(codes[:, j] == lab)[0]] = max(1, w[np.flatnonzero(codes[:, j] == lab)[0]])
    assert (w == 0).any()
    return w


@pytest.fixture
def twin_engine(monkeypatch):
    eng = wc.WeightedTwinEngine()
    monkeypatch.setattr(learning, "counting_engine", lambda device=None: eng)
    return eng


def test_twin_tables_equal_the_expanded_rows():
    _, codes, card = _frame(257, 1)
    w = _weights(codes, card, 0)
    for cols in [(0,), (1, 0), (2, 3, 5), (5, 4, 3, 2, 1, 0)]:
        want = wc.weighted_table(wc.expand(codes, w), card, cols)
        assert np.array_equal(wc.weighted_table(codes, card, cols, w), want)
        assert int(want.sum()) == int(w.sum())
        flat = sc.family_table(wc.expand(codes, w), card, cols[-1], list(cols[:-1]))
        assert np.array_equal(want.reshape(flat.shape), flat)
    assert np.array_equal(wc.weighted_table(codes, card, (0, 1)), wc.weighted_table(codes, card, (0, 1), np.ones(len(codes))))
    assert wc.weighted_table(codes[:0], card, (0, 1), np.zeros(0)).sum() == 0


def test_bootstrap_twin():
    for n_rows in (1, 2, 257, 1000):
        five, one = wc.bootstrap_sets(n_rows, 5, 7), wc.bootstrap_sets(n_rows, 1, 7)
        assert five.dtype == np.uint32 and five.shape == (5, n_rows)
        assert (five.sum(axis=1) == n_rows).all()  # every set sums to n_rows
        assert np.array_equal(five[0], one[0])  # set s does not depend on n_sets
        assert np.array_equal(wc.bootstrap_sets(n_rows, 3, 7)[2], five[2])
    assert not np.array_equal(wc.bootstrap_sets(257, 2, 7), wc.bootstrap_sets(257, 2, 8))  # seeds differ
    assert not np.array_equal(wc.bootstrap_sets(257, 2, 7)[0], wc.bootstrap_sets(257, 2, 7)[1])  # sets differ
    assert wc.bootstrap_sets(1, 3, 0).tolist() == [[1], [1], [1]]  # n_rows = 1: all the weight on row 0
    assert wc.bootstrap_sets(0, 2, 0).shape == (2, 0)
    zeros = float((wc.bootstrap_sets(20000, 1, 1) == 0).mean())
    assert abs(zeros - np.exp(-1.0)) < 0.02  # about 37 % of the rows are left out


def test_learning_calls_with_weights_equal_the_expanded_frame(twin_engine):
    X, codes, card = _frame()
    w = _weights(codes, card, 1)
    Xe = X.iloc[np.repeat(np.arange(len(X)), w)].reset_index(drop=True)
    cols = list(X.columns)
    for score in ("bic", "bdeu"):
        assert structure.hill_climb(X, score=score, weights=w, return_trace=True) == structure.hill_climb(Xe, score=score, return_trace=True)
    a, b = structure.pc(X, weights=w, return_trace=True), structure.pc(Xe, return_trace=True)
    assert (a.directed, a.undirected, a.sepsets, a.tests_per_level, a.trace) == (b.directed, b.undirected, b.sepsets, b.tests_per_level, b.trace)
    fams = [(cols[1], [cols[0]]), (cols[4], [cols[1], cols[3]]), (cols[2], [])]
    for score in learning.SCORES:
        assert np.array_equal(structure.family_scores(X, fams, score=score, weights=w), structure.family_scores(Xe, fams, score=score))
    tests = [(cols[0], cols[1], []), (cols[0], cols[5], [cols[1], cols[2]])]
    for test in learning.CI_TESTS:
        pd.testing.assert_frame_equal(structure.ci_tests(X, tests, test=test, dof="adjusted", weights=w),
                                      structure.ci_tests(Xe, tests, test=test, dof="adjusted"), check_exact=True)
    edges = [e for e in structure.hill_climb(X, weights=w)]
    got, want = sorobn_amd.BayesNet(*edges).fit(X, weights=w), sorobn_amd.BayesNet(*edges).fit(Xe)
    assert set(got.P) == set(want.P)
    for node in want.P:
        pd.testing.assert_series_equal(got.P[node], want.P[node], check_exact=True)
    assert got.score(X, weights=w) == want.score(Xe)
    # floats are taken when integral; partial_fit adds up
    parts = sorobn_amd.BayesNet(*edges)
    parts.partial_fit(X.iloc[:150], weights=w[:150].astype(np.float64))
    parts.partial_fit(X.iloc[150:], weights=pd.Series(w[150:]))
    for node in want.P:
        pd.testing.assert_series_equal(parts.P[node], want.P[node], check_exact=True)


def test_weights_as_a_column_of_the_frame(twin_engine):
    """The aggregated-frame case: one row per distinct pattern plus a frequency column."""
    X, _, _ = _frame(600, 5)
    agg = X.value_counts(sort=False).rename("count").reset_index()
    assert len(agg) < len(X) and "count" in agg.columns
    Xs = X.sort_values(list(X.columns)).reset_index(drop=True)  # the expansion of `agg`, in its order
    assert structure.hill_climb(agg, weights="count", return_trace=True) == structure.hill_climb(Xs, return_trace=True)
    assert "count" not in {c for e in structure.hill_climb(agg, weights="count") for c in (e if isinstance(e, tuple) else (e,))}
    assert structure.pc(agg, weights="count").directed == structure.pc(Xs).directed
    edges = structure.hill_climb(Xs)
    got, want = sorobn_amd.BayesNet(*edges).fit(agg, weights="count"), sorobn_amd.BayesNet(*edges).fit(Xs)
    for node in want.P:
        pd.testing.assert_series_equal(got.P[node], want.P[node], check_exact=True)


@pytest.mark.parametrize("args", [{}, {"score": "bdeu", "ess": 2.0, "max_parents": 2}, {"max_iter": 3}])
def test_bootstrap_equals_the_plain_loop(twin_engine, args):
    X, codes, card = _frame(300, 2)
    cols = list(X.columns)
    strength, reps = structure.bootstrap(X, n_boot=5, seed=11, return_replicates=True, return_trace=True, **args)
    search = {k: v for k, v in args.items() if k in ("max_parents", "max_iter")}
    want = wc.bootstrap_loop(codes, card, 5, 11, kind=args.get("score", "bic"), ess=args.get("ess", 1.0), **search)
    assert len(reps) == 5 and strength.n_boot == 5
    for (result, trace, total), (w_edges, w_trace, w_total) in zip(reps, want):
        assert {e for e in result if isinstance(e, tuple)} == {(cols[u], cols[v]) for u, v in w_edges}
        assert [(op, cols.index(u), cols.index(v), g) for op, u, v, g in trace] == w_trace
        assert total == w_total
    # ... and every replicate is the learner called alone under its set
    sets = wc.bootstrap_sets(len(X), 5, 11)
    for r in (0, 4):
        assert reps[r] == structure.hill_climb(X, weights=sets[r], return_trace=True, **args)


def test_bootstrap_pc_replicates_are_pc_under_the_sets(twin_engine):
    X, _, _ = _frame(300, 2)
    strength, reps = structure.bootstrap(X, n_boot=4, learner="pc", seed=5, return_replicates=True, return_trace=True, alpha=0.05, max_cond=2)
    sets = wc.bootstrap_sets(len(X), 4, 5)
    for r, rep in enumerate(reps):
        alone = structure.pc(X, weights=sets[r], return_trace=True, alpha=0.05, max_cond=2)
        assert (rep.directed, rep.undirected, rep.sepsets, rep.tests_per_level, rep.trace) == \
            (alone.directed, alone.undirected, alone.sepsets, alone.tests_per_level, alone.trace)
    again = structure.bootstrap(X, n_boot=4, learner="pc", seed=5, alpha=0.05, max_cond=2)
    pd.testing.assert_frame_equal(strength.frame, again.frame, check_exact=True)


def test_lockstep_asks_for_no_pair_twice_and_once_per_iteration(twin_engine):
    X, _, _ = _frame(300, 2)
    _, reps = structure.bootstrap(X, n_boot=6, seed=3, return_replicates=True, return_trace=True)
    calls = [pairs for kind, pairs in twin_engine.calls if kind == "score"]
    asked = [p for pairs in calls for p in pairs]
    assert len(asked) == len(set(asked))  # no (family, set) pair twice
    assert len(calls) <= 1 + max(len(trace) for _, trace, _ in reps)  # one call per search iteration of the longest replicate
    n = X.shape[1]
    assert len(calls[0]) == 6 * n * n  # the first sweep of every replicate: n + n (n - 1) families each
    assert all(sorted(pairs) == pairs for pairs in calls)  # the tables of one scope lie next to each other
    twin_engine.calls.clear()
    structure.bootstrap(X, n_boot=3, learner="pc", seed=3)
    calls = [pairs for kind, pairs in twin_engine.calls if kind == "ci"]
    asked = [p for pairs in calls for p in pairs]
    assert len(asked) == len(set(asked)) and len(calls) <= 4  # levels 0 .. max_cond


class _PC:
    def __init__(self, directed, undirected):
        self.directed, self.undirected = directed, undirected


def test_arc_strength_by_hand():
    cols = ["a", "b", "c", "d", "e"]
    reps = [
        [("a", "b"), ("b", "c"), ("c", "a"), "d", "e"],          # (a cycle over the replicates, not within one)
        ([("b", "a"), ("b", "c"), "d", "e"], [], 0.0),           # a (result, trace, total) triple
        [("a", "b"), ("c", "b"), ("c", "a"), ("d", "e")],
        _PC([("a", "b")], [("b", "c"), ("d", "e")]),             # a PCResult: b - c and d - e undirected
    ]
    s = learning.ArcStrength(cols, reps)
    f = s.frame
    assert f[["from", "to"]].values.tolist() == [["a", "b"], ["a", "c"], ["b", "c"], ["d", "e"]]
    assert f["strength"].tolist() == [1.0, 0.5, 1.0, 0.5]
    # a - b: 3 of 4 forward; a - c: never a -> c; b - c: 2 forward + half of the undirected one of 4; d - e: 1 + 0.5 of 2
    assert f["direction"].tolist() == [0.75, 0.0, 0.625, 0.75]
    # descending strength, ties by position: a -> b, b -> c, then c -> a would close a cycle: skipped; d -> e
    assert s.edges(0.5) == [("a", "b"), ("b", "c"), ("d", "e")]
    assert s.edges(0.75) == [("a", "b"), ("b", "c"), "d", "e"]
    assert s.edges(1.01) == cols
    sorobn_amd.BayesNet(*s.edges(0.5))
    # a tie in direction goes to from -> to; an undirected edge alone is such a tie
    t = learning.ArcStrength(["x", "y", "z"], [[("y", "x"), "z"], [("x", "y"), "z"], _PC([], [("y", "z")])])
    assert t.frame["direction"].tolist() == [0.5, 0.5] and t.frame["strength"].tolist() == [2 / 3, 1 / 3]
    assert t.edges(0.3) == [("x", "y"), ("y", "z")]
    assert learning.ArcStrength(["x", "y"], [["x", "y"]]).frame.empty


def test_argument_errors_come_before_any_engine(monkeypatch):
    def no_engine(device=None):
        raise AssertionError("an engine was asked for")

    monkeypatch.setattr(learning, "counting_engine", no_engine)
    X, codes, _ = _frame(50, 1, spec=netspec.grid_spec(2, 2, 2, seed=1))
    n = len(X)
    bad = [np.ones(n - 1), np.ones((n, 1)), np.full(n, -1), np.full(n, 0.5), np.array(["1"] * n), np.full(n, np.nan), np.ones(n, bool),
           np.full(n, 2 ** 32 // n + 1, np.int64), "no such column", 3]
    bn = sorobn_amd.BayesNet(*structure_edges(X))
    for w in bad:
        for call in (lambda: structure.hill_climb(X, weights=w), lambda: structure.pc(X, weights=w),
                     lambda: structure.family_scores(X, [(X.columns[0], [])], weights=w),
                     lambda: structure.ci_tests(X, [(X.columns[0], X.columns[1], [])], weights=w),
                     lambda: bn.fit(X, weights=w), lambda: bn.partial_fit(X, weights=w), lambda: bn.score(X, weights=w)):
            with pytest.raises(ValueError):
                call()
    for kw in ({"n_boot": 0}, {"n_boot": 2.5}, {"learner": "chow_liu"}, {"seed": 0.5}, {"weights": np.ones(n)}, {"bogus": 1},
               {"alpha": 0.1}, {"learner": "pc", "score": "bic"}, {"score": "nope"}, {"max_parents": -1}, {"learner": "pc", "alpha": 2.0},
               {"start": [("no", "such")]}):
        with pytest.raises(ValueError):
            structure.bootstrap(X, **kw)
    holes = X.astype(np.float64)
    holes.iloc[3, 1] = np.nan
    with pytest.raises(ValueError, match="missing values"):
        structure.bootstrap(holes, n_boot=2)


def structure_edges(X):
    cols = list(X.columns)
    return [(cols[0], cols[1]), *cols[2:]]


def test_binding_declares_the_five_symbols():
    five = ["mibn_dataset_set_weights", "mibn_dataset_bootstrap", "mibn_score_families_w", "mibn_ci_tests_w", "mibn_count_tables_w"]
    assert all(s in _capi.SYMBOLS for s in five)
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mibn.h")).read()
    assert all(f"int {s}(" in header for s in five)
    if os.path.exists(_capi.LIB_PATH):
        L = _capi.lib()
        assert all(getattr(L, s).argtypes for s in five)
