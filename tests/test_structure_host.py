"""Score-based structure learning, host logic (no GPU): `learning.hill_climb` over a numpy test double of
`Dataset.score_families` built on the brute-force twin (tests/structure_check.py).  With the same scorer on both sides the
gains are bit-equal, so the searches must agree exactly."""
import math
import os

import numpy as np
import pandas as pd
import pytest

import netspec
import structure_check as sc
import sorobn_amd
from sorobn_amd import learning, structure

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _example(name):
    return next(n for n in netspec.load(os.path.join(GOLDEN, "examples.json")) if n["spec"]["name"] == name)["spec"]


def _data(spec, n_rows, seed):
    """(frame of integer codes, codes re-encoded over the labels that occur, cards) - what the product will encode."""
    names, raw, _ = sc.forward_sample(spec, n_rows, seed)
    X = pd.DataFrame(raw.astype(np.int64), columns=names)
    cols = [np.unique(raw[:, j], return_inverse=True) for j in range(raw.shape[1])]
    codes = np.stack([np.asarray(inv).reshape(-1) for _, inv in cols], axis=1).astype(np.uint8)
    return X, codes, [len(u) for u, _ in cols]


def _cases():
    """24 seeded data sets: sprinkler, asia and random DAGs, a few hundred to a few thousand rows."""
    out = []
    for seed in range(6):
        out.append((_example("sprinkler"), 300 + 400 * seed, seed))
        out.append((_example("asia"), 500 + 500 * seed, 10 + seed))
    for seed in range(12):
        out.append((netspec.random_dag_spec(100 + seed, n_nodes=4 + seed % 5, p_zero=0.0, p_missing=0.0), 400 + 150 * seed, 20 + seed))
    return out


@pytest.fixture
def twin_engine(monkeypatch):
    eng = sc.TwinEngine()
    monkeypatch.setattr(learning, "counting_engine", lambda device=None: eng)
    return eng


def _split(result):
    edges = {e for e in result if isinstance(e, tuple)}
    return edges, [e for e in result if not isinstance(e, tuple)]


def _assert_dag(columns, edges, max_parents):
    pos = {c: j for j, c in enumerate(columns)}
    parents = [set() for _ in columns]
    for u, v in edges:
        parents[pos[v]].add(pos[u])
    assert not sc.has_cycle(len(columns), parents)
    assert all(len(p) <= max_parents for p in parents)
    return parents


def test_twin_by_hand():
    """Columns A (2 states) and B (2 states), 8 rows: counts A = [5, 3]; B | A: A=0 -> [4, 1], A=1 -> [1, 2]."""
    codes = np.array([[0, 0]] * 4 + [[0, 1]] + [[1, 0]] + [[1, 1]] * 2)
    card = [2, 2]
    ll_a = 5 * math.log(5 / 8) + 3 * math.log(3 / 8)
    ll_b_a = 4 * math.log(4 / 5) + 1 * math.log(1 / 5) + 1 * math.log(1 / 3) + 2 * math.log(2 / 3)
    got, S = sc.family_score(codes, card, 0, [], "loglik")
    assert abs(got - ll_a) <= 1e-14 and abs(S - abs(ll_a)) <= 1e-14
    assert abs(got - (-5.292505905263857)) <= 1e-12
    got, S = sc.family_score(codes, card, 1, [0], "loglik")
    assert abs(got - ll_b_a) <= 1e-14 and abs(S + ll_b_a) <= 1e-14
    assert abs(got - (-4.411554622575379)) <= 1e-12
    assert abs(sc.family_score(codes, card, 1, [0], "bic")[0] - (ll_b_a - 0.5 * math.log(8) * 2 * 1)) <= 1e-14
    assert abs(sc.family_score(codes, card, 1, [0], "aic")[0] - (ll_b_a - 2.0)) <= 1e-14
    assert abs(sc.family_score(codes, card, 0, [], "bic")[0] - (ll_a - 0.5 * math.log(8))) <= 1e-14
    # k2, root A: Gamma(2) / Gamma(2 + 8) * 5! * 3! = 720 / 362880
    assert abs(sc.family_score(codes, card, 0, [], "k2")[0] - math.log(120 * 6 / 362880)) <= 1e-13
    # k2, B | A: [1! / 6! * 4! * 1!] * [1! / 4! * 1! * 2!] = (24 / 720) * (2 / 24)
    assert abs(sc.family_score(codes, card, 1, [0], "k2")[0] - math.log((24 / 720) * (2 / 24))) <= 1e-13
    # bdeu with ess 2 on root A: a/q = 2, a/(q r) = 1: Gamma(2) / Gamma(10) * Gamma(6) / Gamma(1) * Gamma(4) / Gamma(1) - k2's value
    assert abs(sc.family_score(codes, card, 0, [], "bdeu", 2.0)[0] - math.log(120 * 6 / 362880)) <= 1e-13
    # bdeu with ess 4 on B | A: a/q = 2, a/(q r) = 1 -> [Gamma(2)/Gamma(7) 4! 1!] [Gamma(2)/Gamma(5) 1! 2!], k2's value again
    assert abs(sc.family_score(codes, card, 1, [0], "bdeu", 4.0)[0] - math.log((24 / 720) * (2 / 24))) <= 1e-13
    # an empty data set: 0 under loglik / bdeu / k2, the plain penalty otherwise (ln max(N, 1) = 0)
    empty = np.zeros((0, 2), np.int64)
    assert sc.family_score(empty, card, 1, [0], "loglik") == (0.0, 0.0)
    assert sc.family_score(empty, card, 1, [0], "bic")[0] == 0.0
    assert sc.family_score(empty, card, 1, [0], "aic")[0] == -2.0
    assert sc.family_score(empty, card, 1, [0], "bdeu")[0] == 0.0 and sc.family_score(empty, card, 1, [0], "k2")[0] == 0.0
    # the search on it: B depends on A, so one edge is worth adding under loglik; ties go to the lower child: A -> B is (op add,
    # child B), B -> A is (op add, child A) with the SAME loglik gain (mutual information is symmetric) - child A comes first
    score = sc.scorer(codes, card, "loglik")
    best, second = sc.best_move(score, 2, [set(), set()])
    assert best[1:] == ("add", 1, 0) and abs(best[0] - second) <= 1e-12
    assert abs(best[0] - (ll_b_a - ll_a)) <= 1e-12 and abs(best[0] - 0.8809512826884784) <= 1e-9  # B's counts are [5, 3] too
    parents, trace, total, gap = sc.hill_climb(score, 2)
    assert sc.edges_of(parents) == {(1, 0)} and len(trace) == 1 and abs(total - (ll_a + ll_b_a)) <= 1e-12
    # ... and under bic the edge costs 0.5 ln 8 = 1.04 > 0.88: the empty graph stays
    assert sc.hill_climb(sc.scorer(codes, card, "bic"), 2)[1] == []
    assert not sc.is_legal(2, [set(), {0}], "add", 1, 0) and sc.is_legal(2, [set(), {0}], "reverse", 0, 1)
    assert not sc.is_legal(2, [set(), {0}], "delete", 0, 1, required={(0, 1)})
    assert not sc.is_legal(3, [set(), {0}, {1}], "add", 2, 0) and not sc.is_legal(3, [set(), {0}, {0, 1}], "reverse", 0, 2)


@pytest.mark.parametrize("score", ["bic", "bdeu"])
def test_hill_climb_equals_the_twin(twin_engine, score):
    for spec, n_rows, seed in _cases():
        X, codes, card = _data(spec, n_rows, seed)
        cols = list(X.columns)
        result, trace, total = structure.hill_climb(X, score=score, return_trace=True)
        parents, want_trace, want_total, _ = sc.hill_climb(sc.scorer(codes, card, score), len(cols))
        edges, loose = _split(result)
        assert edges == {(cols[u], cols[v]) for u, v in sc.edges_of(parents)}, (spec["name"], seed)
        assert [(op, cols.index(u), cols.index(v), g) for op, u, v, g in trace] == want_trace, (spec["name"], seed)
        assert total == want_total
        assert set(loose) == {c for c in cols if all(c not in e for e in edges)}
        _assert_dag(cols, edges, 3)
        bn = sorobn_amd.BayesNet(*result)
        assert set(bn.nodes) == set(cols)
        assert {(p, c) for c, ps in bn.parents.items() for p in ps} == edges


def test_constraints_start_and_max_iter(twin_engine):
    spec = _example("asia")
    X, codes, card = _data(spec, 3000, 7)
    cols = list(X.columns)
    score = sc.scorer(codes, card, "bic")
    free, _ = _split(structure.hill_climb(X))
    assert free, "the unconstrained search finds edges on 3 000 rows of asia"
    # forbid what the free search found (both directions of its first two edges), require an edge it did not choose
    some = sorted(free)[:2]
    forbidden = [e for u, v in some for e in ((u, v), (v, u))]
    absent = next((u, v) for u in cols for v in cols if u != v and (u, v) not in free and (v, u) not in free and (u, v) not in forbidden)
    for max_parents in (1, 2):
        result, trace, total = structure.hill_climb(X, max_parents=max_parents, required=[absent], forbidden=forbidden, return_trace=True)
        edges, _ = _split(result)
        _assert_dag(cols, edges, max_parents)
        assert absent in edges and not (set(forbidden) & edges)
        ix = lambda es: [(cols.index(u), cols.index(v)) for u, v in es]
        parents, want_trace, want_total, _ = sc.hill_climb(score, len(cols), max_parents=max_parents, required=ix([absent]), forbidden=ix(forbidden))
        assert edges == {(cols[u], cols[v]) for u, v in sc.edges_of(parents)}
        assert [(op, cols.index(u), cols.index(v), g) for op, u, v, g in trace] == want_trace and total == want_total
    # a start shaped like chow_liu's result: a tree of (parent, child) tuples rooted at the first column
    tree = [(cols[(j - 1) // 2], cols[j]) for j in range(1, len(cols))]
    result, trace, total = structure.hill_climb(X, start=tree, return_trace=True)
    parents, want_trace, want_total, _ = sc.hill_climb(score, len(cols), start=[(cols.index(u), cols.index(v)) for u, v in tree])
    assert _split(result)[0] == {(cols[u], cols[v]) for u, v in sc.edges_of(parents)} and total == want_total
    assert [(op, cols.index(u), cols.index(v), g) for op, u, v, g in trace] == want_trace
    assert {t[0] for t in trace} - {"add"}, "from a poor tree the search deletes or reverses"
    tree_total = math.fsum(score(cols.index(v), {cols.index(u) for u, w in tree if w == v}) for v in cols)
    assert total >= tree_total
    # max_iter stops early: the first k moves of the full run
    full = structure.hill_climb(X, return_trace=True)[1]
    assert len(full) > 2
    for k in (0, 1, 2):
        result, trace, _ = structure.hill_climb(X, max_iter=k, return_trace=True)
        assert trace == full[:k] and len(_split(result)[0]) <= k
    assert structure.hill_climb(X, max_iter=0) == cols  # nothing but isolated columns
    assert sorobn_amd.BayesNet(*structure.hill_climb(X, max_iter=0)).nodes == sorted(cols)
    # epsilon: a huge threshold accepts nothing
    assert structure.hill_climb(X, epsilon=1e12) == cols


def test_cache_asks_for_few_families_and_never_twice(twin_engine):
    for spec, n_rows, seed in _cases()[:10] + [(netspec.random_dag_spec(7, n_nodes=12, p_zero=0.0, p_missing=0.0), 1500, 3)]:
        X, _, _ = _data(spec, n_rows, seed)
        n = X.shape[1]
        twin_engine.calls.clear()
        _, trace, _ = structure.hill_climb(X, return_trace=True)
        calls = twin_engine.calls
        assert len(calls[0]) == n + n * (n - 1)  # every column alone and with every single parent
        assert len(calls) <= 1 + len(trace)
        assert all(len(c) <= 4 * n for c in calls[1:])
        asked = [(f[-1], frozenset(f[:-1])) for c in calls for f in c]
        assert len(asked) == len(set(asked)), "a family was requested twice"
        assert all(list(f[:-1]) == sorted(f[:-1]) for c in calls for f in c)  # parents in column order, child last


def test_family_scores_and_net_score_through_the_double(twin_engine):
    X, codes, card = _data(_example("asia"), 800, 1)
    cols = list(X.columns)
    fams = [(cols[3], []), (cols[0], [cols[5], cols[2]]), (cols[7], cols[1])]
    got = structure.family_scores(X, fams, score="k2")
    # family_scores encodes only the columns it needs, in X's column order
    want = [sc.family_score(codes, card, 3, [], "k2")[0], sc.family_score(codes, card, 0, [2, 5], "k2")[0], sc.family_score(codes, card, 7, [1], "k2")[0]]
    assert got.tolist() == want
    bn = netspec.build(_example("asia"), sorobn_amd.BayesNet)
    want = math.fsum(sc.family_score(codes, card, cols.index(v), sorted(cols.index(p) for p in bn.parents.get(v, [])), "bdeu", 3.0)[0] for v in bn.nodes)
    assert bn.score(X, "bdeu", ess=3.0) == want
    assert len(structure.family_scores(X, [])) == 0


def test_argument_errors_before_any_engine(monkeypatch):
    def no_engine(device=None):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(learning, "counting_engine", no_engine)
    X = pd.DataFrame({"a": [0, 1, 0, 1], "b": [0, 0, 1, 1], "c": [1, 1, 0, 1]})
    bad = [
        dict(score="mdl"),
        dict(ess=0.0),
        dict(ess=-1.0),
        dict(score="bdeu", ess=float("nan")),
        dict(start=[("a", "b"), ("b", "c"), ("c", "a")]),
        dict(start=[("a", "b")], required=[("b", "a")]),
        dict(required=[("a", "b")], forbidden=[("a", "b")]),
        dict(start=[("a", "b")], forbidden=[("a", "b")]),
        dict(start=[("a", "zz")]),
        dict(required=[("zz", "a")]),
        dict(forbidden=[("a", "zz")]),
        dict(start=[("a", "a")]),
        dict(start=["a"]),
        dict(start=[("a", "c"), ("b", "c")], max_parents=1),
        dict(max_parents=-1),
        dict(max_iter=-1),
        dict(epsilon=-1.0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            structure.hill_climb(X, **kw)
    # missing values: the column is named and fit_em pointed to
    for hole in (np.nan, None):
        Y = pd.DataFrame({"a": [0, 1, 0, 1], "b": ["x", hole, "y", "x"]})
        with pytest.raises(ValueError, match=r"'b'.*fit_em"):
            structure.hill_climb(Y)
        with pytest.raises(ValueError, match=r"'b'.*fit_em"):
            structure.family_scores(Y, [("a", ["b"])])
        with pytest.raises(ValueError, match=r"'b'.*fit_em"):
            sorobn_amd.BayesNet(("a", "b")).score(Y)
    # more than 256 labels keeps encode_columns' error
    Z = pd.DataFrame({"a": np.arange(300), "b": np.arange(300) % 2})
    with pytest.raises(ValueError, match="distinct labels"):
        structure.hill_climb(Z)
    for kw in (dict(score="mdl"), dict(ess=0.0)):
        with pytest.raises(ValueError):
            structure.family_scores(X, [("a", ["b"])], **kw)
    for fams in ([("a", ["zz"])], [("zz", [])], [("a", ["a"])], [("a", ["b", "b"])]):
        with pytest.raises(ValueError):
            structure.family_scores(X, fams)


def test_binding_declares_the_symbols():
    from sorobn_amd import _capi
    assert {"mibn_dataset_create", "mibn_dataset_destroy", "mibn_score_families"} <= set(_capi.SYMBOLS)
    assert _capi.SCORE_KINDS == {"loglik": 0, "bic": 1, "aic": 2, "bdeu": 3, "k2": 4}
    assert hasattr(_capi.Engine, "dataset") and hasattr(_capi.Dataset, "score_families")
