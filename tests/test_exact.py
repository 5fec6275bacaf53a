"""Exact structure learning on the GPU: `mibn_best_dag` (csrc/dag_kernel.hip.h under the schedule of csrc/dag_plan.h) against
the numpy twin of tests/dag_check.py bit for bit - under the default passes and under the test-hook options that force multi-pass
schedules at small n -, a known answer at the limit of 24 variables (the only tables above 2^31 bytes), repeatability, the error
paths, and `structure.exact_search` end to end against twin-scored candidates."""
import math
import os

import numpy as np
import pandas as pd
import pytest

import dag_check as dc
import netspec
import structure_check as sc
import sorobn_amd
from sorobn_amd import _capi, learning, structure

pytestmark = pytest.mark.gpu

TOL = 1e-12  # as tests/test_exact_host.py: relative to the sum of the chosen families' |scores|
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DAG_TILE_BITS, DAG_GROUP_BITS = 12, 6  # kDagTileBits / kDagGroupBits of csrc/dag_plan.h: the first pass's bits, a later pass's
WAVE = 64
OPTION_PAIRS = [(3, 2), (3, 3), (1, 1), (2, 5)]  # (dag_tile_bits, dag_group_bits) beside the defaults
SIZES = [1, 2, 3, 5, 8, 9, 13, 16]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(_bits([a[2]]), _bits([b[2]]))


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
def tie_cases():
    """The score sets of the host test with the twin's answer, computed once."""
    out = {}
    for n in SIZES:
        cand = dc.tie_candidates(n, seed=100 + n)
        out[n] = (cand, dc.best_dag(n, *cand))
    return out


def _chain(n):
    """{} at 0 for every child, {v - 1} at 1 for v >= 1, {n - 1} at 0.5 for child 0 - taking it costs a chain edge."""
    children = list(range(n)) + list(range(1, n)) + [0]
    masks = [0] * n + [1 << (v - 1) for v in range(1, n)] + [1 << (n - 1)]
    return children, masks, [0.0] * n + [1.0] * (n - 1) + [0.5]


def _small_dataset(engine):
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 2, (500, 3)).astype(np.uint8)
    return engine.dataset(codes, [2, 2, 2])


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_twin_bit_for_bit(engine, hooked, tie_cases, n):
    # both sides of every boundary of the schedule: n - 1 below, at and above the first pass's bits; fewer entries per child than one
    # wave; under the option pairs a number of later bits that is (n = 8 under (3, 2), n = 13 under (3, 3)) and is not (n = 9
    # under (3, 2)) a multiple of the group
    assert {s - 1 < DAG_TILE_BITS for s in SIZES} == {True, False} and DAG_TILE_BITS + 1 in SIZES and any(s - 1 > DAG_TILE_BITS for s in SIZES)
    assert any(1 << (s - 1) < WAVE for s in SIZES) and any(1 << (s - 1) > WAVE for s in SIZES)
    assert (8 - 1 - 3) % 2 == 0 and (13 - 1 - 3) % 3 == 0 and (9 - 1 - 3) % 2 == 1 and 16 - 1 - DAG_TILE_BITS < DAG_GROUP_BITS
    cand, want = tie_cases[n]
    got = engine.best_dag(n, *cand)
    assert np.array_equal(got[0], want[0]), n
    assert np.array_equal(got[1], want[1]), n
    assert np.array_equal(_bits([got[2]]), _bits([want[2]])), (n, got[2], want[2])
    for e, pair in zip(hooked, OPTION_PAIRS):
        assert _same(e.best_dag(n, *cand), got), (n, pair)


def test_a_full_later_group_of_the_default_schedule(engine, hooked):
    """n = 19: the defaults take 12 + 6 bits, the one size up to 20 whose later bits are a whole group.  The twin needs 3 s here, so
    the yardstick is the device under the option pairs, whose schedules the twin pins at the smaller sizes above."""
    n = DAG_TILE_BITS + DAG_GROUP_BITS + 1
    cand = dc.tie_candidates(n, seed=100 + n)
    got = engine.best_dag(n, *cand)
    assert sorted(got[1].tolist()) == list(range(n))
    for e, pair in zip(hooked, OPTION_PAIRS):
        if pair != (1, 1):  # (one bit per pass at this size is 18 passes of 2-entry tiles: covered at n <= 16)
            assert _same(e.best_dag(n, *cand), got), pair


@pytest.mark.parametrize("n", [17, 24])
def test_known_answer_up_to_the_limit(engine, n):
    """n = 24: the only tables above 2^31 bytes (2.6 GB; 2.0e8 entries and byte offsets up to 1.6e9 in the score array) - the
    64-bit indexing; n = 17 tells a failure of the construction from a failure at the limit."""
    assert n <= _capi.BEST_DAG_MAX_VARS and (n < 24 or 12 * n * 2 ** (n - 1) + 9 * 2 ** n > 2 ** 31)
    parents, order, total = engine.best_dag(n, *_chain(n))
    assert parents.tolist() == [0] + [1 << (v - 1) for v in range(1, n)]
    assert order.tolist() == list(range(n))
    assert total == float(n - 1)


def test_repeatable_in_any_call_and_through_any_handle(engine, tie_cases):
    cand, want = tie_cases[13]
    first = engine.best_dag(13, *cand)
    assert _same(first, want)
    for _ in range(2):
        assert _same(engine.best_dag(13, *cand), first)
    other = _capi.Engine(0)
    try:
        assert _same(other.best_dag(13, *cand), first)
    finally:
        other.close()
    with _small_dataset(engine) as ds:
        ds.score_families([(0,), (0, 1), (0, 1, 2)], "bic")
    assert _same(engine.best_dag(13, *cand), first)


def test_error_paths_leave_the_engine_usable(engine):
    with _small_dataset(engine) as ds:
        fams = [(0,), (0, 1), (0, 1, 2)]
        ok = ds.score_families(fams, "bic")
        nan, inf = float("nan"), float("inf")
        bad = [(0, [], [], [], _capi.E_ARG), (25, [0], [0], [0.0], _capi.E_LIMIT), (3, [3], [0], [0.0], _capi.E_ARG), (3, [-1], [0], [0.0], _capi.E_ARG),
               (3, [1], [2], [0.0], _capi.E_ARG), (3, [0], [8], [0.0], _capi.E_ARG), (3, [0], [0], [nan], _capi.E_ARG), (3, [0], [0], [inf], _capi.E_ARG),
               (3, [0], [0], [-inf], _capi.E_ARG), (3, [0, 1, 0], [6, 0, 6], [0.0, 0.0, 1.0], _capi.E_ARG)]
        for n, ch, ms, ss, code in bad:
            with pytest.raises(_capi.MibnError) as e:
                engine.best_dag(n, ch, ms, ss)
            assert e.value.code == code, (n, ch, ms, ss, e.value)
            assert np.array_equal(_bits(ds.score_families(fams, "bic")), _bits(ok))
        # candidates without a DAG: 0 <- 1 and 1 <- 0 only
        parents, order, total = engine.best_dag(2, [0, 1], [2, 1], [0.0, 0.0])
        assert total == -math.inf and parents.tolist() == [_capi.NO_PARENTS] * 2 and order.tolist() == [-1, -1]
        # a child without any candidate
        parents, _, total = engine.best_dag(3, [0, 1], [0, 1], [0.0, 0.0])
        assert total == -math.inf and parents.tolist() == [_capi.NO_PARENTS] * 3
        assert np.array_equal(_bits(ds.score_families(fams, "bic")), _bits(ok))
    with pytest.raises(ValueError, match="no DAG"):
        structure.best_dag(["a", "b"], [("a", ["b"]), ("b", ["a"])], [0.0, 0.0])
    assert structure.best_dag(["a", "b"], [("a", []), ("b", []), ("b", ["a"])], [0.0, 0.0, 1.0]) == [("a", "b")]


def test_statistics_rows(engine):
    cand = dc.tie_candidates(9, seed=109)
    engine.best_dag(9, *cand)
    rows = {k["name"]: k for k in engine.kernel_stats()}
    assert set(rows) == {"dag_subset_kernel", "dag_sink_kernel"}
    assert rows["dag_subset_kernel"]["launches"] == 3 and rows["dag_sink_kernel"]["launches"] == 9 + 2  # fill, scatter, one pass; levels 0 .. 9, traceback
    assert rows["dag_subset_kernel"]["alg_bytes"] > 0 and rows["dag_subset_kernel"]["items"] == len(cand[0])
    total_before = engine.total_kernel_stats()
    one_bit = _capi.Engine(0)
    try:
        one_bit.set_option("dag_tile_bits", 1)
        one_bit.set_option("dag_group_bits", 1)
        one_bit.best_dag(9, *cand)
        slow = {k["name"]: k for k in one_bit.kernel_stats()}
        assert slow["dag_subset_kernel"]["launches"] == 2 + 8 > rows["dag_subset_kernel"]["launches"]
        assert slow["dag_subset_kernel"]["alg_bytes"] > rows["dag_subset_kernel"]["alg_bytes"]
    finally:
        one_bit.close()
    engine.best_dag(9, *cand)
    assert engine.total_kernel_stats() == total_before, "best_dag books last-call statistics only"


def _example(name):
    return next(n for n in netspec.load(os.path.join(GOLDEN, "examples.json")) if n["spec"]["name"] == name)["spec"]


@pytest.mark.parametrize("name", ["sprinkler", "asia"])
def test_exact_search_end_to_end(engine, name):
    names, raw, _ = sc.forward_sample(_example(name), 2000, seed=3)
    X = pd.DataFrame(raw.astype(np.int64), columns=names)
    cols = [np.unique(raw[:, j], return_inverse=True) for j in range(raw.shape[1])]
    codes = np.stack([np.asarray(inv).reshape(-1) for _, inv in cols], axis=1)
    card = [len(u) for u, _ in cols]
    n = len(names)
    cand = dc.bounded_candidates(n, 3)
    children, masks = [v for v, _ in cand], [pm for _, pm in cand]
    for kind in ("bic", "bdeu"):
        score = sc.scorer(codes, card, kind)
        want_scores = np.array([score(v, [u for u in range(n) if (pm >> u) & 1]) for v, pm in cand])
        want_parents, _, want_total = dc.best_dag(n, children, masks, want_scores)
        result, info = structure.exact_search(X, kind, return_info=True)
        at = dict(zip(cand, want_scores.tolist()))
        bound = TOL * math.fsum(abs(at[(v, int(want_parents[v]))]) for v in range(n))
        print(f"{name} {kind}: dp_total {info['dp_total']!r} twin {want_total!r} fsum {info['total']!r} bound {bound:.3e}")
        assert info["n_families"] == len(cand)
        assert abs(info["dp_total"] - want_total) <= bound and abs(info["total"] - info["dp_total"]) <= bound
        edges = {e for e in result if isinstance(e, tuple)}
        want_edges = {(names[u], names[v]) for v in range(n) for u in range(n) if (int(want_parents[v]) >> u) & 1}
        if n <= 5:  # the same graph only where the twin's runner-up is further away than the bound
            second, _ = dc.all_dags_best(n, children, masks, want_scores, exclude=tuple(int(p) for p in want_parents))
            print(f"  runner-up {second!r}")
            if want_total - second > bound:
                assert edges == want_edges
        pos = {c: j for j, c in enumerate(names)}
        parents = [set() for _ in names]
        for u, v in edges:
            parents[pos[v]].add(pos[u])
        assert not sc.has_cycle(n, parents) and all(len(p) <= 3 for p in parents)
        where = {c: k for k, c in enumerate(info["order"])}
        assert sorted(where) == sorted(names) and all(where[u] < where[v] for u, v in edges)
        _, _, hc_total = structure.hill_climb(X, kind, return_trace=True)
        print(f"  hill_climb {hc_total!r}")
        assert info["total"] >= hc_total - bound
        # all rows twice by weight = the rows written out twice
        _, iw = structure.exact_search(X, kind, weights=np.full(len(X), 2), return_info=True)
        _, i2 = structure.exact_search(pd.concat([X, X], ignore_index=True), kind, return_info=True)
        assert np.array_equal(_bits([iw["dp_total"]]), _bits([i2["dp_total"]]))
    bn = sorobn_amd.BayesNet(*result).fit(X)
    assert set(bn.nodes) == set(names)
