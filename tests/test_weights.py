"""Integer row weights on the GPU: `mibn_count_tables_w`, `mibn_dataset_set_weights` / `mibn_dataset_bootstrap`,
`mibn_score_families_w` / `mibn_ci_tests_w` (count_weighted_kernel, count_big_weighted_kernel, bootstrap_weights_kernel) and the
Python surface on top (`weights=`, `structure.bootstrap`).

Every comparison is EXACT: counts are integers, and a weighted call is bit for bit the unweighted call on the rows written out
w[i] times each - the reduction kernels are the same and read the same counts - so there is no tolerance anywhere in this file.
On the parent commit the five symbols do not exist: every test here fails there."""
import itertools

import numpy as np
import pandas as pd
import pytest

import netspec
import structure_check as sc
import weights_check as wc
import sorobn_amd
from sorobn_amd import _capi, learning, structure

pytestmark = pytest.mark.gpu

TOP = 2 ** 32 - 1
# a column of cardinality 1, small ones, 17 x 17 x 8 = 2 312-cell triples (nine of them straddle a 16 384-cell LDS group) and two
# 200-label columns (200 x 200 = 40 000 cells: the global-atomic path)
CARD = [1, 2, 3, 4, 17, 17, 8, 200, 200, 5]
NINE = [p for p in itertools.permutations((4, 5, 6))] + [(4, 5, 3, 1), (5, 4, 3, 1), (6, 4, 5)]
TABLES = [(0,), (1,), (0, 1), (9, 0, 2), (3, 2, 1), *NINE, (7, 8), (8, 7), (2,), (6, 9), (6, 9)]  # (the last two: one scope twice in a row)


def _codes(n_rows, card=CARD, seed=0):
    rng = np.random.default_rng(seed + n_rows)
    return np.stack([rng.integers(0, c, n_rows) for c in card], axis=1).astype(np.uint8).reshape(n_rows, len(card))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _row(eng, name):
    return next((k for k in eng.kernel_stats() if k["name"] == name), None)


@pytest.fixture(scope="module")
def engine():
    assert _capi.device_count() > 0, "no HIP device visible"
    return learning.counting_engine()


# ------------------------------------------------------------------------------------------------------------ counts
@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257, 1000])
def test_weighted_counts_against_numpy(engine, n_rows):
    assert len(NINE) == 9 and all(np.prod([CARD[c] for c in t]) == 2312 for t in NINE) and 7 * 2312 < 16384 < 8 * 2312
    codes = _codes(n_rows)
    rng = np.random.default_rng(n_rows)
    vectors = [rng.integers(0, 4, n_rows), np.zeros(n_rows, np.int64), np.ones(n_rows, np.int64)]
    if n_rows:
        lone = np.zeros(n_rows, np.int64)
        lone[n_rows // 2] = TOP  # one row carries 2^32 - 1, the rest nothing
        vectors.append(lone)
        assert n_rows == 1 or (vectors[0] == 0).any()
    for w in vectors:
        for layout in (codes, np.asfortranarray(codes)):
            got = engine.count_tables(layout, CARD, TABLES, weights=w)
            for t, g in zip(TABLES, got):
                assert g.dtype == np.int64 and np.array_equal(g, wc.weighted_table(codes, CARD, t, w)), (n_rows, t)
    assert all(np.array_equal(a, b) for a, b in zip(engine.count_tables(codes, CARD, TABLES, weights=vectors[2]), engine.count_tables(codes, CARD, TABLES)))


def test_weighted_counts_at_the_edge_of_32_bits(engine):
    same = np.array([[0, 1, 2, 3, 16, 16, 7, 199, 199, 4]] * 3, np.uint8)  # three rows in one cell of every table
    w = np.array([2 ** 31, 2 ** 31 - 1, 0], np.int64)
    for t, g in zip(TABLES, engine.count_tables(same, CARD, TABLES, weights=w)):
        assert int(g.sum()) == TOP and int(g.max()) == TOP and np.array_equal(g, wc.weighted_table(same, CARD, t, w)), t
    with pytest.raises(_capi.MibnError) as e:  # W = 2^32
        engine.count_tables(same, CARD, TABLES, weights=np.array([2 ** 31, 2 ** 31 - 1, 1], np.int64))
    assert e.value.code == _capi.E_LIMIT
    assert int(engine.count_tables(same, CARD, [(1,)])[0].sum()) == 3  # the engine still answers


# ------------------------------------------------------------------------------------------------------ bit identity
CARD6 = [2, 3, 4, 3, 2, 5]
FAMS = [(0,), (5,), (0, 1), (1, 0), (2, 3, 4), (0, 1, 2, 5), (5, 4, 3, 2), (1, 2, 3, 4, 5, 0)]
CI = [(0, 1), (4, 5), (2, 0, 1), (0, 1, 2, 3), (5, 3, 1, 0, 2), (1, 2, 3, 4, 5, 0)]
OTHERS = [p for k in (2, 3, 4) for p in itertools.permutations(range(6), k)][:300]


@pytest.fixture(scope="module")
def six(engine):
    """6 columns x 1 000 rows resident with two weight sets - all 2s, and random 0 .. 3 - beside the rows written out."""
    codes = _codes(1000, CARD6, seed=1)
    sets = np.stack([np.full(1000, 2), np.random.default_rng(2).integers(0, 4, 1000)]).astype(np.uint32)
    assert (sets[1] == 0).any()
    cut = _capi.Engine(0)
    ds = engine.dataset(codes, CARD6)
    ds.set_weights(sets)
    out = {"ds": ds, "cut": cut, "cut_ds": cut.dataset(codes, CARD6), "sets": sets,
           "plain": [engine.dataset(codes, CARD6), engine.dataset(np.concatenate([codes, codes]), CARD6), engine.dataset(wc.expand(codes, sets[1]), CARD6)]}
    out["cut_ds"].set_weights(sets)
    yield out
    for d in [ds, out["cut_ds"], *out["plain"]]:
        d.close()
    cut.close()


def _sub_batches(cells, budget):
    """How many sub-batches the engine cuts: consecutive tables while they fit the budget, a larger one alone."""
    n = run = 0
    for c in cells:
        if n == 0 or run + c > budget:
            n, run = n + 1, 0
        run += c
    return n


def _check_identity(six, tables, call, want_of, count_row):
    """`call(ds, tables, wset)` -> tuple of arrays; want_of(plain ds, tables) the unweighted answer on the written-out rows."""
    ds, cut, cut_ds = six["ds"], six["cut"], six["cut_ds"]
    want = {s: want_of(six["plain"][s + 1], tables) for s in (-1, 0, 1)}

    def same(got, sets):
        for k, s in enumerate(sets):
            assert all(_bits(g[k:k + 1]).tolist() == _bits(w[k:k + 1]).tolist() for g, w in zip(got, want[s])), (tables[k], s)

    for s in (-1, 0, 1):  # a set at a time: the whole list in one call, and one table per call
        same(call(ds, tables, [s] * len(tables)), [s] * len(tables))
        for k in (0, len(tables) - 1):
            got = call(ds, [tables[k]], [s])
            assert all(_bits(g).tolist() == _bits(w[k:k + 1]).tolist() for g, w in zip(got, want[s]))
    mixed = [(-1, 0, 1)[(k + k // 3) % 3] for k in range(len(tables))]  # tables of one LDS group under sets 0, 1 and -1
    same(call(ds, tables, mixed), mixed)
    # among 300 other tables
    rng = np.random.default_rng(0)
    pad = [tuple(t) for t in OTHERS]
    got = call(ds, pad[:100] + tables[:3] + pad[100:] + tables[3:], rng.integers(-1, 2, 100).tolist() + mixed[:3] + rng.integers(-1, 2, 200).tolist() + mixed[3:])
    same(tuple(np.concatenate([g[100:103], g[303:]]) for g in got), mixed)
    # three sub-batches
    cells = [int(np.prod([CARD6[c] for c in t])) for t in tables]
    cut.set_option("score_cells", next(b for b in range(1, sum(cells) + 1) if _sub_batches(cells, b) == 3))
    same(call(cut_ds, tables, mixed), mixed)
    assert _row(cut, "count_weighted_kernel")["launches"] == 3 and _row(cut, "count_kernel") is None
    assert _row(cut, count_row)["launches"] >= 3
    st = _row(cut, "count_weighted_kernel")
    assert st["alg_bytes"] == 1000 * sum(len(t) for t in tables) + 4 * 1000 * len(tables) + 8 * sum(cells) and st["items"] == len(tables)


@pytest.mark.parametrize("kind", ["loglik", "bic", "aic", "bdeu", "k2"])
def test_weighted_scores_are_the_scores_of_the_written_out_rows(six, kind):
    _check_identity(six, FAMS, lambda ds, t, w: (ds.score_families(t, kind, 1.5, wset=w),), lambda ds, t: (ds.score_families(t, kind, 1.5),), "score_kernel")


@pytest.mark.parametrize("kind", ["g2", "x2"])
def test_weighted_ci_tests_are_the_tests_of_the_written_out_rows(six, kind):
    _check_identity(six, CI, lambda ds, t, w: ds.ci_tests(t, kind, wset=w), lambda ds, t: ds.ci_tests(t, kind), "citest_kernel")


def test_share_scope_option_changes_no_bit(six, engine):
    tables = sorted(FAMS * 3)
    wset = [(-1, 0, 1)[k % 3] for k in range(len(tables))]
    want = six["ds"].score_families(tables, "bic", wset=wset)
    six["cut"].set_option("score_cells", 1 << 22)
    for share in (0, 1):
        six["cut"].set_option("weighted_share", share)
        assert np.array_equal(_bits(six["cut_ds"].score_families(tables, "bic", wset=wset)), _bits(want))


# --------------------------------------------------------------------------------------------------------- bootstrap
@pytest.mark.parametrize("n_rows", [1, 257, 1000])
def test_device_bootstrap_sets_equal_the_twin(engine, n_rows):
    with engine.dataset(_codes(n_rows, CARD6), CARD6) as ds:
        three = ds.bootstrap(3, seed=2 ** 40 + 9, return_weights=True)
        assert three.dtype == np.uint32 and np.array_equal(three, wc.bootstrap_sets(n_rows, 3, 2 ** 40 + 9))
        assert (three.sum(axis=1) == n_rows).all()
        two = ds.bootstrap(2, seed=2 ** 40 + 9, return_weights=True)
        assert np.array_equal(two, three[:2])  # set s is a function of (seed, s, n_rows), not of n_sets
        assert ds.bootstrap(2, seed=5) is None
        # the sets drawn last are the ones in use: loglik of a root under set 1 is that of the twin's set
        w = wc.bootstrap_sets(n_rows, 2, 5)[1]
        t = wc.weighted_table(_codes(n_rows, CARD6), CARD6, (5,), w).astype(np.float64)
        nz = t[t > 0]
        assert abs(float(ds.score_families([(5,)], "loglik", wset=[1])[0]) - float((nz * np.log(nz / n_rows)).sum())) <= 1e-9 * n_rows


@pytest.fixture(scope="module")
def grid_frame():
    spec = netspec.grid_spec(2, 3, 3)
    names, codes, card = sc.forward_sample(spec, 500, 1)
    assert codes.shape == (500, 6) and all(len(np.unique(codes[:, j])) == card[j] for j in range(6))
    true = {frozenset((p, nm)) for nm in names for p in spec["cpts"][nm]["names"][:-1]}
    return pd.DataFrame(codes.astype(np.int64), columns=names), true


def _pc_tuple(r):
    return r.directed, r.undirected, r.sepsets, r.tests_per_level, r.trace


@pytest.mark.parametrize("learner", ["hill_climb", "pc"])
def test_bootstrap_replicates_are_the_learner_under_the_downloaded_sets(engine, grid_frame, learner):
    X, true = grid_frame
    strength, reps = structure.bootstrap(X, n_boot=4, learner=learner, seed=3, return_replicates=True, return_trace=True)
    with engine.dataset(learning.encode_complete(X, list(X.columns))[0], [3] * 6) as ds:
        sets = ds.bootstrap(4, seed=3, return_weights=True)
    assert np.array_equal(sets, wc.bootstrap_sets(500, 4, 3))
    for rep, w in zip(reps, sets):
        if learner == "hill_climb":
            assert rep == structure.hill_climb(X, weights=w, return_trace=True)
        else:
            assert _pc_tuple(rep) == _pc_tuple(structure.pc(X, weights=w, return_trace=True))
    again = structure.bootstrap(X, n_boot=4, learner=learner, seed=3)
    pd.testing.assert_frame_equal(strength.frame, again.frame, check_exact=True)
    edges = strength.edges()
    bn = sorobn_amd.BayesNet(*edges)  # accepted, hence acyclic: checked again by hand
    cols = list(X.columns)
    parents = [set() for _ in cols]
    for e in edges:
        if isinstance(e, tuple):
            parents[cols.index(e[1])].add(cols.index(e[0]))
    assert not sc.has_cycle(6, parents) and set(bn.nodes) == set(cols)
    f = strength.frame
    hit = [frozenset(p) in true for p in zip(f["from"], f["to"])]
    # printed, not asserted: on random-CPT grids recovery is not a property of the method
    print(f"\n[weights] {learner}, 4 replicates of 500 rows: strengths of the generating edges {f['strength'][hit].tolist()} "
          f"({len(true) - sum(hit)} of {len(true)} never seen), of non-adjacent pairs {f['strength'][[not h for h in hit]].tolist()}")


# ------------------------------------------------------------------------------------------------------------ python
def test_python_calls_with_weights_equal_the_expanded_frame(engine, grid_frame):
    X, _ = grid_frame
    codes = X.to_numpy()
    w = np.random.default_rng(4).integers(0, 4, len(X))
    for j in range(6):  # every label of every column survives the expansion (else the cardinalities, and so BIC, differ)
        for lab in range(3):
            w[np.flatnonzero(codes[:, j] == lab)[0]] = 2
    assert (w == 0).any()
    Xe = X.iloc[np.repeat(np.arange(len(X)), w)].reset_index(drop=True)
    got = structure.hill_climb(X, weights=w, return_trace=True)
    assert got == structure.hill_climb(Xe, return_trace=True) and got[1]
    assert _pc_tuple(structure.pc(X, weights=w, return_trace=True)) == _pc_tuple(structure.pc(Xe, return_trace=True))
    a, b = sorobn_amd.BayesNet(*got[0]).fit(X, weights=w), sorobn_amd.BayesNet(*got[0]).fit(Xe)
    for node in b.P:
        pd.testing.assert_series_equal(a.P[node], b.P[node], check_exact=True)
    assert a.score(X, weights=w) == b.score(Xe)
    agg = X.value_counts(sort=False).rename("count").reset_index()
    c = sorobn_amd.BayesNet(*got[0]).fit(agg, weights="count")
    d = sorobn_amd.BayesNet(*got[0]).fit(X)
    for node in d.P:
        pd.testing.assert_series_equal(c.P[node], d.P[node], check_exact=True)


# ------------------------------------------------------------------------------------------------------- error paths
def test_error_paths_leave_the_engine_answering(engine):
    codes = _codes(300, CARD6, seed=7)
    with engine.dataset(codes, CARD6) as ds:
        want = ds.score_families(FAMS, "bic")

        def still_answers():
            assert np.array_equal(_bits(ds.score_families(FAMS, "bic")), _bits(want))

        def refused(code, call):
            with pytest.raises(_capi.MibnError) as e:
                call()
            assert e.value.code == code, e.value
            still_answers()

        refused(_capi.E_ARG, lambda: ds.score_families(FAMS, "bic", wset=[0] * len(FAMS)))  # no sets yet
        ds.set_weights(np.ones((2, 300), np.uint32))
        for bad in (2, -2, 1 << 20):
            refused(_capi.E_ARG, lambda: ds.score_families(FAMS, "bic", wset=[0] * (len(FAMS) - 1) + [bad]))
            refused(_capi.E_ARG, lambda: ds.ci_tests(CI, "g2", wset=[bad] + [1] * (len(CI) - 1)))
        refused(_capi.E_ARG, lambda: ds.score_families([(0, 0)], "bic", wset=[0]))
        refused(_capi.E_ARG, lambda: ds.score_families([(0, 9)], "bic", wset=[-1]))
        over = np.zeros((2, 300), np.uint32)
        over[1, :2] = 2 ** 31
        refused(_capi.E_LIMIT, lambda: ds.set_weights(over))  # W_1 = 2^32
        assert np.array_equal(_bits(ds.score_families(FAMS, "bic", wset=[1] * len(FAMS))), _bits(want))  # ... and the old sets stay
        over[1, 1] = 2 ** 31 - 1
        ds.set_weights(over)  # W_1 = 2^32 - 1: accepted, counted exactly ...
        t = wc.weighted_table(codes, CARD6, (0,), over[1]).astype(np.float64)
        assert int(t.sum()) == TOP
        ll = float(sum(n * np.log(n / TOP) for n in t.tolist() if n))
        assert abs(float(ds.score_families([(0,)], "loglik", wset=[1])[0]) - ll) <= 1e-12 * abs(ll) + 1e-300
        refused(_capi.E_LIMIT, lambda: ds.ci_tests(CI, "g2", wset=[1] * len(CI)))  # ... but 2^31 or more is too much for the CI products
        ds.set_weights(None)
        refused(_capi.E_ARG, lambda: ds.ci_tests(CI, "x2", wset=[0] * len(CI)))
        assert np.array_equal(_bits(ds.score_families(FAMS, "bic", wset=[-1] * len(FAMS))), _bits(want))
        assert len(ds.score_families([], "bic", wset=[])) == 0
    gone = engine.dataset(codes, CARD6)
    gone.close()
    for call in (lambda: gone.set_weights(np.ones((1, 300), np.uint32)), lambda: gone.bootstrap(2)):
        with pytest.raises(_capi.MibnError) as e:
            call()
        assert e.value.code == _capi.E_ARG
    with engine.dataset(codes, CARD6) as ds:
        assert np.array_equal(_bits(ds.score_families(FAMS, "bic")), _bits(want))
