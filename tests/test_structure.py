"""Score-based structure learning on the GPU: `mibn_score_families` (count_kernel + score_kernel over a resident data set)
and `hill_climb` on top of it, against the brute-force twin of tests/structure_check.py (the reference has no such search).

Tolerance of a family score: |got - want| <= TOL * max(S, 1) with S = fsum(|term|) over the twin's terms.  TOL = 1e-12 (the
project's parity tolerance, 1e-9, is the ceiling).  Where it comes from: every term is a product / difference of device `log` or
`lgamma` values, each within a few ulp (2^-52 = 2.2e-16) of the twin's libm value relative to the term's own magnitude or to the
magnitude of the two values it is the difference of - both are part of S for the rows drawn here (no column is close to
deterministic, so |ln N_jk - ln N_j| is not small against ln N_j) - and a lane adds at most 64 configurations before the six
steps of the butterfly, the chunked form another 4 + 64 + 6 values: about a hundred roundings of at most 1.1e-16 * S each.  Both
together stay near 1e-14 * S; 1e-12 leaves two orders of magnitude.  The largest ratio observed is printed by the test."""
import itertools
import math
import os

import numpy as np
import pandas as pd
import pytest

import netspec
import structure_check as sc
import sorobn_amd
from sorobn_amd import _capi, learning, structure

pytestmark = pytest.mark.gpu

TOL = 1e-12
SCORE_WAVE_CELLS = 4096  # kScoreWaveCells of csrc/score_kernel.hip.h: larger tables take the chunked form
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("loglik", "bic", "aic", "bdeu", "k2")
# columns of the scoring data: cardinalities 1, 2, 3, 4, 17 and 100, some of them dependent on an earlier column
CARD = [1, 2, 2, 3, 3, 4, 4, 4, 4, 17, 17, 17, 17, 17, 100, 100, 2, 4]
# (child, parents): 0 to 5 parents
FAMILIES = [
    (0, []), (1, []), (3, []), (5, []), (9, []), (14, []),            # roots of every cardinality
    (1, [0]), (0, [1]), (2, [1]), (16, [1]), (17, [5]), (5, [17]),     # one parent (16 and 17 depend on 1 and 5)
    (6, [5, 3]), (9, [1, 3]), (14, [2, 5]), (3, [14]), (1, [14, 15]),   # 100-state columns as child and as parents
    (7, [5, 6, 8]), (4, [1, 2, 3, 5]), (8, [1, 2, 3, 5, 6]),           # three to five parents
    (10, [9, 11]),                                                   # 17^3 = 4 913 cells: above the one-wave limit, LDS-counted
    (5, [14, 15]),                                                   # 100 * 100 * 4 = 40 000 cells: the count_big path
    (12, [9, 10, 11]),                                               # 17^4 = 83 521 cells
]
HUGE = (6, [9, 10, 11, 12, 13])  # 17^5 * 4 = 5 679 428 cells: a sub-batch of its own, 1 387 chunks


def _codes(n_rows, seed=0):
    rng = np.random.default_rng(seed)
    cols = [rng.integers(0, c, n_rows) for c in CARD]
    cols[16] = (cols[1] + (rng.random(n_rows) < 0.2)) % 2
    cols[17] = (cols[5] + rng.integers(0, 2, n_rows)) % 4
    cols[6] = (cols[5] + cols[3] + (rng.random(n_rows) < 0.3)) % 4
    return np.stack(cols, axis=1).astype(np.uint8)


def _fam_cols(families):
    return [tuple(sorted(ps)) + (c,) for c, ps in families]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _example(name):
    return next(n for n in netspec.load(os.path.join(GOLDEN, "examples.json")) if n["spec"]["name"] == name)["spec"]


@pytest.fixture(scope="module")
def engine():
    assert _capi.device_count() > 0, "no HIP device visible"
    return learning.counting_engine()


def test_family_scores_against_the_twin(engine):
    assert SCORE_WAVE_CELLS < 17 ** 3 <= 16384 < 40000
    worst = (0.0, None)
    small_budget = _capi.Engine(0)
    small_budget.set_option("score_cells", 3000)  # several sub-batches; every family above 3 000 cells goes alone
    try:
        for n_rows in (1, 7, 1000, 200_000):
            codes = _codes(n_rows, seed=n_rows)
            fams = FAMILIES + ([HUGE] if n_rows in (1000, 200_000) else [])
            with engine.dataset(codes, CARD) as row_major, engine.dataset(np.asfortranarray(codes), CARD) as col_major, \
                    small_budget.dataset(codes, CARD) as cut:
                for kind in KINDS:
                    ess = 2.5 if kind == "bdeu" else 1.0
                    got = row_major.score_families(_fam_cols(fams), kind, ess)
                    assert np.array_equal(_bits(got), _bits(col_major.score_families(_fam_cols(fams), kind, ess))), (n_rows, kind)
                    assert np.array_equal(_bits(got), _bits(cut.score_families(_fam_cols(fams), kind, ess))), (n_rows, kind)
                    if kind == "bic":
                        assert small_budget.kernel_stats()[0]["launches"] > 2, "the small budget did not cut the call"
                    for (child, parents), g in zip(fams, got):
                        if (child, parents) == HUGE and kind not in ("bic", "bdeu"):
                            continue  # (the twin walks 1.4 M configurations in Python: two kinds of it are enough)
                        want, S = sc.family_score(codes, CARD, child, sorted(parents), kind, ess)
                        ratio = abs(float(g) - want) / max(S, 1.0)
                        if ratio > worst[0]:
                            worst = (ratio, (n_rows, kind, child, parents, float(g), want, S))
                        assert ratio <= TOL, (n_rows, kind, child, parents, float(g), want, S, ratio)
    finally:
        small_budget.close()
    print(f"\n[structure] family scores vs twin: largest |got - want| / max(S, 1) = {worst[0]:.3e} at {worst[1]}")


def test_empty_data_set_and_single_rows(engine):
    empty = np.zeros((0, 3), np.uint8)
    card = [2, 3, 4]
    with engine.dataset(empty, card) as ds:
        fams = [(2,), (0, 1, 2), (1, 0)]
        assert ds.score_families(fams, "loglik").tolist() == [0.0, 0.0, 0.0]
        assert ds.score_families(fams, "bic").tolist() == [0.0, 0.0, 0.0]
        assert ds.score_families(fams, "aic").tolist() == [-3.0, -18.0, -3.0]
        assert ds.score_families(fams, "bdeu").tolist() == [0.0, 0.0, 0.0]
        assert ds.score_families(fams, "k2").tolist() == [0.0, 0.0, 0.0]
        assert len(ds.score_families([], "bic")) == 0
    with engine.dataset(np.array([[1, 2, 3]], np.uint8), card) as ds:  # one row: every family is one cell of count 1
        assert ds.score_families([(2,), (0, 1, 2)], "loglik").tolist() == [0.0, 0.0]
        assert ds.score_families([(2,), (0, 1, 2)], "k2").tolist() == pytest.approx([math.lgamma(4) - math.lgamma(5)] * 2, abs=1e-14)


def test_bit_for_bit_repeatability(engine):
    codes = _codes(50_000, seed=5)
    fams = _fam_cols(FAMILIES)
    rng = np.random.default_rng(1)
    lone = _capi.Engine(0)
    lone.set_option("threads", 1)
    try:
        with engine.dataset(codes, CARD) as a, engine.dataset(codes.copy(), CARD) as b, lone.dataset(codes, CARD) as c:
            for kind in ("bic", "bdeu", "k2"):
                first = a.score_families(fams, kind, 1.5)
                for _ in range(2):
                    assert np.array_equal(_bits(first), _bits(a.score_families(fams, kind, 1.5)))
                perm = rng.permutation(len(fams))
                shuffled = a.score_families([fams[i] for i in perm], kind, 1.5)
                assert np.array_equal(_bits(first[perm]), _bits(shuffled))
                extra = [(i, j) for i, j in itertools.permutations(range(len(CARD)), 2)]
                mixed = extra[:100] + fams[:7] + extra[100:] + fams[7:]
                got = a.score_families(mixed, kind, 1.5)
                assert np.array_equal(_bits(first), _bits(np.concatenate([got[100:107], got[len(extra) + 7:]])))
                for f, s in zip(fams, first):  # ... and one at a time
                    if len(f) in (1, 3, 4):
                        assert _bits(a.score_families([f], kind, 1.5))[0] == _bits(s)
                assert np.array_equal(_bits(first), _bits(b.score_families(fams, kind, 1.5))), "second handle of the same rows"
                assert np.array_equal(_bits(first), _bits(c.score_families(fams, kind, 1.5))), "threads = 1 engine"
    finally:
        lone.close()


@pytest.mark.parametrize("kind", ["bic", "bdeu"])
def test_score_equivalence(engine, kind):
    """score(u) + score(v | u) == score(v) + score(u | v): both orientations of one edge describe the same distributions."""
    codes = _codes(30_000, seed=9)
    rng = np.random.default_rng(2)
    pairs = [tuple(rng.choice(len(CARD), 2, replace=False).tolist()) for _ in range(50)]
    worst = 0.0
    with engine.dataset(codes, CARD) as ds:
        got = ds.score_families([f for u, v in pairs for f in ((u,), (u, v), (v,), (v, u))], kind, 3.0).reshape(-1, 4)
    for (u, v), (s_u, s_vu, s_v, s_uv) in zip(pairs, got):
        S = math.fsum(sc.family_score(codes, CARD, c, ps, kind, 3.0)[1] for c, ps in ((u, []), (v, [u]), (v, []), (u, [v])))
        ratio = abs((s_u + s_vu) - (s_v + s_uv)) / max(S, 1.0)
        worst = max(worst, ratio)
        assert ratio <= TOL, (u, v, s_u, s_vu, s_v, s_uv, S)
    print(f"\n[structure] score equivalence ({kind}): largest |lhs - rhs| / max(S, 1) = {worst:.3e}")


@pytest.mark.parametrize("name", ["asia", "alarm"])
def test_loglik_score_is_the_fitted_log_likelihood(name):
    spec = _example(name)
    bn = netspec.build(spec, sorobn_amd.BayesNet)
    bn.seed = 11
    X = bn.sample(20_000)
    if name == "alarm":
        # both roots true has probability 2e-6.  A parent configuration that never occurs leaves a row out of the fitted CPT, the
        # joint then has mass below 1 and log_likelihood renormalises it - a different quantity.  Rows sampled with the roots
        # forced make every configuration of Alarm's parents occur.
        forced = [bn.sample(2000, init={"Burglary": b, "Earthquake": e}) for b in (False, True) for e in (False, True)]
        X = pd.concat([X, *forced], ignore_index=True)
    for v, ps in bn.parents.items():  # precondition of the comparison: every parent configuration occurs
        assert X.groupby(list(ps)).ngroups == int(np.prod([X[p].nunique() for p in ps])), (v, ps)
    fitted = netspec.build(spec, sorobn_amd.BayesNet).fit(X)
    want = fitted.log_likelihood(X)
    got = fitted.score(X, "loglik")
    assert math.isfinite(want) and abs(got - want) <= 1e-9 * abs(want), (got, want)
    n_par = sum(int(np.prod([X[p].nunique() for p in bn.parents.get(v, [])])) * (X[v].nunique() - 1) for v in bn.nodes)
    assert abs(fitted.score(X, "bic") - (got - 0.5 * math.log(len(X)) * n_par)) <= 1e-9 * abs(want)
    assert abs(fitted.score(X, "aic") - (got - n_par)) <= 1e-9 * abs(want)


# ------------------------------------------------------------------------------------------------------------ search
SEARCH_ROWS = 20_000
# sampling seeds (BayesNet.seed before bn.sample): the exact comparison below needs the twin's run on the sampled rows to have no
# two best gains closer than 1e-6 at any step; DESIGN.md section 13 lists the seeds tried
SEEDS = {"sprinkler": 1, "asia": 1, "alarm": 1, "dag31": 1, "dag32": 1}


def _search_spec(name):
    if name == "dag31":
        return netspec.random_dag_spec(31, n_nodes=8, p_zero=0.0, p_missing=0.0)
    if name == "dag32":
        return netspec.random_dag_spec(32, n_nodes=10, p_zero=0.0, p_missing=0.0)
    return _example(name)


def _rows(name):
    bn = netspec.build(_search_spec(name), sorobn_amd.BayesNet)
    bn.seed = SEEDS[name]
    X = bn.sample(SEARCH_ROWS)
    codes, _, card = learning.encode_complete(X, list(X.columns))
    return X, np.ascontiguousarray(codes), card


class _TrackingScore:
    """The twin's scorer, remembering the largest S it saw per child: S_total is their sum."""

    def __init__(self, codes, card, kind):
        self.codes, self.card, self.kind, self.S = codes, card, kind, {}

    def __call__(self, child, parents):
        s, S = sc.family_score(self.codes, self.card, child, sorted(parents), self.kind)
        self.S[child] = max(self.S.get(child, 1.0), S)
        return s

    def total(self):
        return math.fsum(self.S.values())


def _replay(X, codes, card, result, trace, total, start=(), epsilon=1e-4, max_parents=3, forbidden=()):
    """The product's run checked by the twin: every move legal and within the slack of the twin's best, the end a local optimum."""
    cols = list(X.columns)
    n = len(cols)
    score = _TrackingScore(codes, card, "bic")
    parents = [set() for _ in range(n)]
    for u, v in start:
        parents[cols.index(v)].add(cols.index(u))
    forb = {(cols.index(u), cols.index(v)) for u, v in forbidden}
    for op, u, v, gain in trace:
        u, v = cols.index(u), cols.index(v)
        assert sc.is_legal(n, parents, op, u, v, max_parents, (), forb), (op, u, v)
        best, _ = sc.best_move(score, n, parents, max_parents, (), forb)
        mine = sc.move_gain(score, parents, op, u, v)
        slack = 2 * TOL * score.total()
        assert mine >= best[0] - slack, (op, u, v, mine, best)
        assert abs(gain - mine) <= slack and mine > epsilon - slack
        parents = sc.apply_move(parents, op, u, v)
    best, _ = sc.best_move(score, n, parents, max_parents, (), forb)
    assert best is None or best[0] <= epsilon + 2 * TOL * score.total(), best
    edges = {e for e in result if isinstance(e, tuple)}
    assert edges == {(cols[u], cols[v]) for u, v in sc.edges_of(parents)}
    assert not sc.has_cycle(n, parents) and all(len(p) <= max_parents for p in parents)
    twin_total = math.fsum(score(v, parents[v]) for v in range(n))
    assert abs(total - twin_total) <= TOL * score.total()
    return parents, twin_total, score


@pytest.mark.parametrize("name", list(SEEDS))
def test_hill_climb_is_a_valid_greedy_run_to_a_local_optimum(name):
    X, codes, card = _rows(name)
    cols = list(X.columns)
    result, trace, total = structure.hill_climb(X, return_trace=True)
    parents, twin_total, score = _replay(X, codes, card, result, trace, total)
    empty_total = math.fsum(score(v, set()) for v in range(len(cols)))
    assert twin_total >= empty_total
    assert trace, "20 000 rows of a connected network are worth at least one edge"
    bn = sorobn_amd.BayesNet(*result).fit(X)  # the result is a structure fit() accepts
    assert set(bn.nodes) == set(cols)
    # started from the Chow-Liu tree it does not end below the tree
    tree = structure.chow_liu(X)
    result_t, trace_t, total_t = structure.hill_climb(X, start=tree, return_trace=True)
    _, twin_total_t, score_t = _replay(X, codes, card, result_t, trace_t, total_t, start=tree)
    tree_total = math.fsum(score_t(cols.index(v), {cols.index(u) for u, w in tree if w == v}) for v in cols)
    assert twin_total_t >= tree_total
    print(f"\n[structure] {name}: {len(trace)} moves from the empty graph to BIC {total:.3f} (empty {empty_total:.3f}); "
          f"{len(trace_t)} moves from the Chow-Liu tree ({tree_total:.3f}) to {total_t:.3f}")


@pytest.mark.parametrize("name", ["sprinkler", "asia"])
def test_hill_climb_equals_the_twin_exactly(name):
    """The edge set must be the twin's, which needs the twin's own run to be free of near-ties: no gap below 1e-6 between the gains
    of its best two moves at any step (asserted first).  Under a score-equivalent score such as BIC that cannot hold for the
    unconstrained search: adding u -> v and adding v -> u to two nodes with the same parents - every pair of the empty graph -
    gain the same amount mathematically (N * MI(u, v) minus a penalty symmetric in u and v), so the best two moves of the first
    step always tie up to rounding, for every seed.  The comparison therefore runs under a causal order - every edge against the
    column order is forbidden, as a K2-style search has it - where an edge has one legal direction and the precondition can hold.
    (The unconstrained runs on the same rows are checked move by move in the test above.)"""
    X, codes, card = _rows(name)
    cols = list(X.columns)
    n = len(cols)
    back = [(cols[v], cols[u]) for u in range(n) for v in range(u + 1, n)]
    back_ix = {(v, u) for u in range(n) for v in range(u + 1, n)}
    parents, want_trace, want_total, gap = sc.hill_climb(sc.scorer(codes, card, "bic"), n, forbidden=back_ix)
    print(f"\n[structure] {name} seed {SEEDS[name]}: twin run of {len(want_trace)} moves, smallest gap between the best two gains {gap:.3e}")
    assert want_trace and gap >= 1e-6, gap
    result, trace, total = structure.hill_climb(X, forbidden=back, return_trace=True)
    assert {e for e in result if isinstance(e, tuple)} == {(cols[u], cols[v]) for u, v in sc.edges_of(parents)}
    assert [(op, cols.index(u), cols.index(v)) for op, u, v, _ in trace] == [t[:3] for t in want_trace]
    _replay(X, codes, card, result, trace, total, forbidden=back)


# ----------------------------------------------------------------------------------------------------------- handles
def test_handles_errors_and_no_side_effects():
    spec = _example("asia")
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    eng = bn.backend.engine
    request = (("Lung cancer",), {"Smoker": True, "Positive X-ray": True})
    codes = _codes(20_000, seed=3)
    tables = [(1, 2), (5, 6, 7), (14, 15), (9,)]
    before_q = bn.query(*request[0], event=request[1]).to_numpy().copy()
    before_c = eng.count_tables(codes, CARD, tables)
    total_before = eng.total_kernel_stats()
    a = eng.dataset(codes, CARD)
    b = eng.dataset(codes[:5000, :9], CARD[:9])  # two data sets alive at once
    fams = _fam_cols(FAMILIES)
    sa = a.score_families(fams, "bic")
    names = {k["name"]: k for k in eng.kernel_stats()}
    assert set(names) == {"count_kernel", "score_kernel"} and names["score_kernel"]["items"] == len(fams)
    assert names["count_kernel"]["launches"] == 2 and names["score_kernel"]["launches"] == 3  # LDS + big counting; wave, chunk, finish
    sb = b.score_families([(1, 2), (3, 4, 5)], "bic")
    assert np.array_equal(_bits(sa), _bits(a.score_families(fams, "bic")))
    with eng.dataset(codes[:5000, :9].copy(), CARD[:9]) as b2:
        assert np.array_equal(_bits(sb), _bits(b2.score_families([(1, 2), (3, 4, 5)], "bic")))
    assert eng.total_kernel_stats() == total_before, "scoring books last-call statistics only"
    assert np.array_equal(before_q, bn.query(*request[0], event=request[1]).to_numpy())
    assert all(np.array_equal(x, y) for x, y in zip(before_c, eng.count_tables(codes, CARD, tables)))
    assert bn.backend.engine is eng
    # argument errors: checked on the host, nothing launched
    for fam, code in (([(1, 99)], _capi.E_ARG), ([()], _capi.E_ARG), ([(1, 1)], _capi.E_ARG), ([(-1,)], _capi.E_ARG)):
        with pytest.raises(_capi.MibnError) as e:
            a.score_families(fam, "bic")
        assert e.value.code == code, fam
    with pytest.raises(_capi.MibnError) as e:
        a.score_families([(1, 2)], "bdeu", ess=0.0)
    assert e.value.code == _capi.E_ARG
    with pytest.raises(_capi.MibnError) as e:
        a.score_families([tuple(range(9, 16))], "bic")  # 17^5 * 100^2 cells
    assert e.value.code == _capi.E_LIMIT
    with pytest.raises(ValueError):
        a.score_families([(1, 2)], "mdl")
    for card in ([0, 2], [2, 257]):
        with pytest.raises(_capi.MibnError) as e:
            eng.dataset(np.zeros((4, 2), np.uint8), card)
        assert e.value.code == _capi.E_LIMIT
    with pytest.raises(_capi.MibnError) as e:
        eng.dataset(np.array([[0, 1], [2, 0]], np.uint8), [2, 2])  # a code outside its column's cardinality
    assert e.value.code == _capi.E_ARG
    assert np.array_equal(_bits(sa), _bits(a.score_families(fams, "bic"))), "failed calls leave the data sets as they were"
    # closing
    b.close()
    with pytest.raises(_capi.MibnError) as e:
        b.score_families([(1, 2)], "bic")
    assert e.value.code == _capi.E_ARG
    b.close()  # (twice is fine)
    assert np.array_equal(_bits(sa), _bits(a.score_families(fams, "bic")))
    a.close()
    with pytest.raises(_capi.MibnError) as e:
        a.score_families(fams, "bic")
    assert e.value.code == _capi.E_ARG
    c = eng.dataset(codes[:100], CARD)  # a fresh id after two were destroyed
    assert c.id not in (-1,) and len(c.score_families(fams[:3], "k2")) == 3
    del c  # closed on garbage collection
    assert np.array_equal(before_q, bn.query(*request[0], event=request[1]).to_numpy())


def test_public_entry_points():
    X = pd.DataFrame(_codes(5000, seed=4)[:, [1, 16, 5, 17, 3]], columns=list("abcde"))
    got = structure.family_scores(X, [("b", ["a"]), ("a", []), ("d", ["c", "e"])], score="bdeu", ess=2.0)
    codes = X.to_numpy()
    card = [2, 2, 4, 4, 3]
    want = [sc.family_score(codes, card, 1, [0], "bdeu", 2.0), sc.family_score(codes, card, 0, [], "bdeu", 2.0),
            sc.family_score(codes, card, 3, [2, 4], "bdeu", 2.0)]
    assert all(abs(g - w) <= TOL * max(S, 1) for g, (w, S) in zip(got, want))
    edges = {e for e in structure.hill_climb(X) if isinstance(e, tuple)}
    assert {frozenset(e) for e in edges} >= {frozenset("ab"), frozenset("cd")}, edges  # b follows a, d follows c
    bn = sorobn_amd.BayesNet(*structure.hill_climb(X)).fit(X)
    assert bn.score(X) == pytest.approx(structure.hill_climb(X, return_trace=True)[2], rel=1e-12)
