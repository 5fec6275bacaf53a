"""Constraint-based structure learning on the GPU: `mibn_ci_tests` (count_kernel + the kernels of csrc/citest_kernel.hip.h over
a resident data set) and `structure.pc` on top of it, against the brute-force twin of tests/ci_check.py.

Tolerances.  adj_dof is an integer and must be equal.  With A = fsum(|term|) over the twin's terms and N = n_rows:

  G2:  |got - want| <= 1e-12 * max(1, A) + 2e-15 * N
       The first term is the summation, as for the family scores (tests/test_structure.py): a lane or a wave adds at most a few
       hundred terms before the six steps of the butterfly, each rounding at most 1.1e-16 * A; 1e-12 leaves two orders of
       magnitude.  The second term is what the summation bound cannot see: a cell's term is 2 N_xyz ln(quotient), and where the
       quotient is close to 1 (a nearly independent cell) the term is small against N_xyz while its ABSOLUTE error is not - the
       quotient of the two exact integer products is rounded once (relative 2^-53, which moves ln by 2^-53 at quotient 1) and
       the device's log is within an ulp or so of that; each is at most about 2 * 2^-53 * N_xyz of the doubled sum, and the
       N_xyz of a table add up to N: 2 * (2 * 2^-53) * N = 4.4e-16 * N, granted as 2e-15 * N.  The twin takes log1p of the exact
       integer difference there and carries neither.
  X2:  |got - want| <= 1e-12 * max(1, stat): every term is non-negative, so A = stat; the numerator is an exact 64-bit integer.

The largest observed ratios are printed.  NOT run: a data set of 2^31 rows (MIBN_E_LIMIT; 2 GB per column) and a table of 2^28
cells (the legal maximum; 2 GB) - a table ABOVE 2^28 cells is refused before anything is allocated, and that is checked."""
import itertools
import math
import os

import numpy as np
import pandas as pd
import pytest

import ci_check as cc
import netspec
import structure_check as sc
import sorobn_amd
from sorobn_amd import _capi, learning, structure

pytestmark = pytest.mark.gpu

TOL = 1e-12
G2_PER_ROW = 2e-15
CI_LANE_CELLS = 64    # kCiLaneCells of csrc/citest_kernel.hip.h: a larger stratum takes the wave form
CI_WAVE_CELLS = 4096  # kCiWaveCells: a larger table is cut into chunks of whole strata
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("g2", "x2")
# columns: cardinalities 1, 2, 3, 4, 17, 100 and 256, plus 16, 63 and 65 for the thresholds; 14 and 15 depend on 1 and 5, 6 on 5
# and 3; 18 has three labels of which only two occur
CARD = [1, 2, 2, 3, 3, 4, 4, 4, 4, 17, 17, 17, 100, 100, 2, 4, 256, 256, 3, 63, 65, 16]
TESTS = [
    (1, 2), (5, 6), (3, 15), (1, 14), (5, 15),              # q = 1
    (0, 5), (5, 0), (1, 0, 3), (1, 3, 0), (0, 12), (12, 0),  # rx or ry = 1 (1 x 100 and 100 x 1: wave form)
    (19, 1, 3), (5, 6, 7, 1, 3), (20, 1, 3),                # q = 63 / 64 / 65: a full group, and one lane with a second stratum
    (2, 5, 6), (3, 1, 2), (3, 4, 5, 15), (9, 1, 14),         # q = 2, 3, 9, 17: groups of 2, 4, 16 and 32 lanes
    (19, 0), (21, 5), (20, 0), (9, 5), (1, 9, 8),            # strata of 63 and 64 cells (lane form), 65 and 68 (wave form)
    (9, 10), (1, 9, 10),                                   # 17 x 17
    (12, 13), (1, 12, 13),                                 # 100 x 100: one and two chunks of one stratum
    (16, 17), (1, 16, 17),                                 # 256 x 256
    (5, 6, 7, 8, 1, 3), (5, 6, 7, 8, 15, 14),                # 256 strata of 6 and of 8 cells: 1 536 and 2 048 cells
    (5, 6, 7, 21, 8, 15),                                  # 1 024 strata of 16 cells: 16 384 cells, four full chunks
    (9, 10, 5, 6),                                         # 289 strata of 16 cells = 4 624: just above one wave, chunks of 256 + 33
    (9, 10, 11, 1, 2),                                     # 4 913 strata of 4 cells: four chunks of 1 024 and one of 817
    (5, 6, 9, 10),                                         # 16 strata of 289 cells = 4 624: wave-form chunks of 14 + 2
    (12, 13, 1, 2),                                        # 10 000 strata, most of which no row reaches
    (18, 1, 2), (1, 18, 3), (1, 3, 18),                     # an unobserved state, as condition, row and column
]


def _codes(n_rows, seed=0):
    rng = np.random.default_rng(seed)
    cols = [rng.integers(0, c, n_rows) for c in CARD]
    cols[14] = (cols[1] + (rng.random(n_rows) < 0.2)) % 2
    cols[15] = (cols[5] + rng.integers(0, 2, n_rows)) % 4
    cols[6] = (cols[5] + cols[3] + (rng.random(n_rows) < 0.3)) % 4
    cols[18] = rng.integers(0, 2, n_rows)
    return np.stack(cols, axis=1).astype(np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _example(name):
    return next(n for n in netspec.load(os.path.join(GOLDEN, "examples.json")) if n["spec"]["name"] == name)["spec"]


@pytest.fixture(scope="module")
def engine():
    assert _capi.device_count() > 0, "no HIP device visible"
    return learning.counting_engine()


_twin_cache = {}


def _twin(n_rows, kind):
    """The twin's answers for TESTS on _codes(n_rows, seed=n_rows): computed once, shared."""
    if (n_rows, kind) not in _twin_cache:
        codes = _codes(n_rows, seed=n_rows)
        _twin_cache[(n_rows, kind)] = [cc.ci_stat(codes, CARD, t[-2], t[-1], list(t[:-2]), kind) for t in TESTS]
    return _twin_cache[(n_rows, kind)]


def _within(kind, got, want, A, n_rows):
    bound = TOL * max(1.0, A) + G2_PER_ROW * n_rows if kind == "g2" else TOL * max(1.0, want)
    return abs(got - want) / bound


def test_the_shapes_cover_every_form():
    cells = lambda t: math.prod(CARD[c] for c in t)
    stratum = lambda t: CARD[t[-2]] * CARD[t[-1]]
    assert {stratum(t) for t in TESTS} >= {CI_LANE_CELLS - 1, CI_LANE_CELLS, CI_LANE_CELLS + 1, 17 * 17, 100 * 100, 256 * 256}
    assert {cells(t) // stratum(t) for t in TESTS if cells(t) <= CI_WAVE_CELLS} >= {1, 2, 3, 9, 17, 63, 64, 65, 256}
    lane_big = [t for t in TESTS if cells(t) > CI_WAVE_CELLS and stratum(t) <= CI_LANE_CELLS]
    wave_big = [t for t in TESTS if cells(t) > CI_WAVE_CELLS and stratum(t) > CI_LANE_CELLS]
    assert any((cells(t) // stratum(t)) % (CI_WAVE_CELLS // stratum(t)) for t in lane_big), "a ragged last chunk, lane form"
    assert any((cells(t) // stratum(t)) % (CI_WAVE_CELLS // stratum(t)) == 0 for t in lane_big), "whole chunks only"
    assert any(stratum(t) < CI_WAVE_CELLS and (cells(t) // stratum(t)) % (CI_WAVE_CELLS // stratum(t)) for t in wave_big)
    assert min(cells(t) for t in lane_big) < CI_WAVE_CELLS + 1024 and any(cells(t) == CI_WAVE_CELLS // 2 for t in TESTS)
    assert any(CARD[t[-2]] == 1 for t in TESTS) and any(CARD[t[-1]] == 1 for t in TESTS)


@pytest.mark.parametrize("n_rows", [1, 7, 1000, 200_000])
def test_statistics_against_the_twin(engine, n_rows):
    codes = _codes(n_rows, seed=n_rows)
    worst = {k: (0.0, None) for k in KINDS}
    small_budget = _capi.Engine(0)
    small_budget.set_option("score_cells", 3000)  # several sub-batches; every table above 3 000 cells goes alone
    try:
        with engine.dataset(codes, CARD) as row_major, engine.dataset(np.asfortranarray(codes), CARD) as col_major, \
                small_budget.dataset(codes, CARD) as cut:
            for kind in KINDS:
                stat, dof = row_major.ci_tests(TESTS, kind)
                for other in (col_major, cut):
                    s2, d2 = other.ci_tests(TESTS, kind)
                    assert np.array_equal(_bits(stat), _bits(s2)) and np.array_equal(dof, d2), (n_rows, kind)
                assert small_budget.kernel_stats()[0]["launches"] > 2, "the small budget did not cut the call"
                for t, g, d, (want, A, adj, classic) in zip(TESTS, stat.tolist(), dof.tolist(), _twin(n_rows, kind)):
                    assert d == adj and adj <= classic, (n_rows, kind, t, d, adj, classic)
                    ratio = _within(kind, g, want, A, n_rows)
                    if ratio > worst[kind][0]:
                        worst[kind] = (ratio, (n_rows, t, g, want, A))
                    assert ratio <= 1.0, (n_rows, kind, t, g, want, A, ratio)
                    if kind == "x2":
                        assert g >= 0.0
    finally:
        small_budget.close()
    for kind in KINDS:
        print(f"\n[citest] {kind} vs twin, {n_rows} rows: largest |got - want| / bound = {worst[kind][0]:.3e} at {worst[kind][1]}")
    if n_rows == 200_000:  # an unobserved state costs degrees of freedom; strata no row reaches cost theirs
        by_test = dict(zip(TESTS, _twin(n_rows, "g2")))
        assert by_test[(1, 18, 3)][2] < by_test[(1, 18, 3)][3] and by_test[(18, 1, 2)][2] < by_test[(18, 1, 2)][3]
        assert by_test[(12, 13, 1, 2)][2] <= 10_000 and by_test[(5, 6)][2] == by_test[(5, 6)][3]


def test_an_exactly_independent_table(engine):
    """N_xyz = a_x * b_y * c_z in every stratum (one stratum empty): X2 is exactly 0, G2 within its tolerance of 0."""
    a, b, c = [1, 2, 3], [4, 1, 0, 5], [2, 0, 7]
    rows = [(z, x, y) for z in range(3) for x in range(3) for y in range(4) for _ in range(a[x] * b[y] * c[z])]
    codes = np.array(rows * 37, np.uint8)
    wide = np.repeat(np.arange(3 * 17 * 17), 5)  # 17 x 17 strata (the wave form), five rows per cell of the strata 0 and 2
    wide = wide[(wide // 289) != 1]
    codes_w = np.stack([wide // 289, (wide // 17) % 17, wide % 17], axis=1).astype(np.uint8)
    for m, card, tests in ((codes, [3, 3, 4], [(0, 1, 2), (1, 2)]), (codes_w, [3, 17, 17], [(0, 1, 2), (1, 2)])):
        with engine.dataset(m, card) as ds:
            x2, dof = ds.ci_tests(tests, "x2")
            assert x2.tolist() == [0.0, 0.0]
            g2, dof2 = ds.ci_tests(tests, "g2")
            assert np.array_equal(dof, dof2)
            for t, g, d in zip(tests, g2.tolist(), dof.tolist()):
                want, A, adj, _ = cc.ci_stat(m, card, t[-2], t[-1], list(t[:-2]), "g2")
                assert want == 0.0 and d == adj and abs(g) <= TOL * max(1.0, A) + G2_PER_ROW * len(m), (t, g)
    assert dof.tolist() == [2 * 16 * 16, 16 * 16]


def test_empty_data_set_single_rows_and_no_tests(engine):
    with engine.dataset(np.zeros((0, 3), np.uint8), [2, 3, 4]) as ds:
        for kind in KINDS:
            stat, dof = ds.ci_tests([(0, 1), (0, 1, 2), (2, 1, 0)], kind)
            assert stat.tolist() == [0.0, 0.0, 0.0] and dof.tolist() == [0, 0, 0]
        stat, dof = ds.ci_tests([], "g2")
        assert len(stat) == 0 and len(dof) == 0
    with engine.dataset(np.array([[1, 2, 3]], np.uint8), [2, 3, 4]) as ds:  # one row: one cell of count 1, quotient 1
        stat, dof = ds.ci_tests([(0, 1), (0, 1, 2)], "g2")
        assert stat.tolist() == [0.0, 0.0] and dof.tolist() == [0, 0]


def test_bit_for_bit_repeatability(engine):
    codes = _codes(50_000, seed=5)
    rng = np.random.default_rng(1)
    cut = _capi.Engine(0)
    cut.set_option("score_cells", 3000)
    try:
        with engine.dataset(codes, CARD) as a, engine.dataset(codes.copy(), CARD) as b, \
                engine.dataset(np.asfortranarray(codes), CARD) as f, cut.dataset(codes, CARD) as c:
            for kind in KINDS:
                first, dof = a.ci_tests(TESTS, kind)
                for _ in range(2):
                    again, d2 = a.ci_tests(TESTS, kind)
                    assert np.array_equal(_bits(first), _bits(again)) and np.array_equal(dof, d2)
                back, d2 = a.ci_tests(TESTS[::-1], kind)
                assert np.array_equal(_bits(first[::-1]), _bits(back)) and np.array_equal(dof[::-1], d2)
                perm = rng.permutation(len(TESTS))
                shuffled, d2 = a.ci_tests([TESTS[i] for i in perm], kind)
                assert np.array_equal(_bits(first[perm]), _bits(shuffled)) and np.array_equal(dof[perm], d2)
                extra = [(i, j) for i, j in itertools.permutations(range(len(CARD)), 2)]
                mixed = extra[:100] + TESTS[:7] + extra[100:] + TESTS[7:]
                got, d2 = a.ci_tests(mixed, kind)
                assert np.array_equal(_bits(first), _bits(np.concatenate([got[100:107], got[len(extra) + 7:]])))
                assert np.array_equal(dof, np.concatenate([d2[100:107], d2[len(extra) + 7:]]))
                for t, s, d in zip(TESTS, first, dof):  # ... and one at a time
                    one, d1 = a.ci_tests([t], kind)
                    assert _bits(one)[0] == _bits(s) and d1[0] == d, t
                for name, other in (("second handle of the same rows", b), ("column-major input", f), ("3 000-cell budget", c)):
                    s2, d2 = other.ci_tests(TESTS, kind)
                    assert np.array_equal(_bits(first), _bits(s2)) and np.array_equal(dof, d2), name
    finally:
        cut.close()


def test_statistics_rows_errors_and_no_side_effects():
    spec = _example("asia")
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    eng = bn.backend.engine
    request = (("Lung cancer",), {"Smoker": True, "Positive X-ray": True})
    codes = _codes(20_000, seed=3)
    before_q = bn.query(*request[0], event=request[1]).to_numpy().copy()
    total_before = eng.total_kernel_stats()
    fams = [(1,), (1, 2), (5, 6, 7), (9, 10, 11), (12, 13, 5)]
    with eng.dataset(codes, CARD) as a:
        scores = a.score_families(fams, "bic")
        stat, dof = a.ci_tests(TESTS, "g2")
        names = {k["name"]: k for k in eng.kernel_stats()}
        assert set(names) == {"count_kernel", "citest_kernel"}
        assert names["citest_kernel"]["items"] == len(TESTS) and names["count_kernel"]["items"] == len(TESTS)
        assert names["count_kernel"]["launches"] == 2 and names["citest_kernel"]["launches"] == 3  # LDS + big counting; lane, wave, finish
        a.ci_tests([(1, 2), (5, 6, 7)], "x2")
        names = {k["name"]: k for k in eng.kernel_stats()}
        assert names["count_kernel"]["launches"] == 1 and names["citest_kernel"]["launches"] == 1 and names["citest_kernel"]["items"] == 2
        assert np.array_equal(_bits(scores), _bits(a.score_families(fams, "bic"))), "score_families after an interleaved ci_tests"
        assert eng.total_kernel_stats() == total_before, "the tests book last-call statistics only"
        assert np.array_equal(before_q, bn.query(*request[0], event=request[1]).to_numpy())
        # argument errors: checked on the host, nothing launched
        for tests in ([(1, 99)], [(1,)], [()], [(1, 1)], [(1, 2, 1)], [(-1, 2)], [(1, 2), (3,)]):
            with pytest.raises(_capi.MibnError) as e:
                a.ci_tests(tests, "g2")
            assert e.value.code == _capi.E_ARG, tests
        C = _capi.C
        one = np.zeros(1, np.float64)
        rc = eng._L.mibn_ci_tests(eng._h, a.id, 2, 1, _capi._p(np.array([0, 2], np.int64), C.c_int64), _capi._p(np.array([1, 2], np.int32), C.c_int32),
                                  _capi._p(one, C.c_double), _capi._p(np.zeros(1, np.int64), C.c_int64))
        assert rc == _capi.E_ARG, "unknown kind"
        with pytest.raises(ValueError):
            a.ci_tests([(1, 2)], "fisher")
        with pytest.raises(_capi.MibnError) as e:
            a.ci_tests([(9, 10, 11, 12, 13, 16, 17)], "g2")  # 17^3 * 100^2 * 256^2 cells
        assert e.value.code == _capi.E_LIMIT
        again, d2 = a.ci_tests(TESTS, "g2")
        assert np.array_equal(_bits(stat), _bits(again)) and np.array_equal(dof, d2), "failed calls leave the data set as it was"
    with pytest.raises(_capi.MibnError) as e:
        a.ci_tests([(1, 2)], "g2")  # closed
    assert e.value.code == _capi.E_ARG
    assert np.array_equal(before_q, bn.query(*request[0], event=request[1]).to_numpy())


def test_public_ci_tests():
    codes = _codes(5000, seed=4)[:, [1, 14, 5, 15, 3, 18]]
    X = pd.DataFrame(codes, columns=list("abcdef"))
    card = [2, 2, 4, 4, 3, 2]  # (the encoder sees two labels in f)
    asked = [("a", "b", []), ("c", "d", ["e"]), ("b", "e", ["a", "c"]), ("a", "f", "d")]
    for test in ("g2", "x2", "mi"):
        for dof in ("classic", "adjusted"):
            got = structure.ci_tests(X, asked, test=test, dof=dof)
            for (x, y, given), row in zip(asked, got.itertuples()):
                Z = sorted("abcdef".index(z) for z in given)
                kind = "x2" if test == "x2" else "g2"
                want, A, adj, classic = cc.ci_stat(codes, card, "abcdef".index(x), "abcdef".index(y), Z, kind)
                d = adj if dof == "adjusted" else classic
                scale = 2 * len(X) if test == "mi" else 1
                assert row.dof == d and _within(kind, row.stat * scale, want, A, len(X)) <= 1.0 + 1e-3
                assert row.p_value == learning.chi2_sf(row.stat * scale, d) or test == "mi"
    assert got["p_value"].iloc[0] < 1e-100 and got["p_value"].iloc[1] < 1e-100  # b follows a, d follows c


# ----------------------------------------------------------------------------------------------------------- search
PC_ROWS = 20_000
ALPHA = 0.01
# seeds of structure_check.forward_sample, chosen on the CPU with the twin: the twin's run on these rows has no p-value within
# relative 1e-6 of ALPHA (asserted below); seed 1 was the first one tried for both networks
PC_SEEDS = {"sprinkler": 1, "asia": 1}


@pytest.mark.parametrize("name", list(PC_SEEDS))
def test_pc_equals_the_twin_on_sampled_rows(name):
    names, raw, _ = sc.forward_sample(_example(name), PC_ROWS, PC_SEEDS[name])
    X = pd.DataFrame(raw.astype(np.int64), columns=names)
    codes, _, card = learning.encode_complete(X, names)
    codes = np.ascontiguousarray(codes)
    n = len(names)
    seen = []

    def p_of(x, y, S):
        stat, _, _, classic = cc.ci_stat(codes, card, x, y, list(S), "g2")
        seen.append(learning.chi2_sf(stat, classic))
        return seen[-1]

    arrows, und, sepsets = cc.pc_brute(n, p_of, ALPHA)
    gap = min(abs(p - ALPHA) / ALPHA for p in seen)
    print(f"\n[citest] {name} seed {PC_SEEDS[name]}: twin run of {len(seen)} tests, closest p-value to alpha at relative {gap:.3e}")
    assert gap >= 1e-6, gap
    res = structure.pc(X, alpha=ALPHA, return_trace=True)
    ix = lambda e: (names.index(e[0]), names.index(e[1]))
    assert {ix(e) for e in res.directed} == arrows and {ix(e) for e in res.undirected} == und
    assert {ix(k): tuple(names.index(z) for z in S) for k, S in res.sepsets.items()} == sepsets
    assert sum(res.tests_per_level) == len(res.trace) and res.tests_per_level[0] == n * (n - 1) // 2
    skeleton = {frozenset(e) for e in arrows | und}
    truth = {frozenset((names.index(p), v)) for v, nm in enumerate(names) for p in _example(name)["cpts"][nm]["names"][:-1]}
    print(f"[citest] {name}: {len(skeleton & truth)} of {len(truth)} edges of the network in the skeleton, {len(skeleton - truth)} others")
    bn = sorobn_amd.BayesNet(*res.dag()).fit(X)  # the result is a structure fit() accepts
    assert set(bn.nodes) == set(names)
