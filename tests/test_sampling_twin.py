"""sample_kernel (forward sampling, rejection, likelihood weighting) and the Gibbs kernels (gibbs_kernel generic / FAST,
gibbs_kernel8) against the exact numpy twin of their Philox stream, tests/sample_check.py: the samples and every histogram
have to be EQUAL - a shared counter or key, a dropped seed word, an off-by-one in the inverse-CDF compare, a counted tail
lane or a swapped histogram stride cannot hide behind a statistical tolerance.  Only the likelihood sums carry a bound, the
one of adding n non-negative doubles in another order (LDS atomics, then global atomics): |got - fsum| <= n_cell * 2^-52 * fsum.

CPTs are drawn from a seeded rng, unnormalised on purpose, with zeros at the start, the middle and the end of some rows.

The network contract caps a network at 1 024 variables (kMaxVars, the planner's bitset; mibn_set_network refuses more), so the
LDS-resident state of sample_kernel is at most 64 KiB and a forward-sampling launch never needs the raised dynamic-LDS limit:
test_variable_cap_bounds_the_sample_state pins that.  The raised limit, the exact 150 KiB boundary and MIBN_E_LIMIT behind it are
reached the way the library can reach them - state + histogram of a sampling query."""
import ctypes as C

import numpy as np
import pytest

import gibbs_cases as gc
import sample_check as sc
from gibbs_cases import chain_net as _chain_net, example as _example, grid_net as _grid_net, random_net as _random_net, tables as _tables
from sorobn_amd import _capi

pytestmark = pytest.mark.gpu

REJECTION, LIKELIHOOD = 1, 2


# ----------------------------------------------------------------------------------------------------------- networks

MIXED = dict(card=[3, 2, 5, 4, 2, 3], parents=[[], [0], [0, 1], [2], [1, 3], [2, 4]])
# a zero row of variable 1 behind 0 = 0, a zero in the middle of its other row, a deterministic last variable
ZERO_ROW = ([2, 3, 2, 3], [[], [0], [1], [1]],
            [np.array([0.5, 0.5]), np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.8]]), np.array([[1.0, 1.0], [1.0, 1.0], [0.5, 1.5]]),
             np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0]])])


def _engine(net):
    eng = _capi.Engine(0)
    eng.set_network(*net.engine_args())
    return eng


@pytest.fixture(scope="module")
def asia():
    net = _example("asia")
    return net, _engine(net)


@pytest.fixture(scope="module")
def mixed():
    net = _random_net(MIXED["card"], MIXED["parents"], seed=21)
    return net, _engine(net)


# ----------------------------------------------------------------------------------------------------- forward samples

@pytest.mark.parametrize("n_samples", [1, 63, 64, 65, 262_144 + 65])
def test_forward_samples_equal_the_twin(asia, n_samples):
    """One lane, a partial wave, a full wave, a wave and a lane, and the second grid-stride trip (the launch is capped at
    4096 blocks x 64 lanes) with a partial wave."""
    net, eng = asia
    got = eng.sample(n_samples, seed=5)
    want, _ = sc.forward(net, n_samples, 5)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("seed", [0, 5, 1 << 32, 2 ** 64 - 1])
def test_forward_seed_words(asia, mixed, seed):
    for net, eng in (asia, mixed):
        got = eng.sample(65, seed=seed)
        assert np.array_equal(got, sc.forward(net, 65, seed)[0])
        assert not np.array_equal(got, eng.sample(65, seed=seed ^ (1 << 32)))  # the high word matters


def test_forward_large_codes_and_cardinalities():
    """State codes >= 128 in the byte state, cardinality 255, cardinality 1; the 200- and 255-state variables are parents."""
    card, parents = [200, 255, 1, 2], [[], [0], [1], [0, 1, 2]]
    tabs = _tables(np.random.default_rng(3), card, parents)
    tabs[0][-1] += 20.0  # the last states are drawn often
    tabs[1][:, -1] += 20.0
    net = sc.make_net(card, parents, tabs)
    eng = _engine(net)
    got = eng.sample(2000, seed=8)
    want, _ = sc.forward(net, 2000, 8)
    assert want[:, 0].max() == 199 and want[:, 1].max() == 254 and (want[:, 1] >= 128).sum() > 500 and (want[:, 2] == 0).all()
    assert len(set(want[:, 3].tolist())) == 2
    assert np.array_equal(got, want)
    wsum, counts = eng.sampling_query(REJECTION, [1], [3], [1], 3000, seed=2)  # a 255-cell histogram indexed by those codes
    assert np.array_equal(counts, sc.rejection(net, [1], {3: 1}, 3000, 2))
    big = _engine(sc.make_net([256, 2], [[], [0]], _tables(np.random.default_rng(4), [256, 2], [[], [0]])))
    with pytest.raises(_capi.MibnError) as e:
        big.sample(4)
    assert e.value.code == _capi.E_LIMIT
    with pytest.raises(_capi.MibnError) as e:
        big.gibbs([1], [], [], 8, 8)
    assert e.value.code == _capi.E_LIMIT


def test_variable_cap_bounds_the_sample_state():
    """1 024 variables = exactly 64 KiB of state, the largest network the library takes: 64 + 1 samples equal the twin.  1 025
    variables are refused by mibn_set_network (kMaxVars), so the forward-sampling launch never exceeds the default 64 KiB of
    dynamic LDS; whoever raises the cap has to bring a test for the raised LDS limit of SAMPLE mode with it."""
    net = _chain_net(1024, seed=6)
    eng = _engine(net)
    got = eng.sample(65, seed=(9 << 32) | 1)
    assert np.array_equal(got, sc.forward(net, 65, (9 << 32) | 1)[0])
    with pytest.raises(_capi.MibnError) as e:
        _engine(_chain_net(1025, seed=6))
    assert e.value.code == _capi.E_ARG


def test_forward_clamps(asia, mixed):
    net, eng = mixed
    for clamp in ({0: 2}, {2: 4}, {5: 0}, {0: 1, 2: 0, 5: 2}, {3: 3, 1: 1}):  # a root, an interior node, a leaf, all of them
        got = eng.sample(130, list(clamp), list(clamp.values()), seed=12)
        want, _ = sc.forward(net, 130, 12, clamp=clamp)
        assert np.array_equal(got, want), clamp
        assert all((got[:, v] == c).all() for v, c in clamp.items())
    net, eng = asia
    assert np.array_equal(eng.sample(65, [0, 7], [1, 0], seed=3), sc.forward(net, 65, 3, clamp={0: 1, 7: 0})[0])
    for var, code in ((0, 2), (0, -1), (8, 0), (-1, 0)):  # outside the domain / unknown variable
        with pytest.raises(_capi.MibnError) as e:
            eng.sample(4, [var], [code])
        assert e.value.code == _capi.E_ARG


def test_zero_row_under_a_clamp():
    """A clamp can select a conditional row that is all zero (sparse CPT): the draw falls through to card - 1 and the sample's
    likelihood is 0 - the samples are counted, they add nothing to the likelihood sum.  (Engine level; what the pandas API makes
    of it is not decided here.)"""
    net = sc.make_net(*ZERO_ROW)
    eng = _engine(net)
    got = eng.sample(70, [0], [0], seed=1)
    want, lik = sc.forward(net, 70, 1, clamp={0: 0})
    assert np.array_equal(got, want) and (got[:, 1] == 2).all() and (lik == 0).all()
    wsum, counts = eng.sampling_query(LIKELIHOOD, [1], [0], [0], 70, seed=1)
    assert counts.tolist() == [0, 0, 70] and wsum.tolist() == [0.0, 0.0, 0.0]
    got = eng.sample(70, [0], [1], seed=1)
    assert np.array_equal(got, sc.forward(net, 70, 1, clamp={0: 1})[0]) and set(got[:, 1].tolist()) == {0, 2}


# ----------------------------------------------------------------------------------- rejection / likelihood weighting

def _check_query(eng, net, mode, q, ev, n, seed):
    """counts equal; wsum within the reordering bound per cell.  -> (counts, largest |got - fsum| / bound)."""
    wsum, counts = eng.sampling_query(mode, q, list(ev), list(ev.values()), n, seed=seed)
    if mode == REJECTION:
        want = sc.rejection(net, q, ev, n, seed)
        assert np.array_equal(counts, want), (q, ev, n)
        return counts, 0.0
    want, fsum = sc.likelihood(net, q, ev, n, seed)
    assert np.array_equal(counts, want), (q, ev, n)
    bound = want * 2.0 ** -52 * fsum
    diff = np.abs(wsum - fsum)
    assert (diff <= bound).all(), (q, ev, n, float(np.max(diff - bound)))
    assert (wsum[fsum == 0] == 0).all()
    return counts, float(np.max(diff[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("mode", [REJECTION, LIKELIHOOD])
def test_query_histograms_equal_the_twin(mixed, mode):
    net, eng = mixed
    worst = 0.0
    cases = [([0, 2], {4: 1}), ([2, 0], {4: 1}),   # cards 3 and 5 in both orders: a swapped stride fails
             ([2], {3: 1}),                         # the query variable is a parent of the evidence
             ([5, 1, 3], {0: 2, 2: 3}), ([1], {})]
    for q, ev in cases:
        counts, r = _check_query(eng, net, mode, q, ev, 20_000, seed=(1 << 32) | 7)
        worst = max(worst, r)
        if mode == LIKELIHOOD or not ev:
            assert counts.sum() == 20_000
        else:
            assert 0 < counts.sum() < 20_000
    a = eng.sampling_query(mode, [0, 2], [4], [1], 20_000, seed=7)[1].reshape(3, 5)
    b = eng.sampling_query(mode, [2, 0], [4], [1], 20_000, seed=7)[1].reshape(5, 3)
    assert np.array_equal(a, b.T) and not np.array_equal(a.reshape(-1), b.reshape(-1))
    print("largest |wsum - fsum| / bound:", worst)


@pytest.mark.parametrize("n_samples", [1, 65, 262_144 + 65])
def test_query_sample_counts(mixed, n_samples):
    net, eng = mixed
    worst = 0.0
    for mode in (REJECTION, LIKELIHOOD):
        counts, r = _check_query(eng, net, mode, [2, 5], {1: 0}, n_samples, seed=4)
        worst = max(worst, r)
        assert mode == REJECTION or counts.sum() == n_samples  # no tail lane of the last wave is counted
    print("largest |wsum - fsum| / bound:", worst)


def test_query_zero_evidence_and_zero_likelihoods():
    card, parents = MIXED["card"], MIXED["parents"]
    tabs = _tables(np.random.default_rng(22), card, parents)
    tabs[3][:, 3] = 0.0      # state 3 of variable 3 has no mass anywhere: evidence nobody satisfies
    tabs[4][0, :, 0] = 0.0   # state 0 of variable 4 has no mass behind 1 = 0: a clamp that zeroes SOME likelihoods
    net = sc.make_net(card, parents, tabs)
    eng = _engine(net)
    counts, _ = _check_query(eng, net, REJECTION, [0, 2], {3: 3}, 5000, seed=3)
    assert counts.sum() == 0
    assert eng.sampling_query(REJECTION, [0, 2], [3], [7], 5000, seed=3)[1].sum() == 0  # a label outside the domain
    _, lik = sc.forward(net, 5000, 3, clamp={4: 0})
    assert (lik == 0).sum() > 500 and (lik > 0).sum() > 500
    counts, r = _check_query(eng, net, LIKELIHOOD, [1, 5], {4: 0}, 5000, seed=3)
    assert counts.sum() == 5000  # the samples of likelihood 0 are counted
    counts, _ = _check_query(eng, net, LIKELIHOOD, [0], {3: 3}, 5000, seed=3)  # every likelihood is 0
    assert counts.sum() == 5000
    with pytest.raises(_capi.MibnError) as e:
        eng.sampling_query(LIKELIHOOD, [0], [3], [4], 10)  # a clamp outside the domain
    assert e.value.code == _capi.E_ARG
    print("largest |wsum - fsum| / bound:", r)


def test_query_histograms_up_to_the_lds_limit():
    """4 913 cells (59 KB of histogram, below the default dynamic-LDS limit); 9 826 cells (state + histogram cross 64 KiB: the
    raised limit); state + histogram of exactly 150 KiB (6 variables, 32 x 21 x 19 cells x 12 bytes + 384) runs, 64 bytes more
    (a seventh variable) is MIBN_E_LIMIT."""
    net = _random_net([17, 17, 17, 2, 3], [[], [0], [1], [2], [3]], seed=31)
    eng = _engine(net)
    worst = 0.0
    for q in ([0, 1, 2], [2, 0, 1, 3]):
        for mode in (REJECTION, LIKELIHOOD):
            counts, r = _check_query(eng, net, mode, q, {4: 2}, 30_000, seed=6)
            worst = max(worst, r)
            assert (counts > 0).sum() > 1000
    card = [32, 21, 19, 2, 2, 2, 2]
    parents = [[], [0], [1], [2], [3], [4], [5]]
    tabs = _tables(np.random.default_rng(32), card, parents)
    fits = sc.make_net(card[:6], parents[:6], tabs[:6])
    assert 6 * 64 + 32 * 21 * 19 * 12 == 150 * 1024
    eng = _engine(fits)
    for mode in (REJECTION, LIKELIHOOD):
        counts, r = _check_query(eng, fits, mode, [0, 1, 2], {5: 1}, 30_000, seed=7)
        worst = max(worst, r)
        assert (counts > 0).sum() > 1000
    eng = _engine(sc.make_net(card, parents, tabs))
    for mode in (REJECTION, LIKELIHOOD):
        with pytest.raises(_capi.MibnError) as e:
            eng.sampling_query(mode, [0, 1, 2], [5], [1], 100)
        assert e.value.code == _capi.E_LIMIT
    print("largest |wsum - fsum| / bound:", worst)


# -------------------------------------------------------------------------------------------------------- Gibbs chains

def _gibbs_all_forms(eng, net, q, ev, chains, iters, seed, cycle=None, chain_first=0):
    """gibbs_lds 1 (tables in LDS, the 8-lane form where it applies), 2 (LDS, one chain per lane: FAST on grids) and 0 (tables in L2)."""
    want = sc.gibbs(net, q, ev, chains, iters, seed, cycle=cycle, chain_first=chain_first)
    assert want.sum() == chains * iters
    try:
        for mode in (1, 2, 0):
            eng.set_option("gibbs_lds", mode)
            got = eng.gibbs(q, list(ev), list(ev.values()), chains, iters, seed=seed, cycle=cycle, chain_first=chain_first)
            assert np.array_equal(got, want), (mode, q, ev, chains, iters, np.flatnonzero(got != want)[:8])
    finally:
        eng.set_option("gibbs_lds", 1)
    return want


@pytest.mark.parametrize("name", list(gc.GIBBS_CASES))
def test_gibbs_histograms_equal_the_twin(name):
    """Every case under gibbs_lds 1, 2 and 0: the launch forms its table entry names (tests/test_sampler_plan_host.py holds the plan to them)."""
    make, q, ev, cycle, _, ((chains, iters), (shard_chains, shard_iters)) = gc.GIBBS_CASES[name]
    net = make()
    cycle = gc.cycle_of(net, ev, cycle)
    eng = _engine(net)
    counts = _gibbs_all_forms(eng, net, q, ev, chains, iters, seed=(3 << 32) | 9, cycle=cycle)
    assert (counts > 0).sum() > 1
    _gibbs_all_forms(eng, net, q, ev, shard_chains, shard_iters, seed=2, cycle=cycle, chain_first=7)
    _gibbs_all_forms(eng, net, q, ev, shard_chains, shard_iters, seed=2, cycle=cycle, chain_first=(1 << 32) + 5)  # the high word of the chain index


@pytest.mark.parametrize("name", ["grid3x3k8", "dag-5-children-3-parents", "tree-17-255", "two-255-state-variables", "grid32x32k2"])
def test_gibbs_conditionals_equal_the_twin(name):
    """mibn_gibbs_conditional (the COND instantiation of every launch form: gibbs_lds 1, 2 and 0 of cases that between them take all
    six) on a wave and six lanes of forward samples: the weights of the twin, each divided by their sum in ascending state order -
    the same products in the same order, one correctly rounded division: EQUAL.  The one-chain-per-lane FAST form alone carries a bound:
    the compiler contracts its `total += w[x]` into fused multiply-adds, so its sum of at most 8 non-negative terms
    and the twin's are two differently rounded sums, each within 8 x 2^-53 of the exact one: |got - want| <= 2^-48 x want."""
    make, q, ev, cycle, forms, _ = gc.GIBBS_CASES[name]
    net = make()
    states = sc.forward(net, gc.CONDITIONAL_ROWS, 11, clamp=ev)[0]
    w = sc.gibbs_weights(net, q[0], states)
    total = np.zeros(len(w))
    for x in range(w.shape[1]):
        total = total + w[:, x]
    want = np.where(total[:, None] > 0, w / np.where(total > 0, total, 1.0)[:, None], 0.0)
    eng = _engine(net)
    try:
        for mode in gc.LDS_MODES:
            eng.set_option("gibbs_lds", mode)
            got = eng.gibbs_conditional(q[0], states, list(ev), list(ev.values()), cycle=gc.cycle_of(net, ev, cycle))
            diff = np.abs(got - want)
            print(name, forms[mode], "largest |got - want| / want:", float(np.max(diff[want > 0] / want[want > 0])))
            assert (diff <= (2.0 ** -48 * want if forms[mode] == "Fast" else 0.0)).all(), (mode, float(diff.max()))
    finally:
        eng.set_option("gibbs_lds", 1)


def test_gibbs_conditional_refuses_unknown_evidence_ids(asia):
    """Through the raw library handle (the Python wrapper has checks of its own): an evidence id of n_vars or -1 is MIBN_E_ARG with the
    planner's message, a duplicate likewise - before anything is launched: the output keeps its fill (a launch overwrites every row)."""
    net, eng = asia
    n = len(net.card)
    i32 = lambda a: np.asarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    states = np.zeros((3, n), np.uint8)
    for ids, msg in (([n], f"unknown evidence variable id {n}"), ([-1], "unknown evidence variable id -1"), ([2, n], f"unknown evidence variable id {n}"),
                     ([2, 2], "duplicate evidence variable id 2")):
        out = np.full((3, 2), -7.0)
        rc = eng._L.mibn_gibbs_conditional(eng._h, len(ids), i32(ids), i32([0] * len(ids)), None, 0, 3, states.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == _capi.E_ARG and eng._L.mibn_last_error(eng._h).decode() == msg
        assert (out == -7.0).all()
    assert eng.gibbs_conditional(0, states, [2], [0]).shape == (3, 2)  # the handle still works


def test_gibbs_updates_without_mass():
    """Deterministic rows: under 0 = 0 the row of variable 1 is all zero - its update has total == 0 and keeps the state, in every
    form; its trailing / middle zero states are never taken elsewhere.  (The `last` rule itself needs a uniform whose product with
    the total rounds up to the total: probability 2^-53 per update, not reachable by a test.)"""
    net = sc.make_net(*ZERO_ROW)
    eng = _engine(net)
    w = sc.gibbs_weights(net, 1, sc.forward(net, 8, 0, clamp={0: 0})[0])
    assert (w == 0).all()
    counts = _gibbs_all_forms(eng, net, [1, 3], {0: 0}, 65, 257, seed=4)
    assert counts.reshape(3, 3)[2, 2] == 65 * 257  # 1 stays at card - 1, 3 follows it
    counts = _gibbs_all_forms(eng, net, [1, 2], {}, 65, 257, seed=4)
    assert counts.reshape(3, 2)[1].sum() == 0  # the zero in the middle of the row
    _gibbs_all_forms(eng, net, [1], {3: 2}, 9, 100, seed=4)


@pytest.fixture(scope="module")
def grid8():
    net = _grid_net(3, 3, 8, 51)
    return net, _engine(net)


@pytest.mark.parametrize("chains", [1, 8, 9, 61, 65])
def test_gibbs_chain_counts(grid8, chains):
    """The last group of 8 lanes (gibbs_kernel8) / the last wave (gibbs_kernel) partly idle."""
    net, eng = grid8
    _gibbs_all_forms(eng, net, [4, 8], {2: 5}, chains, 9, seed=(1 << 32) | 3)


@pytest.mark.parametrize("iters", [1, 7, 8, 9, 257, 1000])
def test_gibbs_iteration_counts(grid8, iters):
    """gibbs_kernel8 refreshes each lane's uniform at it & 7 == 0: iteration counts around and off the multiples of 8."""
    net, eng = grid8
    _gibbs_all_forms(eng, net, [0, 5], {}, 9, iters, seed=(1 << 32) | 3)
    if iters == 1000:
        _gibbs_all_forms(eng, net, [4], {8: 0}, 65, iters, seed=6)
