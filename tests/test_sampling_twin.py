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
import numpy as np
import pytest

import golden_util as gu
import netspec
import sample_check as sc
import sorobn_amd
from sorobn_amd import _capi
from sorobn_amd.flatten import flatten

pytestmark = pytest.mark.gpu

REJECTION, LIKELIHOOD = 1, 2


# ----------------------------------------------------------------------------------------------------------- networks

def _tables(rng, card, parents, zeros=True):
    """Unnormalised positive tables; every third row gets a zero at the start, the middle or the end (in turn), some rows two
    trailing zeros - never a whole row."""
    out = []
    for v, p in enumerate(parents):
        k = int(card[v])
        t = rng.random([int(card[u]) for u in p] + [k]) * 2 + 0.05
        rows = t.reshape(-1, k)
        if zeros and k > 1:
            for r in range(0, len(rows), 3):
                rows[r, (0, k // 2, k - 1)[(r // 3) % 3]] = 0.0
                if k > 3 and (r // 3) % 4 == 3:
                    rows[r, -2:] = 0.0
        assert (rows.sum(axis=1) > 0).all()
        out.append(t)
    return out


def _random_net(card, parents, seed, zeros=True):
    return sc.make_net(card, parents, _tables(np.random.default_rng(seed), card, parents, zeros))


def _grid_net(R, C, K, seed):
    """Row-major grid, parents = top and left neighbour."""
    parents = [([v - C] if v >= C else []) + ([v - 1] if v % C else []) for v in range(R * C)]
    return _random_net([K] * (R * C), parents, seed)


def _chain_net(n, seed):
    return _random_net([2] * n, [[v - 1] if v else [] for v in range(n)], seed)


def _example(name):
    spec = next(n for n in gu.load("examples.json") if n["spec"]["name"] == name)["spec"]
    return sc.from_flat(flatten(netspec.build(spec, sorobn_amd.BayesNet)))


def _dag():
    """A network of tests/golden/random_dags.json with a node of five children and nodes of three parents (normalised rows, exact
    zeros, missing rows = zeros of the dense table)."""
    spec = next(e["spec"] for e in gu.load("random_dags.json") if e["spec"]["name"] == "dag2")
    net = sc.from_flat(flatten(netspec.build(spec, sorobn_amd.BayesNet)))
    assert max(len(c) for c in net.children) >= 4 and max(len(s) for s in net.scope) - 1 >= 3
    return net


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


def _tree_net():
    """Cards 17 and 255: the `card > 16` update form (variables 0, 1, 3), beside two small ones."""
    return _random_net([17, 255, 3, 17, 2], [[], [0], [1], [0], [3]], seed=41)


GIBBS_CASES = {
    # name: (network, query, evidence, cycle)
    "grid3x3k8": (lambda: _grid_net(3, 3, 8, 51), [4, 8], {}, None),                                  # 8-lane / FAST, no evidence
    "grid4x5k3": (lambda: _grid_net(4, 5, 3, 52), [12], {0: 1, 19: 2, 7: 0}, None),                   # three evidence variables
    "grid4x5k3-reverse-cycle": (lambda: _grid_net(4, 5, 3, 52), [9, 10], {0: 1}, "reverse"),           # a caller's cycle
    "dag-5-children-3-parents": (_dag, [4, 9], {1: 1}, None),                                          # generic `card <= 16` form
    "dag-reverse-cycle": (_dag, [10, 0, 5], {}, "reverse"),
    "tree-17-255": (_tree_net, [1], {4: 1}, None),                                                     # `card > 16` form, 255 cells
    "tree-17-255-two-queries": (_tree_net, [3, 0], {}, "reverse"),
    "asia-five-queries": (lambda: _example("asia"), [0, 2, 4, 5, 7], {}, None),                        # n_q > 4, a deterministic CPT
    "asia-five-queries-evidence": (lambda: _example("asia"), [6, 1, 3, 0, 5], {2: 1, 4: 0, 7: 1}, "reverse"),
    "grid-five-queries": (lambda: _grid_net(3, 3, 2, 53), [8, 0, 4, 2, 6], {5: 1}, None),              # n_q > 4 in the 8-lane / FAST forms
}


@pytest.mark.parametrize("name", list(GIBBS_CASES))
def test_gibbs_histograms_equal_the_twin(name):
    make, q, ev, cycle = GIBBS_CASES[name]
    net = make()
    if cycle == "reverse":
        cycle = [v for v in range(len(net.card) - 1, -1, -1) if v not in ev]
    eng = _engine(net)
    counts = _gibbs_all_forms(eng, net, q, ev, 61, 257, seed=(3 << 32) | 9, cycle=cycle)
    assert (counts > 0).sum() > 1
    _gibbs_all_forms(eng, net, q, ev, 9, 40, seed=2, cycle=cycle, chain_first=7)
    _gibbs_all_forms(eng, net, q, ev, 9, 40, seed=2, cycle=cycle, chain_first=(1 << 32) + 5)  # the high word of the chain index


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
