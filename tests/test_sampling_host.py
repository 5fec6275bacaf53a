"""The twin of the sampling / Gibbs Philox stream (tests/sample_check.py) has to be right on its own before the kernels are
held to it (tests/test_sampling_twin.py): Philox known answers, the uniform's bit layout, the forward walk against the
enumerated joint, likelihood weighting against its enumerated limit, the Gibbs chain against the enumerated posterior, and
the invariants the GPU tests lean on.  No GPU, no reference."""
import itertools

import numpy as np
from scipy.stats import chi2

import golden_util as gu
import netspec
import sample_check as sc
import sorobn_amd
from sorobn_amd.flatten import flatten
from test_sampling import llh_weighting_limit

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _philox_scalar(ctr, key):
    """Philox4x32-10 on Python ints, straight from the Random123 description."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _spec(name):
    return next(n for n in gu.load("examples.json") if n["spec"]["name"] == name)["spec"]


def _example(name):
    bn = netspec.build(_spec(name), sorobn_amd.BayesNet)
    return bn, flatten(bn)


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert _philox_scalar(ctr, key) == want
        got = sc.philox4x32_10([np.array([c], np.uint32) for c in ctr], [np.array([k], np.uint32) for k in key])
        assert tuple(int(g[0]) for g in got) == want
    # vectorised = element by element, counters and keys that differ per element
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(4, 257), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(2, 257), dtype=np.uint64)
    got = sc.philox4x32_10(list(ctr), list(key))
    for j in range(257):
        assert tuple(int(g[j]) for g in got) == _philox_scalar([int(c) for c in ctr[:, j]], [int(k) for k in key[:, j]])


def test_philox_uniform_bits():
    """counter = (i lo, i hi, stream, 0); the result is (((c0 << 21) ^ (c1 >> 11)) & (2^53 - 1)) * 2^-53, in [0, 1)."""
    i = np.array([0, 1, 63, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 12345, 2 ** 64 - 1], np.uint64)
    for stream, k0, k1 in ((0, 0, 0), (1, 5, 0x85EBCA6B), (2 + 254, 0xFFFFFFFF, 0xFFFFFFFF)):
        got = sc.philox_uniform(i, stream, k0, k1)
        for ii, g in zip(i.tolist(), got.tolist()):
            c = _philox_scalar((ii & 0xFFFFFFFF, ii >> 32, stream, 0), (k0, k1))
            m = ((c[0] << 21) ^ (c[1] >> 11)) & (2 ** 53 - 1)
            assert g == m / 2 ** 53 and 0.0 <= g < 1.0
    assert sc.uniform_from_words(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53  # the largest value stays below 1
    assert sc.uniform_from_words(0, 0) == 0.0
    u = sc.philox_uniform(np.arange(100_000, dtype=np.uint64), 2, 7, 9)
    assert u.min() >= 0.0 and u.max() < 1.0
    # 100 000 uniforms: the mean is within 6 sigma (sigma = sqrt(1 / 12 / n)) of 1/2
    assert abs(u.mean() - 0.5) < 6 * np.sqrt(1 / 12 / len(u))


def test_forward_twin_vs_enumerated_joint():
    """200 000 forward samples of the twin against the enumerated joint: Pearson chi-square of the joint-state histogram, cells of
    expected count below 5 pooled into one.  Significance level 1e-3; degrees of freedom = cells after pooling - 1 (printed)."""
    n = 200_000
    alpha = 1e-3
    for name, seed in (("sprinkler", 1), ("asia", 2)):
        _, f = _example(name)
        net = sc.from_flat(f)
        p = sc.joint(net).reshape(-1)
        assert abs(p.sum() - 1.0) < 1e-12
        states, lik = sc.forward(net, n, seed)
        cell = np.ravel_multi_index(tuple(states.T.astype(np.int64)), [int(c) for c in net.card])
        obs = np.bincount(cell, minlength=len(p)).astype(np.float64)
        assert obs[p == 0].sum() == 0  # a state of probability zero is never drawn
        assert np.max(np.abs(lik - p[cell])) <= 1e-15  # the likelihood of an unclamped sample is its joint probability
        exp = n * p
        small = exp < 5
        o = np.concatenate([obs[~small], [obs[small].sum()]])
        e = np.concatenate([exp[~small], [exp[small].sum()]])
        if e[-1] == 0:
            o, e = o[:-1], e[:-1]
        dof = len(e) - 1
        stat = float(((o - e) ** 2 / e).sum())
        crit = float(chi2.ppf(1 - alpha, dof))
        print(f"{name}: chi2 = {stat:.1f}, dof = {dof}, critical value at {alpha} = {crit:.1f}")
        assert dof >= 3 and stat < crit, (name, stat, dof, crit)


def test_likelihood_twin_vs_enumerated_limit():
    """The twin's likelihood-weighting estimate (mean likelihood per query cell, normalised) against llh_weighting_limit.
    Bound: 5 sigma of the delta-method standard error of m_k / sum(m), from the per-cell sample deviations of this run."""
    n = 200_000
    for name, q, ev in (("sprinkler", ("Rain",), {"Sprinkler": True}),
                        ("asia", ("Lung cancer", "Bronchitis"), {"Smoker": True, "Dispnea": False})):
        bn, f = _example(name)
        net = sc.from_flat(f)
        qv = [f.id[x] for x in q]
        evc = {f.id[k]: f.code_of(f.id[k], v) for k, v in ev.items()}
        counts, wsum = sc.likelihood(net, qv, evc, n, seed=3)
        assert counts.sum() == n and (counts > 0).all()
        mean = wsum / counts
        est = mean / mean.sum()
        lim = llh_weighting_limit(bn, q, ev)
        want = np.array([lim[key] for key in itertools.product(*[range(int(net.card[v])) for v in qv])])
        # standard error of every cell's mean, then of the normalised value: d est_k = sum_j (delta_kj - est_k) / S * d m_j
        states, lik = sc.forward(net, n, 3, clamp=evc)
        cell, cells = sc._cells(net, qv, states)
        se = np.array([lik[cell == k].std(ddof=1) / np.sqrt(counts[k]) for k in range(cells)])
        S = mean.sum()
        jac = (np.eye(cells) - est[:, None]) / S
        sigma = np.sqrt((jac ** 2 * se[None, :] ** 2).sum(axis=1))
        print(name, "max |est - limit| =", np.max(np.abs(est - want)), "5 sigma =", 5 * sigma)
        assert (np.abs(est - want) <= 5 * sigma).all(), (name, est, want, sigma)
        assert (5 * sigma < 0.02).all()  # the bound itself means something


def _grid_case():
    f = flatten(netspec.build(netspec.grid_spec(2, 3, 3, seed=4), sorobn_amd.BayesNet))
    assert (f.values > 0).all()
    return sc.from_flat(f)


def test_gibbs_twin_vs_enumerated_posterior():
    """256 chains x 1 000 updates on a 2x3 K=3 grid with strictly positive CPTs, pooled, against the enumerated posterior.
    N = 256 000 recorded states; with an autocorrelation time of at most 50 updates (ten sweeps of the five free variables) a
    cell's frequency has sigma <= sqrt(0.25 * 50 / N) = 0.0070: the bound is 6 sigma = 0.042, as test_gibbs_matches_exact_posterior
    argues for the kernel."""
    net = _grid_case()
    n_chains, n_iter, tau = 256, 1000, 50
    bound = 6 * np.sqrt(0.25 * tau / (n_chains * n_iter))
    p = sc.joint(net)
    for q, ev in (([4], {0: 1}), ([5, 2], {1: 2})):
        counts = sc.gibbs(net, q, ev, n_chains, n_iter, seed=11)
        assert counts.sum() == n_chains * n_iter
        sub = p[tuple(ev.get(v, slice(None)) for v in range(6))]
        free = [v for v in range(6) if v not in ev]
        marg = sub.sum(axis=tuple(i for i, v in enumerate(free) if v not in q))
        kept = [v for v in free if v in q]
        marg = np.transpose(marg, [kept.index(v) for v in q]).reshape(-1)
        marg = marg / marg.sum()
        err = float(np.max(np.abs(counts / counts.sum() - marg)))
        print(q, ev, "max |freq - posterior| =", err, "bound =", bound)
        assert err < bound


def test_twin_invariants():
    net = _grid_case()
    # shards of one Gibbs stream sum to the whole
    whole = sc.gibbs(net, [4, 1], {0: 2}, 21, 40, seed=(7 << 32) | 5)
    parts = sum(sc.gibbs(net, [4, 1], {0: 2}, hi - lo, 40, seed=(7 << 32) | 5, chain_first=lo) for lo, hi in ((0, 8), (8, 9), (9, 21)))
    assert np.array_equal(whole, parts) and whole.sum() == 21 * 40
    # the high word of the seed and the chain index both reach the key
    assert not np.array_equal(whole, sc.gibbs(net, [4, 1], {0: 2}, 21, 40, seed=5))
    assert not np.array_equal(whole, sc.gibbs(net, [4, 1], {0: 2}, 21, 40, seed=(7 << 32) | 5, chain_first=1))
    # a caller's cycle is followed
    assert not np.array_equal(whole, sc.gibbs(net, [4, 1], {0: 2}, 21, 40, seed=(7 << 32) | 5, cycle=[5, 4, 3, 2, 1]))
    # a clamp is honoured, and the free variables keep their uniforms (counter = sample, stream = 2 + variable)
    free, _ = sc.forward(net, 500, 9)
    states, lik = sc.forward(net, 500, 9, clamp={0: 2, 4: 1})
    assert (states[:, 0] == 2).all() and (states[:, 4] == 1).all()
    same = (free[:, 0] == 2)
    assert same.any() and np.array_equal(states[same][:, [1, 2]], free[same][:, [1, 2]])
    assert not np.array_equal(sc.forward(net, 500, 9 + (1 << 32))[0], free)
    # a zero row: the draw falls through to card - 1 and the likelihood is 0
    tabs = [np.array([0.5, 0.5]), np.array([[0.0, 0.0, 0.0], [0.2, 0.0, 0.8]]), np.array([[1.0, 1.0], [1.0, 1.0], [0.5, 1.5]])]
    z = sc.make_net([2, 3, 2], [[], [0], [1]], tabs)
    states, lik = sc.forward(z, 64, 0, clamp={0: 0})
    assert (states[:, 1] == 2).all() and (lik == 0.0).all()
    states, lik = sc.forward(z, 64, 0, clamp={0: 1})
    assert set(states[:, 1].tolist()) == {0, 2} and (lik > 0).all()  # a zero in the middle of a row is never drawn
    # rejection counts what agrees with the event; likelihood weighting counts everything
    assert sc.rejection(z, [1], {0: 1}, 1000, 3).sum() == int((sc.forward(z, 1000, 3)[0][:, 0] == 1).sum())
    counts, wsum = sc.likelihood(z, [1], {0: 0}, 1000, 3)
    assert counts.tolist() == [0, 0, 1000] and wsum.tolist() == [0.0, 0.0, 0.0]
    # a Gibbs update without mass keeps the state; the `last` rule never picks a zero-weight state
    w = sc.gibbs_weights(z, 1, np.array([[0, 1, 0], [1, 0, 0]], np.uint8))
    assert w[0].tolist() == [0.0, 0.0, 0.0] and w[1].tolist() == [0.2, 0.0, 0.8 * 0.5]
    assert sc.gibbs(z, [1], {0: 0}, 8, 10, seed=1).tolist() == [0, 0, 80]
