"""EM on the device (BayesNet.fit_em, mibn_expect_batch: expect_kernel) against the brute-force twin of tests/em_check.py on small
networks - one E-step through the entry point alone (tiny and planned path, NOPRUNE), bitwise repeatability, complete data = fit,
five iterations, a latent column - and against invariants on the C3 grid; no effect on posterior queries; errors.

Observed on one MI355X (the bounds are the tests', not these): acc against the twin at most 1.9e-12 per cell, p_out relative 1.4e-15,
CPTs after five iterations 1.3e-15 - DESIGN section 12."""
import numpy as np
import pandas as pd
import pytest

import em_check as em
import golden_util as gu
import netspec
import sorobn_amd
from sorobn_amd import _capi, learning
from sorobn_amd.flatten import flatten

pytestmark = pytest.mark.gpu

N_ROWS = 500


def _dense(spec):
    """(bn, card, scopes, thetas, domains) of a golden network with every CPT made a dense distribution: absent or all-zero
    parent rows become uniform, every row is renormalised; variable ids follow bn.nodes."""
    bn = netspec.build(spec, sorobn_amd.BayesNet)
    f = flatten(bn)
    card = [int(c) for c in f.card]
    scopes = [[int(u) for u in sc] for sc in f.scope]
    thetas = []
    for v in range(len(card)):
        rows = np.array(f.values[f.value_off[v]:f.value_off[v + 1]], np.float64).reshape(-1, card[v])
        rows[rows.sum(axis=1) <= 0] = 1.0
        thetas.append((rows / rows.sum(axis=1, keepdims=True)).reshape(-1))
    return bn, card, scopes, thetas, [list(d) for d in f.domains]


def _specs():
    """sprinkler, asia, alarm and the first two random DAGs with mixed cardinalities, every CPT present, a joint of at most
    2^16 states and families the structure itself describes (scope = parents + node)."""
    out = [e["spec"] for name in ("sprinkler", "asia", "alarm") for e in gu.load("examples.json") if e["spec"]["name"] == name]
    n_dags = 0
    for e in gu.load("random_dags.json"):
        bn = netspec.build(e["spec"], sorobn_amd.BayesNet)
        f = flatten(bn)
        ok = (not f.missing and len(set(f.card.tolist())) > 1 and np.prod([float(c) for c in f.card]) <= 2 ** 16
              and list(f.names) == list(bn.nodes)
              and all(list(sc) == [f.id[p] for p in bn.parents.get(n, [])] + [v] for v, (n, sc) in enumerate(zip(f.names, f.scope))))
        if ok and n_dags < 2:
            out.append(e["spec"])
            n_dags += 1
    assert len(out) == 5, [s["name"] for s in out]
    return out


def _data(card, scopes, thetas, seed, fraction=0.2):
    rng = np.random.default_rng(seed)
    full = em.sample_rows(card, scopes, thetas, N_ROWS, rng)
    return em.knock_out(full, fraction, rng, drop_column=len(card) // 2)


def _engine(card, scopes, thetas, **options):
    eng = _capi.Engine(0)
    for k, v in options.items():
        eng.set_option(k, v)
    scope_off = np.concatenate([[0], np.cumsum([len(s) for s in scopes])])
    value_off = np.concatenate([[0], np.cumsum([len(t) for t in thetas])])
    eng.set_network(card, scope_off, [u for s in scopes for u in s], value_off, np.concatenate(thetas))
    return eng


def _requests(card, scopes, codes):
    fam_off, strides = learning.em_family_layout(scopes, np.asarray(card))
    return learning.em_requests(codes, np.arange(len(codes)), scopes, strides, fam_off), int(fam_off[-1])


def _expect(eng, rq, acc, flags=0, part=None):
    if part is not None:
        a, b = part
        qa, qb, ea, eb = rq["q_off"][a], rq["q_off"][b], rq["e_off"][a], rq["e_off"][b]
        return eng.expect_batch(rq["q_off"][a:b + 1] - qa, rq["q_vars"][qa:qb], rq["e_off"][a:b + 1] - ea, rq["e_vars"][ea:eb],
                                rq["e_codes"][ea:eb], rq["acc_base"][a:b], rq["acc_stride"][qa:qb], acc, flags=flags)
    return eng.expect_batch(rq["q_off"], rq["q_vars"], rq["e_off"], rq["e_vars"], rq["e_codes"], rq["acc_base"], rq["acc_stride"],
                            acc, flags=flags)


def _install(bn, thetas, domains):
    names = list(bn.nodes)
    doms = {n: pd.Index(domains[v]) for v, n in enumerate(names)}
    bn.P = {n: learning._em_series(n, bn.parents.get(n, []), doms, thetas[v]) for v, n in enumerate(names)}
    return bn.prepare()


def _frame(codes, names, domains, drop_empty=True):
    X = pd.DataFrame({n: [domains[j][c] if c >= 0 else None for c in codes[:, j]] for j, n in enumerate(names)}, dtype=object)
    return X.drop(columns=[n for j, n in enumerate(names) if drop_empty and (codes[:, j] < 0).all()])


def _thetas_of(bn):
    f = flatten(bn)
    return [np.asarray(f.values[a:b], np.float64) for a, b in zip(f.value_off[:-1], f.value_off[1:])]


def _complete(card, scopes, codes):
    """Hard counts of the (row, family) pairs without a missing member - what fit_em counts with the count kernel."""
    out = []
    for sc in scopes:
        rows = codes[(codes[:, sc] >= 0).all(axis=1)][:, sc]
        cells = int(np.prod([card[u] for u in sc]))
        out.append(np.bincount(np.ravel_multi_index(rows.T, [card[u] for u in sc]), minlength=cells).astype(np.float64))
    return np.concatenate(out)


def test_one_e_step_through_the_entry_point():
    """Test 1: acc against the twin within n_rows x 1e-9 per cell, p_out against the twin's P(e_r) at rel 1e-9 - tiny path, planned
    path (tiny = 0), each with and without MIBN_Q_NOPRUNE."""
    worst_acc = worst_p = 0.0
    for k, spec in enumerate(_specs()):
        bn, card, scopes, thetas, _ = _dense(spec)
        codes = _data(card, scopes, thetas, 100 + k)
        want, p_row = em.e_step(card, scopes, thetas, codes)
        want = np.concatenate(want) - _complete(card, scopes, codes)  # (the entry point sees the incomplete families only)
        rq, n_acc = _requests(card, scopes, codes)
        for tiny in (1, 0):
            eng = _engine(card, scopes, thetas, tiny=tiny)
            for flags in (0, _capi.Q_NOPRUNE):
                acc = np.zeros(n_acc)
                p = _expect(eng, rq, acc, flags)
                names = [s["name"] for s in eng.kernel_stats()]
                assert "expect_kernel" in names and (("tiny_kernel" in names) == bool(tiny)), (spec["name"], tiny, names)
                d_acc = float(np.max(np.abs(acc - want)))
                d_p = float(np.max(np.abs(p - p_row[rq["row"]]) / p_row[rq["row"]]))
                print(f"[em] {spec['name']} tiny={tiny} flags={flags}: {len(p)} requests, max|acc - twin| {d_acc:.3e}, max rel p {d_p:.3e}")
                worst_acc, worst_p = max(worst_acc, d_acc), max(worst_p, d_p)
                assert d_acc <= N_ROWS * 1e-9, (spec["name"], tiny, flags, d_acc)
                assert d_p <= 1e-9, (spec["name"], tiny, flags, d_p)
            eng.close()
    print(f"[em] worst over all: acc {worst_acc:.3e}, p {worst_p:.3e}")


def test_family_beyond_the_lds_image():
    """Test 1 on a family table of 4 x 3^6 = 2 916 cells (beyond expect_kernel's 2 048-cell LDS image): requests whose targets span
    more than the image take the global path, the others the slabs - same bounds, and bit for bit the same on a second run."""
    rng = np.random.default_rng(21)
    card, scopes = [3] * 6 + [4], [[v] for v in range(6)] + [[0, 1, 2, 3, 4, 5, 6]]
    thetas = [rng.dirichlet(np.ones(3)) for _ in range(6)] + [rng.dirichlet(np.ones(4), size=3 ** 6).reshape(-1)]
    codes = em.knock_out(em.sample_rows(card, scopes, thetas, N_ROWS, rng), 0.2, rng)
    want, p_row = em.e_step(card, scopes, thetas, codes)
    want = np.concatenate(want) - _complete(card, scopes, codes)
    rq, n_acc = _requests(card, scopes, codes)
    fam_off, strides = learning.em_family_layout(scopes, np.asarray(card))
    span = np.add.reduceat((np.asarray(card)[rq["q_vars"]] - 1) * rq["acc_stride"], rq["q_off"][:-1][np.diff(rq["q_off"]) > 0])
    assert (span >= 2048).any() and (span < 2048).any()
    for tiny in (1, 0):
        eng = _engine(card, scopes, thetas, tiny=tiny)
        acc, again = np.zeros(n_acc), np.zeros(n_acc)
        p = _expect(eng, rq, acc)
        assert np.array_equal(_expect(eng, rq, again).view(np.uint64), p.view(np.uint64))
        assert np.array_equal(acc.view(np.uint64), again.view(np.uint64))
        d_acc = float(np.max(np.abs(acc - want)))
        d_p = float(np.max(np.abs(p - p_row[rq["row"]]) / p_row[rq["row"]]))
        print(f"[em] 2916-cell family tiny={tiny}: {len(p)} requests, max|acc - twin| {d_acc:.3e}, max rel p {d_p:.3e}")
        assert d_acc <= N_ROWS * 1e-9 and d_p <= 1e-9


@pytest.mark.parametrize("tiny", [1, 0])
def test_repeatable_bit_for_bit(tiny):
    """Test 2: the same call three times and once more on an engine with threads = 1: acc and p_out equal bit for bit; the batch
    split into two chained calls agrees within test 1's bound."""
    spec = _specs()[-1]
    bn, card, scopes, thetas, _ = _dense(spec)
    codes = _data(card, scopes, thetas, 7)
    rq, n_acc = _requests(card, scopes, codes)
    runs = []
    eng = _engine(card, scopes, thetas, tiny=tiny)
    single = _engine(card, scopes, thetas, tiny=tiny, threads=1)
    for e in (eng, eng, eng, single):
        acc = np.zeros(n_acc)
        p = _expect(e, rq, acc)
        runs.append((acc, p))
    for acc, p in runs[1:]:
        assert np.array_equal(acc.view(np.uint64), runs[0][0].view(np.uint64))
        assert np.array_equal(p.view(np.uint64), runs[0][1].view(np.uint64))
    B = len(rq["acc_base"])
    acc = np.zeros(n_acc)
    p1 = _expect(eng, rq, acc, part=(0, B // 2))
    p2 = _expect(eng, rq, acc, part=(B // 2, B))
    assert np.array_equal(np.concatenate([p1, p2]).view(np.uint64), runs[0][1].view(np.uint64))
    assert float(np.max(np.abs(acc - runs[0][0]))) <= N_ROWS * 1e-9


def test_complete_data_is_fit():
    """Test 3: no missing cell, prior_count = 0, one iteration from any init: the CPTs equal fit(X)'s - same index, values within
    1e-12.  (EM learns dense CPTs and fit drops the cells it never saw, so the data - 4 000 rows of a 3 x 3 grid with three states -
    are asserted to show every cell of every family.)"""
    spec = netspec.grid_spec(3, 3, 3, seed=2)
    bn, card, scopes, thetas, domains = _dense(spec)
    smooth = [0.5 * t + 0.5 / card[v] for v, t in enumerate(thetas)]  # (sampled from flattened CPTs: no cell is rare)
    codes = em.sample_rows(card, scopes, smooth, 4000, np.random.default_rng(3))
    X = _frame(codes, list(bn.nodes), domains).astype("int64")
    ref = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    ref.prior_count = None
    ref.fit(X)
    assert all(len(ref.P[n]) == len(t) for n, t in zip(bn.nodes, thetas)), "a family cell was never observed"
    for init in ("uniform", "counts", "current"):
        got = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
        got.fit_em(X, n_iter=1, prior_count=0.0, init=init)
        for n in bn.nodes:
            assert got.P[n].index.equals(ref.P[n].index), (init, n)
            assert list(got.P[n].index.names) == list(ref.P[n].index.names)
            assert float(np.max(np.abs(got.P[n].to_numpy() - ref.P[n].to_numpy()))) <= 1e-12, (init, n)


def test_em_is_em():
    """Test 4: five iterations on test 1's data with prior_count = 0: CPTs against the twin iterated five times from the same start
    within 1e-9; em_log_likelihood_[k] against log_likelihood(X) under iteration k's parameters at rel 1e-9; non-decreasing up to
    1e-9 x |ll|."""
    for k, spec in enumerate(_specs()):
        base, card, scopes, thetas, domains = _dense(spec)
        codes = _data(card, scopes, thetas, 100 + k)
        names = list(base.nodes)
        X = _frame(codes, names, domains)
        want, lls, _ = em.em(card, scopes, thetas, codes, 5)
        bn = _install(netspec.build(spec, sorobn_amd.BayesNet).use_device(0), thetas, domains)
        bn.fit_em(X, n_iter=5, tol=0.0, prior_count=0.0, init="current")
        assert bn.em_iterations_ == 5
        d = max(float(np.max(np.abs(g - w))) for g, w in zip(_thetas_of(bn), want))
        print(f"[em] {spec['name']}: five iterations, max|theta - twin| {d:.3e}, ll {bn.em_log_likelihood_}")
        assert d <= 1e-9, (spec["name"], d)
        assert np.allclose(bn.em_log_likelihood_, lls, rtol=1e-9, atol=0)
        step = _install(netspec.build(spec, sorobn_amd.BayesNet).use_device(0), thetas, domains)
        for it in range(5):  # the existing path: log_likelihood under iteration it's parameters
            ll = step.log_likelihood(X)
            assert abs(ll - bn.em_log_likelihood_[it]) <= 1e-9 * abs(ll), (spec["name"], it)
            step.fit_em(X, n_iter=1, prior_count=0.0, init="current")
        got = bn.em_log_likelihood_
        assert all(b >= a - 1e-9 * abs(a) for a, b in zip(got, got[1:])), got


def test_latent_column():
    """Test 5: a two-component naive-Bayes net whose class is never observed, init='current' from asymmetric CPTs: the
    log-likelihood rises and everything matches the twin."""
    rng = np.random.default_rng(12)
    card, scopes = [2, 2, 3, 2, 2], [[0], [0, 1], [0, 2], [0, 3], [0, 4]]
    true = [np.array([0.35, 0.65])] + [rng.dirichlet(np.ones(card[v]) * 0.7, size=2).reshape(-1) for v in range(1, 5)]
    codes = em.sample_rows(card, scopes, true, 600, rng)
    codes[:, 0] = -1
    start = [np.array([0.6, 0.4])] + [rng.dirichlet(np.ones(card[v]) * 2.0, size=2).reshape(-1) for v in range(1, 5)]
    names = ["c", "x1", "x2", "x3", "x4"]
    domains = [["a", "b"], [0, 1], ["h", "l", "m"], [False, True], [0, 1]]
    bn = sorobn_amd.BayesNet(("c", ["x1", "x2", "x3", "x4"])).use_device(0)
    assert bn.nodes == names
    _install(bn, start, domains)
    X = _frame(codes, names, domains)
    assert "c" not in X.columns
    bn.fit_em(X, n_iter=8, tol=0.0, init="current")
    want, lls, _ = em.em(card, scopes, start, codes, 8)
    assert np.allclose(bn.em_log_likelihood_, lls, rtol=1e-9, atol=0)
    assert bn.em_log_likelihood_[-1] > bn.em_log_likelihood_[0]
    assert max(float(np.max(np.abs(g - w))) for g, w in zip(_thetas_of(bn), want)) <= 1e-9
    with pytest.raises(ValueError, match="'c'"):
        sorobn_amd.BayesNet(("c", ["x1", "x2", "x3", "x4"])).use_device(0).fit_em(X, n_iter=1)


@pytest.fixture(scope="module")
def grid():
    entry = gu.load("grid10x10.json")
    spec = gu.grid_spec_from_recipe(entry)
    return spec, netspec.build(spec, sorobn_amd.BayesNet).use_device(0)


def test_c3_grid_invariants(grid):
    """Test 6: the C3 grid (10 x 10, K = 4), 2 000 sampled rows, 15 % of the cells missing, two iterations through the planned
    kernels.  Every family's expected counts sum to n_rows within n_rows x 1e-9; for ten fixed nodes the family table summed over the
    parents equals the sum over rows of the node's posterior from query_frame (rel 1e-9); the per-iteration log-likelihood equals
    log_likelihood(X) and does not decrease."""
    spec, src = grid
    n = 2000
    src.seed = 5
    X = src.sample(n).astype(object)
    rng = np.random.default_rng(15)
    X = X.mask(rng.random(X.shape) < 0.15)
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    lls = []
    for it in range(2):
        ll = bn.log_likelihood(X)
        marg = {}
        if it == 0:
            for v in range(0, 100, 10):
                node = f"{v + v // 10:03d}"
                gone = X[node].isna().to_numpy()
                post = bn.query_frame(node, events=X[gone].drop(columns=[node]))
                seen = X[node][~gone].astype(int).value_counts()
                marg[node] = post.sum(axis=0).to_numpy() + np.array([seen.get(k, 0) for k in post.columns])
        bn.fit_em(X, n_iter=1, prior_count=0.0, init="current")
        assert abs(bn.em_log_likelihood_[0] - ll) <= 1e-9 * abs(ll), (it, bn.em_log_likelihood_, ll)
        lls.append(bn.em_log_likelihood_[0])
        for node, c in bn._counts.items():
            assert abs(float(c.sum()) - n) <= n * 1e-9, (node, float(c.sum()))
        for node, want in marg.items():
            got = bn._counts[node].groupby(level=node).sum().to_numpy() if bn.parents.get(node) else bn._counts[node].to_numpy()
            assert np.max(np.abs(got - want) / want) <= 1e-9, (node, got, want)
    print(f"[em] C3 grid: log-likelihood {lls}")
    assert lls[1] >= lls[0] - 1e-9 * abs(lls[0])


def test_nothing_else_moved(grid):
    """Test 7: posterior queries before and after a fit_em on another net object of the same device: bit for bit; the kernel
    statistics after an expect_batch name expect_kernel."""
    spec, bn = grid
    q, ev, cs = netspec.c3_requests(100, 4, 512, 4, seed=9)
    reqs = [((f"{a:03d}",), {f"{v:03d}": int(c) for v, c in zip(vs, cc)}) for a, vs, cc in zip(q.tolist(), ev.tolist(), cs.tolist())]
    before = bn.query_many(reqs).out.copy()
    other = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    other.seed = 3
    X = other.sample(200).astype(object)
    X = X.mask(np.random.default_rng(1).random(X.shape) < 0.1)
    other.fit_em(X, n_iter=1, init="current")
    after = bn.query_many(reqs).out
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64))
    # and on the SAME engine: an expect call between two identical query calls
    eng = bn.backend.engine
    rq, n_acc = _requests([4] * 100, [list(sc) for sc in bn.backend.flat.scope], np.full((3, 100), -1, np.int32))
    _expect(eng, rq, np.zeros(n_acc))
    names = [s["name"] for s in eng.kernel_stats()]
    assert "expect_kernel" in names and "tiny_kernel" not in names, names
    assert np.array_equal(bn.query_many(reqs).out.view(np.uint64), before.view(np.uint64))


def test_errors():
    """Test 8: a target outside acc -> MIBN_E_ARG with no launch; too many missing members of one family -> ValueError naming the
    node; a zero-probability row -> a -inf entry and no NaN in the CPTs."""
    card, scopes = [2, 2], [[0], [0, 1]]
    thetas = [np.array([0.6, 0.4]), np.array([1.0, 0.0, 0.2, 0.8])]
    eng = _engine(card, scopes, thetas)
    one = dict(q_off=[0, 1], q_vars=[0], e_off=[0, 1], e_vars=[1], e_codes=[0])
    for base, stride in ((5, 1), (4, 2), (0, -1), (-1, 1), (0, 6)):
        with pytest.raises(_capi.MibnError) as err:
            eng.expect_batch(acc_base=[base], acc_stride=[stride], acc=np.zeros(6), **one)
        assert err.value.code == _capi.E_ARG, (base, stride)
    assert eng.total_stats()["n_launches"] == 0
    acc = np.zeros(6)
    p = eng.expect_batch(acc_base=[4], acc_stride=[1], acc=acc, **one)
    assert abs(p[0] - 0.68) <= 1e-15 and np.allclose(acc, [0, 0, 0, 0, 0.6 / 0.68, 0.08 / 0.68], rtol=1e-15, atol=0)
    # ten members, all missing in one row
    parents = [f"p{k}" for k in range(9)]
    wide = sorobn_amd.BayesNet((parents, "child")).use_device(0)
    X = pd.DataFrame([{n: 0 for n in parents + ["child"]}, {n: 1 for n in parents + ["child"]}, {n: None for n in parents + ["child"]}],
                     dtype=object)
    with pytest.raises(ValueError, match="child"):
        wide.fit_em(X, n_iter=1, init="uniform")
    # P(b = 1 | a = 0) = 0: the row (a = 0, b = 1) has probability zero
    bn = _install(sorobn_amd.BayesNet(("a", "b")).use_device(0), thetas, [[0, 1], [0, 1]])
    X = pd.DataFrame({"a": [0, 0, 1, None, 1, None], "b": [1, 0, 1, 0, None, 1]}, dtype=object)
    bn.fit_em(X, n_iter=2, tol=0.0, init="current")
    assert bn.em_log_likelihood_[0] == -np.inf
    assert all(np.isfinite(P.to_numpy()).all() for P in bn.P.values())
    codes = np.array([[0, 1], [0, 0], [1, 1], [-1, 0], [1, -1], [-1, 1]])
    want, lls, _ = em.em(card, scopes, thetas, codes, 2)
    assert max(float(np.max(np.abs(g - w))) for g, w in zip(_thetas_of(bn), want)) <= 1e-12
