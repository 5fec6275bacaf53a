"""EM on the CPU (no GPU needed): the request builder of the E-step against a plain loop over rows, the sub-batch cut, the M-step on
hand-made counts, the brute-force twin (tests/em_check.py) against a hand-computed case, fit_em's host logic end to end over numpy
TEST DOUBLES of the two engine calls it makes (never on the product path), argument errors before any engine, the exported symbol."""
import numpy as np
import pandas as pd
import pytest

import em_check as em
import golden_util as gu
import netspec
import sorobn_amd
from sorobn_amd import _capi, learning


def _random_net(rng, V=6, max_parents=2):
    card = rng.integers(2, 5, size=V).astype(np.int32)
    scopes = [sorted(rng.choice(v, size=min(v, int(rng.integers(0, max_parents + 1))), replace=False).tolist()) + [v] for v in range(V)]
    thetas = []
    for v, sc in enumerate(scopes):
        rows = int(np.prod([card[u] for u in sc[:-1]], dtype=np.int64))
        thetas.append(rng.dirichlet(np.ones(card[v]), size=rows).reshape(-1))
    return card, scopes, thetas


def _loop_requests(codes, rows, scopes, strides, fam_off):
    """The E-step's requests by a plain loop: family-major, rows in the given order, then one empty-query request per row that
    needs no other."""
    reqs = []
    covered = set()
    for v, sc in enumerate(scopes):
        for r in rows:
            miss = [k for k, u in enumerate(sc) if codes[r, u] < 0]
            if not miss:
                continue
            covered.add(int(r))
            base = int(fam_off[v]) + sum(int(codes[r, u]) * int(strides[v][k]) for k, u in enumerate(sc) if codes[r, u] >= 0)
            ev = [u for u in range(codes.shape[1]) if codes[r, u] >= 0]
            reqs.append((int(r), [sc[k] for k in miss], [int(strides[v][k]) for k in miss], base, ev, [int(codes[r, u]) for u in ev]))
    for r in rows:
        if int(r) not in covered:
            ev = [u for u in range(codes.shape[1]) if codes[r, u] >= 0]
            reqs.append((int(r), [], [], 0, ev, [int(codes[r, u]) for u in ev]))
    return reqs


def test_request_builder_against_a_loop_over_rows():
    rng = np.random.default_rng(5)
    for trial in range(6):
        card, scopes, thetas = _random_net(rng, V=int(rng.integers(3, 8)))
        fam_off, strides = learning.em_family_layout(scopes, card)
        assert [int(fam_off[v + 1] - fam_off[v]) for v in range(len(card))] == [len(t) for t in thetas]
        codes = em.sample_rows(card, scopes, thetas, 40, rng)
        codes = em.knock_out(codes, [0.0, 0.2, 0.5, 0.9, 0.3, 1.0][trial], rng)
        rows = rng.permutation(40)[:33]
        got = learning.em_requests(codes, rows, scopes, strides, fam_off)
        want = _loop_requests(codes, rows, scopes, strides, fam_off)
        assert len(got["q_off"]) - 1 == len(want) == len(got["e_off"]) - 1 == len(got["acc_base"]) == len(got["row"])
        for b, (r, q, st, base, ev, ec) in enumerate(want):
            qa, qb = got["q_off"][b], got["q_off"][b + 1]
            ea, eb = got["e_off"][b], got["e_off"][b + 1]
            assert got["row"][b] == r
            assert got["q_vars"][qa:qb].tolist() == q and got["acc_stride"][qa:qb].tolist() == st
            assert (got["acc_base"][b] == base) or not q
            assert got["e_vars"][ea:eb].tolist() == ev and got["e_codes"][ea:eb].tolist() == ec
        assert got["q_vars"].dtype == np.int32 and got["e_vars"].dtype == np.int32 and got["acc_stride"].dtype == np.int64


def test_sub_batches_keep_patterns_together_and_respect_the_size():
    rng = np.random.default_rng(6)
    card, scopes, thetas = _random_net(rng, V=6)
    codes = em.knock_out(em.sample_rows(card, scopes, thetas, 300, rng), 0.25, rng)
    per_row = np.array([max(1, sum(any(codes[r, u] < 0 for u in sc) for sc in scopes)) for r in range(len(codes))])
    for size in (1, 7, 50, 10 ** 6):
        parts = learning.em_sub_batches(codes, scopes, size)
        order = np.concatenate(parts)
        assert sorted(order.tolist()) == list(range(300))
        assert all(per_row[p].sum() <= size or len(p) == 1 for p in parts)
        pats = [tuple((codes[r] >= 0).tolist()) for r in order]
        first = {}
        for i, p in enumerate(pats):  # the rows of a pattern are consecutive
            assert first.setdefault(p, i) == i or pats[i - 1] == p


def test_m_step_on_hand_made_counts():
    counts = np.array([3.0, 1.0, 0.0, 0.0, 2.0, 2.0])
    prev = np.array([0.5, 0.5, 0.9, 0.1, 0.3, 0.7])
    got = learning.em_mstep(counts, prev, 2)
    assert got.tolist() == [0.75, 0.25, 0.9, 0.1, 0.5, 0.5]  # the zero-mass parent row keeps its previous values
    got = learning.em_mstep(counts, prev, 2, prior_count=1.0)
    assert np.allclose(got, [4 / 6, 2 / 6, 0.5, 0.5, 0.5, 0.5], rtol=0, atol=1e-15)
    assert em.m_step([counts], [prev], [2])[0].tolist() == [0.75, 0.25, 0.9, 0.1, 0.5, 0.5]


def test_twin_against_a_hand_computed_two_node_case():
    """A -> B, binary.  P(A) = (0.6, 0.4), P(B | A) = ((0.9, 0.1), (0.2, 0.8)); rows: (A=0, B=1), (A=?, B=0), (A=1, B=?)."""
    card, scopes = [2, 2], [[0], [0, 1]]
    thetas = [np.array([0.6, 0.4]), np.array([0.9, 0.1, 0.2, 0.8])]
    codes = np.array([[0, 1], [-1, 0], [1, -1]])
    counts, p = em.e_step(card, scopes, thetas, codes)
    pb0 = 0.6 * 0.9 + 0.4 * 0.2
    a0 = 0.6 * 0.9 / pb0
    assert np.allclose(p, [0.6 * 0.1, pb0, 0.4], rtol=1e-15, atol=0)
    assert np.allclose(counts[0], [1 + a0, 1 - a0 + 1], rtol=1e-15, atol=0)
    assert np.allclose(counts[1], [a0, 1.0, 1 - a0 + 0.2, 0.8], rtol=1e-15, atol=0)
    new = em.m_step(counts, thetas, card)
    assert np.allclose(new[0], np.array([1 + a0, 2 - a0]) / 3, rtol=1e-15, atol=0)
    assert np.allclose(new[1], [a0 / (a0 + 1), 1 / (a0 + 1), (1.2 - a0) / (2 - a0), 0.8 / (2 - a0)], rtol=1e-15, atol=0)
    th, lls, _ = em.em(card, scopes, thetas, codes, 4)
    assert all(b >= a - 1e-12 for a, b in zip(lls, lls[1:]))


class NumpyCounter:
    """TEST DOUBLE for Engine.count_tables (never on the product path)."""

    def count_tables(self, codes, card, tables):
        out = []
        for t in tables:
            shape = [int(card[c]) for c in t]
            flat = np.zeros(len(codes), np.int64)
            for c in t:
                flat = flat * int(card[c]) + codes[:, c].astype(np.int64)
            out.append(np.bincount(flat, minlength=int(np.prod(shape))).astype(np.int64).reshape(shape))
        return out


class EnumerationEngine:
    """TEST DOUBLE for the engine behind a Backend (never on the product path): expect_batch by enumeration of the joint."""

    def __init__(self, device=0, planner_only=False):
        pass

    def set_network(self, card, scope_off, scope_vars, value_off, values):
        self.card = np.asarray(card, np.int32)
        scopes = [[int(u) for u in scope_vars[a:b]] for a, b in zip(scope_off[:-1], scope_off[1:])]
        self.table = em.joint(self.card, scopes, [values[a:b] for a, b in zip(value_off[:-1], value_off[1:])])

    def set_order_hints(self, hints):
        pass

    def expect_batch(self, q_off, q_vars, e_off, e_vars, e_codes, acc_base, acc_stride, acc, weight=None, flags=0):
        B = len(q_off) - 1
        p = np.zeros(B)
        for b in range(B):
            q = [int(v) for v in q_vars[q_off[b]:q_off[b + 1]]]
            ev = {int(v): int(c) for v, c in zip(e_vars[e_off[b]:e_off[b + 1]], e_codes[e_off[b]:e_off[b + 1]])}
            hidden = [v for v in range(len(self.card)) if v not in ev]
            sub = self.table[tuple(ev.get(v, slice(None)) for v in range(len(self.card)))]
            sub = sub.sum(axis=tuple(i for i, v in enumerate(hidden) if v not in q)) if hidden else sub
            kept = [v for v in hidden if v in q]
            sub = np.transpose(sub, [kept.index(v) for v in q]) if q else sub
            p[b] = sub.sum()
            if q and p[b] > 0:
                st = acc_stride[q_off[b]:q_off[b + 1]]
                idx = np.indices(sub.shape).reshape(len(q), -1)
                acc[acc_base[b] + (idx * np.asarray(st)[:, None]).sum(axis=0)] += (sub / p[b]).reshape(-1)
        return p


def _frame(codes, names, domains):
    return pd.DataFrame({n: [domains[j][c] if c >= 0 else None for c in codes[:, j]] for j, n in enumerate(names)}, dtype=object)


def _structure(scopes, names):
    edges = [(names[p], names[sc[-1]]) for sc in scopes for p in sc[:-1]]
    lone = [names[sc[-1]] for sc in scopes if len(sc) == 1 and not any(sc[-1] in s[:-1] for s in scopes)]
    return sorobn_amd.BayesNet(*edges, *lone)


def _thetas_of(bn):
    f = learning_flat(bn)
    return [np.asarray(f.values[a:b]) for a, b in zip(f.value_off[:-1], f.value_off[1:])]


def learning_flat(bn):
    from sorobn_amd.flatten import flatten
    return flatten(bn)


def test_fit_em_host_logic_against_the_twin(monkeypatch):
    """fit_em with the two engine calls replaced by numpy test doubles: CPTs, log-likelihoods and expected counts equal the twin's
    after three iterations (missing cells, one latent column with init='current', 'uniform' and 'counts' starts)."""
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", EnumerationEngine)
    monkeypatch.setattr(learning, "counting_engine", lambda device=None: NumpyCounter())
    rng = np.random.default_rng(11)
    card, scopes, thetas = _random_net(rng, V=6)
    V = len(card)
    names = [f"n{v}" for v in range(V)]
    domains = [[f"s{k}" for k in range(card[v])] for v in range(V)]
    full = em.sample_rows(card, scopes, thetas, 400, rng)
    assert all(len(np.unique(full[:, v])) == card[v] for v in range(V))
    codes = em.knock_out(full, 0.2, rng)
    X = _frame(codes, names, domains)
    # the library numbers the variables in bn.nodes order: the twin runs on the same network renumbered
    order = [names.index(n) for n in _structure(scopes, names).nodes]
    hidden = em.knock_out(full, 0.1, rng, drop_column=1)
    card, scopes, thetas, codes = em.relabel(card, scopes, thetas, codes, order)
    hidden = hidden[:, order]
    names, domains = [names[o] for o in order], [domains[o] for o in order]
    for init in ("uniform", "counts"):
        bn = _structure(scopes, names)
        assert bn.nodes == names
        bn.fit_em(X, n_iter=3, tol=0.0, init=init, sub_batch=150)
        if init == "uniform":
            start = [np.full(len(t), 1.0 / card[v]) for v, t in enumerate(thetas)]
        else:
            hard = [np.zeros(len(t)) for t in thetas]
            for row in codes:
                for v, sc in enumerate(scopes):
                    if all(row[u] >= 0 for u in sc):
                        hard[v][int(np.ravel_multi_index([row[u] for u in sc], [card[u] for u in sc]))] += 1
            start = em.m_step([h + 1.0 for h in hard], hard, card)
        want, lls, counts = em.em(card, scopes, start, codes, 3)
        got = _thetas_of(bn)
        assert max(float(np.max(np.abs(g - w))) for g, w in zip(got, want)) <= 1e-12, init
        assert np.allclose(bn.em_log_likelihood_, lls, rtol=1e-12, atol=0) and bn.em_iterations_ == 3
        assert max(float(np.max(np.abs(bn._counts[names[v]].to_numpy() - counts[v]))) for v in range(V)) <= 1e-9
    # a latent column: never observed, CPTs in place
    bn = _structure(scopes, names)
    for v in range(V):
        bn.P[names[v]] = learning._em_series(names[v], [names[u] for u in scopes[v][:-1]], {n: pd.Index(d) for n, d in zip(names, domains)}, thetas[v])
    bn.prepare()
    Xh = _frame(hidden, names, domains).drop(columns=["n1"])
    bn.fit_em(Xh, n_iter=2, tol=0.0)
    want, lls, _ = em.em(card, scopes, thetas, hidden, 2)
    assert max(float(np.max(np.abs(g - w))) for g, w in zip(_thetas_of(bn), want)) <= 1e-12
    assert np.allclose(bn.em_log_likelihood_, lls, rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="n1"):
        _structure(scopes, names).fit_em(Xh, n_iter=1)


def test_fit_em_argument_errors_before_any_engine(monkeypatch):
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    bn = netspec.build(spec, sorobn_amd.BayesNet)

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", no_engine)
    monkeypatch.setattr(learning._capi, "Engine", no_engine)
    X = pd.DataFrame({"Burglary": [True, False, None], "Alarm": [True, None, False]}, dtype=object)
    with pytest.raises(ValueError):
        bn.fit_em(X, n_iter=0)
    with pytest.raises(ValueError):
        bn.fit_em(X, prior_count=-1.0)
    with pytest.raises(ValueError):
        bn.fit_em(X, init="random")
    with pytest.raises(KeyError):
        bn.fit_em(pd.DataFrame({"Burglary": [True], "Not a variable": [1]}))
    with pytest.raises(ValueError):  # latent columns without usable CPTs
        sorobn_amd.BayesNet(("A", "B")).fit_em(pd.DataFrame({"A": [0, 1]}), init="counts")


def test_expect_batch_is_declared_and_exported():
    assert "mibn_expect_batch" in _capi.SYMBOLS
    assert hasattr(_capi.lib(), "mibn_expect_batch")
    assert hasattr(_capi.Engine, "expect_batch") and hasattr(sorobn_amd.BayesNet, "fit_em")
