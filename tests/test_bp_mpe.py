"""Approximate MPE by max-product belief propagation on the device (mibn_bp_mpe_batch, bp_max_kernel; BayesNet.mpe / mpe_frame with
algorithm="lbp") against the numpy twin of what include/mibn.h pins (tests/bp_mpe_check.py), against the exact mpe where max-product is
exact, and against itself: bit for bit alone or in a batch, in LDS or in slabs of the arena.

The rule of the comparison with the twin: iterations and residual bits always; log_p within 1e-12 * max(1, |log_p|) - the device's
logarithm may differ from numpy's in the last bit -; codes, best_iteration, sweeps and moves whenever the twin's two best distinct
candidate scores are more than 1e-9 apart (otherwise the last bit of a logarithm may choose the other candidate: the fallback, counted
in FALLBACK and printed; it must not fire on a polytree and fires on no more than one loopy case in ten)."""
import numpy as np
import pandas as pd
import pytest

import bp_check as bc
import bp_mpe_check as mm
import likelihood_check as lc
import mpe_check as mc
import netspec
import sorobn_amd
import test_bp as tb
import test_bp_host as host
import test_bp_mpe_host as mh
from sorobn_amd import _capi

pytestmark = pytest.mark.gpu

GAP = 1e-9
FALLBACK = {"cases": 0, "fired": 0}
device = tb.device


def close(a, b):
    return a == b or abs(a - b) <= 1e-12 * max(1.0, abs(b))


def run(eng, reqs, max_iterations, tol, damping, polish):
    """reqs: [(evidence {id: code}, findings [(id, weights)])] -> (codes [B, n], log_p, iterations, residual, info [B, 3])"""
    e_off = np.zeros(len(reqs) + 1, np.int64)
    np.cumsum([len(ev) for ev, _ in reqs], out=e_off[1:])
    ev_ids = [v for ev, _ in reqs for v in ev]
    ev_codes = [c for ev, _ in reqs for c in ev.values()]
    block = lc.block([fs for _, fs in reqs]) if any(fs for _, fs in reqs) else None
    return eng.bp_mpe_batch(e_off, ev_ids, ev_codes, max_iterations, tol, damping, polish, likelihoods=block)


def hold(got, b, T, ctx, loopy=True):
    """Request b of a device result against the twin's namespace T."""
    codes, log_p, it, res, info = got
    gap = mm.score_gap(T.trajectory)
    print(f"{ctx}[{b}]: log_p {log_p[b]!r} (twin {T.log_p!r}), iterations {it[b]} (twin {T.iterations}), residual {res[b]!r} (twin {T.residual!r}), "
          f"info {info[b].tolist()} (twin {[T.best_iteration, T.sweeps, T.moves]}), score gap {gap:.2e}")
    assert it[b] == T.iterations, (ctx, b, it[b], T.iterations)
    assert res[b] == T.residual, (ctx, b, res[b], T.residual)
    assert close(float(log_p[b]), T.log_p), (ctx, b, log_p[b], T.log_p)
    if loopy:
        FALLBACK["cases"] += 1
    if gap > GAP:
        assert np.array_equal(codes[b], T.codes), (ctx, b, codes[b], T.codes)
        assert info[b].tolist() == [T.best_iteration, T.sweeps, T.moves], (ctx, b)
    else:
        assert loopy, (ctx, b, "the fallback fired on a polytree")
        FALLBACK["fired"] += 1


ITERATIONS, DAMPINGS, POLISHES = (1, 2, 7, 60), (0.0, 0.5), (0, 10)


def matrix(eng, f, reqs, ctx, iterations=ITERATIONS, dampings=DAMPINGS, polishes=POLISHES, loopy=True):
    for d in dampings:
        twins = [mm.run_many(f, ev, fs, iterations, 0.0, d, polishes) for ev, fs in reqs]
        for m in iterations:
            for q in polishes:
                got = run(eng, reqs, m, 0.0, d, q)
                for b in range(len(reqs)):
                    hold(got, b, twins[b][(m, q)], f"{ctx} it={m} d={d} polish={q}", loopy)


# ------------------------------------------------------------------------------------------------------------------- polytrees
@pytest.mark.parametrize("name", list(mh.POLYTREES))
def test_polytrees_against_twin_and_exact_mpe(name):
    bn, f = device(mh.POLYTREES[name]())
    n = len(f.card)
    reqs = host.requests_of(f, 7)
    got = run(bn.backend.engine, reqs, 2 * n + 1, 0.0, 0.0, 10)
    for b, (ev, fs) in enumerate(reqs):
        hold(got, b, mm.run(f, ev, fs, 2 * n + 1, 0.0, 0.0, 10), name, loopy=False)
        assert got[3][b] == 0.0 and got[4][b, 2] == 0
        event = {f.names[v]: f.domains[v][c] for v, c in ev.items()}
        lik = {f.names[v]: dict(zip(f.domains[v], w)) for v, w in fs} or None
        want, want_lp = bn.mpe(event, return_log_prob=True, likelihood=lik)
        mine, lp = bn.mpe(event, return_log_prob=True, likelihood=lik, algorithm="lbp", n_iterations=2 * n + 1, tol=0.0, damping=0.0)
        assert list(mine) == list(want) and list(mine.index) == list(want.index), (name, b)
        # both are within 1e-12 of the brute-force maximum (mpe_check.check_against_brute holds the exact call to that)
        assert abs(lp - want_lp) <= 2e-12 * max(1.0, abs(want_lp)), (name, b, lp, want_lp)
        assert lp == got[1][b]


# ---------------------------------------------------------------------------------------------------------------- loopy networks
LOOPY = mh.MATRIX
loopy_requests = mh.matrix_requests


@pytest.mark.parametrize("name", list(LOOPY))
def test_loopy_against_twin(name):
    bn, f = device(LOOPY[name]())
    matrix(bn.backend.engine, f, loopy_requests(name, f), name)


def test_fallback_is_rare():
    """How often only log_p could be held, over the loopy cases that ran before this test (file order; run alone it has nothing to
    count - tests/test_bp_mpe_host.py holds the same bound on the twin alone, where it is decided)."""
    print(f"fallback fired on {FALLBACK['fired']} of {FALLBACK['cases']} loopy cases")
    assert FALLBACK["fired"] * 10 <= FALLBACK["cases"], FALLBACK


# ------------------------------------------------------------------------------------------------------------------- edge shapes
SHAPES = {
    **tb.SHAPES,  # a single variable, an isolated one, cards 1 and 70, four parents, a hub with 40 children, 280 edges on 256 lanes
    "chain130": lambda: netspec.chain_spec(130, (2, 3, 4), seed=5),  # three score rows, the last of 2 terms
    "chain600": lambda: netspec.chain_spec(600, (2,), seed=6),       # 2 colours of 300 members: more than the 256 lanes
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_edge_shapes_against_twin(name):
    bn, f = device(SHAPES[name]())
    n = len(f.card)
    rng = np.random.default_rng(5)
    last = n - 1
    reqs = [({}, []), ({last: int(rng.integers(f.card[last]))}, []), ({}, [(0, rng.uniform(0.1, 2.0, int(f.card[0])))]),
            ({v: int(rng.integers(f.card[v])) for v in range(n)}, []),  # every variable observed
            ({last: int(f.card[last])}, []), ({0: -1}, []),             # evidence out of domain
            ({}, [(last, np.zeros(int(f.card[last])))])]                # an all-zero finding
    matrix(bn.backend.engine, f, reqs, name, iterations=(1, 6), dampings=(0.0, 0.5), polishes=(0, 10))
    codes, log_p, it, res, info = run(bn.backend.engine, reqs, 6, 0.0, 0.5, 10)
    assert np.array_equal(codes[3], [reqs[3][0][v] for v in range(n)])
    for b, (ev, _) in enumerate(reqs[4:], start=4):  # no mass: -inf, -1 off the evidence, iteration 0
        assert log_p[b] == -np.inf and it[b] == 0 and res[b] == 0.0 and info[b].tolist() == [0, 0, 0]
        assert all(codes[b, v] == (ev[v] if v in ev else -1) for v in range(n))
    if name == "card1":
        assert codes[0, 1] == 0
    if name == "chain600":
        colour, members = mm.colouring(bc.graph(f))
        assert [len(m) for m in members] == [300, 300]


# ------------------------------------------------------------------------------------------------------------------- bit for bit
def same(a, i, b, j):
    return all(np.array_equal(x[i], y[j]) for x, y in zip(a, b))


def test_a_request_is_the_same_bits_anywhere_in_any_batch():
    bn, f = device(LOOPY["grid4x4k2"]())
    eng = bn.backend.engine
    reqs = tb.some_requests(f, 31)
    me, other1, other2 = reqs[2], reqs[1], reqs[3]
    alone = run(eng, [me], 9, 0.0, 0.5, 10)
    for pos, batch in enumerate(([me, other1, other2], [other1, me, other2], [other1, other2, me])):
        assert same(alone, 0, run(eng, batch, 9, 0.0, 0.5, 10), pos), pos
    many = run(eng, [me] * 300, 9, 0.0, 0.5, 10)  # more requests than CUs
    assert all(same(alone, 0, many, i) for i in range(300))
    eng.set_option("chunk", 7)  # ... and under any chunking
    try:
        cut = run(eng, [other1, me] * 10, 9, 0.0, 0.5, 10)
    finally:
        eng.set_option("chunk", 32768)
    assert all(same(alone, 0, cut, i) for i in range(1, 20, 2))


@pytest.mark.parametrize("name", ["asia", "grid3x3k3", "dag_zeros"])
def test_lds_and_global_forms_bit_for_bit(name):
    bn, f = device(LOOPY[name]())
    eng = bn.backend.engine
    reqs = tb.some_requests(f, 31)
    a = run(eng, reqs, 7, 0.0, 0.5, 10)
    assert eng.stats()["arena_bytes"] == 0
    ks = {k["name"]: k for k in eng.kernel_stats() if k["launches"] > 0}
    assert list(ks) == ["bp_max_kernel"] and ks["bp_max_kernel"]["items"] == len(reqs) and ks["bp_max_kernel"]["alg_bytes"] > 0
    eng.set_option("bp_lds", 0)
    try:
        b = run(eng, reqs, 7, 0.0, 0.5, 10)
        assert eng.stats()["arena_bytes"] > 0
    finally:
        eng.set_option("bp_lds", 1)
    c = run(eng, reqs, 7, 0.0, 0.5, 10)
    for i in range(len(reqs)):
        assert same(a, i, b, i) and same(a, i, c, i)


# ---------------------------------------------------------------------------------------------------------------------- findings
def test_findings():
    bn, f = device(tb.LOOPY["grid4x4mixed"]())
    eng = bn.backend.engine
    v, c = 5, 1
    onehot = np.zeros(int(f.card[v]))
    onehot[c] = 1.0
    hard = run(eng, [({v: c, 0: 0}, [])], 12, 0.0, 0.5, 10)
    soft = run(eng, [({0: 0}, [(v, onehot)])], 12, 0.0, 0.5, 10)
    assert same(hard, 0, soft, 0)
    lam = np.random.default_rng(3).uniform(0.2, 1.5, int(f.card[v]))
    reqs = [({0: 0}, [(v, lam)]), ({}, [(v, np.zeros(int(f.card[v])))]), ({}, [(v, 2.0 * lam)])]
    matrix(eng, f, reqs, "findings", iterations=(12,), dampings=(0.5,), polishes=(10,))
    codes, log_p, it, res, info = run(eng, reqs, 12, 0.0, 0.5, 10)
    assert log_p[1] == -np.inf and it[1] == 0 and np.all(codes[1] == -1)
    assert close(float(log_p[0]), mm.log_weighted_joint(f, codes[0], *reqs[0]))  # (the weights are part of log_p)
    # a block of another B
    eng.set_likelihoods(lc.block([[(v, lam)], []]))
    with pytest.raises(_capi.MibnError) as e:
        eng.bp_mpe_batch([0, 0], [], [], 5, 0.0, 0.5, 10)
    assert e.value.code == _capi.E_ARG
    assert same(run(eng, [({0: 0}, [])], 3, 0.0, 0.5, 10), 0, run(eng, [({0: 0}, [])], 3, 0.0, 0.5, 10), 0)  # (the block is gone)


# ------------------------------------------------------------------------------------------------------------------- error paths
def test_error_paths_leave_the_engine_usable():
    bn, f = device(tb.LOOPY["asia"]())
    eng = bn.backend.engine
    n = len(f.card)
    name = f.names[0]
    before = bn.query(name, event={}).to_numpy()
    bp_before = eng.bp_batch([0, 0], [], [], 5, 0.0, 0.0)
    v0 = np.ones(int(f.card[1]))
    none = dict(e_off=[0, 0], e_vars=[], e_codes=[])
    bad = [
        (dict(e_off=[0, 1], e_vars=[n], e_codes=[0]), {}, None),                        # unknown evidence variable
        (dict(e_off=[0, 1], e_vars=[-1], e_codes=[0]), {}, None),
        (dict(e_off=[0, 2], e_vars=[2, 2], e_codes=[0, 1]), {}, None),                  # duplicate
        (dict(e_off=[0, 2, 1], e_vars=[1, 2], e_codes=[0, 0]), {}, None),               # descending e_off
        (dict(e_off=[0, 1], e_vars=[1], e_codes=[0]), {}, lc.block([[(1, v0)]])),       # a finding variable that is evidence
        (none, dict(max_iterations=0), None), (none, dict(max_iterations=-4), None),
        (none, dict(damping=1.0), None), (none, dict(damping=-0.25), None), (none, dict(damping=float("nan")), None),
        (none, dict(tol=-1e-12), None), (none, dict(tol=float("nan")), None),
        (none, dict(polish_sweeps=-1), None),
    ]
    for args, more, block in bad:
        with pytest.raises(_capi.MibnError) as e:
            eng.bp_mpe_batch(**args, **{"max_iterations": 5, "tol": 0.0, "damping": 0.0, "polish_sweeps": 3, **more}, likelihoods=block)
        assert e.value.code == _capi.E_ARG, (args, more, e.value)
        assert np.array_equal(bn.query(name, event={}).to_numpy(), before), (args, more)
        assert all(np.array_equal(x, y) for x, y in zip(eng.bp_batch([0, 0], [], [], 5, 0.0, 0.0), bp_before)), (args, more)
    fresh = _capi.Engine(0)
    fresh.card = np.array([2], np.int32)  # (what set_network would have left: the binding sizes its output rows from it)
    with pytest.raises(_capi.MibnError) as e:
        fresh.bp_mpe_batch([0, 0], [], [], 5, 0.0, 0.0, 3)
    assert e.value.code == _capi.E_STATE
    fresh.set_network([256, 2], [0, 1, 3], [0, 0, 1], [0, 256, 768], np.full(768, 1.0 / 256))
    with pytest.raises(_capi.MibnError) as e:
        fresh.bp_mpe_batch([0, 0], [], [], 5, 0.0, 0.0, 3)
    assert e.value.code == _capi.E_LIMIT and "255" in e.value.msg
    assert abs(fresh.query_fixed([[1]], np.zeros((1, 0), np.int32), np.zeros((1, 0), np.int32))[0].sum() - 1.0) <= 1e-12
    fresh.close()


# ------------------------------------------------------------------------------------------------------------------------ Python
def test_python_surface_agrees_with_itself_and_names_like_mpe():
    bn, f = device(tb.example("asia"))
    names = bn._all_names()
    a, b = names[0], names[3]
    label = lambda n, k: f.domains[f.id[n]][k]
    event = {a: label(a, 0), b: label(b, 1)}
    exact = bn.mpe(event)
    got, lp, info = bn.mpe(event, return_log_prob=True, algorithm="lbp", return_info=True)
    assert set(info) == {"iterations", "residual", "converged", "best_iteration", "sweeps", "moves"}
    assert info["converged"] == (info["residual"] <= 1e-9)
    assert list(got.index) == list(exact.index) and got.dtype == exact.dtype and got[a] == event[a] and got[b] == event[b]
    ev = [f.id[a], f.id[b]]
    codes, log_p, it, res, extra = bn.backend.engine.bp_mpe([ev], [[f.code_of(v, event[n]) for v, n in zip(ev, (a, b))]], 100, 1e-9, 0.5, 10)
    assert lp == log_p[0] and [got[n] for n in names] == [f.domains[f.id[n]][codes[0, f.id[n]]] for n in names]
    assert (info["iterations"], info["residual"], info["best_iteration"], info["sweeps"], info["moves"]) == (it[0], res[0], *extra[0])
    frame, lps = bn.mpe_frame(pd.DataFrame({a: [event[a], None, event[a]], b: [event[b], None, np.nan]}).astype(object),
                              return_log_prob=True, algorithm="lbp", return_info=True)
    assert list(frame.columns[:len(names)]) == names and len(frame) == 3 and lps[0] == lp
    assert [frame.loc[0, n] for n in names] == list(got)
    assert frame[("info", "iterations")][0] == info["iterations"] and frame[("info", "moves")][0] == info["moves"]
    free, free_lp = bn.mpe(return_log_prob=True, algorithm="lbp")
    assert [frame.loc[1, n] for n in names] == list(free) and lps[1] == free_lp
    plain = bn.mpe_frame(pd.DataFrame({a: [event[a]]}).astype(object), algorithm="lbp")
    assert list(plain.columns) == names
    # impossible evidence: None off the evidence, -inf, like the exact call
    zero = tb.device(host.zero_spec())[0]
    z, zlp = zero.mpe({"000": 0, "001": 1}, return_log_prob=True, algorithm="lbp")
    e, elp = zero.mpe({"000": 0, "001": 1}, return_log_prob=True)
    assert zlp == elp == -np.inf and list(z) == list(e) and z["002"] is None
    # a likelihood finding reaches the call
    soft = bn.mpe(event, return_log_prob=True, algorithm="lbp", likelihood={names[1]: {label(names[1], 0): 0.2, label(names[1], 1): 0.9}})
    assert soft[1] != lp


# ------------------------------------------------------------------------------------------------- beyond the reach of exact calls
def test_grid_20x20_where_exact_mpe_raises():
    """400 four-state variables: the exact call raises, the approximate one returns an assignment whose log_p the test recomputes
    from the CPTs, equal to the twin's, and a local optimum."""
    bn, f = device(netspec.grid_spec(20, 20, 4, seed=1))
    eng = bn.backend.engine
    ev = {0: 1, 399: 2, 210: 0}
    event = {f.names[v]: f.domains[v][c] for v, c in ev.items()}
    with pytest.raises(_capi.MibnError) as e:
        bn.mpe(event)
    assert e.value.code in (_capi.E_NOMEM, _capi.E_LIMIT)
    got = run(eng, [(ev, [])], 30, 1e-9, 0.5, 10)
    assert eng.stats()["arena_bytes"] == 0  # (MsgLds: the decoder's state fits next to the messages)
    T = mm.run(f, ev, [], 30, 1e-9, 0.5, 10)
    hold(got, 0, T, "20x20")
    codes, log_p, it, res, info = got
    assert np.isfinite(log_p[0]) and close(float(log_p[0]), mc.log_joint(f, codes[0]))
    assert info[0, 1] == 10 or mm.one_opt(f, codes[0], ev)
    assert info[0, 1] < 10, "the prototype needed 2 to 5 sweeps"
    series, lp, meta = bn.mpe(event, return_log_prob=True, algorithm="lbp", n_iterations=30, return_info=True)
    assert lp == log_p[0] and meta["sweeps"] == info[0, 1] and len(series) == 400 and all(x is not None for x in series)
