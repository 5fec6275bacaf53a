"""Loopy belief propagation on the device (mibn_bp_batch, bp_kernel; BayesNet.marginals / marginals_frame / query(algorithm="lbp"))
against the numpy twin of the schedule include/mibn.h pins (tests/bp_check.py), against the exact query where belief propagation is
exact, and against itself: bit for bit alone or in a batch, in LDS or in slabs of the arena, call after call."""
import numpy as np
import pandas as pd
import pytest

import bp_check as bc
import golden_util as gu
import likelihood_check as lc
import netspec
import sorobn_amd
import test_bp_host as host
from sorobn_amd import _capi

pytestmark = pytest.mark.gpu

TWIN = 1e-12   # the bound of the project's other twins: the orders are pinned, what is left is the last bit of a division
EXACT = 1e-9   # the project's marginal tolerance


def device(spec, **options):
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    for k, v in options.items():
        bn.backend.engine.set_option(k, v)
    return bn, bn.backend.flat


def run(eng, reqs, max_iterations, tol, damping):
    """reqs: [(evidence {id: code}, findings [(id, weights)])] -> (beliefs [B, sum card], iterations, residual)"""
    e_off = np.zeros(len(reqs) + 1, np.int64)
    np.cumsum([len(ev) for ev, _ in reqs], out=e_off[1:])
    ev_ids = [v for ev, _ in reqs for v in ev]
    ev_codes = [c for ev, _ in reqs for c in ev.values()]
    block = lc.block([fs for _, fs in reqs]) if any(fs for _, fs in reqs) else None
    return eng.bp_batch(e_off, ev_ids, ev_codes, max_iterations, tol, damping, likelihoods=block)


def against_twin(eng, f, reqs, max_iterations, tol, damping, ctx):
    bel, it, res = run(eng, reqs, max_iterations, tol, damping)
    for b, (ev, fs) in enumerate(reqs):
        want, want_it, want_res = bc.run(f, ev, fs, max_iterations, tol, damping)
        err = float(np.max(np.abs(bel[b] - want)))
        print(f"{ctx}[{b}] it={max_iterations} d={damping}: iterations {it[b]} (twin {want_it}), residual {res[b]!r} (twin {want_res!r}), max|belief - twin| {err:.2e}")
        assert it[b] == want_it, (ctx, b, it[b], want_it)
        assert err <= TWIN, (ctx, b, err)
        assert abs(res[b] - want_res) <= TWIN, (ctx, b, res[b], want_res)
    return bel, it, res


def example(name):
    return next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == name)


def some_requests(f, seed):
    """No evidence; evidence on two variables; evidence and a finding; two findings."""
    rng = np.random.default_rng(seed)
    n = len(f.card)
    a, b, c, d = (int(v) for v in rng.choice(n, size=4, replace=False))
    code = lambda v: int(rng.integers(f.card[v]))
    lam = lambda v: rng.uniform(0.1, 2.0, int(f.card[v]))
    return [({}, []), ({a: code(a), b: code(b)}, []), ({a: code(a)}, [(c, lam(c))]), ({}, [(d, lam(d)), (b, lam(b))])]


# ------------------------------------------------------------------------------------------------------------------- polytrees
@pytest.mark.parametrize("name", ["chain5", "hub", "polytree8"])
def test_polytrees_against_twin_and_exact_query(name):
    spec = host.polytrees()[name]
    bn, f = device(spec)
    n = len(f.card)
    reqs = host.requests_of(f, 7)
    bel, it, res = against_twin(bn.backend.engine, f, reqs, 2 * n + 1, 0.0, 0.0, name)
    assert np.all(res == 0.0)
    off = np.concatenate([[0], np.cumsum(f.card)])
    for b, (ev, fs) in enumerate(reqs):
        event = {f.names[v]: f.domains[v][c] for v, c in ev.items()}
        lik = {f.names[v]: dict(zip(f.domains[v], w)) for v, w in fs} or None
        for v in range(n):
            if v in ev:
                continue
            want = bn.query(f.names[v], event=event, likelihood=lik).reindex(f.domains[v], fill_value=0.0).to_numpy()
            assert float(np.max(np.abs(bel[b, off[v]:off[v + 1]] - want))) <= EXACT, (name, b, v)


# ---------------------------------------------------------------------------------------------------------------- loopy networks
LOOPY = {
    "sprinkler": lambda: example("sprinkler"),
    "asia": lambda: example("asia"),
    "grid3x3": lambda: netspec.grid_spec(3, 3, 2, seed=4),
    "grid4x4mixed": lambda: netspec.mixed_grid_spec(4, 4, (2, 3, 4, 3), seed=6),
    "dag_zeros": lambda: netspec.random_dag_spec(21, n_nodes=9, p_zero=0.15),  # (20 edges, loops, 53 zero cells)
}


@pytest.fixture(scope="module")
def loopy():
    nets = {}
    for name, make in LOOPY.items():
        bn, f = device(make())
        nets[name] = (bn, f, some_requests(f, 31))
    return nets


@pytest.mark.parametrize("name", list(LOOPY))
def test_loopy_against_twin(loopy, name):
    bn, f, reqs = loopy[name]
    for max_iterations in (1, 2, 7):
        for damping in (0.0, 0.5):
            against_twin(bn.backend.engine, f, reqs, max_iterations, 0.0, damping, name)


@pytest.mark.parametrize("name", list(LOOPY))
def test_lds_and_global_forms_bit_for_bit(loopy, name):
    bn, f, reqs = loopy[name]
    eng = bn.backend.engine
    a = run(eng, reqs, 7, 0.0, 0.5)
    assert eng.stats()["arena_bytes"] == 0
    eng.set_option("bp_lds", 0)
    try:
        b = run(eng, reqs, 7, 0.0, 0.5)
        assert eng.stats()["arena_bytes"] > 0
    finally:
        eng.set_option("bp_lds", 1)
    c = run(eng, reqs, 7, 0.0, 0.5)  # ... and two calls in a row
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


STOP_TOL = 1e-8
# (picked on a CPU: these reach a fixed point in a few steps, their residuals fall from above 1e-7 to 1e-16 or 0 in one step; the grids
#  with evidence converge geometrically and pass through the band)
STOP_CASES = [("sprinkler", 1), ("sprinkler", 2), ("sprinkler", 3), ("asia", 1), ("asia", 2), ("asia", 3), ("grid3x3", 0), ("grid4x4mixed", 0)]


def test_stopping_on_tol(loopy):
    """iterations equal the twin's for tol = 1e-8, on cases whose twin residuals keep a factor of 10 away from the tolerance - asserted
    on the twin first -, so that the last bits cannot move the stop."""
    for name, k in STOP_CASES:
        bn, f, reqs = loopy[name]
        ev, fs = reqs[k]
        seq = []
        want, want_it, want_res = bc.run(f, ev, fs, 200, STOP_TOL, 0.0, residuals=seq)
        assert not any(STOP_TOL / 10 < r < STOP_TOL * 10 for r in seq), (name, k, seq)
        assert want_it < 200 and want_res <= STOP_TOL
        bel, it, res = run(bn.backend.engine, [(ev, fs)], 200, STOP_TOL, 0.0)
        print(f"{name}[{k}]: stops after {it[0]} (twin {want_it}), residual {res[0]!r}")
        assert it[0] == want_it and res[0] <= STOP_TOL
        assert float(np.max(np.abs(bel[0] - want))) <= TWIN


# ------------------------------------------------------------------------------------------------------------------- edge shapes
def dag(name, card, parents, seed=1):
    rng = np.random.default_rng(seed)
    return netspec._dag_spec(name, card, parents, lambda i: rng.dirichlet(np.ones(card[i])))


SHAPES = {
    "single": lambda: dag("single", [3], [[]]),
    "isolated": lambda: dag("isolated", [2, 3, 2], [[], [0], []]),
    "card1": lambda: dag("card1", [2, 1, 3, 2], [[], [0], [1], [0, 2]]),
    "card70": lambda: dag("card70", [70, 3, 2], [[], [0], [0, 1]]),
    "four_parents": lambda: dag("four_parents", [2, 3, 2, 3, 4, 2], [[], [], [0], [], [0, 1, 2, 3], [1, 4]]),
    "hub40": lambda: netspec.hub_spec(8, 3, (2,), (2,) * 40),
    "grid10x10": lambda: netspec.grid_spec(10, 10, 2, seed=2),  # 280 edges, 560 message cells: more than the 256 lanes, no multiple
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_edge_shapes_against_twin(name):
    bn, f = device(SHAPES[name]())
    n = len(f.card)
    rng = np.random.default_rng(5)
    last = n - 1
    reqs = [({}, []), ({last: int(rng.integers(f.card[last]))}, []), ({}, [(0, rng.uniform(0.1, 2.0, int(f.card[0])))]),
            ({v: int(rng.integers(f.card[v])) for v in range(n)}, [])]  # ... and every variable observed
    for max_iterations, damping in ((1, 0.0), (6, 0.0), (6, 0.5)):
        against_twin(bn.backend.engine, f, reqs, max_iterations, 0.0, damping, name)
    if name == "grid10x10":
        assert len(bc.graph(f).edges) == 280 and bc.graph(f).cells == 560


# ------------------------------------------------------------------------------------------------------------------- bit for bit
def test_a_request_is_the_same_bits_anywhere_in_any_batch(loopy):
    bn, f, reqs = loopy["asia"]
    eng = bn.backend.engine
    me, other1, other2 = reqs[2], reqs[1], reqs[3]
    alone = run(eng, [me], 9, 0.0, 0.0)
    for pos, batch in enumerate(([me, other1, other2], [other1, me, other2], [other1, other2, me])):
        got = run(eng, batch, 9, 0.0, 0.0)
        for x, y in zip(alone, got):
            assert np.array_equal(x[0], y[pos]), pos
    many = run(eng, [me] * 300, 9, 0.0, 0.0)  # more requests than CUs
    for x, y in zip(alone, many):
        assert all(np.array_equal(x[0], y[i]) for i in range(300))
    eng.set_option("chunk", 7)  # ... and under any chunking
    try:
        cut = run(eng, [other1, me] * 10, 9, 0.0, 0.0)
    finally:
        eng.set_option("chunk", 32768)
    for x, y in zip(alone, cut):
        assert all(np.array_equal(x[0], y[i]) for i in range(1, 20, 2))


# ---------------------------------------------------------------------------------------------------------------------- findings
def test_findings(loopy):
    bn, f, reqs = loopy["grid4x4mixed"]
    eng = bn.backend.engine
    v, c = 5, 1
    onehot = np.zeros(int(f.card[v]))
    onehot[c] = 1.0
    hard = run(eng, [({v: c, 0: 0}, [])], 12, 0.0, 0.0)
    soft = run(eng, [({0: 0}, [(v, onehot)])], 12, 0.0, 0.0)
    for x, y in zip(hard, soft):
        assert np.array_equal(x, y)
    lam = np.random.default_rng(3).uniform(0.2, 1.5, int(f.card[v]))
    base = run(eng, [({0: 0}, [(v, lam)])], 12, 0.0, 0.0)
    twice = run(eng, [({0: 0}, [(v, 2.0 * lam)])], 12, 0.0, 0.0)  # (a power of two: exact)
    other = run(eng, [({0: 0}, [(v, 3.7 * lam)])], 12, 0.0, 0.0)
    assert all(np.array_equal(x, y) for x, y in zip(base, twice))
    assert float(np.max(np.abs(base[0] - other[0]))) <= TWIN and base[1][0] == other[1][0]
    # zero mass through a finding and through a code of -1: zeros, iteration 0, residual 0
    bel, it, res = run(eng, [({}, [(v, np.zeros(int(f.card[v])))]), ({3: -1}, []), ({}, [])], 12, 0.0, 0.0)
    assert not bel[:2].any() and list(it[:2]) == [0, 0] and list(res[:2]) == [0.0, 0.0] and it[2] == 12 and bel[2].any()
    # a block of another B
    eng.set_likelihoods(lc.block([[(v, lam)], []]))
    with pytest.raises(_capi.MibnError) as e:
        eng.bp_batch([0, 0], [], [], 5, 0.0, 0.0)
    assert e.value.code == _capi.E_ARG
    assert np.array_equal(run(eng, [({0: 0}, [])], 3, 0.0, 0.0)[0], run(eng, [({0: 0}, [])], 3, 0.0, 0.0)[0])  # (the block is gone)


# ------------------------------------------------------------------------------------------------------------------- error paths
def test_error_paths_leave_the_engine_usable(loopy):
    bn, f, reqs = loopy["asia"]
    eng = bn.backend.engine
    n = len(f.card)
    name = f.names[0]
    before = bn.query(name, event={}).to_numpy()
    v0 = np.ones(int(f.card[1]))
    bad = [
        (dict(e_off=[0, 1], e_vars=[n], e_codes=[0]), {}, None),                        # unknown evidence variable
        (dict(e_off=[0, 1], e_vars=[-1], e_codes=[0]), {}, None),
        (dict(e_off=[0, 2], e_vars=[2, 2], e_codes=[0, 1]), {}, None),                  # duplicate
        (dict(e_off=[0, 2, 1], e_vars=[1, 2], e_codes=[0, 0]), {}, None),               # descending e_off
        (dict(e_off=[0, 1], e_vars=[1], e_codes=[0]), {}, lc.block([[(1, v0)]])),       # a finding variable that is evidence
        (dict(e_off=[0, 0], e_vars=[], e_codes=[]), dict(max_iterations=0), None),
        (dict(e_off=[0, 0], e_vars=[], e_codes=[]), dict(max_iterations=-4), None),
        (dict(e_off=[0, 0], e_vars=[], e_codes=[]), dict(damping=1.0), None),
        (dict(e_off=[0, 0], e_vars=[], e_codes=[]), dict(damping=-0.25), None),
        (dict(e_off=[0, 0], e_vars=[], e_codes=[]), dict(damping=float("nan")), None),
        (dict(e_off=[0, 0], e_vars=[], e_codes=[]), dict(tol=-1e-12), None),
        (dict(e_off=[0, 0], e_vars=[], e_codes=[]), dict(tol=float("nan")), None),
    ]
    for args, more, block in bad:
        with pytest.raises(_capi.MibnError) as e:
            eng.bp_batch(**args, **{"max_iterations": 5, "tol": 0.0, "damping": 0.0, **more}, likelihoods=block)
        assert e.value.code == _capi.E_ARG, (args, more, e.value)
        assert np.array_equal(bn.query(name, event={}).to_numpy(), before), (args, more)
    fresh = _capi.Engine(0)
    fresh.card = np.array([2], np.int32)  # (what set_network would have left: the binding sizes its output row from it)
    with pytest.raises(_capi.MibnError) as e:
        fresh.bp_batch([0, 0], [], [], 5, 0.0, 0.0)
    assert e.value.code == _capi.E_STATE
    fresh.set_network([256, 2], [0, 1, 3], [0, 0, 1], [0, 256, 768], np.full(768, 1.0 / 256))
    with pytest.raises(_capi.MibnError) as e:
        fresh.bp_batch([0, 0], [], [], 5, 0.0, 0.0)
    assert e.value.code == _capi.E_LIMIT and "255" in e.value.msg
    assert abs(fresh.query_fixed([[1]], np.zeros((1, 0), np.int32), np.zeros((1, 0), np.int32))[0].sum() - 1.0) <= 1e-12
    fresh.close()


# ------------------------------------------------------------------------------------------------------------------------ Python
def test_python_surface_agrees_with_itself_and_names_like_query():
    bn, f = device(example("asia"))
    names = bn._all_names()
    a, b = names[0], names[3]
    label = lambda n, k: f.domains[f.id[n]][k]
    event = {a: label(a, 0), b: label(b, 1)}
    got, info = bn.marginals(event, return_info=True)
    assert sorted(got) == [n for n in names if n not in event]
    assert set(info) == {"iterations", "residual", "converged"} and info["converged"] == (info["residual"] <= 1e-9)
    frame = bn.marginals_frame(pd.DataFrame({a: [event[a], None, event[a]], b: [event[b], None, np.nan]}).astype(object), return_info=True)
    assert list(frame.columns.names) == ["variable", "state"] and len(frame) == 3
    assert frame[("info", "iterations")][0] == info["iterations"] and frame[("info", "residual")][0] == info["residual"]
    free = bn.marginals()
    for n, s in got.items():
        exact = bn.query(n, event=event)
        assert s.name == exact.name == f"P({n})" and s.index.name == exact.index.name == n
        assert list(s.index) == list(exact.index)  # (Asia's posteriors have no zero rows here)
        one = bn.query(n, event=event, algorithm="lbp")
        assert one.name == s.name and one.index.equals(s.index) and np.array_equal(one.to_numpy(), s.to_numpy())
        row = frame.loc[0, n]
        assert np.array_equal(row.to_numpy(dtype=float), s.reindex(list(row.index), fill_value=0.0).to_numpy())
        assert np.array_equal(frame.loc[1, n].to_numpy(dtype=float), free[n].reindex(list(row.index), fill_value=0.0).to_numpy())
    with pytest.raises(ValueError):
        bn.query(names[1], names[2], event=event, algorithm="lbp")
    # a likelihood finding reaches the call
    soft = bn.marginals(event, likelihood={names[1]: {label(names[1], 0): 0.2, label(names[1], 1): 0.9}})
    assert not np.array_equal(soft[names[2]].to_numpy(), got[names[2]].to_numpy())


# ------------------------------------------------------------------------------------------------- beyond the reach of exact calls
def test_grid_20x20_runs_in_lds():
    """400 four-state variables, a frontier of 4^20 cells for any exact call: one request, 30 iterations, message state in LDS."""
    bn, f = device(netspec.grid_spec(20, 20, 4, seed=1))
    eng = bn.backend.engine
    G = bc.graph(f)
    assert len(G.edges) == 1160 and 24 * G.cells + 8 * G.lam_cells + 64 <= 160 * 1024
    ev = {0: 1, 399: 2, 210: 0}
    bel, it, res = run(eng, [(ev, [])], 30, 1e-9, 0.0)
    assert eng.stats()["arena_bytes"] == 0  # (MsgGlobal books its slabs)
    ks = {k["name"]: k for k in eng.kernel_stats() if k["launches"] > 0}
    assert list(ks) == ["bp_kernel"] and ks["bp_kernel"]["items"] == 1
    want, want_it, want_res = bc.run(f, ev, [], 30, 1e-9, 0.0)
    err = float(np.max(np.abs(bel[0] - want)))
    print(f"20x20: {it[0]} iterations (twin {want_it}), residual {res[0]:.3e} (twin {want_res:.3e}), max|belief - twin| {err:.2e}")
    assert it[0] == want_it and err <= TWIN and abs(res[0] - want_res) <= TWIN
    marg, info = bn.marginals({f.names[v]: f.domains[v][c] for v, c in ev.items()}, n_iterations=30, return_info=True)
    assert info["iterations"] == it[0] and info["converged"] == bool(res[0] <= 1e-9) and len(marg) == 397
