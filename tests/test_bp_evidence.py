"""The Bethe log Z and the family beliefs of loopy belief propagation on the device (mibn_bp_evidence_batch, bp_evidence_kernel,
bp_accumulate_kernel; BayesNet.evidence_proba / log_likelihood / family_marginals / fit_em with algorithm="lbp") against the numpy
twin of what include/mibn.h pins (tests/bp_evidence_check.py), against mibn_bp_batch byte for byte, against the exact calls where
belief propagation is exact, and against itself: bit for bit alone or in a batch, under any chunking, in LDS or in slabs."""
import numpy as np
import pandas as pd
import pytest

import bp_check as bc
import bp_evidence_check as bev
import likelihood_check as lc
import netspec
import sorobn_amd
import test_bp as tb
import test_bp_evidence_host as evh
import test_bp_host as host
import test_em_host as em_host
from sorobn_amd import _capi, learning

pytestmark = pytest.mark.gpu

TWIN = 1e-12   # the bound of the project's other twins: the orders are pinned, what is left is the last bit of a division or a logarithm
EXACT = 1e-9   # the project's marginal tolerance
device, example = tb.device, tb.example


def csr(reqs):
    e_off = np.zeros(len(reqs) + 1, np.int64)
    np.cumsum([len(ev) for ev, _ in reqs], out=e_off[1:])
    block = lc.block([fs for _, fs in reqs]) if any(fs for _, fs in reqs) else None
    return e_off, [v for ev, _ in reqs for v in ev], [c for ev, _ in reqs for c in ev.values()], block


def run(eng, reqs, max_iterations, tol, damping, weight=None, acc=None):
    """reqs: [(evidence {id: code}, findings [(id, weights)])] -> (log_z, beliefs, fbeliefs, iterations, residual); acc in place"""
    e_off, ids, codes, block = csr(reqs)
    return eng.bp_evidence_batch(e_off, ids, codes, max_iterations, tol, damping, likelihoods=block, weight=weight, acc=acc, beliefs=True, fbeliefs=True)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def close_log(got, want, empty=False):
    """1e-12 relative.  `empty` - a request without evidence and findings, whose log_z is log 1 = 0 up to rounding, where a relative
    bound says nothing: 1e-12 absolute, log_z being a sum of n terms of order 1, each a few logarithms' last bits."""
    return got == want or abs(got - want) <= TWIN * (max(1.0, abs(want)) if empty else abs(want))


def against_twin(eng, f, reqs, max_iterations, tol, damping, ctx):
    fcells = int(eng.family_off[-1])
    rng = np.random.default_rng(17)
    start, weight = rng.uniform(0.0, 3.0, fcells), rng.uniform(0.0, 2.0, len(reqs))
    acc = start.copy()
    log_z, bel, fb, it, res = run(eng, reqs, max_iterations, tol, damping, weight=weight, acc=acc)
    twins = [bev.run(f, ev, fs, max_iterations, tol, damping) for ev, fs in reqs]
    want_acc = bev.accumulate(start, [t.fbeliefs for t in twins], weight)
    for b, t in enumerate(twins):
        eb, ef = float(np.max(np.abs(bel[b] - t.beliefs))), float(np.max(np.abs(fb[b] - t.fbeliefs)))
        print(f"{ctx}[{b}] it={max_iterations} d={damping}: iterations {it[b]} (twin {t.iterations}), residual {res[b]!r} (twin {t.residual!r}), "
              f"log_z {log_z[b]!r} (twin {t.log_z!r}), max|belief - twin| {eb:.2e}, max|family belief - twin| {ef:.2e}")
        assert it[b] == t.iterations and res[b] == t.residual, (ctx, b, it[b], t.iterations, res[b], t.residual)
        assert close_log(log_z[b], t.log_z, empty=not reqs[b][0] and not reqs[b][1]), (ctx, b, log_z[b], t.log_z)
        assert eb <= TWIN and ef <= TWIN, (ctx, b, eb, ef)
    ea = float(np.max(np.abs(acc - want_acc))) if fcells else 0.0
    print(f"{ctx} it={max_iterations} d={damping}: max|acc - twin| {ea:.2e}")
    assert ea <= TWIN, (ctx, ea)
    return log_z, bel, fb, it, res


NETS = {
    "chain5": lambda: host.polytrees()["chain5"],
    "hub": lambda: host.polytrees()["hub"],
    "polytree8": lambda: host.polytrees()["polytree8"],
    "sprinkler": lambda: example("sprinkler"),
    "asia": lambda: example("asia"),
    "grid3x3k3": lambda: netspec.grid_spec(3, 3, 3, seed=4),
    "grid4x4k2": lambda: netspec.grid_spec(4, 4, 2, seed=6),
    "dag_zeros": lambda: netspec.random_dag_spec(21, n_nodes=9, p_zero=0.15),
}
POLYTREES = ("chain5", "hub", "polytree8")


@pytest.fixture(scope="module")
def nets():
    out = {}
    for name, make in NETS.items():
        bn, f = device(make())
        out[name] = (bn, f, host.requests_of(f, 7) if name in POLYTREES else tb.some_requests(f, 31))
    return out


# ------------------------------------------------------------------------------------------------------------------ against the twin
@pytest.mark.parametrize("name", list(NETS))
def test_device_against_twin(nets, name):
    bn, f, reqs = nets[name]
    for max_iterations in (1, 2, 7):
        for damping in (0.0, 0.5):
            against_twin(bn.backend.engine, f, reqs, max_iterations, 0.0, damping, name)


@pytest.mark.parametrize("name", list(NETS))
def test_beliefs_are_bp_batch_byte_for_byte(nets, name):
    bn, f, reqs = nets[name]
    eng = bn.backend.engine
    for max_iterations, tol, damping in ((1, 0.0, 0.0), (7, 0.0, 0.5), (50, 1e-8, 0.0)):
        _, bel, _, it, res = run(eng, reqs, max_iterations, tol, damping)
        want = tb.run(eng, reqs, max_iterations, tol, damping)
        assert bel.tobytes() == want[0].tobytes() and it.tobytes() == want[1].tobytes() and res.tobytes() == want[2].tobytes()


@pytest.mark.parametrize("name", POLYTREES)
def test_polytrees_against_the_exact_calls(nets, name):
    bn, f, reqs = nets[name]
    n = len(f.card)
    log_z, _, fb, _, res = run(bn.backend.engine, reqs, 2 * n + 1, 0.0, 0.0)
    assert np.all(res == 0.0)
    foff = bn.backend.engine.family_off
    for b, (ev, fs) in enumerate(reqs):
        event = {f.names[v]: f.domains[v][c] for v, c in ev.items()}
        if not fs:
            want = np.log(bn.evidence_proba(event)) if event else 0.0
            assert abs(log_z[b] - want) <= EXACT, (name, b, log_z[b], want)
        lik = {f.names[v]: dict(zip(f.domains[v], w)) for v, w in fs} or None
        for v in range(n):
            if any(u in ev for u in f.scope[v]):
                continue  # (query refuses a family member in the event)
            members = [f.names[u] for u in f.scope[v]]
            ans = bn.query(*members, event=event, likelihood=lik)
            if len(members) > 1:
                ans = ans.reorder_levels(members).reindex(pd.MultiIndex.from_product([f.domains[u] for u in f.scope[v]], names=members), fill_value=0.0)
            else:
                ans = ans.reindex(f.domains[v], fill_value=0.0)
            assert float(np.max(np.abs(fb[b, foff[v]:foff[v + 1]] - ans.to_numpy()))) <= EXACT, (name, b, v)


# ------------------------------------------------------------------------------------------------------------------- edge shapes
SHAPES = {
    "single": lambda: tb.dag("single", [3], [[]]),
    "isolated": lambda: tb.dag("isolated", [2, 3, 2], [[], [0], []]),
    "card1": lambda: tb.dag("card1", [2, 1, 3, 2], [[], [0], [1], [0, 2]]),
    "card70": lambda: tb.dag("card70", [70, 3, 2], [[], [0], [0, 1]]),
    "four_parents": lambda: tb.dag("four_parents", [2, 3, 2, 3, 4, 2], [[], [], [0], [], [0, 1, 2, 3], [1, 4]]),
    "hub40": lambda: netspec.hub_spec(8, 3, (2,), (2,) * 40),
    "grid10x10k4": lambda: netspec.grid_spec(10, 10, 4, seed=2),  # 280 edges on 256 lanes, 100 variables over the 64 partials
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_edge_shapes_against_twin(name):
    bn, f = device(SHAPES[name]())
    n = len(f.card)
    rng = np.random.default_rng(5)
    last = n - 1
    everything = {v: int(rng.integers(f.card[v])) for v in range(n)}
    reqs = [({}, []), ({last: int(rng.integers(f.card[last]))}, []), ({}, [(0, rng.uniform(0.1, 2.0, int(f.card[0])))]), (everything, [])]
    for max_iterations, damping in ((1, 0.0), (6, 0.5)):
        log_z, *_ = against_twin(bn.backend.engine, f, reqs, max_iterations, 0.0, damping, name)
    G = bc.graph(f)
    want = float(sum(np.log(G.table[v][tuple(everything[u] for u in G.scope[v])]) for v in range(n)))  # every variable observed
    assert abs(log_z[3] - want) <= TWIN * abs(want), (name, log_z[3], want)
    if name == "grid10x10k4":
        assert len(G.edges) == 280 and n == 100


# ------------------------------------------------------------------------------------------------------------------- bit for bit
def test_a_request_is_the_same_bits_anywhere_in_any_batch(nets):
    bn, f, reqs = nets["asia"]
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


def test_chunking_budget_form_and_weights_leave_every_bit_acc_included(nets):
    bn, f, reqs = nets["grid3x3k3"]
    eng = bn.backend.engine
    batch = (reqs * 5)[:19]
    fcells = int(eng.family_off[-1])
    start = np.random.default_rng(2).uniform(0.0, 5.0, fcells)

    def call(weight=None):
        acc = start.copy()
        out = run(eng, batch, 7, 0.0, 0.5, weight=weight, acc=acc)
        launches = {k["name"]: k["launches"] for k in eng.kernel_stats() if k["launches"] > 0}
        return (*out, acc), launches, eng.stats()["arena_bytes"]
    base, launches, arena = call()
    assert launches == {"bp_evidence_kernel": 1, "bp_accumulate_kernel": 1} and arena == 0
    ones, _, _ = call(np.ones(len(batch)))  # weight NULL against all ones
    assert same(base, ones)
    eng.set_option("chunk", 4)  # across chunk boundaries
    try:
        cut, launches, _ = call()
        assert launches == {"bp_evidence_kernel": 5, "bp_accumulate_kernel": 5} and same(base, cut)
    finally:
        eng.set_option("chunk", 32768)
    eng.set_option("bp_lds", 0)  # LDS against slabs, and a budget that forces several launches against one that does not
    try:
        slabs, launches, arena = call()
        assert launches["bp_evidence_kernel"] == 1 and arena > 0 and same(base, slabs)
        per = arena / len(batch) + 8 * fcells  # a slab and a family-belief row
        eng.set_option("arena_gb", 5.5 * per / 1e9)
        try:
            tight, launches, _ = call()
            assert launches == {"bp_evidence_kernel": 4, "bp_accumulate_kernel": 4} and same(base, tight)
            eng.set_option("arena_gb", 0.5 * per / 1e9)
            with pytest.raises(_capi.MibnError) as e:
                call()
            assert e.value.code == _capi.E_NOMEM
        finally:
            eng.set_option("arena_gb", 200.0)
    finally:
        eng.set_option("bp_lds", 1)
    assert same(base, call()[0])


def test_acc_adds_to_what_was_passed_and_weights_scale_it(nets):
    bn, f, reqs = nets["asia"]
    eng = bn.backend.engine
    fcells = int(eng.family_off[-1])
    _, _, fb, _, _ = run(eng, reqs, 7, 0.0, 0.0)
    zero, seven = np.zeros(fcells), np.full(fcells, 7.0)
    run(eng, reqs, 7, 0.0, 0.0, acc=zero)
    run(eng, reqs, 7, 0.0, 0.0, acc=seven)
    assert np.array_equal(zero, bev.accumulate(np.zeros(fcells), fb)) and np.array_equal(seven, bev.accumulate(np.full(fcells, 7.0), fb))
    w = np.array([2.0, 0.0, 0.5, 4.0])  # (powers of two: the products are exact)
    acc = np.zeros(fcells)
    run(eng, reqs, 7, 0.0, 0.0, weight=w, acc=acc)
    assert np.array_equal(acc, bev.accumulate(np.zeros(fcells), fb, w))
    twice = np.zeros(fcells)
    run(eng, reqs, 7, 0.0, 0.0, weight=2.0 * w, acc=twice)
    assert np.array_equal(twice, 2.0 * acc)
    # only log_z: no buffer, no second kernel
    e_off, ids, codes, block = csr(reqs)
    log_z, bel, none, it, res = eng.bp_evidence_batch(e_off, ids, codes, 7, 0.0, 0.0, likelihoods=block)
    assert bel is None and none is None and [k["name"] for k in eng.kernel_stats() if k["launches"] > 0] == ["bp_evidence_kernel"]
    assert np.array_equal(log_z, run(eng, reqs, 7, 0.0, 0.0)[0])
    ks = eng.kernel_stats()
    G = bc.graph(f)
    per_iter = 8 * sum(len(G.scope[v]) * G.table[v].size for v in range(G.n))
    row = next(k for k in ks if k["name"] == "bp_evidence_kernel")
    assert row["items"] == len(reqs) and row["alg_bytes"] == per_iter * int(it.sum()) + 8 * fcells * len(reqs)


# ----------------------------------------------------------------------------------------------------- zero mass and error paths
def test_zero_mass_rows_and_error_paths_leave_the_engine_usable():
    bn, f = device(host.zero_spec())
    eng = bn.backend.engine
    name = f.names[2]
    before = bn.query(name, event={}).to_numpy()
    fcells = int(eng.family_off[-1])
    reqs = [({0: 0, 1: 1}, []), ({2: -1}, []), ({}, [(1, np.zeros(2))]), ({0: 0, 1: 0}, [])]
    acc = np.full(fcells, 1.0)
    log_z, bel, fb, it, res = run(eng, reqs, 20, 0.0, 0.0, acc=acc)
    assert np.all(np.isneginf(log_z[:3])) and not bel[:3].any() and not fb[:3].any() and not res[:3].any()
    assert it[0] >= 1 and list(it[1:3]) == [0, 0]
    t = bev.run(f, *reqs[3], 20, 0.0, 0.0)
    assert it[0] == bev.run(f, *reqs[0], 20, 0.0, 0.0).iterations and close_log(log_z[3], t.log_z)
    assert float(np.max(np.abs(acc - (1.0 + t.fbeliefs)))) <= TWIN  # the zero-mass rows add nothing
    assert np.array_equal(bn.query(name, event={}).to_numpy(), before)
    root0, g = device(netspec._dag_spec("root0", [2], [[]], lambda i: np.array([0.0, 1.0])))
    log_z, bel, fb, it, res = run(root0.backend.engine, [({0: 0}, [])], 5, 0.0, 0.0)  # only the final phase shows it
    assert log_z[0] == -np.inf and not bel.any() and not fb.any() and res[0] == 0.0 and it[0] == bev.run(g, {0: 0}, [], 5, 0.0).iterations
    # ---- errors: nothing runs, acc untouched, the engine answers afterwards
    n = len(f.card)
    v0 = np.ones(int(f.card[1]))
    none = dict(e_off=[0, 0], e_vars=[], e_codes=[])
    bad = [
        (dict(e_off=[0, 1], e_vars=[n], e_codes=[0]), {}),                                   # unknown evidence variable
        (dict(e_off=[0, 1], e_vars=[-1], e_codes=[0]), {}),
        (dict(e_off=[0, 2], e_vars=[2, 2], e_codes=[0, 1]), {}),                             # duplicate
        (dict(e_off=[0, 2, 1], e_vars=[1, 2], e_codes=[0, 0]), {}),                          # descending e_off
        (dict(e_off=[0, 1], e_vars=[1], e_codes=[0]), dict(likelihoods=lc.block([[(1, v0)]]))),  # a finding variable that is evidence
        (none, dict(max_iterations=0)), (none, dict(damping=1.0)), (none, dict(damping=float("nan"))), (none, dict(tol=-1e-12)),
        (none, dict(tol=float("nan"))),
        (none, dict(acc=np.zeros(fcells + 1))), (none, dict(acc=np.zeros(fcells - 1))),      # n_acc is not fcells
        (none, dict(weight=[-1.0])), (none, dict(weight=[float("nan")])), (none, dict(weight=[float("inf")]), ),
        (none, dict(weight=[-1.0], acc=np.zeros(fcells))),
    ]
    for args, more in bad:
        acc = more.get("acc")
        with pytest.raises(_capi.MibnError) as e:
            eng.bp_evidence_batch(**args, **{"max_iterations": 5, "tol": 0.0, "damping": 0.0, **more})
        assert e.value.code == _capi.E_ARG, (args, more, e.value)
        assert acc is None or not acc.any()
        assert np.array_equal(bn.query(name, event={}).to_numpy(), before), (args, more)
    eng.set_likelihoods(lc.block([[(1, v0)], []]))  # a block of another B
    with pytest.raises(_capi.MibnError) as e:
        eng.bp_evidence_batch([0, 0], [], [], 5, 0.0, 0.0)
    assert e.value.code == _capi.E_ARG
    assert np.array_equal(bn.query(name, event={}).to_numpy(), before)
    fresh = _capi.Engine(0)
    fresh.card, fresh.family_off = np.array([2], np.int32), np.array([0, 2])  # (what set_network would have left)
    with pytest.raises(_capi.MibnError) as e:
        fresh.bp_evidence_batch([0, 0], [], [], 5, 0.0, 0.0)
    assert e.value.code == _capi.E_STATE
    fresh.set_network([256, 2], [0, 1, 3], [0, 0, 1], [0, 256, 768], np.full(768, 1.0 / 256))
    with pytest.raises(_capi.MibnError) as e:
        fresh.bp_evidence_batch([0, 0], [], [], 5, 0.0, 0.0)
    assert e.value.code == _capi.E_LIMIT and "255" in e.value.msg
    assert abs(fresh.query_fixed([[1]], np.zeros((1, 0), np.int32), np.zeros((1, 0), np.int32))[0].sum() - 1.0) <= 1e-12
    fresh.close()


# ------------------------------------------------------------------------------------------------------------------------ Python
def test_evidence_proba_and_family_marginals_against_exact_on_a_polytree():
    bn, f = device(host.polytrees()["polytree8"])
    a, b, c = f.names[0], f.names[5], f.names[7]
    lab = lambda n, k: f.domains[f.id[n]][k]
    X = pd.DataFrame({a: [lab(a, 0), None, lab(a, 1), "no such label"], b: [lab(b, 1), lab(b, 0), None, None], c: [None, lab(c, 0), None, None]},
                     dtype=object)
    exact, exact_log = bn.evidence_proba(X), bn.evidence_proba(X, log=True)
    got, info = bn.evidence_proba(X, algorithm="lbp", n_iterations=40, tol=0.0, return_info=True)
    got_log = bn.evidence_proba(X, log=True, algorithm="lbp", n_iterations=40, tol=0.0)
    assert float(np.max(np.abs(got.to_numpy() - exact.to_numpy()))) <= EXACT and got.index.equals(X.index)
    assert float(np.max(np.abs(got_log.to_numpy()[:3] - exact_log.to_numpy()[:3]))) <= EXACT
    assert got.to_numpy()[3] == 0.0 and got_log.to_numpy()[3] == -np.inf and info["converged"].all()
    part = X.iloc[:3]
    assert abs(bn.log_likelihood(part, algorithm="lbp", n_iterations=40, tol=0.0) - bn.log_likelihood(part)) <= EXACT
    one, one_info = bn.evidence_proba({a: lab(a, 0), b: lab(b, 1)}, algorithm="lbp", n_iterations=40, tol=0.0, return_info=True)
    assert abs(one - exact.to_numpy()[0]) <= EXACT and one_info["converged"] and one_info["residual"] == 0.0
    event = {c: lab(c, 0)}  # (a leaf: no family but its own holds it)
    fams, info = bn.family_marginals(event, n_iterations=40, tol=0.0, return_info=True)
    assert info["converged"] and sorted(fams) == sorted(f.names)
    del fams[c]
    for node, s in fams.items():
        members = [f.names[u] for u in f.scope[f.id[node]]]
        want = bn.query(*members, event=event)
        want = want.reorder_levels(members) if len(members) > 1 else want
        assert list(s.index.names) == members and s.name == bn.P[node].name
        assert float(np.max(np.abs(s.to_numpy() - want.reindex(s.index, fill_value=0.0).to_numpy()))) <= EXACT, node
    free = bn.family_marginals(n_iterations=40, tol=0.0)
    exact_fams = bn.family_marginals(algorithm="exact")
    for node in f.names:
        assert free[node].index.equals(exact_fams[node].index)
        assert float(np.max(np.abs(free[node].to_numpy() - exact_fams[node].to_numpy()))) <= EXACT, node
    with pytest.raises(ValueError):
        bn.family_marginals(event, algorithm="exact")  # query refuses a family member in the event


def test_fit_em_lbp_against_exact_em_on_a_polytree():
    """Missing values and one latent column; on a polytree the family beliefs are the exact posteriors, so the CPTs agree within
    1e-9 after three iterations.  A fourth iteration on rows that miss every column of a nine-member family goes through."""
    card, scopes, thetas, codes, names, domains = evh.em_case()
    X = em_host._frame(codes, names, domains)
    fitted = {}
    for algorithm in ("exact", "lbp"):
        bn = em_host._structure(scopes, names).use_device(0)
        bn.fit_em(X, n_iter=3, tol=0.0, init="counts", sub_batch=50, algorithm=algorithm, bp_iterations=2 * len(card) + 1, bp_tol=0.0)
        fitted[algorithm] = (em_host._thetas_of(bn), bn.em_log_likelihood_)
    err = max(float(np.max(np.abs(g - w))) for g, w in zip(fitted["lbp"][0], fitted["exact"][0]))
    print(f"max|theta lbp - theta exact| after three iterations: {err:.2e}; log-likelihoods {fitted['lbp'][1]} vs {fitted['exact'][1]}")
    assert err <= EXACT and np.allclose(fitted["lbp"][1], fitted["exact"][1], rtol=1e-9, atol=0)
    latent = names[1]
    for algorithm in ("exact", "lbp"):
        bn = em_host._structure(scopes, names).use_device(0)
        for v in range(len(card)):
            bn.P[names[v]] = learning._em_series(names[v], [names[u] for u in scopes[v][:-1]], {n: pd.Index(d) for n, d in zip(names, domains)}, thetas[v])
        bn.prepare()
        bn.fit_em(X.drop(columns=[latent]), n_iter=3, tol=0.0, algorithm=algorithm, bp_iterations=2 * len(card) + 1, bp_tol=0.0)
        fitted[algorithm] = (em_host._thetas_of(bn), bn.em_log_likelihood_)
    err = max(float(np.max(np.abs(g - w))) for g, w in zip(fitted["lbp"][0], fitted["exact"][0]))
    print(f"one latent column: max|theta lbp - theta exact| {err:.2e}")
    assert err <= EXACT and np.allclose(fitted["lbp"][1], fitted["exact"][1], rtol=1e-9, atol=0)


def test_fit_em_lbp_takes_a_row_that_misses_more_than_eight_members_of_a_family():
    spec = netspec.hub_spec(3, 2, (2,) * 9, (2,))  # the hub's family has ten members
    nodes = spec["nodes"]
    hub = nodes[9]
    dom = netspec.domains(spec)
    rng = np.random.default_rng(8)
    X = pd.DataFrame({n: [dom[n][int(k)] for k in rng.integers(0, 2, size=40)] for n in nodes}, dtype=object)
    X.iloc[:5, :10] = None  # five rows miss all ten members of the hub's family
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    with pytest.raises(ValueError, match="more than 8"):
        bn.fit_em(X, n_iter=1, init="current")
    bn.fit_em(X, n_iter=2, tol=0.0, init="current", algorithm="lbp", bp_iterations=10, bp_tol=0.0)
    assert bn.em_iterations_ == 2 and np.all(np.isfinite(bn.em_log_likelihood_))
    assert abs(float(bn._counts[hub].sum()) - len(X)) <= 1e-9  # every row, the five included, gave the family one unit of count


# ------------------------------------------------------------------------------------------------- beyond the reach of exact calls
def test_grid_20x20_where_the_exact_call_raises():
    bn, f = device(netspec.grid_spec(20, 20, 4, seed=1))
    ev = {0: 1, 399: 2, 210: 0}
    event = {f.names[v]: f.domains[v][c] for v, c in ev.items()}
    with pytest.raises(_capi.MibnError) as e:
        bn.evidence_proba(event)
    assert e.value.code in (_capi.E_NOMEM, _capi.E_LIMIT)
    got, info = bn.evidence_proba(event, log=True, algorithm="lbp", n_iterations=30, return_info=True)
    assert bn.backend.engine.stats()["arena_bytes"] == 0  # (in LDS)
    want = bev.run(f, ev, [], 30, 1e-9, 0.0)
    print(f"20x20: log_z {got!r} (twin {want.log_z!r}), {info['iterations']} iterations (twin {want.iterations}), residual {info['residual']:.3e}")
    assert np.isfinite(got) and close_log(got, want.log_z) and info["iterations"] == want.iterations
    fams = bn.family_marginals(event, n_iterations=30)
    foff = bev.family_layout(bc.graph(f))[0]
    v = f.id[f.names[211]]
    assert float(np.max(np.abs(fams[f.names[211]].to_numpy() - want.fbeliefs[foff[v]:foff[v + 1]]))) <= TWIN


def test_chain_of_1000_fully_observed_has_a_finite_log_where_the_probability_underflows():
    """1 000 four-state variables (the library takes 1 024 at most, so the 1 200 first thought of do not load): 240 n + 544 bytes of
    state, MsgGlobal from n = 681; P(e) is far below the smallest double and the logarithm is still the sum of the log CPT entries."""
    n = 1000
    bn, f = device(netspec.chain_spec(n, (4,), seed=9))
    G = bc.graph(f)
    codes = np.random.default_rng(4).integers(0, 4, size=n)
    event = {f.names[v]: f.domains[v][int(codes[v])] for v in range(n)}
    want = float(sum(np.log(G.table[v][tuple(int(codes[u]) for u in G.scope[v])]) for v in range(n)))
    assert want < np.log(np.finfo(np.float64).tiny) - 100 and np.isfinite(want)
    got = bn.evidence_proba(event, log=True, algorithm="lbp", n_iterations=5)
    assert bn.backend.engine.stats()["arena_bytes"] > 0  # (MsgGlobal books its slabs)
    print(f"chain {n}: log_z {got!r}, sum of the log CPT entries {want!r}")
    assert abs(got - want) <= EXACT * abs(want)
    assert bn.evidence_proba(event, algorithm="lbp", n_iterations=5) == 0.0
    assert bn.log_likelihood(pd.DataFrame([event], dtype=object), algorithm="lbp", n_iterations=5) == got
