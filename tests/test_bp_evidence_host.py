"""The Bethe log Z and the family beliefs of loopy belief propagation on a CPU: the numpy twin of what include/mibn.h pins for
mibn_bp_evidence_batch (tests/bp_evidence_check.py) against brute force where belief propagation is exact, against bp_check's twin of
mibn_bp_batch bit for bit, the zero-mass rules, the host plan (sorobn_amd/csrc/bp_plan.h through tools/bp_plan_sim.cpp) against
layouts worked out here, and the Python surface over TEST DOUBLES of the engine (never on the product path)."""
import os
import subprocess
import types

import numpy as np
import pandas as pd
import pytest

import bp_check as bc
import bp_evidence_check as bev
import em_check as em
import netspec
import sim_tools
import sorobn_amd
import test_bp_host as host
import test_em_host as em_host
from sorobn_amd import _capi, learning

E_ARG, E_LIMIT = -1, -6
KIB = 1024
GRIDS = [(3, 3, 3), (3, 3, 2), (4, 3, 2), (3, 4, 3)]


def grid(R, C, K):
    return host.flat(netspec.grid_spec(R, C, K, seed=4))


# ---------------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("name", ["chain5", "hub", "polytree8"])
def test_twin_is_exact_on_polytrees(name):
    """With tol = 0 and 2 n + 1 iterations the residual is exactly 0, log_z the brute-force log mass and every family belief the
    brute-force family posterior, within 1e-12; beliefs, iterations and residual are bp_check.run's bit for bit."""
    f = host.flat(host.polytrees()[name])
    n = len(f.card)
    for k, (ev, fs) in enumerate(host.requests_of(f, 7)):
        got = bev.run(f, ev, fs, max_iterations=2 * n + 1, tol=0.0)
        want_z, want_fb = bev.brute(f, ev, fs)
        ez, eb = abs(got.log_z - want_z), float(np.max(np.abs(got.fbeliefs - want_fb)))
        print(f"{name}[{k}]: {got.iterations} iterations, residual {got.residual!r}, |log_z - brute| {ez:.2e}, max|family belief - brute| {eb:.2e}")
        assert got.residual == 0.0 and 1 <= got.iterations <= 2 * n + 1
        assert ez <= 1e-12 and eb <= 1e-12, (name, k, ez, eb)
        bel, it, r = bc.run(f, ev, fs, max_iterations=2 * n + 1, tol=0.0)
        assert np.array_equal(got.beliefs, bel) and got.iterations == it and got.residual == r


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_twin_beliefs_are_bp_checks_bit_for_bit_on_a_loopy_grid(damping):
    f = grid(3, 3, 3)
    for ev in ({}, {0: 1, 8: 2}):
        for its in (1, 2, 7):
            got = bev.run(f, ev, [], its, 0.0, damping)
            bel, it, r = bc.run(f, ev, [], its, 0.0, damping)
            assert np.array_equal(got.beliefs, bel) and got.iterations == it and got.residual == r


@pytest.mark.parametrize("R,C,K", GRIDS)
def test_log_z_without_evidence_is_zero_on_loopy_grids(R, C, K):
    """Child-to-parent messages of a normalised network without evidence are uniform: the Bethe value is log 1."""
    got = bev.run(grid(R, C, K), {}, [], max_iterations=200, tol=1e-12)
    print(f"grid {R}x{C} K={K}: log_z {got.log_z!r} after {got.iterations} iterations")
    assert abs(got.log_z) <= 1e-12


@pytest.mark.parametrize("R,C,K", GRIDS)
def test_log_z_with_evidence_on_loopy_grids_is_finite(R, C, K):
    """The approximation's error against the exact log P(e) is printed, not bounded: there is no bound."""
    f = grid(R, C, K)
    rng = np.random.default_rng(R * 100 + C * 10 + K)
    for n_ev in (1, 2, 3):
        ev = {int(v): int(rng.integers(K)) for v in rng.choice(R * C, size=n_ev, replace=False)}
        got = bev.run(f, ev, [], max_iterations=200, tol=1e-12)
        want, _ = bev.brute(f, ev)
        print(f"grid {R}x{C} K={K} evidence {ev}: log_z {got.log_z:.6f}, exact {want:.6f}, error {got.log_z - want:+.2e}, residual {got.residual:.1e}")
        assert np.isfinite(got.log_z)


@pytest.mark.parametrize("make", [lambda: host.flat(host.polytrees()["polytree8"]), lambda: grid(3, 4, 3)])
def test_every_variable_observed_gives_the_sum_of_the_log_cpt_entries(make):
    f = make()
    G = bc.graph(f)
    rng = np.random.default_rng(3)
    ev = {v: int(rng.integers(G.card[v])) for v in range(G.n)}
    got = bev.run(f, ev, [], max_iterations=50, tol=0.0)
    want = float(sum(np.log(G.table[v][tuple(ev[u] for u in G.scope[v])]) for v in range(G.n)))
    assert abs(got.log_z - want) <= 1e-12 * abs(want), (got.log_z, want)
    fb = got.fbeliefs
    assert np.all((fb == 0.0) | (np.abs(fb - 1.0) <= 1e-15)) and abs(fb.sum() - G.n) <= 1e-12  # one-hot families


def test_zero_mass_rules():
    f = host.flat(host.zero_spec())
    width, fcells = int(np.sum(f.card)), bev.family_layout(bc.graph(f))[1]

    def dead(r, it_min):
        assert r.log_z == -np.inf and r.residual == 0.0 and r.iterations >= it_min
        assert np.array_equal(r.beliefs, np.zeros(len(r.beliefs))) and np.array_equal(r.fbeliefs, np.zeros(len(r.fbeliefs)))
    r = bev.run(f, {0: 0, 1: 1}, [], max_iterations=20, tol=0.0)  # impossible evidence, seen in a step
    dead(r, 1)
    assert (len(r.beliefs), len(r.fbeliefs)) == (width, fcells) == (6, 10)
    assert bev.brute(f, {0: 0, 1: 1})[0] == -np.inf
    g = host.flat(netspec._dag_spec("root0", [2], [[]], lambda i: np.array([0.0, 1.0])))
    r = bev.run(g, {0: 0}, [], max_iterations=5, tol=0.0)  # a root observed at prior 0: only the final phase shows it
    dead(r, 1)
    assert r.iterations == bc.run(g, {0: 0}, [], max_iterations=5, tol=0.0)[1]
    for ev, fs in (({2: -1}, []), ({}, [(1, np.zeros(2))])):  # lambda alone shows it
        r = bev.run(f, ev, fs, max_iterations=20, tol=0.0)
        dead(r, 0)
        assert r.iterations == 0
    r = bev.run(f, {0: 0, 1: 0}, [], max_iterations=20, tol=0.0)  # possible evidence next to them
    assert abs(r.log_z - np.log(0.3 * 1.0)) <= 1e-12


def test_accumulation_rule_is_sequential():
    rows = [np.array([0.1, 0.2]), np.array([0.3, 0.4]), np.array([1e-17, 0.0])]
    got = bev.accumulate(np.array([1.0, 2.0]), rows, [1.0, 2.0, 1.0])
    assert got.tolist() == [((1.0 + 0.1) + 2.0 * 0.3) + 1e-17, ((2.0 + 0.2) + 2.0 * 0.4) + 0.0]
    assert np.array_equal(bev.accumulate(np.zeros(2), rows), bev.accumulate(np.zeros(2), rows, np.ones(3)))


# ------------------------------------------------------------------------------------------------------------------ the host plan
def parse(line):
    """One output line of bp_plan_sim's ev modes: key=value pairs (foff a list), or error=<code> msg=<to the end of the line>."""
    if line.startswith("error="):
        code, msg = line.split(" ", 1)
        return {"error": int(code[6:]), "msg": msg[4:]}
    out = {}
    for kv in line.split():
        k, v = kv.split("=")
        out[k] = v if k == "form" else [int(x) for x in v.split(",") if x] if k == "foff" else int(v)
    return out


@pytest.fixture(scope="module")
def ev_sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bp_ev") / "bp_plan_sim")
    r = subprocess.run(["g++", "-O2", "-mpopcnt", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(host.ROOT, "tools", "bp_plan_sim.cpp"),
                        os.path.join(host.ROOT, "sorobn_amd", "csrc", "planner.cpp"), "-lpthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(f, lines):
        out = subprocess.run([exe], input="\n".join(sim_tools.network_prefix(f) + list(lines)) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        res = [parse(ln) for ln in out.stdout.splitlines()]
        assert len(res) == len(lines)
        return res
    return run


@host.needs_gxx
@pytest.mark.parametrize("name", ["sprinkler", "asia", "grid3x3"])
def test_ev_plan_layout(ev_sim, name):
    """mu0 | mu1 | nu of 8 * cells bytes each, lambda of 8 * sum(card), zf and term of 8 * n_vars, 64 partials, 128 bytes of reduction
    slots; the family-belief row: the tables back to back."""
    f = host.flat(netspec.grid_spec(3, 3, 2, seed=4)) if name == "grid3x3" else host.example(name)
    edges, variables, _, _, cells, lam = bc.edge_records(f)
    n = len(f.card)
    sizes = [rec[7] for rec in variables]
    for q, form in zip(ev_sim(f, ["ev 1", "ev 0"]), ("MsgLds", "MsgGlobal")):
        assert q["form"] == form
        assert (q["mu0"], q["mu1"], q["nu"], q["lam"]) == (0, 8 * cells, 16 * cells, 24 * cells)
        zf = 24 * cells + 8 * lam
        assert (q["zf"], q["term"], q["part"], q["red"]) == (zf, zf + 8 * n, zf + 16 * n, zf + 16 * n + 512)
        assert q["total"] == zf + 16 * n + 512 + 128 and q["slab"] == (q["total"] + 15) // 16 * 16
        assert q["foff"] == [sum(sizes[:v]) for v in range(n + 1)] and q["fcells"] == sum(sizes)
        assert q["foff"] == bev.family_layout(bc.graph(f))[0].tolist()
        assert q["foff"] == learning.em_family_layout(bc.graph(f).scope, f.card)[0].tolist()
        assert q["threads"] == min(256, max(64, (len(edges) + 63) // 64 * 64))
        assert q["iter_bytes"] == 8 * sum(rec[5] * rec[7] for rec in variables)


@host.needs_gxx
def test_ev_plan_forms_and_launches(ev_sim):
    """A chain of n four-state variables has 2 n - 1 edges: 24 * 4 (2 n - 1) + 32 n + 16 n + 512 + 128 = 240 n + 544 bytes.  n = 680
    is the last that fits 160 KiB."""
    under, over = host.chain_prefix(680, 4), host.chain_prefix(681, 4)
    assert 240 * 680 + 544 <= 160 * KIB < 240 * 681 + 544
    (a, a0), (b,) = ev_sim(under, ["ev 1", "ev 0"]), ev_sim(over, ["ev 1"])
    assert (a["total"], a["form"], a0["form"]) == (240 * 680 + 544, "MsgLds", "MsgGlobal")
    assert (b["total"], b["form"]) == (240 * 681 + 544, "MsgGlobal")
    # launches: with the family-belief buffer every request needs a row of 8 * fcells bytes, in the global form a slab besides
    slab, row = b["slab"], 8 * b["fcells"]
    assert b["fcells"] == 4 + 16 * 680 and slab == (b["total"] + 15) // 16 * 16
    res = ev_sim(over, ["ev_launch 1 0 32768 1e12", f"ev_launch 1 0 32768 {10 * slab + 5}", f"ev_launch 1 1 32768 {10 * slab + 5}",
                        f"ev_launch 1 1 32768 {10 * (slab + row)}", f"ev_launch 1 1 4 {10 * (slab + row)}", f"ev_launch 1 1 32768 {slab + row - 1}",
                        f"ev_launch 1 0 32768 {slab + row - 1}", f"ev_launch 1 0 32768 {slab - 1}"])
    assert [r["requests"] for r in res] == [32768, 10, 10 * slab // (slab + row), 10, 4, 0, 1, 0]
    row = 8 * a["fcells"]
    res = ev_sim(under, ["ev_launch 1 0 32768 0", f"ev_launch 1 1 32768 {7 * row}", f"ev_launch 1 1 32768 {row - 1}", "ev_launch 0 0 100 1e12",
                         "ev_launch 0 0 100 0"])
    assert [r["requests"] for r in res] == [32768, 7, 0, 100, 0]


@host.needs_gxx
def test_ev_plan_argument_errors(ev_sim):
    f = host.example("sprinkler")
    fcells = bev.family_layout(bc.graph(f))[1]
    good = [f"ev_acc 1 {fcells} 0", f"ev_acc 1 -1 3 0 1.5 1e300", f"ev_acc 1 {fcells} 2 1 1"]
    bad = [f"ev_acc 1 {fcells + 1} 0", "ev_acc 1 0 0", f"ev_acc 1 {fcells} 2 1 -1e-300", "ev_acc 1 -1 2 nan 1", "ev_acc 1 -1 1 inf"]
    res = ev_sim(f, good + bad)
    assert all(r == {"ok": 1} for r in res[:3]), res[:3]
    assert all(r.get("error") == E_ARG for r in res[3:]), res[3:]
    assert "n_acc" in res[3]["msg"] and "weight" in res[5]["msg"] and "request 0" in res[6]["msg"]
    big = types.SimpleNamespace(card=[256, 2], scope_off=[0, 1, 2], scope_vars=[0, 1], value_off=[0, 256, 258],
                                values=np.concatenate([np.full(256, 1 / 256), [0.5, 0.5]]))
    for line in ("ev 1", "ev_launch 1 1 8 1e9", "ev_acc 1 -1 0"):
        (r,) = ev_sim(big, [line])
        assert r["error"] == E_LIMIT and "cardinality above 255" in r["msg"], r


# -------------------------------------------------------------------------------------------------------------- the Python surface
class Recorder:
    """Stands in for the engine: answers the exact calls, fails the approximate one."""

    def __init__(self, card):
        self.card, self.calls = np.asarray(card, np.int32), []

    def query_fixed(self, qvars, evars, ecodes, flags=0, likelihoods=None):
        self.calls.append("query_fixed")
        return np.full((len(qvars), 1), 0.25)

    def bp_evidence_batch(self, *a, **k):
        raise AssertionError("algorithm='exact' must not reach bp_evidence_batch")

    bp_evidence = bp_evidence_batch


def test_argument_errors_need_no_engine_and_exact_takes_the_old_path():
    bn = host.sim_net("sprinkler")
    a = bn._all_names()[0]
    label = bn.backend.flat.domains[bn.backend.flat.id[a]][0]
    frame = pd.DataFrame({a: [label, None]}).astype(object)
    bn.backend.engine = None  # (any use of an engine below is an AttributeError)
    calls = (lambda **k: bn.evidence_proba({a: label}, **k), lambda **k: bn.evidence_proba(frame, **k), lambda **k: bn.log_likelihood(frame, **k),
             lambda **k: bn.family_marginals({a: label}, **k))
    for call in calls[:3]:
        with pytest.raises(ValueError, match="exact, lbp"):
            call(algorithm="gibbs")
    with pytest.raises(ValueError, match="lbp, exact"):
        bn.family_marginals(algorithm="gibbs")
    for call in calls:
        for bad in (dict(damping=1.0), dict(damping=-0.1), dict(damping=float("nan")), dict(tol=-1.0), dict(tol=float("nan")),
                    dict(n_iterations=0), dict(n_iterations=2.5)):
            with pytest.raises(ValueError, match=next(iter(bad))):
                call(algorithm="lbp", **bad)
    with pytest.raises(KeyError):
        bn.evidence_proba({"no such node": 1}, algorithm="lbp")
    with pytest.raises(KeyError):
        bn.family_marginals({"no such node": 1})
    X = pd.DataFrame({a: [label]}).astype(object)
    for bad in (dict(algorithm="bp"), dict(algorithm="lbp", bp_iterations=0), dict(algorithm="lbp", bp_tol=-1.0), dict(algorithm="lbp", damping=1.0)):
        with pytest.raises(ValueError):
            bn.fit_em(X, **bad)
    rec = bn.backend.engine = Recorder(bn.backend.flat.card)
    assert bn.evidence_proba({a: label}) == 0.25 and rec.calls == ["query_fixed"]
    p, info = bn.evidence_proba({a: label}, log=True, algorithm="exact", return_info=True)
    assert p == np.log(0.25) and info == {"iterations": 0, "residual": 0.0, "converged": True}
    s, table = bn.evidence_proba(frame, return_info=True)
    assert s.tolist() == [0.25, 0.25] and list(table.columns) == ["iterations", "residual", "converged"] and table["converged"].all()
    assert table.index.equals(frame.index)
    assert bn.log_likelihood(frame) == 2 * np.log(0.25)


class TwinEngine:
    """TEST DOUBLE for the engine behind a Backend (never on the product path): bp_evidence_batch by the numpy twin."""

    calls = []  # the requests of every call, of every engine of the class (a Backend makes a new one when the CPTs change)

    def __init__(self, device=0, planner_only=False):
        pass

    def set_network(self, card, scope_off, scope_vars, value_off, values):
        self.card = np.asarray(card, np.int32)
        self.f = types.SimpleNamespace(card=self.card, scope_off=np.asarray(scope_off), scope_vars=np.asarray(scope_vars),
                                       value_off=np.asarray(value_off), values=np.asarray(values, np.float64))
        self.family_off = bev.family_layout(bc.graph(self.f))[0]

    def set_order_hints(self, hints):
        pass

    def bp_evidence_batch(self, e_off, e_vars, e_codes, max_iterations=100, tol=1e-9, damping=0.0, likelihoods=None, weight=None, acc=None,
                          beliefs=False, fbeliefs=False):
        B = len(e_off) - 1
        self.calls.append(B)
        runs = [bev.run(self.f, {int(v): int(c) for v, c in zip(e_vars[e_off[b]:e_off[b + 1]], e_codes[e_off[b]:e_off[b + 1]])}, [],
                        max_iterations, tol, damping) for b in range(B)]
        if acc is not None:
            acc[:] = bev.accumulate(acc, [r.fbeliefs for r in runs], weight)
        stack = lambda rows, width: np.array(rows).reshape(B, width)
        return (np.array([r.log_z for r in runs]), stack([r.beliefs for r in runs], int(self.card.sum())) if beliefs else None,
                stack([r.fbeliefs for r in runs], int(self.family_off[-1])) if fbeliefs else None,
                np.array([r.iterations for r in runs], np.int32), np.array([r.residual for r in runs]))

    def bp_evidence(self, evars, ecodes, max_iterations=100, tol=1e-9, damping=0.0, **more):
        evars = np.asarray(evars, np.int32).reshape(len(evars), -1)
        e_off = np.arange(len(evars) + 1, dtype=np.int64) * evars.shape[1]
        return self.bp_evidence_batch(e_off, evars.reshape(-1), np.asarray(ecodes, np.int32).reshape(-1), max_iterations, tol, damping, **more)


def polytree_net(rng, V=6):
    """(card, scopes, thetas) of a random polytree in the numbering of em_check: node v takes up to two earlier parents from
    different components."""
    card = rng.integers(2, 4, size=V).astype(np.int32)
    comp, scopes, thetas = list(range(V)), [], []
    for v in range(V):
        ps, want = [], int(rng.integers(0, 3))
        for p in rng.permutation(v).tolist():
            if len(ps) < want and all(comp[p] != comp[q] for q in ps):
                ps.append(p)
        for p in ps:
            old = comp[p]
            comp = [v if c == old else c for c in comp]
        scopes.append(sorted(ps) + [v])
        rows = int(np.prod([card[u] for u in ps], dtype=np.int64))
        thetas.append(rng.dirichlet(np.ones(card[v]), size=rows).reshape(-1))
    return card, scopes, thetas


def em_case(seed=12, n_rows=120):
    """A polytree with missing cells, named and numbered as the library will number it -> (card, scopes, thetas, codes, names, domains)."""
    rng = np.random.default_rng(seed)
    card, scopes, thetas = polytree_net(rng)
    V = len(card)
    names = [f"n{v}" for v in range(V)]
    domains = [[f"s{k}" for k in range(card[v])] for v in range(V)]
    full = em.sample_rows(card, scopes, thetas, n_rows, rng)
    codes = em.knock_out(full, 0.3, rng)
    assert all(len(np.unique(codes[codes[:, v] >= 0, v])) == card[v] for v in range(V))  # (every label is observed: the domains are the net's)
    order = [names.index(n) for n in em_host._structure(scopes, names).nodes]
    card, scopes, thetas, codes = em.relabel(card, scopes, thetas, codes, order)
    return card, scopes, thetas, codes, [names[o] for o in order], [domains[o] for o in order]


def test_fit_em_lbp_with_the_twin_as_engine_reproduces_brute_force_em(monkeypatch):
    """On a polytree the family beliefs are the exact family posteriors, so EM with the approximate E-step is EM: CPTs, expected
    counts and log-likelihoods within 1e-9 of tests/em_check.py after three iterations - one request per row, rows in X's order in
    calls of sub_batch, no count-kernel pass."""
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", TwinEngine)

    def no_counting(device=None):
        raise AssertionError("algorithm='lbp' with init='uniform' needs no count kernel")
    monkeypatch.setattr(learning, "counting_engine", no_counting)
    card, scopes, thetas, codes, names, domains = em_case()
    TwinEngine.calls.clear()
    assert max(len(sc) for sc in scopes) == 3 and (codes < 0).any(axis=1).sum() > 20
    X = em_host._frame(codes, names, domains)
    bn = em_host._structure(scopes, names)
    assert bn.nodes == names
    bn.fit_em(X, n_iter=3, tol=0.0, init="uniform", sub_batch=50, algorithm="lbp", bp_iterations=2 * len(card) + 1, bp_tol=0.0)
    start = [np.full(len(t), 1.0 / card[v]) for v, t in enumerate(thetas)]
    want, lls, counts = em.em(card, scopes, start, codes, 3)
    got = em_host._thetas_of(bn)
    err = max(float(np.max(np.abs(g - w))) for g, w in zip(got, want))
    print(f"max|theta - brute-force EM| after three iterations: {err:.2e}; log-likelihoods {bn.em_log_likelihood_} vs {lls}")
    assert err <= 1e-9
    assert np.allclose(bn.em_log_likelihood_, lls, rtol=1e-9, atol=0) and bn.em_iterations_ == 3
    assert max(float(np.max(np.abs(bn._counts[names[v]].to_numpy() - counts[v].reshape(-1)))) for v in range(len(card))) <= 1e-9
    assert TwinEngine.calls == [50, 50, 20] * 3


def test_python_surface_over_the_twin(monkeypatch):
    """evidence_proba / log_likelihood / family_marginals with algorithm='lbp' through the twin: the row's log_z itself with `log`,
    0 / -inf for a label outside its domain, the families in the layout of bn.P."""
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", TwinEngine)
    spec = host.polytrees()["polytree8"]
    bn = netspec.build(spec, sorobn_amd.BayesNet)
    f = bn.backend.flat
    a, b = f.names[0], f.names[5]
    X = pd.DataFrame({a: [f.domains[0][0], None, "no such label"], b: [f.domains[5][1], f.domains[5][0], None]}, dtype=object)
    lz, info = bn.evidence_proba(X, log=True, algorithm="lbp", n_iterations=20, tol=0.0, return_info=True)
    want = [bev.brute(host.flat(spec), ev)[0] for ev in ({0: 0, 5: 1}, {5: 0})]
    assert np.allclose(lz.to_numpy()[:2], want, rtol=0, atol=1e-12) and lz.to_numpy()[2] == -np.inf
    assert info["converged"].tolist() == [True, True, True] and info["iterations"].tolist()[2] == 0
    p = bn.evidence_proba(X, algorithm="lbp", n_iterations=20, tol=0.0)
    assert np.array_equal(p.to_numpy(), np.exp(lz.to_numpy())) and p.to_numpy()[2] == 0.0
    assert bn.log_likelihood(X.iloc[:2], algorithm="lbp", n_iterations=20, tol=0.0) == float(lz.iloc[:2].sum())
    v, info = bn.evidence_proba({a: f.domains[0][0], b: None}, algorithm="lbp", n_iterations=20, tol=0.0, return_info=True, log=True)
    assert abs(v - bev.brute(host.flat(spec), {0: 0})[0]) <= 1e-12 and info["converged"]
    fams = bn.family_marginals({a: f.domains[0][0]}, n_iterations=20, tol=0.0)
    _, want_fb = bev.brute(host.flat(spec), {0: 0})
    foff = bev.family_layout(bc.graph(host.flat(spec)))[0]
    assert sorted(fams) == sorted(f.names)
    for i, node in enumerate(f.names):
        s = fams[node]
        assert list(s.index.names) == [f.names[u] for u in f.scope[i]] and s.name == bn.P[node].name
        assert float(np.max(np.abs(s.to_numpy() - want_fb[foff[i]:foff[i + 1]]))) <= 1e-12
        assert abs(s.sum() - 1.0) <= 1e-12


def test_bp_evidence_batch_is_declared_and_exported():
    assert "mibn_bp_evidence_batch" in _capi.SYMBOLS
    assert hasattr(_capi.lib(), "mibn_bp_evidence_batch")
    assert hasattr(_capi.Engine, "bp_evidence_batch") and hasattr(_capi.Engine, "bp_evidence") and hasattr(sorobn_amd.BayesNet, "family_marginals")
