"""Loopy belief propagation on a CPU: the numpy twin of the schedule include/mibn.h pins (tests/bp_check.py) against brute-force
marginals where belief propagation is exact, the zero-mass rules, the host plan (sorobn_amd/csrc/bp_plan.h through tools/bp_plan_sim.cpp)
against records worked out here from the rules in the header - none copied from the tool -, and the parts of the Python surface the CPU
stand-in engine can answer."""
import os
import shutil
import subprocess
import types

import numpy as np
import pandas as pd
import pytest

import bp_check as bc
import golden_util as gu
import mpe_check as mc
import netspec
import sim_tools
import simengine
import sorobn_amd

ROOT = sim_tools.ROOT
E_ARG, E_LIMIT = -1, -6
KIB = 1024


def flat(spec):
    return mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))


def polytree_spec(seed, n=8, cards=(2, 3, 4)):
    """A random polytree: node i takes 0 .. 2 parents among the earlier nodes, no two from one connected component - so the
    undirected graph stays a forest, with nodes of two parents in it."""
    rng = np.random.default_rng(seed)
    comp = list(range(n))
    card = [int(rng.choice(cards)) for _ in range(n)]
    parents = []
    for i in range(n):
        ps, want = [], int(rng.integers(0, 3))
        for p in rng.permutation(i).tolist():
            if len(ps) < want and all(comp[p] != comp[q] for q in ps):
                ps.append(p)
        for p in ps:
            old = comp[p]
            comp = [i if c == old else c for c in comp]
        parents.append(sorted(ps))
    return netspec._dag_spec(f"polytree{seed}", card, parents, lambda i: rng.dirichlet(np.ones(card[i])))


def polytrees():
    """{name: flattened network}: the three networks of the issue, shared with tests/test_bp.py."""
    return {"chain5": netspec.chain_spec(5, (2, 3, 4), seed=3), "hub": netspec.hub_spec(5, 3, (2, 3), (2, 4, 3)), "polytree8": polytree_spec(11)}


def requests_of(f, seed):
    """[(evidence, findings)]: none, evidence on two variables, one finding."""
    rng = np.random.default_rng(seed)
    n = len(f.card)
    a, b, c = (int(v) for v in rng.choice(n, size=3, replace=False))
    return [({}, []), ({a: int(rng.integers(f.card[a])), b: int(rng.integers(f.card[b]))}, []),
            ({a: int(rng.integers(f.card[a]))}, [(c, rng.uniform(0.1, 2.0, int(f.card[c])))])]


def test_polytree_generator_has_a_node_with_two_parents():
    spec = polytree_spec(11)
    assert len(spec["nodes"]) == 8
    assert max(len(c["names"]) for c in spec["cpts"].values()) == 3
    assert {len(netspec.domains(spec)[n]) for n in spec["nodes"]} <= {2, 3, 4}


@pytest.mark.parametrize("name", ["chain5", "hub", "polytree8"])
def test_twin_is_exact_on_polytrees(name):
    """Marginals within 1e-12 of brute force; with tol = 0 the residual reaches exactly 0 within 2 n + 1 iterations - the factor
    graph's diameter bounds it, and a fixed point recomputed from itself is bit-identical."""
    f = flat(polytrees()[name])
    n = len(f.card)
    for k, (ev, fs) in enumerate(requests_of(f, 7)):
        bel, it, r = bc.run(f, ev, fs, max_iterations=2 * n + 1, tol=0.0)
        want = bc.brute(f, ev, fs)
        err = float(np.max(np.abs(bel - want)))
        print(f"{name}[{k}]: {it} iterations, residual {r!r}, max|err| vs brute force {err:.2e}")
        assert r == 0.0 and 1 <= it <= 2 * n + 1, (name, k, it, r)
        assert err <= 1e-12, (name, k, err)
        # damping leaves the fixed point where it is
        bel_d, it_d, r_d = bc.run(f, ev, fs, max_iterations=400, tol=1e-14, damping=0.5)
        assert r_d <= 1e-14 and float(np.max(np.abs(bel_d - want))) <= 1e-12, (name, k, it_d, r_d)


def zero_spec():
    """000 -> 001 with P(001 = 1 | 000 = 0) = 0, and a child 002 of 001."""
    rows = {0: [[0.3, 0.7]], 1: [[1.0, 0.0], [0.4, 0.6]], 2: [[0.5, 0.5], [0.2, 0.8]]}
    it = {i: iter(r) for i, r in rows.items()}
    return netspec._dag_spec("zero", [2, 2, 2], [[], [0], [1]], lambda i: np.array(next(it[i])))


def test_zero_mass_rules():
    f = flat(zero_spec())
    width = int(np.sum(f.card))
    # impossible evidence: seen in an iteration, every belief zero, residual 0
    bel, it, r = bc.run(f, {0: 0, 1: 1}, [], max_iterations=20, tol=0.0)
    assert it >= 1 and r == 0.0 and np.array_equal(bel, np.zeros(width)), (it, r, bel)
    assert np.array_equal(bc.brute(f, {0: 0, 1: 1}), np.zeros(width))
    # ... also where only the beliefs show it: a root observed at a state of prior 0
    g = flat(netspec._dag_spec("root0", [2], [[]], lambda i: np.array([0.0, 1.0])))
    bel, it, r = bc.run(g, {0: 0}, [], max_iterations=5, tol=0.0)
    assert it >= 1 and r == 0.0 and np.array_equal(bel, np.zeros(2)), (it, r, bel)
    # an evidence code of -1 and an all-zero finding: lambda alone shows it, iteration 0
    for ev, fs in (({2: -1}, []), ({}, [(1, np.zeros(2))])):
        bel, it, r = bc.run(f, ev, fs, max_iterations=20, tol=0.0)
        assert it == 0 and r == 0.0 and np.array_equal(bel, np.zeros(width)), (ev, fs, it, r)
    # possible evidence next to them: one-hot beliefs on the evidence, everything normalised
    bel, it, r = bc.run(f, {0: 0, 1: 0}, [], max_iterations=20, tol=0.0)
    assert list(bel[:4]) == [1.0, 0.0, 1.0, 0.0] and abs(bel[4:].sum() - 1.0) <= 1e-15
    assert float(np.max(np.abs(bel - bc.brute(f, {0: 0, 1: 0})))) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ the host plan
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _parse(line):
    if line.startswith("error="):
        code, msg = line.split(" ", 1)
        return {"error": int(code[6:]), "msg": msg[4:]}
    out = {}
    for kv in line.split():
        k, v = kv.split("=")
        out[k] = v if k == "form" else [int(x) for x in v.split(",") if x] if k in ("edges", "vars", "nbr", "nbr_moff") else int(v)
    return out


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bp") / "bp_plan_sim")
    r = subprocess.run(["g++", "-O2", "-mpopcnt", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "bp_plan_sim.cpp"),
                        os.path.join(ROOT, "sorobn_amd", "csrc", "planner.cpp"), "-lpthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(f, lines):
        out = subprocess.run([exe], input="\n".join(sim_tools.network_prefix(f) + list(lines)) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        res = [_parse(ln) for ln in out.stdout.splitlines()]
        assert len(res) == len(lines)
        return res
    return run


def example(name):
    return flat(next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == name))


def chain_prefix(n, card):
    """A chain of n variables of `card` states with uniform CPTs, as the arrays of mibn_set_network."""
    scope, scope_off, value_off = [], [0], [0]
    for v in range(n):
        scope += [v - 1, v] if v else [v]
        scope_off.append(len(scope))
        value_off.append(value_off[-1] + (card * card if v else card))
    return types.SimpleNamespace(card=[card] * n, scope_off=scope_off, scope_vars=scope, value_off=value_off, values=np.full(value_off[-1], 1.0 / card))


@needs_gxx
@pytest.mark.parametrize("name", ["sprinkler", "asia", "grid3x3"])
def test_plan_records(sim, name):
    """Edge numbering, moff, the neighbour lists and the layout, each from the rules: edges by ascending factor then scope position,
    moff the running sum of card(u), N(u) ascending, mu0 | mu1 | nu of 8 * cells bytes each, lambda of 8 * sum(card), 64 bytes of
    reduction slots."""
    f = flat(netspec.grid_spec(3, 3, 2, seed=4)) if name == "grid3x3" else example(name)
    edges, variables, nbr, nbr_moff, cells, lam = bc.edge_records(f)
    p = sim(f, ["plan 1", "plan 0", f"layout {cells} {lam}"])
    for q, form in zip(p[:2], ("MsgLds", "MsgGlobal")):
        assert q["form"] == form
        assert q["n_edges"] == len(edges) == sum(len(bc.graph(f).scope[v]) for v in range(len(f.card)))
        assert q["edges"] == [w for rec in edges for w in rec]
        assert q["vars"] == [w for rec in variables for w in rec]
        assert q["nbr"] == nbr and q["nbr_moff"] == nbr_moff
        assert (q["cells"], q["lam_cells"]) == (cells, lam)
        assert (q["mu0"], q["mu1"], q["nu"], q["lam"], q["red"]) == (0, 8 * cells, 16 * cells, 24 * cells, 24 * cells + 8 * lam)
        assert q["total"] == 24 * cells + 8 * lam + 64 and q["slab"] == (q["total"] + 15) // 16 * 16
        assert q["threads"] == min(256, max(64, (len(edges) + 63) // 64 * 64))
        assert q["iter_bytes"] == 8 * sum(rec[5] * rec[7] for rec in variables)
    assert {k: p[2][k] for k in ("mu0", "mu1", "nu", "lam", "red", "total")} == {k: p[0][k] for k in ("mu0", "mu1", "nu", "lam", "red", "total")}
    # the twin's graph is the same graph
    G = bc.graph(f)
    assert [list(e) for e in G.edges] == [rec[:3] for rec in edges] and G.moff == [rec[4] for rec in edges]


@needs_gxx
def test_plan_forms_and_launches(sim):
    """A chain of n four-state variables has 2 n - 1 edges: 24 * 4 (2 n - 1) + 32 n + 64 = 224 n - 32 bytes.  n = 731 is the last
    that fits 160 KiB."""
    under, over = chain_prefix(731, 4), chain_prefix(732, 4)
    assert 224 * 731 - 32 <= 160 * KIB < 224 * 732 - 32
    (a, a0), (b,) = sim(under, ["plan 1", "plan 0"]), sim(over, ["plan 1"])
    assert (a["total"], a["form"], a0["form"]) == (224 * 731 - 32, "MsgLds", "MsgGlobal")
    assert (b["total"], b["form"]) == (224 * 732 - 32, "MsgGlobal")
    assert a["threads"] == b["threads"] == 256
    # launches: the LDS form takes whole chunks; the global form as many slabs as the budget holds, 0 when not even one fits
    slab = (b["total"] + 15) // 16 * 16
    assert b["slab"] == slab
    res = sim(over, ["launch 1 32768 1e12", f"launch 1 32768 {10 * slab + 5}", f"launch 1 4 {10 * slab}", f"launch 1 32768 {slab - 1}", f"launch 1 32768 {slab}"])
    assert [r["requests"] for r in res] == [32768, 10, 4, 0, 1]
    assert [r["requests"] for r in sim(under, ["launch 1 32768 0", "launch 0 32768 0", "launch 0 100 1e12"])] == [32768, 0, 100]


@needs_gxx
def test_plan_error_paths(sim):
    big = types.SimpleNamespace(card=[256, 2], scope_off=[0, 1, 2], scope_vars=[0, 1], value_off=[0, 256, 258],
                                values=np.concatenate([np.full(256, 1 / 256), [0.5, 0.5]]))
    for line in ("plan 1", "plan 0", "launch 1 8 1e9"):
        (r,) = sim(big, [line])
        assert r["error"] == E_LIMIT and "cardinality above 255" in r["msg"], r
    ok = types.SimpleNamespace(card=[255], scope_off=[0, 1], scope_vars=[0], value_off=[0, 255], values=np.full(255, 1 / 255))
    assert sim(ok, ["plan 1"])[0]["cells"] == 255
    good = ["args 1 0 0", "args 100 1e-9 0.5", "args 7 inf 0.999"]
    bad = ["args 0 1e-9 0", "args -3 1e-9 0", "args 5 -1e-300 0", "args 5 nan 0", "args 5 0 1", "args 5 0 -0.1", "args 5 0 nan"]
    res = sim(ok, good + bad)
    assert all(r == {"ok": 1} for r in res[:3]), res[:3]
    assert all(r.get("error") == E_ARG for r in res[3:]), res[3:]
    assert "max_iterations" in res[3]["msg"] and "tol" in res[5]["msg"] and "damping" in res[7]["msg"]


# -------------------------------------------------------------------------------------------------------------- the Python surface
def sim_net(name):
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == name)
    return simengine.attach(netspec.build(spec, sorobn_amd.BayesNet))


def test_marginals_exact_is_one_query_per_variable():
    bn = sim_net("sprinkler")
    names = bn._all_names()
    event = {names[0]: bn.backend.flat.domains[bn.backend.flat.id[names[0]]][0]}
    for ev in ({}, event):
        got, info = bn.marginals(ev, algorithm="exact", return_info=True)
        assert sorted(got) == [n for n in names if n not in ev]
        assert info == {"iterations": 0, "residual": 0.0, "converged": True}
        for n, s in got.items():
            want = bn.query(n, event=ev)
            assert s.name == want.name and s.index.equals(want.index) and s.index.name == want.index.name
            assert np.array_equal(s.to_numpy(), want.to_numpy())
    frame = bn.marginals_frame(pd.DataFrame({names[0]: [event[names[0]], None]}), algorithm="exact")
    assert list(frame.columns.names) == ["variable", "state"] and len(frame) == 2
    for n in names[1:]:
        want = bn.query(n, event=event)
        got = frame.loc[0, n]
        assert np.array_equal(got.to_numpy(), want.reindex(got.index, fill_value=0.0).to_numpy())
    own = frame.loc[0, names[0]]
    assert own.to_numpy()[list(own.index).index(event[names[0]])] == 1.0 and own.sum() == 1.0


def test_lbp_argument_errors_need_no_engine():
    bn = sim_net("sprinkler")
    a, b = bn._all_names()[:2]
    with pytest.raises(ValueError, match="one query variable"):
        bn.query(a, b, event={}, algorithm="lbp")
    with pytest.raises(ValueError, match="cannot be part of the event"):
        bn.query(a, event={a: True}, algorithm="lbp")
    with pytest.raises(ValueError, match="At least one query variable"):
        bn.query(event={}, algorithm="lbp")
    with pytest.raises(ValueError, match="lbp, exact"):
        bn.marginals(algorithm="gibbs")
    with pytest.raises(ValueError, match="lbp, exact"):
        bn.marginals_frame(pd.DataFrame({a: [True]}), algorithm="bp")
    with pytest.raises(KeyError):
        bn.marginals({"no such node": 1})
