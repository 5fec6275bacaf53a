"""Approximate MPE by max-product belief propagation on a CPU: the numpy twin of what include/mibn.h pins for mibn_bp_mpe_batch
(tests/bp_mpe_check.py) against brute force where max-product is exact, its three guarantees on small loopy networks, the zero-mass,
tie and sparse-CPT rules, the host plan's colouring and layout (sorobn_amd/csrc/bp_plan.h through tools/bp_plan_sim.cpp) against colours
and sizes worked out here, and the parts of the Python surface that need no engine.

What is NOT a guarantee, and so not asserted: with the polish on, log_p may fall when max_iterations grows - a better candidate can
polish into a worse local optimum (3 x 3 K = 3 grid of seed 1, no evidence, damping 0, polish 10: -5.2062 after one step, -5.3030 after
two).  Monotone in max_iterations is the kept candidate's score, that is log_p at polish 0; monotone in polish is log_p at any fixed
max_iterations."""
import json
import os

import numpy as np
import pandas as pd
import pytest

import bp_check as bc
import bp_mpe_check as mm
import likelihood_check as lc
import mpe_check as mc
import netspec
import sim_tools
import sorobn_amd
import test_bp_host as host

ROOT = sim_tools.ROOT
E_ARG = -1
KIB = 1024

POLYTREES = {**{name: (lambda name=name: host.polytrees()[name]) for name in ("chain5", "hub", "polytree8")},
             **{f"polytree{seed}": (lambda seed=seed: host.polytree_spec(seed)) for seed in range(12, 22)}}
LOOPY = {"grid3x3k3": lambda: netspec.grid_spec(3, 3, 3, seed=2), "grid4x4k2": lambda: netspec.grid_spec(4, 4, 2, seed=2),
         "dag_zeros": lambda: netspec.random_dag_spec(21, n_nodes=9, p_zero=0.15)}


def _tb():
    import test_bp as tb  # (a GPU test module: only its tables of networks and requests are used)
    return tb


# the loopy matrix of tests/test_bp_mpe.py: the small networks of tests/test_bp.py, the ones above, the C3-sized grid
MATRIX = {"sprinkler": lambda: _tb().LOOPY["sprinkler"](), "asia": lambda: _tb().LOOPY["asia"](), **LOOPY,
          "grid10x10k4": lambda: netspec.grid_spec(10, 10, 4, seed=2)}


def matrix_requests(name, f):
    if name != "grid10x10k4":
        return _tb().some_requests(f, 31)
    _, ev, ec = netspec.c3_requests(100, 4, 2, 3, seed=1)  # (three evidence variables a request)
    return [({int(v): int(c) for v, c in zip(ev[b], ec[b])}, []) for b in range(2)]


def brute(f, ev, fs):
    """(log of the best weighted probability, its codes): mpe_check.brute, or the weighted joint where the request has findings."""
    if not fs:
        lp, codes, _, _ = mc.brute(f, ev)
        return lp, codes
    vs, a = lc.weighted_joint(f, ev, list(fs))
    a = np.asarray(a, np.float64)
    at = np.unravel_index(int(np.argmax(a)), a.shape)
    codes = np.zeros(len(f.card), np.int64)
    for u, c in ev.items():
        codes[u] = c
    for u, c in zip(vs, at):
        codes[u] = c
    return float(np.log(a[at])), codes


# ------------------------------------------------------------------------------------------------------------------- polytrees
@pytest.mark.parametrize("name", list(POLYTREES))
def test_twin_is_exact_on_polytrees(name):
    f = host.flat(POLYTREES[name]())
    n = len(f.card)
    for k, (ev, fs) in enumerate(host.requests_of(f, 7)):
        T = mm.run(f, ev, fs, 2 * n + 1, 0.0, 0.0, 10)
        lp, codes = brute(f, ev, fs)
        print(f"{name}[{k}]: {T.iterations} iterations, residual {T.residual!r}, log_p {T.log_p!r} (brute force {lp!r}), margin {T.margin:.2e}")
        assert T.margin > 1e-6, (name, k, "pick another seed: the decode is nearly tied")
        assert np.array_equal(T.codes, codes), (name, k)
        assert abs(T.log_p - lp) <= 1e-12, (name, k)
        assert T.residual == 0.0 and 1 <= T.iterations <= 2 * n + 1, (name, k)
        assert T.moves == 0 and T.sweeps == 1, (name, k)


# ---------------------------------------------------------------------------------------------------------------- loopy networks
@pytest.mark.parametrize("name", list(LOOPY))
@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_loopy_guarantees(name, damping):
    f = host.flat(LOOPY[name]())
    iterations, polishes = (1, 2, 5, 20, 60), (0, 1, 2, 10)
    for k, (ev, fs) in enumerate(host.requests_of(f, 7)):
        R = mm.run_many(f, ev, fs, iterations, 0.0, damping, polishes)
        best, _ = brute(f, ev, fs)
        for (m, q), T in R.items():
            want = mm.log_weighted_joint(f, T.codes, ev, fs)
            assert T.log_p == want or abs(T.log_p - want) <= 1e-12, (name, k, m, q, T.log_p, want)  # 1. the log-probability of the codes
            assert T.log_p <= best + 1e-12, (name, k, m, q)
            if T.sweeps < q:                                                                        # 3. a local optimum
                assert mm.one_opt(f, T.codes, ev, fs), (name, k, m, q)
        kept = [R[(m, 0)].log_p for m in iterations]                                                # 2. never decreasing
        assert all(a <= b for a, b in zip(kept, kept[1:])), (name, k, kept)
        for m in iterations:
            polished = [R[(m, q)].log_p for q in polishes]
            assert all(a <= b for a, b in zip(polished, polished[1:])), (name, k, m, polished)
        print(f"{name}[{k}] d={damping}: brute force {best:.4f}; kept {[round(x, 4) for x in kept]}; polished at 60 {[round(R[(60, q)].log_p, 4) for q in polishes]}")


def test_the_gpu_matrix_rarely_needs_its_fallback():
    """tests/test_bp_mpe.py holds codes only where the twin's two best distinct candidate scores are more than 1e-9 apart.  That is a
    property of the twin alone: on the loopy cases of that matrix it may fail for one case in ten, on the polytrees for none."""
    cases = fired = 0
    for name, make in MATRIX.items():
        f = host.flat(make())
        for ev, fs in matrix_requests(name, f):
            for d in (0.0, 0.5):
                for T in mm.run_many(f, ev, fs, (1, 2, 7, 60), 0.0, d, (0,)).values():
                    cases += 1
                    fired += mm.score_gap(T.trajectory) <= 1e-9
    print(f"fallback: {fired} of {cases} loopy cases")
    assert fired * 10 <= cases
    for name, make in POLYTREES.items():
        f = host.flat(make())
        for ev, fs in host.requests_of(f, 7):
            assert mm.score_gap(mm.run(f, ev, fs, 2 * len(f.card) + 1, 0.0, 0.0, 10).trajectory) > 1e-9, name


# --------------------------------------------------------------------------------------------------------------------- zero mass
def test_zero_mass_rules():
    f = host.flat(host.zero_spec())
    # impossible evidence: seen in an iteration; -inf, -1 off the evidence, residual 0, info 0
    T = mm.run(f, {0: 0, 1: 1}, [], 20, 0.0, 0.0, 10)
    assert T.iterations >= 1 and T.residual == 0.0 and T.log_p == -np.inf and list(T.codes) == [0, 1, -1]
    assert (T.best_iteration, T.sweeps, T.moves) == (0, 0, 0)
    assert mc.brute(f, {0: 0, 1: 1})[0] == -np.inf
    # ... with damping a message decays towards 0 and never is 0: no normalising sum vanishes, the call returns an assignment - and
    # its true log-probability, -inf (BayesNet.mpe turns that into None labels)
    T = mm.run(f, {0: 0, 1: 1}, [], 20, 0.0, 0.5, 10)
    assert T.iterations == 20 and T.residual > 0.0 and T.log_p == -np.inf and list(T.codes[:2]) == [0, 1] and T.codes[2] >= 0
    # ... also where only the max-marginals show it: a root observed at a state of prior 0
    g = host.flat(netspec._dag_spec("root0", [2], [[]], lambda i: np.array([0.0, 1.0])))
    T = mm.run(g, {0: 0}, [], 5, 0.0, 0.0, 10)
    assert T.iterations >= 1 and T.residual == 0.0 and T.log_p == -np.inf and list(T.codes) == [0]
    # an evidence code of -1 and an all-zero finding: lambda alone shows it, iteration 0
    for ev, fs in (({2: -1}, []), ({}, [(1, np.zeros(2))])):
        T = mm.run(f, ev, fs, 20, 0.0, 0.5, 10)
        assert T.iterations == 0 and T.residual == 0.0 and T.log_p == -np.inf, (ev, fs)
        assert list(T.codes) == [ev.get(v, -1) for v in range(3)]
    # possible evidence next to them: the exact answer (a chain)
    T = mm.run(f, {0: 0, 1: 0}, [], 20, 0.0, 0.5, 10)
    lp, codes = brute(f, {0: 0, 1: 0}, [])
    assert np.array_equal(T.codes, codes) and abs(T.log_p - lp) <= 1e-12


# ---------------------------------------------------------------------------------------------------------- ties and sparse CPTs
def test_ties_go_to_the_lowest_code():
    card, parents = [2, 3, 4, 2, 3], [[], [0], [0, 1], [2], [2, 3]]
    f = host.flat(netspec._dag_spec("uniform", card, parents, lambda i: np.full(card[i], 1.0 / card[i])))
    for d in (0.0, 0.5):
        T = mm.run(f, {}, [], 7, 0.0, d, 10)
        assert not T.codes.any() and T.moves == 0 and T.best_iteration == 1, (d, T.codes)
        want = -float(np.sum(np.log(card)))
        assert abs(T.log_p - want) <= 1e-12
    T = mm.run(f, {3: 1}, [], 7, 0.0, 0.5, 10)
    assert list(T.codes) == [0, 0, 0, 1, 0]


def test_a_candidate_of_score_minus_infinity_is_replaced():
    """Sparse CPTs: the decode of an early step hits a zero cell; a later, finite candidate replaces it, the polish is not needed."""
    f = host.flat(LOOPY["dag_zeros"]())
    ev, fs = host.requests_of(f, 7)[2]
    R = mm.run_many(f, ev, fs, (1, 5), 0.0, 0.0, (0,))
    assert R[(1, 0)].log_p == -np.inf and R[(1, 0)].trajectory == [-np.inf]
    T = R[(5, 0)]
    assert np.isfinite(T.log_p) and T.best_iteration > 1 and T.trajectory[0] == -np.inf
    assert abs(T.log_p - mm.log_weighted_joint(f, T.codes, ev, fs)) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ the host plan
def colours_of(f):
    """The greedy colouring, from an adjacency matrix of the moral graph - not bp_mpe_check's sets."""
    n = len(f.card)
    A = np.zeros((n, n), bool)
    for v in range(n):
        sc = np.asarray(f.scope_vars[f.scope_off[v]:f.scope_off[v + 1]], np.int64)
        A[np.ix_(sc, sc)] = True
    np.fill_diagonal(A, False)
    colour = np.full(n, -1)
    for v in range(n):
        seen = set(colour[:v][A[v, :v]].tolist())
        colour[v] = next(c for c in range(n) if c not in seen)
    return colour.tolist()


def _parse(line):
    out = {}
    for kv in line.split():
        k, v = kv.split("=")
        out[k] = v if k == "form" else [int(x) for x in v.split(",") if x] if k in ("colour", "col_off", "col_members") else int(v)
    return out


@pytest.fixture(scope="module")
def sim_raw(tmp_path_factory):
    import subprocess
    exe = str(tmp_path_factory.mktemp("bp_mpe") / "bp_plan_sim")
    r = subprocess.run(["g++", "-O2", "-mpopcnt", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "bp_plan_sim.cpp"),
                        os.path.join(ROOT, "sorobn_amd", "csrc", "planner.cpp"), "-lpthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(f, lines):
        out = subprocess.run([exe], input="\n".join(sim_tools.network_prefix(f) + list(lines)) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout
    return run


@host.needs_gxx
@pytest.mark.parametrize("name", ["sprinkler", "asia", "grid3x3", "chain9"])
def test_colouring_and_layout(sim_raw, name):
    f = (host.flat(netspec.grid_spec(3, 3, 2, seed=4)) if name == "grid3x3" else host.chain_prefix(9, 4) if name == "chain9"
         else host.example(name))
    n = len(f.card)
    want = colours_of(f)
    for v in range(n):      # a proper colouring: the variables of a CPT scope all differ
        sc = [int(u) for u in f.scope_vars[f.scope_off[v]:f.scope_off[v + 1]]]
        assert len({want[u] for u in sc}) == len(sc), (name, v)
    if name == "grid3x3":   # the moral graph has the grid's edges and the diagonals between the two parents of a node: 4 colours
        assert max(want) + 1 == 4
    if name == "chain9":
        assert want == [v % 2 for v in range(9)]
    assert want == mm.colouring(bc.graph(f))[0]
    lds, glob = (_parse(ln) for ln in sim_raw(f, ["mpe 1", "mpe 0"]).splitlines())
    for p, form in ((lds, "MsgLds"), (glob, "MsgGlobal")):
        assert p["form"] == form and p["colour"] == want and p["n_colours"] == max(want) + 1
        assert p["col_off"] == [0] + np.cumsum(np.bincount(want)).tolist()
        assert p["col_members"] == [v for c in range(max(want) + 1) for v in range(n) if want[v] == c]
        cells, lam = bc.edge_records(f)[4:6]
        term = 24 * cells + 8 * lam
        assert (p["mu0"], p["mu1"], p["nu"], p["lam"], p["term"]) == (0, 8 * cells, 16 * cells, 24 * cells, term)
        assert (p["part"], p["cur"], p["kept"]) == (term + 8 * n, term + 8 * n + 512, term + 12 * n + 512)
        assert p["red"] == (term + 16 * n + 512 + 7) // 8 * 8 and p["total"] == p["red"] + 128
        assert p["slab"] == (p["total"] + 15) // 16 * 16
        assert p["threads"] == min(256, max(64, (len(bc.edge_records(f)[0]) + 63) // 64 * 64))


@host.needs_gxx
def test_form_boundary_and_arguments(sim_raw):
    """A chain of n four-state variables: 24 * 4 (2 n - 1) + 32 n of messages and lambda, 16 n + 512 of decoder state, 128 of slots =
    240 n + 544 bytes.  n = 680 is the last that fits 160 KiB - mibn_bp_batch's own boundary stays at 731 / 732."""
    assert 240 * 680 + 544 <= 160 * KIB < 240 * 681 + 544
    a, a0 = (_parse(ln) for ln in sim_raw(host.chain_prefix(680, 4), ["mpe 1", "mpe 0"]).splitlines())
    (b,) = (_parse(ln) for ln in sim_raw(host.chain_prefix(681, 4), ["mpe 1"]).splitlines())
    assert (a["total"], a["form"], a0["form"]) == (240 * 680 + 544, "MsgLds", "MsgGlobal")
    assert (b["total"], b["form"]) == (240 * 681 + 544, "MsgGlobal")
    assert a["n_colours"] == 2 and a["threads"] == 256
    out = sim_raw(host.chain_prefix(3, 2), ["mpe_args 100 1e-9 0.5 10", "mpe_args 1 0 0 0", "mpe_args 5 0 0 -1", "mpe_args 0 0 0 3", "mpe_args 5 0 1 3"]).splitlines()
    assert out[:2] == ["ok=1", "ok=1"]
    assert all(ln.startswith(f"error={E_ARG} ") for ln in out[2:]) and "polish_sweeps" in out[2] and "max_iterations" in out[3]


@host.needs_gxx
def test_existing_invocations_print_what_the_parent_printed(sim_raw):
    """tests/golden/bp_plan_sim_existing.json: the output of the tool before the `mpe` mode existed, byte for byte."""
    with open(os.path.join(ROOT, "tests", "golden", "bp_plan_sim_existing.json")) as fh:
        golden = json.load(fh)
    nets = {"asia": lambda: host.example("asia"), "sprinkler": lambda: host.example("sprinkler"), "chain60": lambda: host.chain_prefix(60, 4)}
    assert sorted(golden["output"]) == sorted(nets)
    for name, make in nets.items():
        assert sim_raw(make(), golden["lines"]) == golden["output"][name], name


# -------------------------------------------------------------------------------------------------------------- the Python surface
class Recorder:
    """Stands in for the engine: answers the exact call, fails the approximate one."""

    def __init__(self, n):
        self.n, self.calls = n, []

    def mpe(self, evars, ecodes, **more):
        self.calls.append("mpe")
        return np.zeros((len(evars), self.n), np.int32), np.full(len(evars), -1.5)

    def bp_mpe(self, *a, **k):
        raise AssertionError("algorithm='exact' must not reach bp_mpe")


def test_argument_errors_need_no_engine_and_exact_takes_the_old_path():
    bn = host.sim_net("sprinkler")
    a = bn._all_names()[0]
    label = bn.backend.flat.domains[bn.backend.flat.id[a]][0]
    frame = pd.DataFrame({a: [label]}).astype(object)
    bn.backend.engine = None  # (any use of an engine below is an AttributeError)
    for call in (lambda **k: bn.mpe({a: label}, **k), lambda **k: bn.mpe_frame(frame, **k)):
        with pytest.raises(ValueError, match="exact, lbp"):
            call(algorithm="gibbs")
        for bad in (dict(damping=1.0), dict(damping=-0.1), dict(damping=float("nan")), dict(tol=-1.0), dict(tol=float("nan")),
                    dict(n_iterations=0), dict(n_iterations=2.5), dict(polish=-1), dict(polish=1.5)):
            with pytest.raises(ValueError, match=next(iter(bad)) if "n_iter" not in next(iter(bad)) else "n_iterations"):
                call(algorithm="lbp", **bad)
    with pytest.raises(KeyError):
        bn.mpe({"no such node": 1}, algorithm="lbp")
    rec = bn.backend.engine = Recorder(len(bn.backend.flat.card))
    s, lp = bn.mpe({a: label}, return_log_prob=True)
    assert rec.calls == ["mpe"] and lp == -1.5 and list(s.index) == bn._all_names() and s[a] == label
    s2, lp2, info = bn.mpe({a: label}, return_log_prob=True, algorithm="exact", return_info=True)
    assert list(s2) == list(s) and info == {"iterations": 0, "residual": 0.0, "converged": True, "best_iteration": 0, "sweeps": 0, "moves": 0}
    fr = bn.mpe_frame(frame)
    assert rec.calls == ["mpe"] * 3 and list(fr.columns) == bn._all_names()
    assert isinstance(bn.mpe({a: label}), pd.Series)
