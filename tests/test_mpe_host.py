"""Most probable explanation on the CPU: the max programs and traceback records the planner emits for mibn_mpe_batch, run by a host
interpreter (tools/prog_sim.cpp max, linked against planner.cpp) and checked against plain numpy; plus the argument errors of
BayesNet.mpe / mpe_frame, raised before any engine exists."""
import shutil

import numpy as np
import pandas as pd
import pytest

import golden_util as gu
import mpe_check as mc
import netspec
import sorobn_amd

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")


@pytest.fixture(scope="module")
def max_sim(tmp_path_factory):
    return mc.build_max_sim(tmp_path_factory.mktemp("max_sim"))


def _evidence_sets(f, rng, n_sets):
    n = len(f.card)
    sets = [({}, "none")]
    for k in range(n_sets):
        m = int(rng.integers(1, max(2, n // 2) + 1))
        vs = sorted(rng.choice(n, size=min(m, n), replace=False).tolist())
        sets.append(({v: int(rng.integers(0, f.card[v])) for v in vs}, f"set{k}"))
    return sets


def _small_specs():
    for fname in ("examples.json", "random_dags.json"):
        for entry in gu.load(fname):
            spec = entry["spec"]
            bn = netspec.build(spec, sorobn_amd.BayesNet)
            f = mc.flat_of(bn)
            if f.missing or np.prod([float(c) for c in f.card]) > 2 ** 20:
                continue
            yield spec["name"], f


def test_max_programs_match_brute_force(max_sim, tmp_path):
    """Case 1 on the CPU: every network of examples.json / random_dags.json with at most 2^20 joint states, several evidence sets
    each - log_p within 1e-12 of the dense joint's best, the assignment equal where the best is unique (max_sim itself checks
    that programs are GENERIC only, that every elimination carries an argmax table and that no argmax table overlaps another
    one or a live intermediate)."""
    rng = np.random.default_rng(5)
    n_nets = 0
    for name, f in _small_specs():
        sets = _evidence_sets(f, rng, 4)
        reqs = [(list(ev), [ev[v] for v in ev]) for ev, _ in sets]
        lp, codes = mc.run_max_sim(max_sim, tmp_path, f, reqs)
        for (ev, tag), l, c in zip(sets, lp, codes):
            mc.check_against_brute(f, ev, l, c, ctx=f"{name}/{tag}")
        n_nets += 1
    assert n_nets >= 5


def test_max_programs_reproduce_reference_imputation(max_sim, tmp_path):
    """Case 2 on the CPU: every impute.json case whose sample names every variable - the MPE of the observed values, restricted to
    the missing ones, is the reference's own imputation (a golden tie is accepted at the same probability)."""
    n_cases = 0
    for entry in gu.load("impute.json"):
        bn = netspec.build(entry["spec"], sorobn_amd.BayesNet)
        f = mc.flat_of(bn)
        for case in entry["cases"]:
            sample = dict((k, v) for k, v in case["sample"])
            if "expect" not in case or set(sample) != set(f.names):
                continue
            ev = {f.id[k]: f.code_of(f.id[k], v) for k, v in sample.items() if v is not None}
            lp, codes = mc.run_max_sim(max_sim, tmp_path, f, [(list(ev), list(ev.values()))])
            want = dict((k, v) for k, v in case["expect"])
            got = {k: f.domains[f.id[k]][codes[0, f.id[k]]] for k in sample if sample[k] is None}
            if any(got[k] != want[k] for k in got):
                alt = codes[0].copy()
                for k in got:
                    alt[f.id[k]] = f.code_of(f.id[k], want[k])
                assert abs(mc.log_joint(f, alt) - lp[0]) <= 1e-12, (entry["spec"]["name"], sample, got, want)
            n_cases += 1
    assert n_cases >= 5


def test_max_programs_on_the_c3_grid(max_sim, tmp_path):
    """Case 3 on the CPU: the 10 x 10 K = 4 grid with 0, 1, 4 and 16 evidence variables against a row-major numpy max-product VE,
    and the decoded assignment's own log probability equal to log_p."""
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet)
    f = mc.flat_of(bn)
    rng = np.random.default_rng(3)
    reqs = []
    for ne in (0, 1, 4, 16):
        vs = sorted(rng.choice(100, size=ne, replace=False).tolist())
        reqs.append((vs, [int(rng.integers(0, 4)) for _ in vs]))
    lp, codes = mc.run_max_sim(max_sim, tmp_path, f, reqs)
    row_major = [f.id[f"{i:03d}"] for i in range(100)]
    for (vs, cs), l, c in zip(reqs, lp, codes):
        ev = dict(zip(vs, cs))
        assert abs(l - mc.ve_max(f, ev, row_major)) <= 1e-12, (len(vs), l)
        assert abs(mc.log_joint(f, c) - l) <= 1e-12
        assert all(c[v] == x for v, x in ev.items())


def test_max_program_zero_probability_and_out_of_domain(max_sim, tmp_path):
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    f = mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))
    lp, codes = mc.run_max_sim(max_sim, tmp_path, f, [([0], [-1])])
    assert lp[0] == -np.inf and (codes[0][1:] == -1).all()


def test_mpe_argument_errors_before_any_engine(monkeypatch):
    """Case 8: unknown names in mpe / mpe_frame raise the KeyError of `query` before an engine is created."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    bn = netspec.build(spec, sorobn_amd.BayesNet)

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", no_engine)
    with pytest.raises(KeyError):
        bn.mpe({"Nope": True})
    with pytest.raises(KeyError):
        bn.mpe_frame(pd.DataFrame({"Burglary": [True], "Not a variable": [1]}))
