"""Exact posterior sampling on the CPU: the draw programs and draw records the planner emits for mibn_posterior_sample_batch, run
by the host twin (tools/prog_sim.cpp draw, linked against planner.cpp: same programs, same Philox stream, same arithmetic of the
draw) and checked against the dense posterior in plain numpy; plus the argument errors of BayesNet.sample(method="posterior") /
sample_frame, raised before any engine exists.

The seeds are the literals 0, 1 and 2, fixed before the first run.  The chi-square bound (draw_check.P_MIN = 1e-6) is the
false-alarm rate per check: the few hundred checks of this file and of tests/test_posterior_sampling.py together fail by chance
less than once in a thousand runs."""
import shutil

import numpy as np
import pandas as pd
import pytest

import draw_check as dc
import evidence_check as ec
import golden_util as gu
import mpe_check as mc
import netspec
import sorobn_amd

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")

N_SAMPLES = 20000


@pytest.fixture(scope="module")
def draw_sim(tmp_path_factory):
    return dc.build_draw_sim(tmp_path_factory.mktemp("draw_sim"))


def _evidence_sets(f, rng, n_sets):  # (the generator of test_mpe_host.py)
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


def fit_by_hand(bn, X):
    """The CPTs `fit` estimates from complete rows (relative frequencies per observed parent configuration), built with pandas:
    the CPU suite has no device to count on."""
    for node in bn.nodes:
        parents = list(bn.parents.get(node, []))
        if parents:
            joint = X.groupby(parents + [node]).size()
            bn.P[node] = (joint / joint.groupby(level=list(range(len(parents)))).transform("sum")).rename(node)
        else:
            bn.P[node] = (X.groupby(node).size() / len(X)).rename(node)
    return bn.prepare()


def notebook_examples():
    """The two networks of the reference's notebook on forward sampling that "only produces valid data", from their data rows."""
    x1 = pd.DataFrame([[True, True, True], [False, False, False]], columns=["A", "B", "C"])
    x2 = pd.DataFrame([[1, 1, 1, 1], [2, 1, 2, 1]], columns=["A", "B", "C", "D"])
    return [((["A", "B"], "C"),), x1], [(("A", "B"), ("B", "C"), (["A", "C"], "D")), x2]


def check_only_data_rows(names, labels, X, ctx=""):
    """Every sampled row (labels [n, len(names)]) is a row of X, in the proportions of X's rows (equal here) within the chi-square
    bound."""
    rows = [tuple(r) for r in X[list(names)].itertuples(index=False)]
    got = pd.Series([tuple(r) for r in labels]).value_counts()
    assert set(got.index) <= set(rows), (ctx, set(got.index) - set(rows))
    counts = np.array([got.get(r, 0) for r in rows], np.float64)
    p = dc.chi_square_p(counts, np.full(len(rows), 1.0 / len(rows)))
    assert p >= dc.P_MIN, (ctx, counts, p)


def test_draw_programs_sample_the_dense_posterior(draw_sim, tmp_path):
    """Case 1: every network of examples.json / random_dags.json with at most 2^20 joint states, no evidence + 4 random evidence
    sets, without the prune flag and - where every CPT is a distribution - with it, 20 000 samples per request: every sample
    agrees with the evidence and has positive probability, the full-state histogram passes the chi-square test against the dense
    posterior, p_e is the dense mass within 1e-12 relative (case 4).  draw_sim itself checks that programs are GENERIC only, that
    no kept table overlaps another, and that every variable a draw reads is evidence or drawn before."""
    rng = np.random.default_rng(5)
    n_nets = n_pruned = n_checks = 0
    for name, f in _small_specs():
        sets = _evidence_sets(f, rng, 4)
        reqs = [(list(ev), [ev[v] for v in ev], N_SAMPLES, 0) for ev, _ in sets]
        modes = [0, 1] if dc.cpts_are_distributions(f) else [0]
        n_pruned += len(modes) - 1
        for prune in modes:
            res = dc.run_draw_sim(draw_sim, tmp_path, f, 0, prune, reqs)
            for (ev, tag), r in zip(sets, res):
                ctx = f"{name}/{tag}/prune={prune}"
                _, _, mass = dc.dense_posterior(f, ev)
                if not mass > 0:
                    assert r["p_e"] == 0.0, ctx
                    assert all((r["codes"][:, v] == (ev[v] if v in ev else -1)).all() for v in range(len(f.card))), ctx
                    continue
                assert abs(r["p_e"] - mass) <= 1e-12 * mass, (ctx, r["p_e"], mass)
                dc.check_samples(f, ev, r["codes"], ctx=ctx)
                n_checks += 1
        n_nets += 1
    assert n_nets >= 5 and n_pruned >= 1 and n_checks >= 50


def test_notebook_examples_sample_only_rows_of_the_data(draw_sim, tmp_path):
    """Case 2: the notebook's two examples, CPTs from their data rows (sparse: parent configurations that never occur have no
    row).  10 000 posterior samples contain only rows seen in the data, in their proportions.

    What this replaces: on example 1, `sample(method="forward")` draws A and B independently, so half of its rows are (A, B) =
    (True, False) or (False, True) - configurations for which C has no CPT row.  The reference raises KeyError there; this
    package's forward kernel falls through to the last code of the all-zero row and returns a state of probability zero."""
    for structure, X in notebook_examples():
        bn = fit_by_hand(sorobn_amd.BayesNet(*structure), X)
        f = mc.flat_of(bn)
        assert not dc.cpts_are_distributions(f)
        r = dc.run_draw_sim(draw_sim, tmp_path, f, 1, 0, [([], [], 10000, 0)])[0]
        labels = [[f.domains[v][c] for v, c in enumerate(row)] for row in r["codes"]]
        check_only_data_rows(f.names, labels, X, ctx=str(structure))
        dc.check_samples(f, {}, r["codes"], ctx=str(structure))


def test_stream_is_a_function_of_the_global_row(draw_sim, tmp_path):
    """Case 3: one run with B = 3 requests equals three runs of the single requests at their row offsets; a pruned program
    without evidence has no elimination step at all (pure forward sampling), and then p_e is the empty product."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "asia")
    f = mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))
    assert dc.cpts_are_distributions(f)
    rng = np.random.default_rng(11)
    sets = [ev for ev, _ in _evidence_sets(f, rng, 2)]
    counts = [700, 1300, 999]
    offs = np.concatenate([[0], np.cumsum(counts)])
    for prune in (0, 1):
        reqs = [(list(ev), list(ev.values()), n, int(g)) for ev, n, g in zip(sets, counts, offs)]
        together = dc.run_draw_sim(draw_sim, tmp_path, f, 2, prune, reqs)
        for rq, want in zip(reqs, together):
            alone = dc.run_draw_sim(draw_sim, tmp_path, f, 2, prune, [rq])[0]
            assert np.array_equal(alone["codes"], want["codes"])
            shifted = dc.run_draw_sim(draw_sim, tmp_path, f, 2, prune, [rq[:3] + (rq[3] + 1,)])[0]
            assert not np.array_equal(shifted["codes"], want["codes"])
    none = dc.run_draw_sim(draw_sim, tmp_path, f, 2, 1, [([], [], 64, 0)])[0]
    assert none["n_steps"] == 0 and none["n_back"] == 0 and none["n_fwd"] == len(f.card) and none["p_e"] == 1.0
    full = dc.run_draw_sim(draw_sim, tmp_path, f, 2, 0, [([], [], 64, 0)])[0]
    assert full["n_back"] == len(f.card) and full["n_fwd"] == 0


def test_mass_of_the_evidence_on_the_c3_grid(draw_sim, tmp_path):
    """Case 4 beyond the dense joint: on the 10 x 10 K = 4 grid p_e equals the P(e) of the evidence path's host interpreter
    (tools/prog_sim.cpp ev) within 1e-12 relative, pruned or not, and the samples keep the evidence."""
    entry = gu.load("grid10x10.json")
    f = mc.flat_of(netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet))
    rng = np.random.default_rng(3)
    vs = sorted(rng.choice(100, size=4, replace=False).tolist())
    ev = {v: int(rng.integers(0, 4)) for v in vs}
    ev_sim = ec.build_ev_sim(tmp_path)
    want = float(ec.run_ev_sim(ev_sim, tmp_path, f, [(0, [], list(ev), list(ev.values()))])[0][0])
    for prune in (0, 1):
        r = dc.run_draw_sim(draw_sim, tmp_path, f, 0, prune, [(list(ev), list(ev.values()), 256, 0)])[0]
        assert abs(r["p_e"] - want) <= 1e-12 * want, (prune, r["p_e"], want)
        assert all((r["codes"][:, v] == c).all() for v, c in ev.items())
        assert (r["codes"] >= 0).all() and (r["codes"] < 4).all()
        assert r["n_back"] + r["n_fwd"] == 96 and (r["n_fwd"] > 0) == bool(prune)


def test_out_of_domain_evidence_gives_no_sample(draw_sim, tmp_path):
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    f = mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))
    r = dc.run_draw_sim(draw_sim, tmp_path, f, 0, 0, [([0], [-1], 5, 0)])[0]
    assert r["p_e"] == 0.0 and (r["codes"][:, 1:] == -1).all() and (r["codes"][:, 0] == -1).all()


def test_sum_and_max_requests_do_not_know_draw_mode():
    """Case 5 (with test_planner_output_is_pinned and the MPE / evidence host tests, which run unmodified): the new request mode
    is off by default."""
    import ctypes as C
    from sorobn_amd import _capi
    assert "mibn_posterior_sample_batch" in _capi.SYMBOLS and _capi.DRAW_PRUNE == 1
    assert C.sizeof(C.c_uint64) == 8


def test_argument_errors_before_any_engine(monkeypatch):
    """Case 6: unknown names, a node without a CPT and n < 1 raise before an engine is created; other unknown methods keep the
    existing ValueError."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    bn = netspec.build(spec, sorobn_amd.BayesNet)

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", no_engine)
    with pytest.raises(KeyError):
        bn.sample(3, {"Nope": True}, method="posterior")
    with pytest.raises(ValueError):
        bn.sample(0, {"Burglary": True}, method="posterior")
    with pytest.raises(ValueError):
        bn.sample_frame(pd.DataFrame({"Burglary": [True]}), n=0)
    with pytest.raises(KeyError):
        bn.sample_frame(pd.DataFrame({"Burglary": [True], "Not a variable": [1]}))
    with pytest.raises(ValueError, match="Unknown method"):
        bn.sample(1, method="gibbs")
    draws = getattr(bn, "_draws", 0)
    assert draws == 0  # (no seed was consumed by a call that did not run)
    lonely = sorobn_amd.BayesNet(("A", "B"))
    lonely.P["A"] = pd.Series({True: 0.5, False: 0.5})
    lonely.prepare()
    with pytest.raises(KeyError):
        lonely.sample(2, {"A": True}, method="posterior")
