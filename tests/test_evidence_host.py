"""Evidence likelihood P(e) on the CPU: the MIBN_Q_UNNORMALISED programs the host planner emits, run by a host interpreter
(tools/prog_sim.cpp ev, linked against planner.cpp) and checked against numpy enumeration; the programs of flagged requests against the
unflagged ones word for word; the validation of zero query variables; and the argument errors of BayesNet.evidence_proba, raised
before any engine exists."""
import shutil

import numpy as np
import pandas as pd
import pytest

import evidence_check as ec
import golden_util as gu
import mpe_check as mc
import netspec
import sorobn_amd

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")


@pytest.fixture(scope="module")
def ev_sim(tmp_path_factory):
    return ec.build_ev_sim(tmp_path_factory.mktemp("ev_sim"))


def test_zero_query_variables_need_the_flag(ev_sim, tmp_path):
    """validate_request rejects nq = 0 with the reference's message unless the request is flagged (the flagged ones are planned
    and run in the next tests)."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    f = mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))
    lines = ec.run_ev_sim(ev_sim, tmp_path, f, [(0, [], [], []), (0, [], [1], [0]), (1, [], [1, 2], [0, 1]), (0, [0], [1], [0])],
                          mode="reject")
    assert lines[:3] == ["At least one query variable has to be specified"] * 3
    assert lines[3] == "ok"
    got = ec.run_ev_sim(ev_sim, tmp_path, f, [(0, [], [], []), (0, [], [1], [0]), (1, [], [1, 2], [0, 1])])
    assert [len(g) for g in got] == [1, 1, 1]


def test_flagged_programs_match_enumeration(ev_sim, tmp_path):
    """Every small network (all steps GENERIC), partial evidence of every kind, with and without pruning, nq = 0 and nq = 1:
    P(q, e) of the program within 1e-12 of numpy enumeration - including the empty evidence with pruning (no factor at all: the
    empty product, 1)."""
    rng = np.random.default_rng(17)
    n_nets = 0
    for name, spec in ec.small_specs():
        f = mc.flat_of(netspec.build(spec, sorobn_amd.BayesNet))
        table = ec.joint(f)
        reqs, want = [], []
        for tag, ev in ec.evidence_sets(f, rng):
            free = [v for v in range(len(f.card)) if v not in ev]
            qsets = [[]] + ([[int(rng.choice(free))]] if free else [])
            for q in qsets:
                for no_prune in (0, 1):
                    reqs.append((no_prune, q, list(ev), list(ev.values())))
                    want.append((tag, ec.brute(f, q, ev, no_prune=bool(no_prune), normalise=False, table=table)))
        got = ec.run_ev_sim(ev_sim, tmp_path, f, reqs)
        for r, (tag, w), g in zip(reqs, want, got):
            assert g.shape == w.shape, (name, tag, r)
            assert np.max(np.abs(g - w)) <= 1e-12, (name, tag, r, g, w)
        empty = [g for r, g in zip(reqs, got) if r == (0, [], [], [])]
        assert empty and all(g[0] == 1.0 for g in empty)
        n_nets += 1
    assert n_nets >= 5


def test_flagged_programs_equal_unflagged_but_for_the_raw_bit(ev_sim, tmp_path):
    """C3 requests (10 x 10 grid, K = 4, 1 query + 4 / 8 / 16 evidence variables: SWEEP, FIBER, MFMA and CHAIN steps): the
    flagged program is the unflagged one word for word, except for the RAW bit of its FINAL step (ev_sim compare)."""
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet)
    f = mc.flat_of(bn)
    ids = np.array([f.id[f"{i:03d}"] for i in range(100)], np.int32)
    reqs = []
    for ne in (4, 8, 16):
        q, ev, cs = netspec.c3_requests(100, 4, 24, ne, seed=ne)
        for a, vs, c in zip(q.tolist(), ev.tolist(), cs.tolist()):
            reqs.append((0, [int(ids[a])], [int(ids[v]) for v in vs], c))
    reqs.append((1, [int(ids[5])], [int(ids[50])], [2]))
    lines = ec.run_ev_sim(ev_sim, tmp_path, f, reqs, mode="compare")
    assert all(int(line.split()[1]) >= 1 for line in lines)


def test_evidence_argument_errors_before_any_engine(monkeypatch):
    """Unknown column names in evidence_proba / log_likelihood raise KeyError before an engine is created."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    bn = netspec.build(spec, sorobn_amd.BayesNet)

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(sorobn_amd.bayes_net._capi, "Engine", no_engine)
    with pytest.raises(KeyError):
        bn.evidence_proba({"Nope": True})
    with pytest.raises(KeyError):
        bn.evidence_proba(pd.DataFrame({"Burglary": [True], "Not a variable": [1]}))
    with pytest.raises(KeyError):
        bn.log_likelihood(pd.DataFrame({"Not a variable": [1]}))
