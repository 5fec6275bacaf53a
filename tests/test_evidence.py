"""Evidence likelihood P(e) on the device (BayesNet.evidence_proba / log_likelihood, mibn_query_batch_ex with MIBN_Q_UNNORMALISED)
against numpy enumeration of small networks (tiny kernel and planned path), the reference's recorded predict_proba values, the chain
rule of the existing posterior path on the C3 grid, per-row missing values, predict_proba on rows too wide for its dense table, the
device planners, and no effect on later posterior queries."""
import numpy as np
import pandas as pd
import pytest

import event_frames as ef
import evidence_check as ec
import golden_util as gu
import mpe_check as mc
import netspec
import sorobn_amd
from sorobn_amd import _capi

pytestmark = pytest.mark.gpu

RAW = _capi.Q_UNNORMALISED


@pytest.fixture(scope="module")
def grid():
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    f = mc.flat_of(bn)
    ids = np.array([f.id[f"{i:03d}"] for i in range(100)], np.int32)
    return bn, f, ids


def _labels(f, ev):
    """{id: code} -> {name: label}; a code of -1 becomes a label outside the domain."""
    return {f.names[v]: (f.domains[v][c] if c >= 0 else "not a label") for v, c in ev.items()}


def _chain(eng, evars, ecodes):
    """P(e_1..e_k) = prod_i P(e_i | e_<i), every factor from the existing (normalised) query path: evars / ecodes [B, k]."""
    B, k = evars.shape
    p = np.ones(B)
    for i in range(k):
        post = eng.query_fixed(evars[:, i:i + 1], evars[:, :i], ecodes[:, :i])
        p *= post[np.arange(B), ecodes[:, i]]
    return p


def test_brute_force_small_networks():
    """Case 1: examples.json / random_dags.json networks whose joint fits; empty, single, half, all, zero-probability and
    out-of-domain evidence - evidence_proba within 1e-12 of the enumerated normalised joint, on the tiny kernel and on the
    planned path (tiny = 0), as dicts and as one frame."""
    rng = np.random.default_rng(23)
    n_nets = 0
    for name, spec in ec.small_specs():
        bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
        f = mc.flat_of(bn)
        table = ec.joint(f)
        sets = ec.evidence_sets(f, rng)
        want = np.array([ec.brute(f, [], ev, normalise=True, table=table)[0] for _, ev in sets])
        frame = pd.DataFrame([_labels(f, ev) for _, ev in sets], columns=f.names)
        for tiny in (1, 0):
            bn.backend.engine.set_option("tiny", tiny)
            got = np.array([bn.evidence_proba(_labels(f, ev)) for _, ev in sets])
            assert np.max(np.abs(got - want)) <= 1e-12, (name, tiny, [t for t, _ in sets], got, want)
            got_frame = bn.evidence_proba(frame).to_numpy()
            assert np.max(np.abs(got_frame - want)) <= 1e-12, (name, tiny)
            zero = [i for i, (t, _) in enumerate(sets) if t in ("zero", "out_of_domain")]
            assert all(got[i] == 0.0 and got_frame[i] == 0.0 for i in zero), name
        bn.backend.engine.set_option("tiny", 1)
        n_nets += 1
    assert n_nets >= 5


def _expected_rows(case):
    """The recorded reference values per row of a `predict` case (the single-column form records the marginal: looked up)."""
    exp = case["expect"]
    vals = [float.fromhex(h) for h in exp["values_hex"]]
    logs = [float.fromhex(h) for h in case["log_values_hex"]]
    if exp["multi"]:
        return np.array(vals), np.array(logs)
    at = {tuple(k): i for i, k in enumerate(exp["index"])}
    pos = [at[tuple(r)] for r in case["rows"]]
    return np.array(vals)[pos], np.array(logs)[pos]


def test_reference_predict_proba_goldens():
    """Case 2: every `predict` case of joint.json (alarm, asia, sprinkler, grades, dag0/3/5) - evidence_proba of its rows equals the
    reference's predict_proba within gu.TOL, the log form its log values within 1e-9; log_likelihood is their sum."""
    n_cases = 0
    for entry in gu.load("joint.json"):
        bn = netspec.build(entry["spec"], sorobn_amd.BayesNet).use_device(0)
        for case in entry["predict"]:
            X = pd.DataFrame(case["rows"], columns=case["columns"])
            want, want_log = _expected_rows(case)
            got = bn.evidence_proba(X)
            assert got.index.equals(X.index) and got.dtype == np.float64
            assert np.max(np.abs(got.to_numpy() - want)) <= gu.TOL, (entry["spec"]["name"], case["columns"])
            got_log = bn.evidence_proba(X, log=True).to_numpy()
            assert np.max(np.abs(got_log - want_log)) <= 1e-9, (entry["spec"]["name"], case["columns"])
            assert abs(bn.log_likelihood(X) - float(np.sum(want_log))) <= 1e-9 * len(want_log)
            n_cases += 1
    assert n_cases >= 7


def test_cpts_that_are_not_distributions():
    """Case 2b: a CPT row that sums to less than 1 and an absent parent row - every CPT takes part (NOPRUNE) and P(e) is divided
    by Z: evidence_proba equals the dense predict_proba table within 1e-12."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "alarm")
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    P = bn.P["John calls"].copy()
    P.iloc[1] = 0.01                         # row Alarm = False sums to 0.96
    bn.P["John calls"] = P
    bn.P["Mary calls"] = bn.P["Mary calls"].iloc[2:]  # the rows of Alarm = False are absent
    rng = np.random.default_rng(4)
    names = bn._all_names()
    for cols in (["Burglary", "John calls"], ["Alarm", "Earthquake", "Mary calls"], names):
        dense = bn.backend.marginal(cols)
        f = bn.backend.flat
        assert not bn._cpts_are_distributions(bn.backend)
        codes = np.stack([rng.integers(0, f.card[f.id[c]], 16) for c in cols], axis=1)
        X = pd.DataFrame({c: [f.domains[f.id[c]][k] for k in codes[:, j]] for j, c in enumerate(cols)})
        want = dense[np.ravel_multi_index(codes.T, [int(f.card[f.id[c]]) for c in cols])]
        got = bn.evidence_proba(X).to_numpy()
        assert np.max(np.abs(got - want)) <= 1e-12, (cols, got, want)


@pytest.mark.parametrize("ne", [4, 8, 16])
def test_c3_chain_rule(grid, ne):
    """Case 3: on the C3 grid, P(e_1..e_k) = prod_i query(e_i | e_<i) relative 1e-12; with the flag and one query variable,
    sum_q P(q, e) = P(e) and P(q, e) / P(e) = the normalised posterior within 1e-13."""
    bn, f, ids = grid
    eng = bn.backend.engine
    q, ev, cs = netspec.c3_requests(100, 4, 64, ne, seed=100 + ne)
    evars, qvars = ids[ev], ids[q].reshape(-1, 1)
    B = len(q)
    pe = eng.query_fixed(np.zeros((B, 0), np.int32), evars, cs, flags=RAW)[:, 0]
    chain = _chain(eng, evars, cs)
    assert np.all(pe > 0)
    assert np.max(np.abs(pe - chain) / chain) <= 1e-12, ne
    frame = pd.DataFrame({f"{v:03d}": [None] * B for v in range(100)}, dtype=object)
    for r in range(B):
        for v, c in zip(ev[r].tolist(), cs[r].tolist()):
            frame.iat[r, v] = int(c)
    api = bn.evidence_proba(frame).to_numpy()
    assert np.max(np.abs(api - chain) / chain) <= 1e-12, ne
    joint = eng.query_fixed(qvars, evars, cs, flags=RAW)
    post = eng.query_fixed(qvars, evars, cs)
    assert np.max(np.abs(joint.sum(axis=1) - pe) / pe) <= 1e-12
    assert np.max(np.abs(joint / pe[:, None] - post)) <= 1e-13


def test_per_row_missing_values(grid):
    """Case 4: a frame with per-row missing values (NaN / None) gives what row-by-row dict calls give; log_likelihood is the sum
    of their logs."""
    bn, f, ids = grid
    rng = np.random.default_rng(8)
    cols = [f"{v:03d}" for v in rng.choice(100, size=12, replace=False).tolist()]
    rows = []
    for r in range(40):
        row = {c: (int(rng.integers(0, 4)) if rng.random() < 0.6 else None) for c in cols}
        rows.append(row)
    rows[3] = {c: None for c in cols}
    rows[7][cols[0]] = 9  # outside the domain: probability 0
    X = pd.DataFrame(rows, columns=cols, dtype=object)
    X.iloc[5, 2] = np.nan
    got = bn.evidence_proba(X)
    one = np.array([bn.evidence_proba({c: v for c, v in row.items() if v is not None and not (isinstance(v, float) and np.isnan(v))})
                    for row in X.to_dict("records")])
    assert got.index.equals(X.index)
    assert np.allclose(got.to_numpy(), one, rtol=1e-13, atol=0)
    assert got.iloc[3] == 1.0 and got.iloc[7] == 0.0
    ok = np.arange(len(X)) != 7
    ll = bn.log_likelihood(X[ok])
    assert abs(ll - float(np.sum(np.log(one[ok])))) <= 1e-12 * abs(ll)
    assert bn.log_likelihood(X) == -np.inf


def test_predict_proba_wide_rows(grid):
    """Case 5: predict_proba with 30 observed columns of the C3 grid (a dense table of 4^30 cells: not buildable) answers per
    row, checked by the chain rule, in the Series shape of the dense path."""
    bn, f, ids = grid
    eng = bn.backend.engine
    rng = np.random.default_rng(30)
    vs = sorted(rng.choice(100, size=30, replace=False).tolist())
    cols = [f"{v:03d}" for v in vs]
    codes = rng.integers(0, 4, size=(10, 30)).astype(np.int32)
    X = pd.DataFrame(codes, columns=cols)
    got = bn.predict_proba(X)
    names = bn._all_names()
    assert got.name == f"P({', '.join(names)})"
    assert isinstance(got.index, pd.MultiIndex) and list(got.index.names) == [n for n in names if n in set(cols)]
    assert [tuple(t) for t in got.index.tolist()] == [tuple(r) for r in X[list(got.index.names)].itertuples(index=False, name=None)]
    chain = _chain(eng, np.broadcast_to(ids[vs], (10, 30)).copy(), codes)
    assert np.max(np.abs(got.to_numpy() - chain) / chain) <= 1e-12
    lp = bn.predict_log_proba(X)
    assert np.allclose(lp.to_numpy(), np.log(chain), rtol=1e-12, atol=0)
    bad = X.copy()
    bad.iloc[2, 0] = 7
    with pytest.raises(KeyError):
        bn.predict_proba(bad)


def test_device_planner_options_do_not_change_flagged_results(grid):
    """Case 6: flagged calls are planned by the host's workers: with gpu_emit = 2 (and gpu_search = 2) they are bit-identical."""
    bn, f, ids = grid
    eng = bn.backend.engine
    q, ev, cs = netspec.c3_requests(100, 4, 2048, 8, seed=61)
    evars, qvars = ids[ev], ids[q].reshape(-1, 1)
    none = np.zeros((len(q), 0), np.int32)
    base_pe = eng.query_fixed(none, evars, cs, flags=RAW)
    base_j = eng.query_fixed(qvars, evars, cs, flags=RAW | _capi.Q_NOPRUNE)
    try:
        for opt in ("gpu_emit", "gpu_search"):
            eng.set_option(opt, 2)
            assert np.array_equal(eng.query_fixed(none, evars, cs, flags=RAW), base_pe), opt
            assert np.array_equal(eng.query_fixed(qvars, evars, cs, flags=RAW | _capi.Q_NOPRUNE), base_j), opt
            eng.set_option(opt, 0)
    finally:
        eng.set_option("gpu_emit", 0)
        eng.set_option("gpu_search", 0)


def test_no_side_effects_on_queries(grid):
    """Case 7: a query_many batch before and after evidence calls on the same BayesNet gives bit-identical posteriors."""
    bn, f, ids = grid
    q, ev, cs = netspec.c3_requests(100, 4, 512, 4, seed=9)
    reqs = [((f"{a:03d}",), {f"{v:03d}": int(c) for v, c in zip(vs, cc)}) for a, vs, cc in zip(q.tolist(), ev.tolist(), cs.tolist())]
    before = bn.query_many(reqs).out.copy()
    events = pd.DataFrame([r[1] for r in reqs[:300]])
    bn.evidence_proba(events)
    bn.log_likelihood(events)
    bn.evidence_proba({"010": 1})
    after = bn.query_many(reqs).out
    assert np.array_equal(before, after)


def test_wide_frame_equals_per_row_dict_calls():
    """A frame of 70 evidence columns with 3 patterns of missing cells: evidence_proba and log_likelihood equal the dict calls row
    by row, bit for bit (log_likelihood of a frame is the pandas sum of its rows' logs: summed here the same way)."""
    bn, f = ef.wide_net()
    X = ef.wide_frame()
    events = [ef.row_event(X.iloc[r]) for r in range(len(X))]
    one = np.array([bn.evidence_proba(e) for e in events])
    logs = np.array([bn.log_likelihood(e) for e in events])
    got = bn.evidence_proba(X)
    assert got.index.equals(X.index)
    assert np.array_equal(got.to_numpy(), one), (got.to_numpy(), one)
    assert np.array_equal(bn.evidence_proba(X, log=True).to_numpy(), logs)
    dead = [ef.OUT_OF_DOMAIN_ROW, ef.ZERO_ROW]
    assert (one[dead] == 0.0).all() and (np.delete(one, dead) > 0).all() and (logs[dead] == -np.inf).all()
    assert bn.log_likelihood(X) == -np.inf
    alive = np.delete(np.arange(len(X)), dead)
    assert bn.log_likelihood(X.iloc[alive]) == float(pd.Series(logs[alive]).sum())
