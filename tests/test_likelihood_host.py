"""Likelihood findings (soft evidence) on the CPU: the dense numpy twin (tests/likelihood_check.py) against answers of the unmodified
reference on augmented networks (tests/golden/likelihood_findings.json); the programs the planner emits for requests with findings,
run by the host interpreter (tools/prog_sim.cpp --lh, which writes the seeds into its NaN-filled arena) against the twin; the layout
of the seeds; and the encoding of `likelihood=` into the CSR block of the C-ABI, against a stub engine that records its arguments."""
import os
import re
import shutil

import numpy as np
import pandas as pd
import pytest

import golden_util as gu
import likelihood_check as lc
import mpe_check as mc
import netspec
import sim_tools
import sorobn_amd
from sorobn_amd import _capi
from sorobn_amd.bayes_net import Backend, CptWatch
from sorobn_amd.flatten import flatten

ROOT = mc.ROOT
needs_gxx = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
STRICT = 1e-9  # the project's margin of a strict winner (mpe_check.check_against_brute)


@pytest.fixture(scope="module")
def prog_sim():
    return sim_tools.build_prog_sim()


def golden_nets():
    """[(spec, requests)] of likelihood_findings.json, every network rebuilt from its example name or its pinned recipe."""
    examples = {e["spec"]["name"]: e["spec"] for e in gu.load("examples.json")}
    out = []
    for entry in gu.load("likelihood_findings.json"):
        net = dict(entry["net"])
        kind = net.pop("kind")
        if kind == "example":
            spec = examples[net["name"]]
        else:
            pin = net.pop("cpt_sum_hex")
            if kind == "grid":
                spec = netspec.grid_spec(net["R"], net["C"], net["K"], seed=net["seed"])
            else:
                spec = netspec.random_dag_spec(net.pop("seed"), cards=tuple(net.pop("cards")), **net)
            assert float(sum(r[-1] for c in spec["cpts"].values() for r in c["rows"])).hex() == pin, "recipe drifted from the generator"
        out.append((spec, entry["requests"]))
    return out


def golden_findings(req):
    return {name: {lab: x for lab, x in pairs} for name, pairs in req["findings"].items()}


def dense_expected(f, req):
    """The reference's Series of a golden request as (ids of the sorted query names, positive values, their label rows)."""
    name, inames, rows, vals, multi = gu.expected(req)
    assert inames == sorted(req["query"])
    return [f.id[n] for n in inames], vals, rows


def assert_matches_golden(f, req, dense, tol, ctx):
    q, vals, rows = dense_expected(f, req)
    keep = np.flatnonzero(dense > 0)
    labels = [tuple(f.domains[v][c] for v, c in zip(q, np.unravel_index(k, [int(f.card[v]) for v in q]))) for k in keep]
    gu.assert_rows_equal(labels, rows, ctx=ctx)
    assert float(np.max(np.abs(dense[keep] - vals))) <= tol, (ctx, dense[keep], vals)


def test_goldens_cover_what_they_should():
    nets = golden_nets()
    assert len(nets) == 4
    n_find = {len(r["findings"]) for _, reqs in nets for r in reqs}
    assert n_find == {1, 2, 3}
    assert any(r["event"] for _, reqs in nets for r in reqs) and any(not r["event"] for _, reqs in nets for r in reqs)
    assert any(set(r["query"]) & set(r["findings"]) for _, reqs in nets for r in reqs), "no finding on a query variable"
    for spec, reqs in nets:  # a root, a leaf and an inner node carry a finding in every network
        parents = {n: [p for p, c in spec["edges"] if c == n] for n in spec["nodes"]}
        children = {n: [c for p, c in spec["edges"] if p == n] for n in spec["nodes"]}
        named = {n for r in reqs for n in r["findings"]}
        assert any(not parents[n] for n in named) and any(not children[n] for n in named), spec["name"]
        assert any(parents[n] and children[n] for n in named), spec["name"]


def test_twin_reproduces_the_reference_and_its_own_augmented_network():
    """Every golden within 1e-9 (the project's parity figure); the twin on augment()'s network with the added event equals the twin
    with findings within 1e-12."""
    n = 0
    for spec, reqs in golden_nets():
        f = flatten(netspec.build(spec, sorobn_amd.BayesNet))
        for k, req in enumerate(reqs):
            findings = golden_findings(req)
            ev = {f.id[name]: f.code_of(f.id[name], lab) for name, lab in req["event"]}
            q = [f.id[x] for x in sorted(req["query"])]
            dense = lc.posterior(f, q, ev, lc.encode(f, findings))
            assert_matches_golden(f, req, dense, gu.TOL, f"{spec['name']}[{k}]")
            aug, add, _ = lc.augment(spec, findings)
            fa = flatten(netspec.build(aug, sorobn_amd.BayesNet))
            ev_a = {fa.id[name]: fa.code_of(fa.id[name], lab) for name, lab in list(req["event"]) + list(add.items())}
            dense_a = lc.posterior(fa, [fa.id[x] for x in sorted(req["query"])], ev_a, [])
            assert float(np.max(np.abs(dense - dense_a))) <= 1e-12, (spec["name"], k)
            n += 1
    assert n >= 15


# ------------------------------------------------------------------------------------------------------------ planner against the twin
def small_nets():
    asia = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "asia")
    yield "asia", flatten(netspec.build(asia, sorobn_amd.BayesNet))
    for seed, n in ((41, 7), (42, 9), (43, 8)):
        spec = netspec.random_dag_spec(seed, n_nodes=n, cards=(2, 3, 4))
        yield spec["name"], flatten(netspec.build(spec, sorobn_amd.BayesNet))


def random_cases(f, rng, n_cases):
    """[(q or M, evidence {id: code}, findings [(id, weights)])]: one to three findings, continuous weights in (0.05, 1] with the
    odd exact zero; a finding variable may be queried, never observed.  The evidence has positive probability."""
    n = len(f.card)
    out = []
    while len(out) < n_cases:
        perm = [int(v) for v in rng.permutation(n)]
        ne = int(rng.integers(0, 3))
        ev = {v: int(rng.integers(0, f.card[v])) for v in perm[:ne]}
        if not lc.mass(f, [], ev, [], prune=False)[0] > 0:
            continue  # (evidence of probability zero - the sparse CPTs have such cells - has a test of its own)
        free = perm[ne:]
        nl = int(rng.integers(1, 4))
        lvars = [int(v) for v in rng.choice(free, size=min(nl, len(free)), replace=False)]
        findings = []
        for v in lvars:
            w = rng.uniform(0.05, 1.0, int(f.card[v]))
            if f.card[v] > 2 and rng.random() < 0.3:
                w[int(rng.integers(0, f.card[v]))] = 0.0
            findings.append((v, w * float(rng.choice([1.0, 3.0, 0.25]))))
        nq = int(rng.integers(1, 3))
        q = [int(v) for v in rng.choice(free, size=min(nq, len(free)), replace=False)]
        out.append((q, ev, findings))
    return out


@needs_gxx
def test_planned_programs_match_the_twin(prog_sim, tmp_path):
    """ev run (the Raw program of a query: tables within 1e-12 relative, pruned and unpruned), max and map (log_p within 1e-12, codes
    equal - the twin shows a strict winner, and prog_sim --ties reports no tie on any traceback path) on Asia and three random DAGs."""
    rng = np.random.default_rng(7)
    n_cmp = 0
    for name, f in small_nets():
        n = len(f.card)
        cases = random_cases(f, rng, 8)
        per_request = [fs for _, _, fs in cases]
        for no_prune in (0, 1):
            rows = [(no_prune, q, list(ev), list(ev.values())) for q, ev, _ in cases]
            tables = lc.parse_tables(lc.run_sim(prog_sim, tmp_path, f, "ev", rows, per_request))
            for (q, ev, fs), got in zip(cases, tables):
                want = lc.mass(f, q, ev, fs, prune=not no_prune)
                assert not np.isnan(got).any(), (name, q, ev)  # (a seed read at a wrong offset is a NaN of the interpreter's arena)
                assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), 1e-300)), (name, q, ev, got, want)
                n_cmp += 1
            # the one-cell mass: no query variable at all
            rows0 = [(no_prune, [], list(ev), list(ev.values())) for _, ev, _ in cases]
            for (q, ev, fs), got in zip(cases, lc.parse_tables(lc.run_sim(prog_sim, tmp_path, f, "ev", rows0, per_request))):
                want = lc.mass(f, [], ev, fs, prune=not no_prune)
                assert abs(got[0] - want[0]) <= 1e-12 * max(want[0], 1e-300), (name, ev)
        r = lc.run_sim(prog_sim, tmp_path, f, "max", [(list(ev), list(ev.values())) for _, ev, _ in cases], per_request, ties=True)
        assert all(t[2] == 0 for t in sim_tools.parse_ties(r.stderr)), (name, "a tie on a traceback path")
        lp, codes = lc.parse_codes(r)
        for (q, ev, fs), l, c in zip(cases, lp, codes):
            want_lp, want_codes, p1, p2 = lc.mpe(f, ev, fs)
            assert p1 > 0 and p1 - p2 > STRICT * p1, (name, ev, "no strict winner", p1, p2)
            assert abs(l - want_lp) <= 1e-12, (name, ev, l, want_lp)
            assert [int(x) for x in c] == [int(x) for x in want_codes], (name, ev, c, want_codes)
            n_cmp += 1
        for no_prune in (0, 1):
            # M: the query variables plus one more free variable (three at most), in the caller's order
            ms = []
            for q, ev, fs in cases:
                extra = [v for v in range(n) if v not in ev and v not in q][:1]
                ms.append(q + extra)
            r = lc.run_sim(prog_sim, tmp_path, f, "map", [(no_prune, m, list(ev), list(ev.values())) for m, (_, ev, _) in zip(ms, cases)],
                           per_request, ties=True)
            assert all(t[2] == 0 for t in sim_tools.parse_ties(r.stderr)), (name, "a tie on a traceback path")
            lp, codes = lc.parse_codes(r)
            for m, (q, ev, fs), l, c in zip(ms, cases, lp, codes):
                want_lp, want_codes, p1, p2 = lc.marginal_map(f, m, ev, fs, prune=not no_prune)
                assert p1 > 0 and p1 - p2 > STRICT * p1, (name, m, ev, "no strict winner", p1, p2)
                assert abs(l - want_lp) <= 1e-12, (name, m, ev, l, want_lp)
                assert c == want_codes, (name, m, ev, c, want_codes)
                n_cmp += 1
    assert n_cmp >= 150


@needs_gxx
def test_zero_mass_findings_in_the_planned_programs(prog_sim, tmp_path):
    """Weights that leave no positive mass: an all-zero table, -inf and codes -1 - like impossible evidence."""
    name, f = next(small_nets())
    v = f.id["Smoker"]
    fs = [[(v, np.zeros(2))]]
    got = lc.parse_tables(lc.run_sim(prog_sim, tmp_path, f, "ev", [(0, [f.id["Dispnea"]], [], [])], fs))[0]
    assert np.array_equal(got, np.zeros(2))
    lp, codes = lc.parse_codes(lc.run_sim(prog_sim, tmp_path, f, "max", [([], [])], fs))
    assert lp[0] == -np.inf and codes[0] == [-1] * len(f.card)
    lp, codes = lc.parse_codes(lc.run_sim(prog_sim, tmp_path, f, "map", [(0, [f.id["Dispnea"], v], [], [])], fs))
    assert lp[0] == -np.inf and codes[0] == [-1, -1]


@needs_gxx
def test_no_findings_plan_word_for_word_as_before(prog_sim, tmp_path):
    """A request without findings - no --lh at all, or an --lh file of zero counts - is the same program, the same arena."""
    rng = np.random.default_rng(5)
    for name, f in small_nets():
        cases = random_cases(f, rng, 6)
        for kind, rows in (("ev", [(0, q, list(ev), list(ev.values())) for q, ev, _ in cases]),
                           ("max", [(list(ev), list(ev.values())) for _, ev, _ in cases]),
                           ("map", [(1, q, list(ev), list(ev.values())) for q, ev, _ in cases])):
            plain = lc.run_sim(prog_sim, tmp_path, f, kind, rows, None, dump=True)
            empty = lc.run_sim(prog_sim, tmp_path, f, kind, rows, [[] for _ in rows], dump=True)
            a, b = lc.parse_dump(plain), lc.parse_dump(empty)
            assert len(a) == len(rows) and a == b, (name, kind)
            assert all(seed == 0 for _, _, seed, _ in a)
            assert plain.stdout == empty.stdout


def step_outputs(words):
    """[(out_off, cells, final, argmax offset or None)] of a program's steps (planner.h: the 10-word header)."""
    out, off = [], 1
    for _ in range(words[0]):
        w = words[off:off + 10]
        flags = w[1] >> 16
        out.append((w[4] | (w[5] << 32), w[2] * w[3], bool(flags & 1), (w[7] | (w[8] << 32)) if flags & (1 << 5) else None))
        off += w[6]
    return out


@needs_gxx
def test_seed_layout(prog_sim, tmp_path):
    """With findings the arena grows by the padded seed cells - against the same request without them, every CPT taking part in
    both (no_prune: a finding then changes neither the relevant set nor the order) - and no step writes its output or its argmax
    table over a seed."""
    rng = np.random.default_rng(6)
    n_checked = n_exact = 0
    for name, f in small_nets():
        cases = random_cases(f, rng, 6)
        per_request = [fs for _, _, fs in cases]
        for kind, rows in (("ev", [(1, q, list(ev), list(ev.values())) for q, ev, _ in cases]),
                           ("max", [(list(ev), list(ev.values())) for _, ev, _ in cases]),
                           ("map", [(1, q, list(ev), list(ev.values())) for q, ev, _ in cases])):
            plain = lc.parse_dump(lc.run_sim(prog_sim, tmp_path, f, kind, rows, None, dump=True))
            seeded = lc.parse_dump(lc.run_sim(prog_sim, tmp_path, f, kind, rows, per_request, dump=True))
            for (q, ev, fs), (_, arena0, _, words0), (_, arena1, seed, words) in zip(cases, plain, seeded):
                want_seed = sum((len(w) + 15) // 16 * 16 for _, w in fs)
                assert seed == want_seed and arena1 >= arena0 + want_seed, (name, kind, arena0, arena1, seed, want_seed)
                if words[0] == words0[0]:  # (as many steps: no product of more than kMaxIn = 6 factors had to be pre-multiplied for the findings)
                    assert arena1 == arena0 + want_seed, (name, kind, arena0, arena1, seed, want_seed)
                    n_exact += 1
                for out_off, cells, final, am in step_outputs(words):
                    assert final or out_off >= seed, (name, kind, "a step's output overlaps a seed")
                    assert am is None or am >= seed, (name, kind, "an argmax table overlaps a seed")
                    assert final or out_off + cells <= arena1
                n_checked += 1
    assert n_checked >= 60 and n_exact >= 50, (n_checked, n_exact)


@needs_gxx
def test_single_state_variable_carries_a_scalar_seed(prog_sim, tmp_path):
    """A finding on a single-state variable is a scalar factor: it scales the unnormalised mass and shifts log_p, nothing else."""
    spec = netspec.chain_spec(4, (2, 1, 3), seed=3)
    f = flatten(netspec.build(spec, sorobn_amd.BayesNet))
    assert list(f.card) == [2, 1, 3, 2]
    fs = [(1, np.array([2.5]))]
    got = lc.parse_tables(lc.run_sim(prog_sim, tmp_path, f, "ev", [(0, [3], [], []), (0, [], [0], [1])], [fs, fs]))
    want = [lc.mass(f, [3], {}, fs), lc.mass(f, [], {0: 1}, fs)]
    for g, w_ in zip(got, want):
        assert np.all(np.abs(g - w_) <= 1e-12 * w_)
    assert np.all(np.abs(want[0] - 2.5 * lc.mass(f, [3], {}, [])) <= 1e-15)
    lp, codes = lc.parse_codes(lc.run_sim(prog_sim, tmp_path, f, "max", [([], [])], [fs]))
    lp0, codes0 = lc.parse_codes(lc.run_sim(prog_sim, tmp_path, f, "max", [([], [])], None))
    assert abs(lp[0] - lp0[0] - np.log(2.5)) <= 1e-12 and codes == codes0


@needs_gxx
def test_requests_with_bad_findings_are_refused(prog_sim, tmp_path):
    """validate_request / validate_mpe_request: a finding variable named twice, or observed as well."""
    name, f = next(small_nets())
    two = [(0, np.ones(2)), (0, np.ones(2))]
    r = lc.run_sim(prog_sim, tmp_path, f, "max", [([], [])], [two], expect_fail=True)
    assert r.returncode == 1 and "duplicate likelihood variable id 0" in r.stderr
    r = lc.run_sim(prog_sim, tmp_path, f, "ev", [(0, [2], [1], [0])], [[(1, np.ones(2))]], expect_fail=True)
    assert r.returncode == 1 and "A likelihood variable cannot be part of the event" in r.stderr
    r = lc.run_sim(prog_sim, tmp_path, f, "map", [(0, [2], [1], [0])], [[(1, np.ones(2))]], expect_fail=True)
    assert r.returncode == 1 and "A likelihood variable cannot be part of the event" in r.stderr


# ------------------------------------------------------------------------------------------------------------ the Python encoding
class StubEngine:
    """Records what the public methods hand to the engine; answers with zeros of the right shape."""

    def __init__(self, flat):
        self.card = np.asarray(flat.card, np.int32)
        self.calls = []

    def query_fixed(self, qvars, evars, ecodes, flags=0, likelihoods=None):
        self.calls.append(("query_fixed", [list(q) for q in qvars], [list(e) for e in evars], [list(c) for c in ecodes], likelihoods))
        return np.ones((len(qvars), int(np.prod(self.card[list(qvars[0])]))))

    def query_batch(self, q_off, q_vars, e_off, e_vars, e_codes, out_off=None, flags=0, likelihoods=None):
        self.calls.append(("query_batch", list(q_off), list(q_vars), list(e_off), list(e_vars), likelihoods))
        cells = [int(np.prod(self.card[q_vars[a:b]])) for a, b in zip(q_off[:-1], q_off[1:])]
        off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
        return np.ones(int(off[-1])), off

    def mpe(self, evars, ecodes, likelihoods=None):
        self.calls.append(("mpe", evars.tolist(), ecodes.tolist(), likelihoods))
        return np.zeros((len(evars), len(self.card)), np.int32), np.zeros(len(evars))

    def map(self, mvars, evars, ecodes, flags=0, likelihoods=None):
        self.calls.append(("map", mvars.tolist(), evars.tolist(), ecodes.tolist(), likelihoods))
        return np.zeros(mvars.shape, np.int32), np.zeros(len(mvars))


@pytest.fixture()
def asia_stub():
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "asia")
    bn = netspec.build(spec, sorobn_amd.BayesNet)
    b = Backend.__new__(Backend)
    b.flat = flatten(bn)
    b.watch = CptWatch(bn)
    b.engine = StubEngine(b.flat)
    b._anc, b._presence, b._device, b._planner_only = {}, None, None, True
    bn._backend = b
    return bn, b.engine, b.flat


def as_lists(block):
    return [np.asarray(a).tolist() for a in block]


def test_likelihood_is_encoded_to_the_csr_block(asia_stub):
    bn, eng, f = asia_stub
    s, x, d = f.id["Smoker"], f.id["Positive X-ray"], f.id["Dispnea"]
    # a dict and a Series are encoded the same way; a label that is not named weighs 0
    bn.query("Lung cancer", event={"Visit to Asia": True}, likelihood={"Smoker": {True: 0.7, False: 0.3}, "Positive X-ray": {True: 2.0}})
    bn.query("Lung cancer", event={"Visit to Asia": True},
             likelihood={"Smoker": pd.Series({False: 0.3, True: 0.7}), "Positive X-ray": pd.Series([2.0], index=[True])})
    (k1, q1, e1, c1, b1), (k2, q2, e2, c2, b2) = eng.calls
    assert k1 == k2 == "query_fixed" and q1 == q2 == [[f.id["Lung cancer"]]] and e1 == e2 and c1 == c2 == [[1]]
    assert as_lists(b1) == as_lists(b2) == [[0, 2], [s, x], [0, 2, 4], [0.3, 0.7, 0.0, 2.0]]
    assert b1[0].dtype == np.int64 and b1[1].dtype == np.int32 and b1[2].dtype == np.int64 and b1[3].dtype == np.float64
    # the finding may sit on the query variable; mpe and map_query take the same argument
    eng.calls.clear()
    bn.query("Dispnea", event={}, likelihood={"Dispnea": {False: 1, True: 3}})
    bn.mpe({"Smoker": True}, likelihood={"Dispnea": {True: 0.5, False: 0.25}})
    bn.map_query("Dispnea", "Smoker", event={}, likelihood={"Dispnea": {True: 1.0}})
    assert as_lists(eng.calls[0][4]) == [[0, 1], [d], [0, 2], [1.0, 3.0]]
    assert eng.calls[1][0] == "mpe" and as_lists(eng.calls[1][3]) == [[0, 1], [d], [0, 2], [0.25, 0.5]]
    assert eng.calls[2][0] == "map" and as_lists(eng.calls[2][4]) == [[0, 1], [d], [0, 2], [0.0, 1.0]]
    # no likelihood, or an empty one: the calls of before, no block at all
    eng.calls.clear()
    bn.mpe({"Smoker": True})
    bn.map_query("Dispnea", event={})
    bn.query("Dispnea", event={}, likelihood={})
    assert eng.calls[0][3] is None and eng.calls[1][4] is None and eng.calls[2][4] is None


def test_query_many_takes_three_tuples(asia_stub):
    bn, eng, f = asia_stub
    s, d = f.id["Smoker"], f.id["Dispnea"]
    reqs = [(("Dispnea",), {"Smoker": True}), (("Smoker", "Bronchitis"), {}, {"Dispnea": {True: 0.9, False: 0.2}, "Smoker": {True: 1.0}}),
            ("Lung cancer", {}, None), (("Dispnea",), {}, {"Smoker": {False: 4.0}})]
    out = bn.query_many(reqs)
    assert len(out) == 4 and len(eng.calls) == 1 and eng.calls[0][0] == "query_batch"
    assert as_lists(eng.calls[0][5]) == [[0, 0, 2, 2, 3], [d, s, s], [0, 2, 4, 6], [0.2, 0.9, 0.0, 1.0, 4.0, 0.0]]
    assert out[1].index.names == ["Bronchitis", "Smoker"] and out[2].name == "P(Lung cancer)"
    # 2-tuples alone: the path of before, which knows nothing of findings
    eng.calls.clear()
    bn.query_many(reqs[:1])
    assert eng.calls[0][5] is None


def test_likelihood_argument_errors(asia_stub):
    bn, eng, f = asia_stub
    with pytest.raises(KeyError, match="Nope"):
        bn.query("Dispnea", event={}, likelihood={"Nope": {True: 1.0}})
    with pytest.raises(ValueError, match="not a label"):
        bn.query("Dispnea", event={}, likelihood={"Smoker": {"maybe": 1.0}})
    with pytest.raises(ValueError, match="cannot be part of the event"):
        bn.query("Dispnea", event={"Smoker": True}, likelihood={"Smoker": {True: 1.0}})
    with pytest.raises(ValueError, match="finite and non-negative"):
        bn.query("Dispnea", event={}, likelihood={"Smoker": {True: -1.0}})
    with pytest.raises(ValueError, match="finite and non-negative"):
        bn.mpe({}, likelihood={"Smoker": {True: float("nan")}})
    for algorithm in ("gibbs", "rejection", "likelihood", "nonsense"):
        with pytest.raises(ValueError):
            bn.query("Dispnea", event={}, algorithm=algorithm, likelihood={"Smoker": {True: 1.0}})
    with pytest.raises(KeyError, match="Nope"):
        bn.mpe({}, likelihood={"Nope": {True: 1.0}})
    with pytest.raises(ValueError, match="cannot be part of the event"):
        bn.mpe({"Smoker": True}, likelihood={"Smoker": {True: 1.0}})
    with pytest.raises(KeyError, match="Nope"):
        bn.map_query("Dispnea", event={}, likelihood={"Nope": {True: 1.0}})
    with pytest.raises(ValueError, match="cannot be part of the event"):
        bn.map_query("Dispnea", event={"Smoker": False}, likelihood={"Smoker": {True: 1.0}})
    with pytest.raises(ValueError, match="cannot be part of the event"):
        bn.query_many([(("Dispnea",), {"Smoker": True}, {"Smoker": {True: 1.0}})])
    assert eng.calls == []  # nothing reached the engine


def test_set_likelihoods_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "mibn.h")) as fh:
        header = fh.read()
    assert re.search(r"\bint\s+mibn_set_likelihoods\s*\(\s*mibn_t\s*\*\s*h\s*,\s*int64_t\s+B\s*,\s*const\s+int64_t\s*\*\s*l_off\s*,\s*const\s+int32_t\s*\*\s*l_vars\s*,"
                     r"\s*const\s+int64_t\s*\*\s*v_off\s*,\s*const\s+double\s*\*\s*values\s*\)", header)
    assert "mibn_set_likelihoods" in _capi.SYMBOLS
    for method in ("query_batch", "query_one", "query_fixed", "mpe_batch", "mpe", "map_batch", "map"):
        assert "likelihoods" in getattr(_capi.Engine, method).__code__.co_varnames, method
    lib_path = os.path.join(ROOT, "sorobn_amd", "libmibn.so")
    if os.path.exists(lib_path):
        assert hasattr(_capi.lib(), "mibn_set_likelihoods")
