"""Marginal MAP on the device (BayesNet.map_query / map_frame, mibn_map_batch: ve_map_kernel + map_traceback_kernel): small
networks against the dense numpy twin (tests/map_check.py), grids too big to enumerate against the argmax of the existing
posterior path, M = everything against `mpe`, M = nothing against `evidence_proba`, bitwise determinism under chunk / threads /
arena budget, the frame API, no side effects on later calls, and the limits."""
import numpy as np
import pandas as pd
import pytest

import golden_util as gu
import map_check as mp
import mpe_check as mc
import netspec
import sorobn_amd
from sorobn_amd import _capi

pytestmark = pytest.mark.gpu


def _example(name):
    for fname in ("examples.json", "random_dags.json"):
        for entry in gu.load(fname):
            if entry["spec"]["name"] == name:
                return netspec.build(entry["spec"], sorobn_amd.BayesNet).use_device(0)
    raise KeyError(name)


@pytest.fixture(scope="module")
def grid6():
    bn = netspec.build(netspec.grid_spec(6, 6, 4), sorobn_amd.BayesNet).use_device(0)
    return bn, mc.flat_of(bn)


@pytest.fixture(scope="module")
def grid10():
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    return bn, mc.flat_of(bn)


def _engine_map(bn, reqs, flags):
    """[(mvars ids, {evidence id: code})] -> ([codes of request b], log_p [B]) through one mibn_map_batch call."""
    m_off = np.cumsum([0] + [len(ms) for ms, _ in reqs]).astype(np.int64)
    e_off = np.cumsum([0] + [len(ev) for _, ev in reqs]).astype(np.int64)
    m_vars = [v for ms, _ in reqs for v in ms]
    e_vars = [v for _, ev in reqs for v in ev]
    e_codes = [c for _, ev in reqs for c in ev.values()]
    codes, lp = bn.backend.engine.map_batch(m_off, m_vars, e_off, e_vars, e_codes, flags=flags)
    return [codes[m_off[b]:m_off[b + 1]].tolist() for b in range(len(reqs))], lp


def _check_against_posterior(bn, names, event, labels, log_p, table=None):
    """An answer on a network too big to enumerate against the existing query path: the argmax of query(*names, event) (or of
    `table`, a Series of it) and evidence_proba for the mass, 1e-9 relative - the project's posterior tolerance.  -> the branch."""
    post = bn.query(*names, event=event) if table is None else table
    p_e = bn.evidence_proba(event)
    vals = np.sort(post.to_numpy())[::-1]
    p1, p2 = float(vals[0]), float(vals[1]) if len(vals) > 1 else 0.0
    want = p1 * p_e
    assert abs(np.exp(log_p) - want) <= 1e-9 * want, (event, np.exp(log_p), want)
    order = list(post.index.names)
    got = tuple(labels[names.index(n)] for n in order) if len(names) > 1 else labels[0]
    if p1 - p2 > 1e-9 * p1:
        assert got == post.idxmax(), (event, got, post.idxmax())
        return "strict"
    assert abs(float(post.get(got, 0.0)) - p1) <= 1e-9 * p1, (event, got)
    return "tie"


@pytest.mark.parametrize("name", ["sprinkler", "asia", "dag1", "dag7"])
def test_small_networks_against_brute_force(name):
    """Whole programs here are single segments that hold sum steps and max steps: 5 evidence sets x M in {nothing, one, half,
    all} x pruned / unpruned against the dense twin, and the pandas API on the same answers."""
    bn = _example(name)
    f = mc.flat_of(bn)
    rng = np.random.default_rng(21)
    n = len(f.card)
    cases = []
    for k in range(5):
        vs = [] if k == 0 else sorted(rng.choice(n, size=int(rng.integers(1, max(2, n // 2) + 1)), replace=False).tolist())
        ev = {int(v): int(rng.integers(0, f.card[v])) for v in vs}
        free = [v for v in range(n) if v not in ev]
        for ms in ([], [int(rng.choice(free))], [int(v) for v in rng.permutation(free)[:max(1, len(free) // 2)]],
                   [int(v) for v in rng.permutation(free)]):
            cases.append((ms, ev))
    taken = {"zero": 0, "strict": 0, "tie": 0}
    for flags in (0, _capi.MAP_PRUNE):
        codes, lp = _engine_map(bn, cases, flags)
        for (ms, ev), c, l in zip(cases, codes, lp):
            taken[mp.check(f, ms, ev, float(l), c, prune=bool(flags), ctx=f"{name} M={ms} e={ev} flags={flags}")] += 1
    assert taken["strict"] >= 0.9 * (taken["strict"] + taken["tie"]) and taken["strict"] >= 20, taken
    names = [k["name"] for k in bn.backend.engine.kernel_stats()]
    assert "ve_map_kernel" in names and "map_traceback_kernel" in names and "ve_max_kernel" not in names
    # the pandas API: labels in the order given, the log probability under the normalised joint
    ms, ev = cases[-2]
    z = mp.brute(f, [], {}, prune=False)[0]
    s, l = bn.map_query(*[f.names[v] for v in ms], event={f.names[v]: f.domains[v][c] for v, c in ev.items()}, return_log_prob=True)
    p1, p2, best, _, _ = mp.brute(f, ms, ev, prune=False)
    assert list(s.index) == [f.names[v] for v in ms]
    if p1 > 0:
        assert abs(l - np.log(p1 / z)) <= 1e-12
        if p1 - p2 > 1e-9 * p1:
            assert list(s) == [f.domains[v][c] for v, c in zip(ms, best)]


def _grid6_requests(f, n=16, seed=5):
    rng = np.random.default_rng(seed)
    col = [f"{6 * r + 3:03d}" for r in range(6)]
    others = [f"{i:03d}" for i in range(36) if f"{i:03d}" not in col]
    return col, [{str(v): int(rng.integers(0, 4)) for v in rng.choice(others, size=3, replace=False)} for _ in range(n)]


def _grid6_call(bn, f, col, events):
    return _engine_map(bn, [([f.id[c] for c in col], {f.id[k]: f.code_of(f.id[k], v) for k, v in e.items()}) for e in events], _capi.MAP_PRUNE)


def test_tiles_on_a_grid_column(grid6):
    """6 x 6 K = 4, 3 evidence values, M = one full column, 16 requests, with the step classes forced as the parity tests force
    them (big_iters 256, odd tiles of 3 hi iterations): sum steps and max steps both run as GENERIC tiles of the workgroup path.
    Oracle: the argmax of the 4 096-cell query(*M, event) table, evidence_proba for the mass."""
    bn, f = grid6
    eng = bn.backend.engine
    col, events = _grid6_requests(f)
    eng.set_option("big_iters", 256)
    eng.set_option("tile_h", 3)
    try:
        codes, lp = _grid6_call(bn, f, col, events)
        ks = {k["name"]: k for k in eng.kernel_stats()}
    finally:
        eng.set_option("big_iters", 4096)
        eng.set_option("tile_h", 0)
    assert ks["ve_map_kernel:sum tiles"]["launches"] >= 16 and ks["ve_map_kernel:max tiles"]["launches"] >= 16, ks
    assert ks["ve_map_kernel:sum tiles"]["items"] > ks["ve_map_kernel:sum tiles"]["launches"]  # (more than one workgroup per step)
    assert ks["ve_map_kernel"]["launches"] >= 3 and ks["map_traceback_kernel"]["items"] == 16
    taken = {"strict": 0, "tie": 0}
    for e, c, l in zip(events, codes, lp):
        labels = [f.domains[f.id[n]][k] for n, k in zip(col, c)]
        taken[_check_against_posterior(bn, col, e, labels, float(l))] += 1
    assert taken["strict"] >= 15, taken
    # the default options give the same answers bit for bit (segments where the forced run had tiles)
    codes2, lp2 = _grid6_call(bn, f, col, events)
    assert codes2 == codes and np.array_equal(lp, lp2)


def test_c3_grid_four_map_variables(grid10):
    """64 requests of the C3 stream (10 x 10 K = 4, 4 evidence values) with 4 random MAP variables each, one call; the oracle is
    query_frame on the same variables (a 256-cell table per request) + evidence_proba."""
    bn, f = grid10
    seed = 48  # (chosen on the CPU from the planner's byte counts alone: the cheapest of seeds 40 .. 59)
    q, ev, ec = netspec.c3_requests(100, 4, 64, 4, seed=seed)
    rng = np.random.default_rng(seed)
    reqs, named = [], []
    for r in range(64):
        ms = [f"{v:03d}" for v in rng.choice([v for v in range(100) if v not in ev[r]], size=4, replace=False)]
        e = {f"{v:03d}": int(c) for v, c in zip(ev[r], ec[r])}
        named.append((ms, e))
        reqs.append(([f.id[n] for n in ms], {f.id[k]: f.code_of(f.id[k], c) for k, c in e.items()}))
    codes, lp = _engine_map(bn, reqs, _capi.MAP_PRUNE)
    taken = {"strict": 0, "tie": 0}
    for (ms, e), c, l in zip(named, codes, lp):
        table = bn.query_frame(*ms, events=pd.DataFrame([e])).iloc[0]
        labels = [f.domains[f.id[n]][k] for n, k in zip(ms, c)]
        taken[_check_against_posterior(bn, ms, e, labels, float(l), table=table)] += 1
    assert taken["strict"] >= 58, taken
    s, l0 = bn.map_query(*named[0][0], event=named[0][1], return_log_prob=True)
    assert l0 == lp[0] and list(s) == [f.domains[f.id[n]][k] for n, k in zip(named[0][0], codes[0])]


@pytest.mark.parametrize("name", ["asia", "dag7"])
def test_everything_is_mpe_and_nothing_is_p_e(name):
    """M = every non-evidence variable: log_p within 1e-12 of mpe's; M = nothing: log_p within 1e-12 of log evidence_proba."""
    bn = _example(name)
    f = mc.flat_of(bn)
    rng = np.random.default_rng(3)
    n = len(f.card)
    names = list(f.names)
    for k in range(4):
        vs = [] if k == 0 else rng.choice(n, size=int(rng.integers(1, n // 2 + 1)), replace=False).tolist()
        event = {names[v]: f.domains[v][int(rng.integers(0, f.card[v]))] for v in vs}
        free = [x for x in names if x not in event]
        s_mpe, l_mpe = bn.mpe(event, return_log_prob=True)
        s_all, l_all = bn.map_query(*free, event=event, return_log_prob=True)
        s_none, l_none = bn.map_query(event=event, return_log_prob=True)
        p_e = bn.evidence_proba(event)
        assert len(s_none) == 0
        if p_e > 0:
            z = mp.brute(f, [], {}, prune=False)[0]  # (mpe's log probability is of the unnormalised product)
            assert abs(l_all - (l_mpe - np.log(z))) <= 1e-12, (name, event, l_all, l_mpe)
            assert abs(l_none - np.log(p_e)) <= 1e-12, (name, event, l_none, p_e)
        else:
            assert l_all == l_none == -np.inf and all(v is None for v in s_all)


def test_result_does_not_depend_on_chunk_threads_or_waves():
    """Codes and log_p are bitwise equal under chunk 1 / 64, planning threads 1 / 4 and an arena budget that forces several waves.
    96 requests on the tiles test's grid: `chunk` 64 cuts the call in two, and the planner hands requests out in blocks of 32, so
    a pool of four workers plans the call on several of them.  The worker pool is created at an engine's first call, so every
    thread count gets a fresh engine whose `threads` is set before anything runs."""
    def fresh(threads):
        bn = netspec.build(netspec.grid_spec(6, 6, 4), sorobn_amd.BayesNet).use_device(0)
        bn.backend.engine.set_option("threads", threads)
        return bn, mc.flat_of(bn)

    bn, f = fresh(1)
    eng = bn.backend.engine
    col, events = _grid6_requests(f, n=96)
    base_codes, base_lp = _grid6_call(bn, f, col, events)
    assert np.isfinite(base_lp).all() and len(set(map(tuple, base_codes))) > 1
    need_gb = eng.stats()["arena_bytes"] / 1e9
    largest_gb = 0.0
    for e in events:
        _grid6_call(bn, f, col, [e])
        largest_gb = max(largest_gb, eng.stats()["arena_bytes"] / 1e9)
    small_gb = max(largest_gb * 1.01, need_gb / 4)
    assert small_gb < need_gb, (largest_gb, need_gb)
    for threads in (1, 4):
        if threads != 1:
            bn, f = fresh(threads)
            eng = bn.backend.engine
        for opt, val in ((None, None), ("chunk", 1), ("chunk", 64), ("arena_gb", small_gb)):
            if opt:
                eng.set_option(opt, val)
            codes, lp = _grid6_call(bn, f, col, events)
            assert codes == base_codes and np.array_equal(lp, base_lp), (threads, opt, val)
            if opt == "arena_gb":
                assert eng.stats()["arena_bytes"] / 1e9 <= small_gb
            eng.set_option("chunk", 32768)
            eng.set_option("arena_gb", 200.0)


def test_map_frame_equals_per_row_map_query():
    """Rows with different observed patterns equal per-row map_query; the pandas shapes; None rows for zero-mass evidence."""
    bn = _example("asia")
    f = mc.flat_of(bn)
    names = list(f.names)
    ms = [names[1], names[6], names[3]]
    cols = [n for n in names if n not in ms][:4]
    dom = {c: f.domains[f.id[c]] for c in cols}
    rows = [{cols[0]: dom[cols[0]][0]}, {cols[1]: dom[cols[1]][1], cols[2]: dom[cols[2]][0]}, {},
            {c: dom[c][1] for c in cols}, {cols[0]: "no such label"}, {cols[1]: dom[cols[1]][1], cols[2]: dom[cols[2]][0]}]
    events = pd.DataFrame([{c: r.get(c) for c in cols} for r in rows], index=list("abcdef"), dtype=object)
    frame, lp = bn.map_frame(*ms, events=events, return_log_prob=True)
    assert list(frame.columns) == ms and frame.index.equals(events.index) and lp.shape == (6,)
    for r, e in enumerate(rows):
        s, l = bn.map_query(*ms, event=e, return_log_prob=True)
        assert l == lp[r] and list(frame.iloc[r]) == list(s), (r, e)
    assert lp[4] == -np.inf and all(v is None for v in frame.iloc[4]) and np.isfinite(np.delete(lp, 4)).all()
    assert list(frame.iloc[1]) == list(frame.iloc[5]) and frame.drop(index="e").notna().all().all()
    assert list(bn.map_frame(*ms, events=events).columns) == ms
    with pytest.raises(ValueError):
        bn.map_frame(ms[0], events=pd.DataFrame({ms[0]: [f.domains[f.id[ms[0]]][0]]}))


def test_no_side_effects_on_later_calls(grid10):
    """Posteriors and MPE answers taken before a mibn_map_batch call are bitwise equal to those taken after it; the call books
    nothing into the totals (the same map call repeats bit for bit, too)."""
    bn, f = grid10
    eng = bn.backend.engine
    q, ev, ec = netspec.c3_requests(100, 4, 256, 4, seed=9)
    reqs = [((f"{a:03d}",), {f"{v:03d}": int(c) for v, c in zip(vs, cs)}) for a, vs, cs in zip(q.tolist(), ev.tolist(), ec.tolist())]
    before = bn.query_many(reqs).out.copy()
    mpe_before = eng.mpe(ev[:32], ec[:32])
    totals = eng.total_stats()
    map_reqs = [([f.id[n] for n in reqs[r][0]], {f.id[k]: f.code_of(f.id[k], c) for k, c in reqs[r][1].items()}) for r in range(32)]
    first = _engine_map(bn, map_reqs, _capi.MAP_PRUNE)
    assert eng.total_stats() == totals
    second = _engine_map(bn, map_reqs, _capi.MAP_PRUNE)
    assert first[0] == second[0] and np.array_equal(first[1], second[1])
    after = bn.query_many(reqs).out
    mpe_after = eng.mpe(ev[:32], ec[:32])
    assert np.array_equal(before, after)
    assert np.array_equal(mpe_before[0], mpe_after[0]) and np.array_equal(mpe_before[1], mpe_after[1])
    assert "ve_map_kernel" not in [k["name"] for k in eng.kernel_stats()]
    # one MAP variable is the argmax of its posterior
    for r in range(4):
        post = bn.query(*reqs[r][0], event=reqs[r][1])
        assert f.domains[map_reqs[r][0][0]][first[0][r][0]] == post.idxmax()


def test_limits_and_argument_errors():
    """A MAP variable of 65 537 states: MIBN_E_LIMIT; a variable both in M and in E, a duplicate, an unknown id or flag: MIBN_E_ARG."""
    eng = _capi.Engine(0)
    card = np.array([2, 65537], np.int32)
    scope_off = np.array([0, 1, 2], np.int64)
    values = np.concatenate([[0.5, 0.5], np.full(65537, 1.0 / 65537)])
    eng.set_network(card, scope_off, np.array([0, 1], np.int32), np.array([0, 2, 2 + 65537], np.int64), values)
    one = np.array([[1]], np.int32)
    none = np.zeros((1, 0), np.int32)
    with pytest.raises(_capi.MibnError) as err:
        eng.map(one, none, none)
    assert err.value.code == _capi.E_LIMIT
    codes, lp = eng.map(np.array([[0]], np.int32), one, np.array([[7]], np.int32), flags=_capi.MAP_PRUNE)  # (wide evidence is fine)
    assert codes.tolist() == [[0]] and abs(lp[0] - np.log(0.5 / 65537)) <= 1e-12
    for mv, evs in (([[0]], [[0]]), ([[0, 0]], [[1]]), ([[2]], [[1]]), ([[0]], [[5]])):
        with pytest.raises(_capi.MibnError) as err:
            eng.map(np.array(mv, np.int32), np.array(evs, np.int32), np.zeros((1, 1), np.int32))
        assert err.value.code == _capi.E_ARG, (mv, evs)
    with pytest.raises(_capi.MibnError) as err:
        eng.map(np.array([[0]], np.int32), none, none, flags=2)
    assert err.value.code == _capi.E_ARG
    # an empty program (M empty, no evidence, pruned): log_p = 0, written by the host
    codes, lp = eng.map(none, none, none, flags=_capi.MAP_PRUNE)
    assert codes.shape == (1, 0) and lp[0] == 0.0
