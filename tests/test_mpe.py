"""Most probable explanation on the device (BayesNet.mpe / mpe_frame, mibn_mpe_batch: ve_max_kernel + mpe_traceback_kernel)
against plain numpy: the dense joint of small networks, the reference's own imputations, max-product VE on the C3 grid and on
mixed / large cardinalities, the batched path, and no effect on later posterior queries."""
import numpy as np
import pandas as pd
import pytest

import event_frames as ef
import golden_util as gu
import mpe_check as mc
import netspec
import sorobn_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid():
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    return bn, mc.flat_of(bn)


def _mpe_codes(bn, f, ev_ids):
    """One request through Engine.mpe: evidence {id: code} -> (codes [n], log_p)."""
    vs = list(ev_ids)
    codes, lp = bn.backend.engine.mpe(np.array([vs], np.int32).reshape(1, len(vs)),
                                      np.array([[ev_ids[v] for v in vs]], np.int32).reshape(1, len(vs)))
    return codes[0], float(lp[0])


def test_brute_force_small_networks():
    """Case 1: every network of examples.json / random_dags.json with at most 2^20 joint states, several evidence sets each."""
    rng = np.random.default_rng(11)
    n_nets = 0
    for fname in ("examples.json", "random_dags.json"):
        for entry in gu.load(fname):
            bn = netspec.build(entry["spec"], sorobn_amd.BayesNet).use_device(0)
            f = mc.flat_of(bn)
            if f.missing or np.prod([float(c) for c in f.card]) > 2 ** 20:
                continue
            n = len(f.card)
            sets = [{}]
            for _ in range(4):
                vs = rng.choice(n, size=int(rng.integers(1, max(2, n // 2) + 1)), replace=False).tolist()
                sets.append({int(v): int(rng.integers(0, f.card[v])) for v in vs})
            for ev in sets:
                codes, lp = _mpe_codes(bn, f, ev)
                mc.check_against_brute(f, ev, lp, codes, ctx=f"{entry['spec']['name']} {ev}")
            # the pandas API on the same answers
            names = bn._all_names()
            s, lp_api = bn.mpe({}, return_log_prob=True)
            assert list(s.index) == names and lp_api == _mpe_codes(bn, f, {})[1]
            n_nets += 1
    assert n_nets >= 5


def test_reference_imputation():
    """Case 2: impute.json samples that name every variable - the MPE restricted to the missing ones is the golden `expect`
    (a golden tie is accepted at the same probability)."""
    n_cases = 0
    for entry in gu.load("impute.json"):
        bn = netspec.build(entry["spec"], sorobn_amd.BayesNet).use_device(0)
        f = mc.flat_of(bn)
        for case in entry["cases"]:
            sample = dict((k, v) for k, v in case["sample"])
            if "expect" not in case or set(sample) != set(f.names):
                continue
            ev = {k: v for k, v in sample.items() if v is not None}
            s, lp = bn.mpe(ev, return_log_prob=True)
            want = dict((k, v) for k, v in case["expect"])
            if any(s[k] != want[k] for k in sample if sample[k] is None):
                alt = np.array([f.code_of(f.id[k], want[k]) for k in f.names])
                assert abs(mc.log_joint(f, alt) - lp) <= 1e-12, (entry["spec"]["name"], sample)
            n_cases += 1
    assert n_cases >= 5


@pytest.mark.parametrize("ne", [0, 1, 4, 16])
def test_c3_grid(grid, ne):
    """Case 3: the 10 x 10 K = 4 grid against a row-major numpy max-product VE, and self-consistency."""
    bn, f = grid
    rng = np.random.default_rng(100 + ne)
    row_major = [f.id[f"{i:03d}"] for i in range(100)]
    for _ in range(2):
        vs = sorted(rng.choice(100, size=ne, replace=False).tolist())
        ev = {int(v): int(rng.integers(0, 4)) for v in vs}
        codes, lp = _mpe_codes(bn, f, ev)
        assert abs(lp - mc.ve_max(f, ev, row_major)) <= 1e-12, (ne, lp)
        assert abs(mc.log_joint(f, codes) - lp) <= 1e-12
        assert all(codes[v] == c for v, c in ev.items())


def test_tiles_on_a_small_grid():
    """The tile path of ve_max_kernel at a small size: the 6 x 6 K = 4 grid, 16 rows of one or two evidence values, with the step
    classes forced as the parity tests force them (big_iters 256, odd tiles of 3 hi iterations) - the big max steps run as GENERIC
    tiles of the workgroup path, several workgroups each, where the default options keep them in segments.  Both runs give the
    same codes and log_p bit for bit, and log_p is the log joint of the codes."""
    bn = netspec.build(netspec.grid_spec(6, 6, 4), sorobn_amd.BayesNet).use_device(0)
    f = mc.flat_of(bn)
    eng = bn.backend.engine
    rng = np.random.default_rng(36)
    rows = []
    for r in range(16):
        vs = sorted(rng.choice(36, size=1 + r % 2, replace=False).tolist())
        rows.append((vs, [int(rng.integers(0, 4)) for _ in vs]))
    e_off = np.concatenate([[0], np.cumsum([len(vs) for vs, _ in rows])]).astype(np.int64)
    ev = np.array([v for vs, _ in rows for v in vs], np.int32)
    ec = np.array([c for _, cs in rows for c in cs], np.int32)
    eng.set_option("big_iters", 256)
    eng.set_option("tile_h", 3)
    try:
        codes, lp = eng.mpe_batch(e_off, ev, ec)
        forced = {k["name"]: k for k in eng.kernel_stats()}
    finally:
        eng.set_option("big_iters", 4096)
        eng.set_option("tile_h", 0)
    codes2, lp2 = eng.mpe_batch(e_off, ev, ec)
    default = {k["name"]: k for k in eng.kernel_stats()}
    assert np.array_equal(codes, codes2) and np.array_equal(lp, lp2)
    for (vs, cs), c, l in zip(rows, codes, lp):
        assert abs(mc.log_joint(f, c) - l) <= 1e-12, (vs, cs, l)
        assert all(c[v] == x for v, x in zip(vs, cs))
    # the forced run really tiled: a launch per tiled step, and more than one workgroup per launch
    assert forced["ve_max_kernel"]["launches"] > default["ve_max_kernel"]["launches"], (forced, default)
    assert forced["ve_max_kernel"]["items"] > forced["ve_max_kernel"]["launches"], forced
    assert forced["mpe_traceback_kernel"]["items"] == 16


def _large_cases():
    yield "mixed", netspec.mixed_grid_spec(4, 5, (2, 3, 5, 4, 7), seed=1)
    for entry in gu.load("huge_cards.json"):
        yield "huge", gu.dag_spec_from_recipe(entry)
    for entry in gu.load("many_nodes.json"):
        yield "many", entry["spec"]


def test_mixed_and_large_cardinalities():
    """Case 4: mixed_grid_spec, huge_cards.json, many_nodes.json - the numpy checker (topological order) plus self-consistency."""
    rng = np.random.default_rng(7)
    n = 0
    for tag, spec in _large_cases():
        bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
        f = mc.flat_of(bn)
        if f.missing:
            continue
        order = [f.id[x] for x in spec["nodes"]]
        for ne in (0, 2):
            vs = rng.choice(len(f.card), size=min(ne, len(f.card)), replace=False).tolist()
            ev = {int(v): int(rng.integers(0, f.card[v])) for v in vs}
            codes, lp = _mpe_codes(bn, f, ev)
            want = mc.ve_max(f, ev, order)
            if want == -np.inf:
                assert lp == -np.inf
                continue
            assert abs(lp - want) <= 1e-12, (tag, spec["name"], lp, want)
            assert abs(mc.log_joint(f, codes) - lp) <= 1e-12
        n += 1
    assert n >= 3


def test_batched_frame(grid):
    """Case 5: mpe_frame over 10 000+ C3 events (several chunks) against per-row mpe(); zero-probability / out-of-domain rows;
    a row with every variable named and 30 missing - more than impute can ask of query()."""
    bn, f = grid
    eng = bn.backend.engine
    eng.set_option("chunk", 4096)
    try:
        q, ev, ec = netspec.c3_requests(100, 4, 10240, 4, seed=21)
        cols = [f"{i:03d}" for i in range(100)]
        data = np.full((len(ev), 100), None, dtype=object)
        for r in range(len(ev)):
            data[r, ev[r]] = [int(c) for c in ec[r]]
        events = pd.DataFrame(data, columns=cols)
        events.index = pd.RangeIndex(5, 5 + len(events))
        frame, lp = bn.mpe_frame(events, return_log_prob=True)
        assert list(frame.columns) == bn._all_names() and frame.index.equals(events.index) and np.isfinite(lp).all()
        for r in (0, 1, 4095, 4096, 8191, 10239):
            e = {c: int(v) for c, v in events.iloc[r].items() if v is not None}
            s, l1 = bn.mpe(e, return_log_prob=True)
            assert l1 == lp[r]
            assert list(frame.iloc[r]) == list(s)
    finally:
        eng.set_option("chunk", 32768)
    # zero probability / out of domain
    s, l0 = bn.mpe({"000": 7}, return_log_prob=True)
    assert l0 == -np.inf and s["000"] == 7 and all(s[k] is None for k in s.index if k != "000")
    bad = pd.DataFrame({"000": [7, 0], "001": [None, 1]})
    fr, lpb = bn.mpe_frame(bad, return_log_prob=True)
    assert lpb[0] == -np.inf and fr.iloc[0]["000"] == 7 and fr.iloc[0]["050"] is None and np.isfinite(lpb[1])
    # every variable named, 30 missing
    rng = np.random.default_rng(4)
    miss = set(rng.choice(100, size=30, replace=False).tolist())
    sample = {f"{i:03d}": (None if i in miss else int(rng.integers(0, 4))) for i in range(100)}
    fr, lpr = bn.mpe_frame(pd.DataFrame([sample]), return_log_prob=True)
    assert np.isfinite(lpr[0]) and all(fr.iloc[0][k] is not None for k in sample)
    assert all(fr.iloc[0][k] == v for k, v in sample.items() if v is not None)


def test_no_side_effects_on_queries(grid):
    """Case 6: a query_many batch before and after mpe_frame calls on the same BayesNet gives bit-identical posteriors."""
    bn, f = grid
    q, ev, ec = netspec.c3_requests(100, 4, 512, 4, seed=9)
    reqs = [((f"{a:03d}",), {f"{v:03d}": int(c) for v, c in zip(vs, cs)}) for a, vs, cs in zip(q.tolist(), ev.tolist(), ec.tolist())]
    before = bn.query_many(reqs).out.copy()
    events = pd.DataFrame([r[1] for r in reqs[:300]])
    bn.mpe_frame(events)
    bn.mpe({"010": 1})
    after = bn.query_many(reqs).out
    assert np.array_equal(before, after)
    names = [k["name"] for k in bn.backend.engine.kernel_stats()]
    assert "ve_max_kernel" not in names


def _assert_frame_equals_per_row_mpe(bn, events):
    frame, lp = bn.mpe_frame(events, return_log_prob=True)
    assert list(frame.columns) == bn._all_names() and frame.index.equals(events.index)
    for r in range(len(events)):
        s, l1 = bn.mpe(ef.row_event(events.iloc[r]), return_log_prob=True)
        assert l1 == lp[r], (r, l1, lp[r])
        assert list(frame.iloc[r]) == list(s), r
    return frame, lp


def test_wide_frame_equals_per_row_mpe():
    """A frame of 70 evidence columns (rows grouped by pattern beyond the 62 columns a bit mask holds): every row, the one with
    a label outside its domain and the one of probability zero included, is exactly what mpe() gives for it."""
    bn, f = ef.wide_net()
    frame, lp = _assert_frame_equals_per_row_mpe(bn, ef.wide_frame())
    dead = [ef.OUT_OF_DOMAIN_ROW, ef.ZERO_ROW]
    assert (lp[dead] == -np.inf).all() and np.isfinite(np.delete(lp, dead)).all()
    assert frame.iloc[ef.OUT_OF_DOMAIN_ROW]["050"] == 7 and frame.drop(index=frame.index[dead]).notna().all().all()


def test_narrow_frame_equals_per_row_mpe():
    """The same assertion on the 5-column frame of the Asia example (patterns grouped by bit mask)."""
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "asia")
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    frame, lp = _assert_frame_equals_per_row_mpe(bn, ef.asia_frame())
    assert lp[5] == -np.inf and (frame.loc["f", "Smoker"] == "maybe") and np.isfinite(lp[4])
