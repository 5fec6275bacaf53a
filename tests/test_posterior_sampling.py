"""Exact posterior sampling on the device (BayesNet.sample(method="posterior") / sample_frame, mibn_posterior_sample_batch:
ve_sum_kernel + posterior_draw_kernel) against its host twin tools/prog_sim.cpp draw row for row, against itself under other chunk /
thread / arena settings bit for bit, and against dense posteriors and query_frame marginals by chi-square.

Seeds are the literals 0, 1, 2; the chi-square bound is draw_check.P_MIN (see tests/test_posterior_sampling_host.py)."""
import shutil

import numpy as np
import pandas as pd
import pytest

import draw_check as dc
import event_frames as ef
import golden_util as gu
import mpe_check as mc
import netspec
import sorobn_amd
from sorobn_amd import _capi
from test_posterior_sampling_host import notebook_examples, check_only_data_rows

pytestmark = pytest.mark.gpu

needs_gxx = pytest.mark.skipif(not shutil.which("g++"), reason="no g++")


@pytest.fixture(scope="module")
def draw_sim(tmp_path_factory):
    return dc.build_draw_sim(tmp_path_factory.mktemp("draw_sim"))


@pytest.fixture(scope="module")
def grid():
    entry = gu.load("grid10x10.json")
    bn = netspec.build(gu.grid_spec_from_recipe(entry), sorobn_amd.BayesNet).use_device(0)
    return bn, mc.flat_of(bn)


def _net(name):
    for fname in ("examples.json", "random_dags.json"):
        for e in gu.load(fname):
            if e["spec"]["name"] == name:
                bn = netspec.build(e["spec"], sorobn_amd.BayesNet).use_device(0)
                return bn, mc.flat_of(bn)
    raise KeyError(name)


def _grid_evidence(seed=3):
    rng = np.random.default_rng(seed)
    vs = sorted(rng.choice(100, size=4, replace=False).tolist())
    return {int(v): int(rng.integers(0, 4)) for v in vs}


def _device(bn, reqs, seed, prune):
    """reqs [(evars, ecodes, n, g_first)] with consecutive rows -> (codes, p_e) of one engine call."""
    e_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reqs])]).astype(np.int64)
    s_off = np.array([reqs[0][3]] + [r[3] + r[2] for r in reqs], np.int64)
    assert all(reqs[i][3] + reqs[i][2] == reqs[i + 1][3] for i in range(len(reqs) - 1))
    ev = np.array([v for r in reqs for v in r[0]], np.int32)
    ec = np.array([c for r in reqs for c in r[1]], np.int32)
    return bn.backend.engine.posterior_sample_batch(e_off, ev, ec, s_off, seed=seed, flags=_capi.DRAW_PRUNE if prune else 0)


def _requests(f, rng, n_sets, n):
    sets = [{}]
    nv = len(f.card)
    for _ in range(n_sets):
        vs = sorted(rng.choice(nv, size=int(rng.integers(1, max(2, nv // 2) + 1)), replace=False).tolist())
        sets.append({int(v): int(rng.integers(0, f.card[v])) for v in vs})
    return [(list(ev), list(ev.values()), n, i * n) for i, ev in enumerate(sets)]


def _compare_with_twin(draw_sim, tmp_path, bn, f, reqs, seed, prune, ctx):
    """Case 7's rule: the device rows equal draw_sim's; a row may differ only if draw_sim reports a margin <= 1e-12 for one of
    its draws, at most one such row per test is excused, and it is printed.  Returns the number of excused rows."""
    got, p_e = _device(bn, reqs, seed, prune)
    want = dc.run_draw_sim(draw_sim, tmp_path, f, seed, prune, reqs)
    excused = 0
    row = 0
    for rq, w, p in zip(reqs, want, p_e):
        n = rq[2]
        g = got[row:row + n]
        assert abs(p - w["p_e"]) <= 1e-12 * max(w["p_e"], 1e-300), (ctx, p, w["p_e"])
        diff = np.flatnonzero((g != w["codes"]).any(axis=1))
        for i in diff:
            assert rq[3] + int(i) in w["low"], (ctx, "row", rq[3] + int(i), g[i], w["codes"][i])
            print(f"{ctx}: row {rq[3] + int(i)} differs inside draw_sim's margin of 1e-12: {g[i]} / {w['codes'][i]}")
            excused += 1
        row += n
    return excused


@needs_gxx
def test_device_rows_equal_the_host_twin(draw_sim, tmp_path, grid):
    """Case 7: small networks of the host suite, Asia, and the C3 grid with 4 evidence values, 4 096 samples per request, with
    and without the prune flag where the CPTs allow it."""
    rng = np.random.default_rng(7)
    excused = 0
    for name in ("asia", "alarm", "sprinkler", "grades", "dag8", "dag12", "dag20", "dag23"):
        bn, f = _net(name)
        reqs = _requests(f, rng, 3, 4096)
        for prune in ([0, 1] if dc.cpts_are_distributions(f) else [0]):
            excused += _compare_with_twin(draw_sim, tmp_path, bn, f, reqs, 0, prune, f"{name}/prune={prune}")
    bn, f = grid
    ev = _grid_evidence()
    reqs = [(list(ev), list(ev.values()), 4096, 0), ([], [], 4096, 4096)]
    for prune in (0, 1):
        excused += _compare_with_twin(draw_sim, tmp_path, bn, f, reqs, 1, prune, f"C3/prune={prune}")
    assert excused <= 1


def test_tiles_on_a_small_grid():
    """The tile path of ve_sum_kernel at a small size: the 6 x 6 K = 4 grid, 4 requests of 300 samples (not a multiple of the
    draw kernel's 256: a partial workgroup each), with the step classes forced as the parity tests force them (big_iters 256, odd
    tiles of 3 hi iterations) - the big sum steps run as GENERIC tiles of the workgroup path, several workgroups each, where the
    default options keep them in segments.  Both runs give the same rows and p_e bit for bit."""
    bn = netspec.build(netspec.grid_spec(6, 6, 4), sorobn_amd.BayesNet).use_device(0)
    eng = bn.backend.engine
    rng = np.random.default_rng(36)
    reqs = []
    for r in range(4):
        vs = sorted(rng.choice(36, size=1 + r % 2, replace=False).tolist())
        reqs.append((vs, [int(rng.integers(0, 4)) for _ in vs], 300, 300 * r))
    eng.set_option("big_iters", 256)
    eng.set_option("tile_h", 3)
    try:
        rows, p_e = _device(bn, reqs, 0, 0)
        forced = {k["name"]: k for k in eng.kernel_stats()}
    finally:
        eng.set_option("big_iters", 4096)
        eng.set_option("tile_h", 0)
    rows2, p_e2 = _device(bn, reqs, 0, 0)
    default = {k["name"]: k for k in eng.kernel_stats()}
    assert rows.shape == (1200, 36) and np.array_equal(rows, rows2) and np.array_equal(p_e, p_e2)
    assert (rows >= 0).all() and (rows < 4).all() and (p_e > 0).all()
    for i, (vs, cs, n, g) in enumerate(reqs):
        assert (rows[g:g + n][:, vs] == np.array(cs)).all(), i
    # the forced run really tiled: a launch per tiled step, and more than one workgroup per launch
    assert forced["ve_sum_kernel"]["launches"] > default["ve_sum_kernel"]["launches"], (forced, default)
    assert forced["ve_sum_kernel"]["items"] > forced["ve_sum_kernel"]["launches"], forced


def test_codes_do_not_depend_on_chunk_threads_or_waves(grid):
    """Case 8: the same call under chunk 1 / 64 / default, threads 1 / 4 and an arena budget that forces several waves gives
    bitwise identical codes; a request run alone at its row offset gives its rows."""
    bn, f = grid
    eng = bn.backend.engine
    rng = np.random.default_rng(8)
    reqs = []
    g = 0
    for i in range(12):
        vs = sorted(rng.choice(100, size=int(rng.integers(0, 6)), replace=False).tolist())
        n = int(rng.integers(1, 700))
        reqs.append((vs, [int(rng.integers(0, 4)) for _ in vs], n, g))
        g += n
    for prune in (0, 1):
        base, p0 = _device(bn, reqs, 2, prune)
        assert (base >= 0).all() and (base < 4).all()
        need_gb = eng.stats()["arena_bytes"] / 1e9
        # a budget below the whole call's arena but above the largest single request's: several waves, no MIBN_E_NOMEM
        largest_gb = 0.0
        for rq in reqs:
            _device(bn, [rq[:2] + (1, 0)], 2, prune)
            largest_gb = max(largest_gb, eng.stats()["arena_bytes"] / 1e9)
        small_gb = max(largest_gb * 1.01, need_gb / 4)
        assert small_gb < need_gb, (largest_gb, need_gb)
        try:
            for opt, val in (("chunk", 1), ("chunk", 64), ("threads", 1), ("threads", 4), ("arena_gb", small_gb)):
                eng.set_option(opt, val)
                got, p = _device(bn, reqs, 2, prune)
                assert np.array_equal(got, base), (prune, opt, val)
                assert np.array_equal(p, p0), (prune, opt, val)
                eng.set_option("chunk", 32768)
                eng.set_option("arena_gb", 200.0)
        finally:
            eng.set_option("chunk", 32768)
            eng.set_option("arena_gb", 200.0)
        row = sum(r[2] for r in reqs[:5])
        alone, _ = _device(bn, [reqs[5]], 2, prune)
        assert np.array_equal(alone, base[row:row + reqs[5][2]])


def test_chi_square_on_the_device(grid):
    """Case 9: 100 000 samples - the full-state histogram of Asia and of one random DAG against the dense posterior, and on the
    C3 grid the marginal of every single variable against the query_frame posterior on the same evidence."""
    rng = np.random.default_rng(9)
    for name in ("asia", "dag20"):
        bn, f = _net(name)
        for rq in _requests(f, rng, 2, 100000):
            ev = dict(zip(rq[0], rq[1]))
            if not dc.dense_posterior(f, ev)[2] > 0:
                continue
            for prune in ([0, 1] if dc.cpts_are_distributions(f) else [0]):
                codes, _ = _device(bn, [rq[:3] + (0,)], 0, prune)
                dc.check_samples(f, ev, codes, ctx=f"{name}/{ev}/prune={prune}")
    bn, f = grid
    ev = _grid_evidence()
    event = pd.DataFrame({f.names[v]: [f.domains[v][c]] for v, c in ev.items()})
    for prune in (0, 1):
        codes, _ = _device(bn, [(list(ev), list(ev.values()), 100000, 0)], 1, prune)
        for v in range(100):
            if v in ev:
                assert (codes[:, v] == ev[v]).all()
                continue
            post = bn.query_frame(f.names[v], events=event)
            probs = np.zeros(4)
            for lab, p in zip(post.columns, post.iloc[0].to_numpy()):
                probs[f.code_of(v, lab)] = p
            p = dc.chi_square_p(np.bincount(codes[:, v], minlength=4), probs)
            assert p >= dc.P_MIN, (prune, v, p)


def test_pandas_api_shapes_and_zero_mass():
    """Case 10: shapes, dtypes, labels, evidence columns kept, None rows for zero-mass evidence, the ValueError of `sample`."""
    bn, f = _net("alarm")
    names = bn._all_names()
    s = bn.sample(1, {"Mary calls": True}, method="posterior")
    assert isinstance(s, pd.Series) and sorted(s.index) == names and s["Mary calls"] == True  # noqa: E712
    df = bn.sample(500, {"Mary calls": True, "Burglary": False}, method="posterior")
    assert isinstance(df, pd.DataFrame) and list(df.columns) == names and len(df) == 500
    assert (df["Mary calls"] == True).all() and (df["Burglary"] == False).all()  # noqa: E712
    for name in names:
        assert set(df[name].unique()) <= set(f.domains[f.id[name]])
    with pytest.raises(ValueError, match="probability zero"):
        bn.sample(3, {"Mary calls": "perhaps"}, method="posterior")
    events = pd.DataFrame({"Mary calls": [True, None, "perhaps", False], "Alarm": [None, True, True, False]}, index=list("abcd"))
    frame, proba = bn.sample_frame(events, n=3, seed=1, return_proba=True)
    assert list(frame.columns) == names and len(frame) == 12
    assert list(frame.index.get_level_values(0)) == [k for k in "abcd" for _ in range(3)]
    assert list(frame.index.get_level_values(1)) == [0, 1, 2] * 4
    assert (frame.loc["a", "Mary calls"] == True).all() and (frame.loc["d", "Alarm"] == False).all()  # noqa: E712
    other = [c for c in names if c not in ("Mary calls", "Alarm")]
    assert frame.loc["c", other].isna().all().all() and (frame.loc["c", "Mary calls"] == "perhaps").all()
    assert frame.loc[["a", "b", "d"]].notna().all().all()
    assert proba[2] == 0.0
    want = bn.evidence_proba(events.loc[["a", "b", "d"]]).to_numpy()
    assert np.allclose(proba[[0, 1, 3]], want, rtol=1e-12, atol=0)
    again = bn.sample_frame(events, n=3, seed=1)
    assert frame.equals(again)


def test_sparse_cpts_from_fit_sample_only_rows_of_the_data():
    """Case 2 on the device, through `fit`: 10 000 posterior samples of the notebook's examples are rows of the data."""
    for structure, X in notebook_examples():
        bn = sorobn_amd.BayesNet(*structure).use_device(0)
        bn.fit(X)
        df = bn.sample(10000, method="posterior")
        check_only_data_rows(list(df.columns), df.to_numpy(dtype=object), X, ctx=str(structure))


def test_forward_sampling_is_untouched():
    """Case 10, second half: sample(method="forward") with a fixed seed returns what mibn_sample returns for the seed the parent
    commit derives (same Philox keys), consumes one seed per call, and a posterior call in between consumes its own."""
    bn, f = _net("asia")
    bn.seed = 42
    bn._draws = 0
    a = bn.sample(64)
    seed1 = (42 * 0x9E3779B97F4A7C15 + 1) & (2 ** 64 - 1)
    codes = bn.backend.engine.sample(64, [], [], seed=seed1)
    want = pd.DataFrame({name: np.asarray(f.dom_index[v])[codes[:, v]] for v, name in enumerate(f.names)}).sort_index(axis="columns")
    assert a.equals(want)
    bn.sample(5, method="posterior")
    b = bn.sample(64, {"smoker": True} if "smoker" in f.names else {})
    seed3 = (42 * 0x9E3779B97F4A7C15 + 3) & (2 ** 64 - 1)
    iv = [f.id["smoker"]] if "smoker" in f.names else []
    ic = [f.code_of(iv[0], True)] if iv else []
    codes = bn.backend.engine.sample(64, iv, ic, seed=seed3)
    want = pd.DataFrame({name: np.asarray(f.dom_index[v])[codes[:, v]] for v, name in enumerate(f.names)}).sort_index(axis="columns")
    assert b.equals(want)


def test_limits_and_argument_errors(grid):
    """MIBN_E_ARG for a descending s_off, an unknown flag and a duplicate evidence variable; the cardinality limit is the MPE
    path's 65 536 (sample states are 8 or 16 bits in LDS), and a variable beyond it is MIBN_E_LIMIT."""
    bn, f = grid
    eng = bn.backend.engine
    with pytest.raises(_capi.MibnError) as e:
        eng.posterior_sample_batch([0, 0], [], [], [5, 2], seed=0)
    assert e.value.code == _capi.E_ARG
    with pytest.raises(_capi.MibnError) as e:
        eng.posterior_sample_batch([0, 0], [], [], [0, 2], seed=0, flags=8)
    assert e.value.code == _capi.E_ARG
    with pytest.raises(_capi.MibnError) as e:
        eng.posterior_sample_batch([0, 2], [3, 3], [0, 0], [0, 2], seed=0)
    assert e.value.code == _capi.E_ARG
    codes, p = eng.posterior_sample_batch([0, 0, 0], [], [], [0, 0, 3], seed=0, flags=_capi.DRAW_PRUNE)  # (a request without samples)
    assert codes.shape == (3, 100) and p.tolist() == [1.0, 1.0]
    big = sorobn_amd.BayesNet(("A", "B")).use_device(0)
    big.P["A"] = pd.Series({i: 1.0 / 70000 for i in range(70000)})
    big.P["B"] = pd.Series({(i, b): 0.5 for i in range(70000) for b in (0, 1)})
    big.prepare()
    with pytest.raises(_capi.MibnError) as e:
        big.sample(2, method="posterior")
    assert e.value.code == _capi.E_LIMIT
    wide = sorobn_amd.BayesNet(("A", "B")).use_device(0)  # (above 256 states: the 16-bit state kernel)
    wide.P["A"] = pd.Series({i: (i + 1) / (300 * 301 / 2) for i in range(300)})
    wide.P["B"] = pd.Series({(i, b): (0.25 if b else 0.75) for i in range(300) for b in (0, 1)})
    wide.prepare()
    df = wide.sample(100000, method="posterior")
    fw = mc.flat_of(wide)
    codes = np.stack([[fw.code_of(v, x) for x in df[fw.names[v]]] for v in range(2)], axis=1)
    dc.check_samples(fw, {}, codes, ctx="wide")


def _frame_from_engine_calls(bn, f, events, groups, n, seed):
    """The rows of the frame `sample_frame(events, n, seed)` documents, from direct engine calls: one posterior_sample_batch call
    per entry of `groups` (positions of rows that observe the same columns) in the order given, the samples of the frame
    numbered in the order of the calls (s_off accumulated here), codes decoded by hand, evidence keeping its label."""
    assert dc.cpts_are_distributions(f)  # (sample_frame then prunes: DRAW_PRUNE)
    cols = list(events.columns)
    codes = np.full((len(events), n, len(f.card)), -2, np.int32)
    done = 0
    for rows in groups:
        on = [c for c in cols if not pd.isna(events[c].iloc[rows[0]])]
        e_vars = [f.id[c] for c in on] * len(rows)
        e_codes = [f.code_of(f.id[c], events[c].iloc[r]) for r in rows for c in on]
        e_off = np.arange(len(rows) + 1, dtype=np.int64) * len(on)
        s_off = (done + np.arange(len(rows) + 1, dtype=np.int64)) * n
        got, _ = bn.backend.engine.posterior_sample_batch(e_off, e_vars, e_codes, s_off, seed=seed, flags=_capi.DRAW_PRUNE)
        codes[rows] = got.reshape(len(rows), n, len(f.card))
        done += len(rows)
    assert done == len(events) and (codes >= -1).all()
    want = []
    for r in range(len(events)):
        for d in range(n):
            row = []
            for name in bn._all_names():
                v = f.id[name]
                if name in cols and not pd.isna(events[name].iloc[r]):
                    row.append(events[name].iloc[r])
                else:
                    row.append(f.domains[v][codes[r, d, v]] if codes[r, d, v] >= 0 else None)
            want.append(row)
    return want


def _assert_frame_is(frame, events, n, want, bn):
    assert list(frame.columns) == bn._all_names()
    assert frame.index.equals(pd.MultiIndex.from_product([events.index, range(n)], names=[events.index.name, "draw"]))
    got = frame.to_numpy(dtype=object).tolist()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_narrow_frame_seed_contract():
    """What a seed of sample_frame means below 63 columns, pinned against the engine: rows grouped by their pattern of observed
    columns, groups in ascending order of the packed bit mask (column j is bit j), rows ascending within a group, one call per
    group, sample counters running on from call to call."""
    bn, f = _net("asia")
    events = ef.asia_frame()
    pat = events.notna().to_numpy() @ (1 << np.arange(events.shape[1], dtype=np.int64))
    groups = [np.flatnonzero(pat == p) for p in np.unique(pat)]
    assert [g.tolist() for g in groups] == [[4], [0, 7], [2, 6], [3], [5], [1]]
    want = _frame_from_engine_calls(bn, f, events, groups, 4, 7)
    _assert_frame_is(bn.sample_frame(events, n=4, seed=7), events, 4, want, bn)
    assert want[5 * 4].count(None) == len(f.card) - 4 and "maybe" in want[5 * 4]  # (row f: 4 labels given, one outside its domain)


def test_wide_frame_seed_contract():
    """What a seed of sample_frame means at 63 columns or more: one engine call per row, in row order."""
    bn, f = ef.wide_net()
    events = ef.wide_frame()
    want = _frame_from_engine_calls(bn, f, events, [[r] for r in range(len(events))], 4, 7)
    _assert_frame_is(bn.sample_frame(events, n=4, seed=7), events, 4, want, bn)
    for r in (ef.OUT_OF_DOMAIN_ROW, ef.ZERO_ROW):  # no sample: None wherever the row observes nothing
        assert want[4 * r].count(None) == len(ef.MISSING[ef.ROW_PATTERN[r]])
    assert want[4 * ef.OUT_OF_DOMAIN_ROW][50] == 7
