"""The step matrix on the device (pytest -m gpu): every case of tests/step_cases.py - small pinned networks whose max, map and draw
programs contain, between them, every shape of step at which generic_body and the tracebacks differ - through mibn_mpe_batch,
mibn_map_batch and mibn_posterior_sample_batch, against the dense numpy twins (log_p, p_e within 1e-12) and against the host twin
tools/prog_sim.cpp running the engine's own programs (codes and rows exactly).  tests/test_step_classes_host.py proves on the CPU
that the cases contain the edges they claim and that every case but the exact-tie ones has a strict winner: no comparison here
accepts a tie, and the exact-tie cases pin "the lowest maximising x" through the twin alone."""
import numpy as np
import pytest

import draw_check as dc
import map_check as mp
import mpe_check as mc
import netspec
import sim_tools
import sorobn_amd
import step_cases as sc
from sorobn_amd import _capi

pytestmark = pytest.mark.gpu

LEVEL_KERNEL = {"max": "ve_max_kernel", "map": "ve_map_kernel", "draw": "ve_sum_kernel"}


@pytest.fixture(scope="module")
def prog_sim():
    return sim_tools.build_prog_sim()


def _csr(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64), np.array([v for x in lists for v in x], np.int32)


def _device(eng, flat, case, prune=None):
    """One engine call with the case's requests -> (per request: codes / rows, log_p / p_e; the statistics rows by name)."""
    reqs = case["requests"]
    evs = [sc.evidence(flat, rq) for rq in reqs]
    e_off, ev = _csr([list(e) for e in evs])
    ec = np.array([c for e in evs for c in e.values()], np.int32)
    if case["kind"] == "max":
        codes, lp = eng.mpe_batch(e_off, ev, ec)
        out = [(codes[b], float(lp[b])) for b in range(len(reqs))]
    elif case["kind"] == "map":
        m_off, mv = _csr([sc.ids(flat, rq["M"]) for rq in reqs])
        codes, lp = eng.map_batch(m_off, mv, e_off, ev, ec, flags=_capi.MAP_PRUNE if prune else 0)
        out = [(np.asarray(codes[m_off[b]:m_off[b + 1]]), float(lp[b])) for b in range(len(reqs))]
    else:
        s_off = np.concatenate([[0], np.cumsum([rq["n"] for rq in reqs])]).astype(np.int64)
        rows, p_e = eng.posterior_sample_batch(e_off, ev, ec, s_off, seed=case["seed"], flags=_capi.DRAW_PRUNE if reqs[0].get("prune", 0) else 0)
        out = [(rows[s_off[b]:s_off[b + 1]], float(p_e[b])) for b in range(len(reqs))]
    return out, {k["name"]: k for k in eng.kernel_stats()}


def _twin(prog_sim, tmp_path, flat, case, opt, prune=None):
    """The same requests through prog_sim, planned as an engine with the options `opt` plans them -> per request (codes / rows, log_p / p_e)."""
    reqs = case["requests"]
    evs = [sc.evidence(flat, rq) for rq in reqs]
    if case["kind"] == "max":
        lp, codes = mc.run_max_sim(prog_sim, tmp_path, flat, [(list(e), list(e.values())) for e in evs], options=opt)
        return [(codes[b], float(lp[b])) for b in range(len(reqs))]
    if case["kind"] == "map":
        lp, codes = mp.run_map_sim(prog_sim, tmp_path, flat, [(not prune, sc.ids(flat, rq["M"]), list(e), list(e.values())) for rq, e in zip(reqs, evs)],
                                   options=opt)
        return [(np.asarray(codes[b], np.int64), float(lp[b])) for b in range(len(reqs))]
    rows, g = [], 0
    for rq, e in zip(reqs, evs):
        rows.append((list(e), list(e.values()), rq["n"], g))
        g += rq["n"]
    res = dc.run_draw_sim(prog_sim, tmp_path, flat, case["seed"], reqs[0].get("prune", 0), rows, options=opt)
    assert not any(r["low"] for r in res)  # (proved by the host test: no row is excused below)
    return [(r["codes"], r["p_e"]) for r in res]


def _reference(flat, case, spec, prune=None):
    """Per request the dense twin's (mass or best probability, argmax codes or None): None where the network is one of the two of 70
    variables (numpy max-product VE in topological order instead), or where the case is an exact-tie case (the twin has no unique argmax)."""
    n, out = len(flat.card), []
    small = np.prod([float(c) for c in flat.card]) <= sc.MAX_JOINT
    for rq in case["requests"]:
        ev = sc.evidence(flat, rq)
        if case["kind"] == "draw":
            out.append((dc.dense_posterior(flat, ev)[2], None))
        elif not small:
            out.append((np.exp(mc.ve_max(flat, ev, sc.ids(flat, sorted(int(x) for x in spec["nodes"])))), None))
        elif case["kind"] == "max":
            _, best, p1, _ = mc.brute(flat, ev)
            out.append((p1, None if "tie" in case["edges"] else best))
        else:
            p1, _, best, _, _ = mp.brute(flat, sc.ids(flat, rq["M"]), ev, prune=bool(prune))
            out.append((p1, None if "tie" in case["edges"] else np.asarray(best, np.int64)))
    return out


def _check(case, flat, got, twin, ref, ctx):
    n = len(flat.card)
    for rq, (codes, val), (t_codes, t_val), (mass, best) in zip(case["requests"], got, twin, ref):
        ev = sc.evidence(flat, rq)
        print(f"{ctx} {rq}: device {val!r}, twin {t_val!r}, reference {mass if case['kind'] == 'draw' else np.log(mass) if mass > 0 else -np.inf!r}")
        if case["kind"] == "draw":
            assert abs(val - mass) <= 1e-12 * mass if mass > 0 else val == 0.0, (ctx, val, mass)
            assert np.array_equal(codes, t_codes), (ctx, "rows differ from the twin's", np.flatnonzero((codes != t_codes).any(axis=1))[:8])
            if mass > 0:
                vs, post, _ = dc.dense_posterior(flat, ev)
                assert (codes >= 0).all() and (post[tuple(codes[:, v] for v in vs)] > 0).all(), (ctx, "a row of probability zero")
            else:
                assert all((codes[:, v] == (ev[v] if v in ev else -1)).all() for v in range(n)), ctx
            continue
        if not mass > 0:  # zero mass from a sparse CPT: the program is not empty
            assert val == -np.inf and t_val == -np.inf, (ctx, val)
            want = [ev.get(v, -1) for v in range(n)] if case["kind"] == "max" else [-1] * len(rq["M"])
            assert [int(c) for c in codes] == want, (ctx, list(codes))
            continue
        assert abs(val - np.log(mass)) <= 1e-12, (ctx, val, np.log(mass))
        assert np.array_equal(np.asarray(codes, np.int64), np.asarray(t_codes, np.int64)), (ctx, "codes differ from the twin's", list(codes), list(t_codes))
        if best is not None:
            assert np.array_equal(np.asarray(codes, np.int64), np.asarray(best, np.int64)), (ctx, "codes differ from the dense argmax", list(codes), list(best))
        if case["kind"] == "max":
            assert abs(mc.log_joint(flat, codes) - val) <= 1e-12, ctx


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_step_case_on_the_device(case, prog_sim, tmp_path):
    spec = sc.build_spec(case)
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    eng, flat = bn.backend.engine, mc.flat_of(bn)
    opt, kind = sc.options(case), case["kind"]
    prunes = (0, 1) if kind == "map" else (None,)
    forced = {}
    try:
        for name in sc.OPTION_NAMES:
            eng.set_option(name, opt[name])
        for prune in prunes:
            forced[prune] = _device(eng, flat, case, prune)
    finally:
        for name in sc.OPTION_NAMES:
            eng.set_option(name, sc.DEFAULTS[name])
    tiled = any(e.startswith("tile:") for e in case["edges"])
    for prune in prunes:
        got, ks = forced[prune]
        _check(case, flat, got, _twin(prog_sim, tmp_path, flat, case, opt, prune), _reference(flat, case, spec, prune), f"{case['name']} prune={prune}")
        # the path the case names really ran
        level = ks.get(LEVEL_KERNEL[kind])
        if "zero_mass" not in case["edges"] or level:
            assert level and level["launches"] >= 1, sorted(ks)
        proved = kind != "map" or prune == case["requests"][0]["prune"]  # (the host test proves a map case's edges on the programs of its own prune flag)
        if tiled and proved:
            assert level["items"] > level["launches"], level
        if kind == "map" and proved:
            for what in ("sum", "max"):
                assert (f"map_tile_{what}" in case["edges"]) == (f"ve_map_kernel:{what} tiles" in ks), (what, sorted(ks))
        if kind == "max":
            assert ks["mpe_traceback_kernel"]["items"] == len(case["requests"])
        if kind == "map":
            assert ks["map_traceback_kernel"]["items"] == len(case["requests"])
    # the same requests under the default options: held to the twin under the default options (an option may change the order the
    # search picks, and with it which of two equal maxima wins), and bit for bit the forced run's where the programs are the same
    import dump_plan as dp
    for prune in prunes:
        got, ks = _device(eng, flat, case, prune)
        _check(case, flat, got, _twin(prog_sim, tmp_path, flat, case, sc.DEFAULTS, prune), _reference(flat, case, spec, prune),
               f"{case['name']} prune={prune} default options")
        same = True
        try:
            for rq in case["requests"]:
                words = []
                for o in (opt, sc.DEFAULTS):
                    sc.set_sim_options(o)
                    words.append(dp.program_kind(flat, kind, sc.ids(flat, rq.get("M", [])), sc.ids(flat, rq["ev"]), rq["ec"],
                                                 no_prune=(kind == "map" and not prune) or (kind == "draw" and not rq.get("prune", 0)))[0])
                same = same and np.array_equal(words[0], words[1])
        finally:
            sc.reset_sim_options()
        print(f"{case['name']} prune={prune}: the programs under the default options are {'the same' if same else 'different'}")
        if same:
            for (c1, v1), (c2, v2) in zip(forced[prune][0], got):
                assert np.array_equal(c1, c2) and (v1 == v2), (case["name"], prune, "the default run differs from the forced run of the same program")
        if "gather_gt_64" in case["edges"]:  # M is every free variable: the codes are mpe's on the same evidence, and log_p their log joint
            for rq, (codes, val) in zip(case["requests"], got):
                ev = sc.evidence(flat, rq)
                full, lp = eng.mpe_batch(np.array([0, len(ev)], np.int64), np.array(list(ev), np.int32), np.array(list(ev.values()), np.int32))
                assert np.array_equal(full[0][sc.ids(flat, rq["M"])], codes) and abs(float(lp[0]) - val) <= 1e-12, case["name"]
                assert abs(mc.log_joint(flat, full[0]) - val) <= 1e-12, case["name"]
