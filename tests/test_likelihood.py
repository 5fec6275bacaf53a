"""Likelihood findings (soft evidence) on the device: `likelihood=` of BayesNet.query / mpe / map_query and mibn_set_likelihoods, on the
tiny kernel's twin (tiny_lh_kernel) and on the planned path (likelihood_seed_kernel writes the weights into each request's arena),
against answers of the unmodified reference on augmented networks, the dense numpy twin (tests/likelihood_check.py), the engine's
own hard-evidence calls on the augmented network, and the identities a finding must satisfy."""
import numpy as np
import pandas as pd
import pytest

import golden_util as gu
import likelihood_check as lc
import mpe_check as mc
import netspec
import sorobn_amd
from sorobn_amd import _capi

pytestmark = pytest.mark.gpu

RAW = _capi.Q_UNNORMALISED
STRICT = 1e-9


def kernels(eng):
    return {k["name"]: k for k in eng.kernel_stats() if k["launches"] > 0}


def golden_nets():
    import test_likelihood_host as host
    return host.golden_nets()


def findings_of(req):
    return {name: {lab: x for lab, x in pairs} for name, pairs in req["findings"].items()}


def device(spec, **options):
    bn = netspec.build(spec, sorobn_amd.BayesNet).use_device(0)
    for k, v in options.items():
        bn.backend.engine.set_option(k, v)
    return bn, mc.flat_of(bn)


@pytest.fixture(scope="module")
def asia():
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "asia")
    return spec, *device(spec)


def test_reference_goldens_on_both_paths():
    """Every golden of likelihood_findings.json within 1e-9 through tiny_lh_kernel (option tiny 1) and through the planner with
    likelihood_seed_kernel (tiny 0); the two paths within 1e-12 of each other."""
    n = 0
    for spec, reqs in golden_nets():
        bn, f = device(spec)
        eng = bn.backend.engine
        for k, req in enumerate(reqs):
            ctx = f"{spec['name']}[{k}]"
            event = {name: lab for name, lab in req["event"]}
            answers = {}
            for tiny, kernel in ((1, "tiny_lh_kernel"), (0, "likelihood_seed_kernel")):
                eng.set_option("tiny", tiny)
                ans = bn.query(*req["query"], event=event, likelihood=findings_of(req))
                ran = kernels(eng)
                assert kernel in ran and ran[kernel]["launches"] == 1, (ctx, tiny, sorted(ran))
                assert ("tiny_kernel" in ran, "tiny_lh_kernel" in ran) == (False, tiny == 1), (ctx, tiny, sorted(ran))
                name, inames, rows, vals, multi = gu.expected(req)
                assert ans.name == name and list(ans.index.names) == inames, ctx
                gu.assert_rows_equal(ans.index.tolist(), rows, ctx=ctx)
                err = float(np.max(np.abs(ans.to_numpy() - vals)))
                print(f"{ctx} tiny={tiny}: max|err| vs the reference {err:.2e}")
                assert err <= gu.TOL, (ctx, tiny, err)
                answers[tiny] = ans.to_numpy()
            assert float(np.max(np.abs(answers[0] - answers[1]))) <= 1e-12, ctx
            n += 1
        eng.set_option("tiny", 1)
    assert n >= 15


def test_seed_shapes_on_a_chain():
    """A chain whose variables have 1, 2, 3, 65 and 100 states - 65 and 100 are the smallest cardinalities whose seed takes a second
    stride of the wave that writes it, 1 is the scalar seed - with a finding on each variable in turn and on all at once: the
    normalised posterior, the unnormalised table, the one-cell mass and the MPE against the dense twin."""
    spec = netspec.chain_spec(5, (1, 2, 3, 65, 100), seed=9)
    bn, f = device(spec, tiny=0)
    eng = bn.backend.engine
    assert list(f.card) == [1, 2, 3, 65, 100]
    rng = np.random.default_rng(65)
    lam = [(v, rng.uniform(0.1, 2.0, int(f.card[v]))) for v in range(5)]
    sets = [[x] for x in lam] + [lam, lam[::-1]]
    block = lc.block(sets)
    B = len(sets)
    q = np.full((B, 1), 2, np.int32)
    none = np.zeros((B, 0), np.int32)
    post = eng.query_fixed(q, none, none, likelihoods=block)
    ran = kernels(eng)
    assert ran["likelihood_seed_kernel"]["launches"] == 1 and "tiny_lh_kernel" not in ran, sorted(ran)
    raw = eng.query_fixed(q, none, none, flags=RAW, likelihoods=block)
    mass = eng.query_fixed(np.zeros((B, 0), np.int32), none, none, flags=RAW, likelihoods=block)
    codes, lp = eng.mpe(none, none, likelihoods=block)
    assert kernels(eng)["likelihood_seed_kernel"]["launches"] == 1
    # the findings on the first four variables again, with the last variable observed
    ev = np.full((B - 3, 1), 4, np.int32)
    ec_ = np.full((B - 3, 1), 17, np.int32)
    post_e = eng.query_fixed(q[:B - 3], ev, ec_, likelihoods=lc.block(sets[:B - 3]))
    for b, fs in enumerate(sets):
        ctx = [v for v, _ in fs]
        want = lc.mass(f, [2], {}, fs)
        assert np.all(np.abs(raw[b] - want) <= 1e-12 * want), (ctx, raw[b], want)
        assert float(np.max(np.abs(post[b] - want / want.sum()))) <= 1e-12, (ctx, post[b])
        m = lc.mass(f, [], {}, fs)[0]
        assert abs(mass[b, 0] - m) <= 1e-12 * m, (ctx, mass[b, 0], m)
        want_lp, want_codes, p1, p2 = lc.mpe(f, {}, fs)
        assert p1 - p2 > STRICT * p1, (ctx, "no strict winner")
        assert abs(lp[b] - want_lp) <= 1e-12 and codes[b].tolist() == want_codes.tolist(), (ctx, lp[b], want_lp)
        if b < B - 3:
            assert float(np.max(np.abs(post_e[b] - lc.posterior(f, [2], {4: 17}, fs)))) <= 1e-12, ctx
    # the scalar seed matters for the unnormalised results only
    plain = eng.query_fixed(q[:1], none[:1], none[:1], flags=RAW)
    assert np.all(np.abs(raw[0] - lam[0][1][0] * plain[0]) <= 1e-15)
    assert float(np.max(np.abs(post[0] - eng.query_fixed(q[:1], none[:1], none[:1])[0]))) <= 1e-15


GRID4 = dict(small_cells=16, big_iters=64, tile_h=3)


def ragged_requests(f):
    """Seven requests with 0, 2, 0, 1, 3, 0, 1 findings on the 4 x 4 four-state grid: (query ids, evidence {id: code}, findings)."""
    rng = np.random.default_rng(44)
    ids = [f.id[f"{i:03d}"] for i in range(16)]
    lam = lambda i: (ids[i], rng.uniform(0.1, 1.5, 4))
    return [([ids[15]], {ids[0]: 1}, []),
            ([ids[12]], {ids[3]: 2}, [lam(5), lam(10)]),
            ([ids[3]], {}, []),
            ([ids[9]], {ids[15]: 0, ids[1]: 3}, [lam(9)]),
            ([ids[6]], {ids[12]: 1}, [lam(0), lam(15), lam(7)]),
            ([ids[0]], {ids[15]: 2}, []),
            ([ids[14]], {}, [lam(2)])]


def ragged_call(eng, reqs, which):
    """The requests as ONE call of the query, MPE or marginal-MAP entry point -> comparable arrays."""
    e_off = np.concatenate([[0], np.cumsum([len(ev) for _, ev, _ in reqs])]).astype(np.int64)
    evs = np.array([v for _, ev, _ in reqs for v in ev], np.int32)
    ecs = np.array([c for _, ev, _ in reqs for c in ev.values()], np.int32)
    block = lc.block([fs for _, _, fs in reqs])
    q_off = np.arange(len(reqs) + 1, dtype=np.int64)
    qv = np.array([q[0] for q, _, _ in reqs], np.int32)
    if which == "query":
        return (eng.query_batch(q_off, qv, e_off, evs, ecs, likelihoods=block)[0].reshape(len(reqs), -1),)
    if which == "mpe":
        return eng.mpe_batch(e_off, evs, ecs, likelihoods=block)
    codes, lp = eng.map_batch(q_off, qv, e_off, evs, ecs, likelihoods=block)
    return codes.reshape(len(reqs), -1), lp


@pytest.mark.parametrize("which", ["query", "mpe", "map"])
def test_ragged_batch_is_bit_for_bit_the_requests_alone(which):
    """Seven requests with 0, 2, 0, 1, 3, 0, 1 findings in one call: every answer is bit for bit the answer of the request sent
    alone - in one chunk, in chunks of three, and with an arena budget that cuts the chunk into several waves (the seeds are
    written again for every wave: the count of seed launches says that several waves ran)."""
    bn, f = device(netspec.grid_spec(4, 4, 4), first_chunk=0)  # (no short first chunk of 1 024 requests: option chunk cuts the call)
    eng = bn.backend.engine
    reqs = ragged_requests(f)
    alone, need = [], 0.0
    for r in reqs:
        alone.append(ragged_call(eng, [r], which))
        need = max(need, eng.stats()["arena_bytes"])
        assert ("likelihood_seed_kernel" in kernels(eng)) == bool(r[2])
    want = [np.concatenate([a[k] for a in alone]) for k in range(len(alone[0]))]
    base_launches = None
    for opt, val, seed_launches in ((None, None, 1), ("chunk", 3, 3), ("arena_gb", 2.2 * need / 1e9, None)):
        if opt:
            eng.set_option(opt, val)
        try:
            got = ragged_call(eng, reqs, which)
            ran = kernels(eng)
            st = eng.stats()
        finally:
            eng.set_option("chunk", 32768)
            eng.set_option("arena_gb", 200.0)
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_), (which, opt, g, w_)
        if opt is None:
            base_launches = st["n_launches"]
        n_seed = ran["likelihood_seed_kernel"]["launches"]
        if seed_launches is not None:  # one chunk = one wave; chunks (0 1 2) (3 4 5) (6): each holds a finding
            assert n_seed == seed_launches, (which, opt, n_seed)
        else:  # at most two requests fit a wave: four waves or more, and the findings sit in requests 1, 3, 4 and 6
            assert st["arena_bytes"] <= 2.2 * need * 1.34 + 4096, (st["arena_bytes"], need)
            assert n_seed >= 2 and st["n_launches"] > base_launches, (which, n_seed, st["n_launches"], base_launches)


def test_findings_reach_fiber_and_tiled_steps():
    """The 4 x 4 four-state grid with small_cells, big_iters and tile_h lowered as tests/test_mpe.py::test_tiles_on_a_small_grid lowers
    them: findings on two inner nodes plus two hard evidence nodes, against the AUGMENTED network through the hard-evidence calls of
    the same engine code.  Posteriors within 1e-12 (two plans of one request); MPE and marginal-MAP codes equal on the original
    variables, the augmented log_p = the findings' log_p - sum log max lambda within 1e-12."""
    spec = netspec.grid_spec(4, 4, 4)
    findings = {"005": {0: 0.2, 1: 0.9, 2: 0.4, 3: 0.6}, "010": {0: 1.0, 1: 0.3, 2: 0.0, 3: 2.5}}
    event = {"000": 1, "013": 2}
    aug, add, log_scale = lc.augment(spec, findings)
    bn, f = device(spec, **GRID4)
    bn_a, f_a = device(aug, **GRID4)
    eng = bn.backend.engine
    eng.set_option("split_kinds", 1)  # (the statistics then name every class of work that ran)
    n_cmp = 0
    for q in (("015",), ("012",), ("006", "009"), ("005",)):
        got = bn.query(*q, event=event, likelihood=findings)
        ran = kernels(eng)
        want = bn_a.query(*q, event={**event, **add})
        assert list(got.index) == list(want.index)
        assert float(np.max(np.abs(got.to_numpy() - want.to_numpy()))) <= 1e-12, q
        if q == ("015",):
            assert "likelihood_seed_kernel" in ran
            # (split_kinds names the classes: "segments" are the small steps, every "fiber<..>" and "generic<n>" row is a tiled launch)
            fiber = [n for n in ran if n.startswith("fiber<")]
            tiled = [n for n in ran if n.startswith(("fiber<", "generic<", "ve_sweep"))]
            assert fiber and tiled and "segments" in ran, sorted(ran)
        n_cmp += 1
    eng.set_option("split_kinds", 0)
    got, lp = bn.mpe(event, return_log_prob=True, likelihood=findings)
    ran = kernels(eng)
    assert "likelihood_seed_kernel" in ran
    # (a tiled max step is a level - a launch - of its own: more launches than the same call with the product's options)
    for k, v in dict(small_cells=512, big_iters=4096, tile_h=0).items():
        eng.set_option(k, v)
    got_d, lp_d = bn.mpe(event, return_log_prob=True, likelihood=findings)
    assert ran["ve_max_kernel"]["launches"] > kernels(eng)["ve_max_kernel"]["launches"], ran
    assert got_d.tolist() == got.tolist() and abs(lp_d - lp) <= 1e-12
    for k, v in GRID4.items():
        eng.set_option(k, v)
    want, lp_a = bn_a.mpe({**event, **add}, return_log_prob=True)
    assert [got[n] for n in spec["nodes"]] == [want[n] for n in spec["nodes"]]
    assert abs(lp_a - (lp - log_scale)) <= 1e-12, (lp, lp_a, log_scale)
    m = ("015", "006", "003")
    got, lp = bn.map_query(*m, event=event, return_log_prob=True, likelihood=findings)
    ran = kernels(eng)
    assert "likelihood_seed_kernel" in ran and ran["ve_map_kernel:sum tiles"]["launches"] > 0, sorted(ran)
    want, lp_a = bn_a.map_query(*m, event={**event, **add}, return_log_prob=True)
    assert got.tolist() == want.tolist() and None not in got.tolist()
    assert abs(lp_a - (lp - log_scale)) <= 1e-12, (lp, lp_a, log_scale)
    assert n_cmp == 4


@pytest.mark.parametrize("tiny", [1, 0])
def test_identities(asia, tiny):
    spec, bn, f = asia
    eng = bn.backend.engine
    eng.set_option("tiny", tiny)
    try:
        q, ev = ("Lung cancer", "Bronchitis"), {"Visit to Asia": True}
        plain = bn.query(*q, event=ev).to_numpy()
        # a one-hot lambda is hard evidence
        hard = bn.query(*q, event={**ev, "Dispnea": True}).to_numpy()
        soft = bn.query(*q, event=ev, likelihood={"Dispnea": {True: 1.0}}).to_numpy()
        assert float(np.max(np.abs(hard - soft))) <= 1e-12
        # an all-ones lambda is no finding
        ones = bn.query(*q, event=ev, likelihood={"Dispnea": {True: 1.0, False: 1.0}, "Smoker": {True: 1.0, False: 1.0}}).to_numpy()
        assert float(np.max(np.abs(ones - plain))) <= 1e-12
        # lambda scaled by 4 (a power of two: exact): the same posterior bit for bit, four times the unnormalised mass exactly
        lam = {"Dispnea": {True: 0.7, False: 0.15}, "Positive X-ray": {True: 0.3, False: 0.55}}
        lam4 = {n: {k: 4.0 * x for k, x in d.items()} for n, d in lam.items()}
        a, b = bn.query(*q, event=ev, likelihood=lam).to_numpy(), bn.query(*q, event=ev, likelihood={"Dispnea": lam4["Dispnea"], "Positive X-ray": lam["Positive X-ray"]}).to_numpy()
        assert np.array_equal(a, b)
        qi, evi, eci = [[f.id[n] for n in q]], [[f.id["Visit to Asia"]]], [[1]]
        blk = lambda d: lc.block([lc.encode(f, d)])
        m1 = eng.query_fixed(qi, evi, eci, flags=RAW, likelihoods=blk(lam))
        m4 = eng.query_fixed(qi, evi, eci, flags=RAW, likelihoods=blk({"Dispnea": lam4["Dispnea"], "Positive X-ray": lam["Positive X-ray"]}))
        assert np.array_equal(m4, 4.0 * m1) and m1.sum() > 0
        p1 = eng.query_fixed(np.zeros((1, 0), np.int32), evi, eci, flags=RAW, likelihoods=blk(lam))
        p4 = eng.query_fixed(np.zeros((1, 0), np.int32), evi, eci, flags=RAW, likelihoods=blk(lam4))
        assert p4[0, 0] == 16.0 * p1[0, 0] and abs(p1[0, 0] - m1.sum()) <= 1e-12 * p1[0, 0]
        # a finding on a query variable is posterior * lambda, renormalised
        post = bn.query("Dispnea", event=ev)
        w = np.array([0.25, 0.75])
        assert list(post.index) == [False, True]
        want = post.to_numpy() * w / (post.to_numpy() * w).sum()
        got = bn.query("Dispnea", event=ev, likelihood={"Dispnea": {False: 0.25, True: 0.75}}).to_numpy()
        assert float(np.max(np.abs(got - want))) <= 1e-12
        ran = kernels(eng)
        assert ("tiny_lh_kernel" in ran) == (tiny == 1) and ("likelihood_seed_kernel" in ran) == (tiny == 0), sorted(ran)
        # and the twin agrees with all of it
        twin = lc.posterior(f, [f.id[n] for n in sorted(q)], {evi[0][0]: 1}, lc.encode(f, lam))  # (the Series' order: sorted names)
        assert float(np.max(np.abs(a - twin[twin > 0]))) <= 1e-12
    finally:
        eng.set_option("tiny", 1)


@pytest.mark.parametrize("tiny", [1, 0])
def test_zero_mass(asia, tiny):
    """Weights that are zero on every state of positive posterior behave like impossible evidence."""
    spec, bn, f = asia
    eng = bn.backend.engine
    eng.set_option("tiny", tiny)
    try:
        # "TB or cancer" is a deterministic OR: with Tuberculosis observed True, its state False has no mass
        ev = {"Tuberculosis": True}
        for lam in ({"TB or cancer": {False: 1.0}}, {"Smoker": {True: 0.0, False: 0.0}}, {"Smoker": {}}):
            assert len(bn.query("Dispnea", event=ev, likelihood=lam)) == 0
            s, lp = bn.mpe(ev, return_log_prob=True, likelihood=lam)
            assert lp == -np.inf and all(s[n] is None for n in s.index if n not in ev) and bool(s["Tuberculosis"]) is True
            s, lp = bn.map_query("Dispnea", "Smoker", event=ev, return_log_prob=True, likelihood=lam)
            assert lp == -np.inf and s.tolist() == [None, None]
            blk = lc.block([lc.encode(f, lam)])
            mass = eng.query_fixed(np.zeros((1, 0), np.int32), [[f.id["Tuberculosis"]]], [[1]], flags=RAW, likelihoods=blk)
            assert mass[0, 0] == 0.0
            dense = eng.query_fixed([[f.id["Dispnea"]]], [[f.id["Tuberculosis"]]], [[1]], likelihoods=blk)
            assert np.array_equal(dense, np.zeros((1, 2)))
    finally:
        eng.set_option("tiny", 1)


def _plain(eng, f):
    q = [[f.id["Dispnea"]], [f.id["Smoker"]]]
    ev = [[f.id["Visit to Asia"]], [f.id["Positive X-ray"]]]
    return eng.query_fixed(q, ev, [[1], [0]])


@pytest.mark.parametrize("tiny", [1, 0])
def test_the_staged_block(asia, tiny):
    spec, bn, f = asia
    eng = bn.backend.engine
    L = eng._L
    eng.set_option("tiny", tiny)
    try:
        before = _plain(eng, f)
        s, d = f.id["Smoker"], f.id["Dispnea"]
        good = ([0, 1, 2], [s, d], [0, 2, 4], [0.2, 0.8, 0.6, 0.4])
        q = [[f.id["Dispnea"]], [f.id["Smoker"]]]
        ev = [[f.id["Visit to Asia"]], [f.id["Positive X-ray"]]]
        with_block = eng.query_fixed(q, ev, [[1], [0]], likelihoods=good)
        assert not np.array_equal(with_block, before)
        # consumed by one call: the next plain call is what it was
        assert np.array_equal(_plain(eng, f), before)
        # an empty block - B = 2 and no finding - is the call without a block, bit for bit
        assert np.array_equal(eng.query_fixed(q, ev, [[1], [0]], likelihoods=([0, 0, 0], [], [0], [])), before)
        assert "likelihood_seed_kernel" not in kernels(eng) and "tiny_lh_kernel" not in kernels(eng)

        def refused(call, code, *needles):
            with pytest.raises(_capi.MibnError) as err:
                call()
            assert err.value.code == code, (err.value.code, str(err.value))
            for n in needles:
                assert n in str(err.value), str(err.value)
            assert np.array_equal(_plain(eng, f), before)  # the block is gone, the context works

        # a block for another number of requests
        eng.set_likelihoods(([0, 1], [s], [0, 2], [0.2, 0.8]))
        refused(lambda: _plain(eng, f), _capi.E_ARG, "1 requests", "2")
        # the calls that take no findings refuse a staged block with their codes, and drop it
        eng.set_likelihoods(good)
        refused(lambda: eng.wait(eng.submit_fixed(q, ev, [[1], [0]])), _capi.E_STATE, "mibn_submit_batch")
        eng.set_likelihoods(good)
        acc = np.zeros(4)
        refused(lambda: eng.expect_batch([0, 1, 2], [q[0][0], q[1][0]], [0, 1, 2], [ev[0][0], ev[1][0]], [1, 0], [0, 2], [1, 1], acc), _capi.E_STATE,
                "mibn_expect_batch")
        eng.set_likelihoods(good)
        refused(lambda: eng.posterior_sample(np.array(ev, np.int32), np.array([[1], [0]], np.int32), 2), _capi.E_ARG, "mibn_posterior_sample_batch")
        # validation, all on the host and with the request's index
        bad = {"a wrong length": ([0, 1, 2], [s, d], [0, 2, 5], [0.2, 0.8, 0.6, 0.4, 0.1]),
               "a negative weight": ([0, 1, 2], [s, d], [0, 2, 4], [0.2, 0.8, -0.6, 0.4]),
               "NaN": ([0, 1, 2], [s, d], [0, 2, 4], [0.2, 0.8, float("nan"), 0.4]),
               "infinity": ([0, 1, 2], [s, d], [0, 2, 4], [0.2, 0.8, float("inf"), 0.4]),
               "an id out of range": ([0, 1, 2], [s, len(f.card)], [0, 2, 4], [0.2, 0.8, 0.6, 0.4]),
               "a negative id": ([0, 1, 2], [s, -1], [0, 2, 4], [0.2, 0.8, 0.6, 0.4]),
               "a duplicate": ([0, 0, 2], [d, d], [0, 2, 4], [0.2, 0.8, 0.6, 0.4])}
        for what, block in bad.items():
            refused(lambda: eng.set_likelihoods(block), _capi.E_ARG, "request 1")
        # a finding variable that is evidence of its request: found by the call that consumes the block
        overlap = ([0, 1, 2], [s, ev[1][0]], [0, 2, 4], [0.2, 0.8, 0.6, 0.4])
        refused(lambda: eng.query_fixed(q, ev, [[1], [0]], likelihoods=overlap), _capi.E_ARG, "request 1", "cannot be part of the event")
        refused(lambda: eng.mpe(np.array(ev, np.int32), np.array([[1], [0]], np.int32), likelihoods=overlap), _capi.E_ARG, "request 1")
        refused(lambda: eng.map(np.array(q, np.int32), np.array(ev, np.int32), np.array([[1], [0]], np.int32), likelihoods=overlap), _capi.E_ARG, "request 1")
        # mpe and map consume a block too: the next call of theirs is plain again
        e2, c2 = np.array(ev, np.int32), np.array([[1], [0]], np.int32)
        codes0, lp0 = eng.mpe(e2, c2)
        codes1, lp1 = eng.mpe(e2, c2, likelihoods=good)
        codes2, lp2 = eng.mpe(e2, c2)
        assert np.array_equal(lp0, lp2) and np.array_equal(codes0, codes2) and not np.array_equal(lp0, lp1)
        m0 = eng.map(np.array(q, np.int32), e2, c2)
        m1 = eng.map(np.array(q, np.int32), e2, c2, likelihoods=good)
        m2 = eng.map(np.array(q, np.int32), e2, c2)
        assert np.array_equal(m0[1], m2[1]) and np.array_equal(m0[0], m2[0]) and not np.array_equal(m0[1], m1[1])
        assert np.array_equal(_plain(eng, f), before)
    finally:
        eng.set_option("tiny", 1)


def test_query_many_with_findings_equals_query(asia):
    spec, bn, f = asia
    reqs = [(("Dispnea",), {"Smoker": True}), (("Smoker", "Bronchitis"), {}, {"Dispnea": {True: 0.9, False: 0.2}, "Smoker": pd.Series({True: 2.0})}),
            (("Lung cancer",), {}, None), (("Dispnea",), {"Tuberculosis": False}, {"Smoker": {False: 4.0, True: 0.5}})]
    out = bn.query_many(reqs)
    for r, got in zip(reqs, out):
        want = bn.query(*r[0], event=r[1], likelihood=r[2] if len(r) == 3 else None)
        assert got.name == want.name and list(got.index) == list(want.index)
        assert float(np.max(np.abs(got.to_numpy() - want.to_numpy()))) <= 1e-15
