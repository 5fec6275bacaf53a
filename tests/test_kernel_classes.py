"""The class matrix on the device (pytest -m gpu): every case of tests/class_cases.py - small pinned networks whose programs contain,
between them, every class of work the planner can emit - against the C oracle, request by request and cell by cell, once with one
launch per class (the statistics then name the classes that ran) and once in the product's launch shape (ve_mfma_kernel for the
one-table fp64-MFMA classes, ve_segment_kernel for the segments), plus the level kernel's twin of the MFMA kernel.  The cases with a
SWEEP step - the sweep matrix: every path of ve_sweep_dma_kernel by name - run once more under each of the two sweep kernels, alone
and as a batch of three, bit for bit equal (test_sweep_case_under_both_kernels).  The engine plans with the simulator's settings
(_setup), so the programs on the device are the ones tests/test_kernel_classes_host.py proves on the CPU: that the cases contain
the classes and the edge shapes they claim."""
import time

import numpy as np
import pytest

import class_cases as cc
import golden_util as gu
from test_gpu_parity import amd  # noqa: F401  (the fixture of the GPU parity tests)

pytestmark = pytest.mark.gpu

TWIN_TOL = 1e-13  # two forms of one computation (the bound of test_wide_grids_every_request_vs_oracle between SWEEP and CHAIN)
# the sweep class runs in ve_sweep_dma_kernel unless the engine option sweep_dma is off: the statistics carry the kernel's name
STAT_NAMES = {cc.SWEEP: ("ve_sweep_kernel", "ve_sweep_dma_kernel")}

_worst = {}   # class name -> largest |error| against the oracle over the requests whose programs contain it
_worst_sweep = {}  # sweep tag (class_cases.sweep_edges) -> the same, over both sweep kernels and both launch shapes
_wants = {}    # (recipe, request) -> the oracle's posterior
_oracles = {}  # recipe -> OracleNet: a base of the sweep matrix is shared by two or three cases
SWEEP_CASES = [c for c in cc.CASES if any(e.startswith("sweep:") for e in c["edges"])]
_ran = []     # (case name, seconds)
_ran_sweep = []  # the same, of test_sweep_case_under_both_kernels
_t0 = time.perf_counter()


def _run(eng, flat, requests):
    qv = cc.flat_ids(flat, [q for q, _, _ in requests])
    ev = np.concatenate([cc.flat_ids(flat, e) for _, e, _ in requests]) if requests else np.zeros(0, np.int32)
    ec = np.array([c for _, _, cs in requests for c in cs], np.int32)
    q_off = np.arange(len(requests) + 1, dtype=np.int64)
    e_off = np.concatenate([[0], np.cumsum([len(e) for _, e, _ in requests])]).astype(np.int64)
    out, off = eng.query_batch(q_off, qv, e_off, ev, ec)
    return [out[a:b] for a, b in zip(off[:-1], off[1:])], {k["name"] for k in eng.kernel_stats()}


def _setup(amd, case):
    """(engine, flat network, oracle network, options) of a case: the host plans, with the options of the case and nothing the policy turns."""
    import netspec
    from oracle.oracle import OracleNet
    spec = cc.build_spec(case)
    bn = netspec.build(spec, amd.BayesNet)
    eng, flat = bn.backend.engine, bn.backend.flat
    key = repr(case["recipe"])
    if key not in _oracles:
        _oracles[key] = OracleNet(spec)
    opt = cc.options(case)
    eng.set_option("tiny", 0)       # (the small-network kernel would answer these networks without a program)
    eng.set_option("adaptive", 0)
    eng.set_option("gpu_emit", 0)
    eng.set_option("sweep_adapt", cc.MATRIX_SWEEP_ADAPT)  # a SWEEP step's work items are the sweep_iters tiles of the case
    eng.set_option("minfill_above", cc.MATRIX_MINFILL_ABOVE)  # the order search of the simulator: the programs the host test proved
    eng.set_option("second_above", cc.MATRIX_SECOND_ABOVE)
    for name in cc.OPTION_NAMES:
        eng.set_option(name, opt[name])
    return eng, flat, _oracles[key], opt


def _want(case, flat, on, rq):
    """The oracle's posterior of one request of a case - computed once, shared by the tests and by the cases of one base, left unchanged."""
    q, ev, ec = rq
    key = (repr(case["recipe"]), q, tuple(ev), tuple(ec))
    if key not in _wants:
        _wants[key] = cc.oracle_dense(on, int(flat.card[flat.id[f"{q:03d}"]]), q, ev, ec)
        _wants[key].setflags(write=False)
    return _wants[key]


def _note_sweep_tags(flat, opt, reqs, errs):
    """errs[i] - the largest error of request i - under every sweep tag of its program (the simulator names them)."""
    cc.set_sim_options(opt)
    try:
        for rq, e in zip(reqs, errs):
            for tag in cc.planned(flat, [rq])[1]:
                if tag.startswith("sweep:"):
                    _worst_sweep[tag] = max(_worst_sweep.get(tag, 0.0), e)
    finally:
        cc.reset_sim_options()


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_class_case_vs_oracle(amd, case):
    t0 = time.perf_counter()
    eng, flat, on, opt = _setup(amd, case)
    reqs = case["requests"]
    want = [_want(case, flat, on, rq) for rq in reqs]

    def vs_oracle(post, tag):
        errs = [float(np.max(np.abs(p - w))) for p, w in zip(post, want)]
        print(f"{case['name']} {tag}: max|err| vs oracle {max(errs):.3e}")
        return errs

    # (a) one launch per class of work: the statistics name the classes
    eng.set_option("split_kinds", 1)
    post_a, names_a = _run(eng, flat, reqs)
    missing = [c for c in case["classes"] if not any(n in names_a for n in STAT_NAMES.get(c, (c,)))]
    assert not missing, (missing, sorted(names_a))
    errs_a = vs_oracle(post_a, "split_kinds=1")
    # (b) the product's launch shape
    eng.set_option("split_kinds", 0)
    post_b, names_b = _run(eng, flat, reqs)
    if any(c in cc.MFMA1 for c in case["classes"]):
        assert "ve_mfma_kernel" in names_b, sorted(names_b)
    if cc.SEGMENTS in case["classes"]:
        assert "ve_segment_kernel" in names_b, sorted(names_b)
    errs_b = vs_oracle(post_b, "split_kinds=0")
    ab = max(float(np.max(np.abs(a - b))) for a, b in zip(post_a, post_b))
    print(f"{case['name']}: max|split_kinds 1 - 0| {ab:.3e}")
    errs_c, bc = [], 0.0
    if any(c in cc.MFMA1 for c in case["classes"]):
        # (c) the twin of ve_mfma_kernel inside ve_level_kernel
        eng.set_option("mfma_kernel", 0)
        post_c, names_c = _run(eng, flat, reqs)
        assert "ve_mfma_kernel" not in names_c, sorted(names_c)
        errs_c = vs_oracle(post_c, "mfma_kernel=0")
        bc = max(float(np.max(np.abs(b - c))) for b, c in zip(post_b, post_c))
        print(f"{case['name']}: max|mfma_kernel 1 - 0| {bc:.3e}")
    # the figures per class, for the summary below (the simulator names the classes of every request's program)
    cc.set_sim_options(opt)
    try:
        for i, rq in enumerate(reqs):
            e = max([errs_a[i], errs_b[i]] + errs_c[i:i + 1])
            for c in cc.planned(flat, [rq])[0]:
                _worst[c] = max(_worst.get(c, 0.0), e)
    finally:
        cc.reset_sim_options()
    _note_sweep_tags(flat, opt, reqs, [max(a, b) for a, b in zip(errs_a, errs_b)])
    assert max(errs_a) <= gu.TOL, errs_a
    assert max(errs_b) <= gu.TOL, errs_b
    assert ab <= TWIN_TOL, ab
    if errs_c:
        assert max(errs_c) <= gu.TOL, errs_c
        assert bc <= TWIN_TOL, bc
    _ran.append((case["name"], time.perf_counter() - t0))


@pytest.mark.parametrize("case", SWEEP_CASES, ids=[c["name"] for c in SWEEP_CASES])
def test_sweep_case_under_both_kernels(amd, case):
    """Every case with a SWEEP step under ve_sweep_kernel (sweep_dma 0) and ve_sweep_dma_kernel (1): the case's requests, then three
    copies of them with different evidence codes as ONE batch, so that work items of several requests share a launch (the codes do not
    change the shape of a program: the copies carry the case's tags).  Each run against the oracle request by request, the two
    kernels bit for bit equal (the contract of sweep_kernel.hip.h), the statistics row of the kernel the option names."""
    t0 = time.perf_counter()
    eng, flat, on, opt = _setup(amd, case)
    eng.set_option("split_kinds", 0)
    card = lambda v: int(flat.card[flat.id[f"{v:03d}"]])
    batch = [(q, ev, [(c + j) % card(v) for v, c in zip(ev, ec)]) for j in range(3) for q, ev, ec in case["requests"]]
    for label, reqs in (("requests", case["requests"]), ("batch of 3 copies", batch)):
        want = [_want(case, flat, on, rq) for rq in reqs]
        post = {}
        for dma, row, other in ((0, "ve_sweep_kernel", "ve_sweep_dma_kernel"), (1, "ve_sweep_dma_kernel", "ve_sweep_kernel")):
            eng.set_option("sweep_dma", dma)
            post[dma], names = _run(eng, flat, reqs)
            errs = [float(np.max(np.abs(p - w))) for p, w in zip(post[dma], want)]
            print(f"{case['name']} {label}, sweep_dma={dma}: max|err| vs oracle {max(errs):.3e}")
            assert row in names and other not in names, (dma, sorted(names))
            assert max(errs) <= gu.TOL, (label, dma, errs)
            _note_sweep_tags(flat, opt, reqs, errs)
        differ = [i for i, (a, b) in enumerate(zip(post[0], post[1])) if not np.array_equal(a, b)]
        assert not differ, (label, differ, [float(np.max(np.abs(post[0][i] - post[1][i]))) for i in differ])
    eng.set_option("sweep_dma", 1)
    _ran_sweep.append((case["name"], time.perf_counter() - t0))


def test_level_routing_table(amd):
    """The engine's table of level kernels (engine.hip kLevelKernels, planner.h route_of / level_groups) under every setting of the
    options that choose a launch's kernel and stream: cc.ROUTING_CASES - segments, level-kernel classes, an MFMA1 class and SWEEP
    between them - with overlap, seg_kernel, mfma_kernel and sweep_dma each 0 and 1 in the product's launch shape, and the default
    setting once more with one launch per class.  Posteriors against the oracle and against the default setting's; the statistics
    rows are the kernels the setting names, and their launches and workgroups add up to the call's.
    (The "level:" launch-group row is booked per level in the product's launch shape only: with split_kinds 1 it is absent, overlap or not.)"""
    import netspec
    from oracle.oracle import OracleNet
    GROUP, PLANNER = "level:", "order_kernel+emit_kernel"
    default = dict(overlap=1, seg_kernel=1, mfma_kernel=1, sweep_dma=1, split_kinds=0)
    settings = [default] + [dict(overlap=o, seg_kernel=s, mfma_kernel=m, sweep_dma=d, split_kinds=0)
                            for o in (0, 1) for s in (0, 1) for m in (0, 1) for d in (0, 1) if (o, s, m, d) != (1, 1, 1, 1)]
    settings.append(dict(default, split_kinds=1))
    assert len(settings) == 17
    reached = set()
    for case in [c for c in cc.CASES if c["name"] in cc.ROUTING_CASES]:
        spec = cc.build_spec(case)
        bn = netspec.build(spec, amd.BayesNet)
        eng, flat = bn.backend.engine, bn.backend.flat
        on = OracleNet(spec)
        eng.set_option("tiny", 0)
        eng.set_option("adaptive", 0)
        eng.set_option("gpu_emit", 0)
        eng.set_option("sweep_adapt", cc.MATRIX_SWEEP_ADAPT)
        eng.set_option("minfill_above", cc.MATRIX_MINFILL_ABOVE)
        eng.set_option("second_above", cc.MATRIX_SECOND_ABOVE)
        for name, v in cc.options(case).items():
            eng.set_option(name, v)
        reqs, classes = case["requests"], set(case["classes"])
        want = [cc.oracle_dense(on, int(flat.card[flat.id[f"{q:03d}"]]), q, ev, ec) for q, ev, ec in reqs]
        base = None
        for opt in settings:
            for name, v in opt.items():
                eng.set_option(name, v)
            post, _ = _run(eng, flat, reqs)
            rows, st = eng.kernel_stats(), eng.stats()
            base = post if base is None else base
            err = max(float(np.max(np.abs(p - w))) for p, w in zip(post, want))
            twin = max(float(np.max(np.abs(p - b))) for p, b in zip(post, base))
            names = {k["name"] for k in rows}
            kernels = [k for k in rows if not k["name"].startswith(GROUP) and k["name"] != PLANNER]
            print(f"{case['name']} {opt}: max|err| vs oracle {err:.3e}, vs the default setting {twin:.3e}; {sorted(names)}; "
                  f"launches {sum(k['launches'] for k in kernels):.0f} / {st['n_launches']:.0f}, workgroups {sum(k['items'] for k in kernels):.0f} / {st['n_workgroups']:.0f}")
            assert err <= gu.TOL, (opt, err)
            assert twin <= TWIN_TOL, (opt, twin)
            assert sum(k["launches"] for k in kernels) == st["n_launches"] > 0, opt
            assert sum(k["items"] for k in kernels) == st["n_workgroups"] > 0, opt
            sweep_row = "ve_sweep_dma_kernel" if opt["sweep_dma"] else "ve_sweep_kernel"
            if opt["split_kinds"]:
                expect = {sweep_row if c == cc.SWEEP else c for c in classes}
            else:
                seg = cc.SEGMENTS in classes and opt["seg_kernel"]
                mf = bool(classes & set(cc.MFMA1)) and opt["mfma_kernel"]
                expect = {"ve_segment_kernel"} if seg else set()
                expect |= {"ve_mfma_kernel"} if mf else set()
                expect |= {sweep_row} if cc.SWEEP in classes else set()
                if classes - {cc.SWEEP} - ({cc.SEGMENTS} if seg else set()) - (set(cc.MFMA1) if mf else set()):
                    expect.add("ve_level_kernel")
            assert {k["name"] for k in kernels} == expect, (opt, sorted(names), sorted(expect))
            assert any(n.startswith(GROUP) for n in names) == bool(opt["overlap"] and not opt["split_kinds"]), (opt, sorted(names))
            reached |= expect
        for name, v in default.items():
            eng.set_option(name, v)
    assert {"ve_level_kernel", "ve_segment_kernel", "ve_mfma_kernel", "ve_sweep_kernel", "ve_sweep_dma_kernel"} <= reached, sorted(reached)


def test_class_matrix_summary():
    """A reporting step: prints the largest error against the oracle per class, the number of cases and the wall time of this file
    from what the cases above left in this module - so its assertions hold only when every case ran, and passed, in this process
    (not under -k, not under xdist).  It writes no file: profiles/class_matrix_gpu.log is the captured output of one
    `pytest -m gpu -s -v` run of this file, kept by hand, and does not refresh itself."""
    print(f"class matrix: {len(_ran)} of {len(cc.CASES)} cases, {time.perf_counter() - _t0:.1f} s wall, "
          f"slowest case {max([s for _, s in _ran] or [0.0]):.2f} s")
    for c in sorted(_worst):
        print(f"  {c:28s} max|err| vs oracle {_worst[c]:.3e}")
    print(f"sweep matrix: {len(_ran_sweep)} of {len(SWEEP_CASES)} cases under both kernels, slowest case {max([s for _, s in _ran_sweep] or [0.0]):.2f} s")
    for e in sorted(_worst_sweep):
        print(f"  {e:28s} max|err| vs oracle {_worst_sweep[e]:.3e}")
    if len(_ran) == len(cc.CASES):
        want = set().union(*[c["classes"] for c in cc.CASES])
        assert set(_worst) == want, set(_worst) ^ want
        assert max(_worst.values()) <= gu.TOL
    if len(_ran) == len(cc.CASES) and len(_ran_sweep) == len(SWEEP_CASES):
        want = {e for c in cc.CASES for e in c["edges"] if e.startswith("sweep:")}
        assert set(_worst_sweep) == want == {f"sweep:{e}" for e in cc.REQUIRED_EDGES["sweep"]}, set(_worst_sweep) ^ want
        assert max(_worst_sweep.values()) <= gu.TOL
