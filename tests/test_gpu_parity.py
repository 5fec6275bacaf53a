"""GPU parity tests (run on the MI355X box: pytest -m gpu).  Everything goes through the C-ABI
(libmibn.so via sorobn_amd._capi); the oracle / golden vectors are only the checker."""
import os

import numpy as np
import pandas as pd
import pytest

import golden_util as gu
import netspec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import sorobn_amd
    from sorobn_amd import _capi
    assert _capi.device_count() > 0, "no HIP device visible"
    return sorobn_amd


def _check_requests(bn, requests, ctx):
    # one batched launch for the whole network, then compare request by request
    answers = bn.query_many([(tuple(r["query"]), {k: v for k, v in r["event"]}) for r in requests])
    worst = 0.0
    for r, ans in zip(requests, answers):
        name, inames, rows, vals, multi = gu.expected(r)
        c = f"{ctx} {r['query']} {r['event']}"
        assert ans.name == name, c
        assert list(ans.index.names) == inames, c
        assert isinstance(ans.index, pd.MultiIndex) == multi, c
        assert ans.dtype == np.float64
        gu.assert_rows_equal(ans.index.tolist(), rows, ctx=c)
        if len(vals):
            worst = max(worst, float(np.max(np.abs(ans.to_numpy() - vals))))
    assert worst <= gu.TOL, (ctx, worst)
    return worst


def test_tiny_kernel_with_non_topological_ids(amd):
    """mibn_set_network accepts ANY acyclic numbering of the variables (include/mibn.h); the small-network kernel enumerates the
    hidden states with running prefix products and must therefore walk the variables parents-first whatever their ids
    (round 2 walked them in id order: wrong posteriors when a parent carried a larger id than its child - ADVICE r2).
    Asia and three sparse random DAGs through the raw C-ABI with randomly permuted ids: the tiny kernel against the
    planner path and against the answers with the original numbering."""
    from sorobn_amd import _capi
    from sorobn_amd.flatten import flatten
    nets = [n for n in gu.load("examples.json") if n["spec"]["name"] == "asia"] + gu.load("random_dags.json")
    rng = np.random.default_rng(8)
    n_done = 0
    for net in nets:
        f = flatten(netspec.build(net["spec"], amd.BayesNet))
        n = len(f.card)
        if n > 32 or len(f.values) > 4096 or float(np.prod(f.card.astype(np.float64))) > 65536 or n_done >= 5:
            continue  # (not a network of the small-network kernel: csrc/tiny_kernel.hip.h tiny_eligible)
        n_done += 1
        perm = rng.permutation(n).astype(np.int32)  # new id of variable v
        assert any(perm[u] > perm[v] for v in range(n) for u in f.scope_vars[f.scope_off[v]:f.scope_off[v + 1] - 1]) or n < 3
        inv = np.argsort(perm)
        card = f.card[inv]
        scopes = [perm[f.scope_vars[f.scope_off[v]:f.scope_off[v + 1]]] for v in inv]
        vals = [f.values[f.value_off[v]:f.value_off[v + 1]] for v in inv]
        scope_off = np.concatenate([[0], np.cumsum([len(x) for x in scopes])]).astype(np.int64)
        value_off = np.concatenate([[0], np.cumsum([len(x) for x in vals])]).astype(np.int64)
        engines = []
        for ids in ("original", "permuted"):
            e = _capi.Engine(0)
            if ids == "original":
                e.set_network(f.card, f.scope_off, f.scope_vars, f.value_off, f.values)
            else:
                e.set_network(card, scope_off, np.concatenate(scopes).astype(np.int32), value_off, np.concatenate(vals))
            engines.append(e)
        B = 400
        qv = rng.integers(0, n, size=B)
        ne = rng.integers(0, 3, size=B)
        evs = [rng.choice([v for v in range(n) if v != qv[b]], size=ne[b], replace=False) for b in range(B)]
        ecs = [[int(rng.integers(0, f.card[v])) for v in evs[b]] for b in range(B)]
        q_off = np.arange(B + 1, dtype=np.int64)
        e_off = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
        flat_e = np.array([v for ev in evs for v in ev], np.int32)
        flat_c = np.array([c for ec in ecs for c in ec], np.int32)
        base, off = engines[0].query_batch(q_off, qv.astype(np.int32), e_off, flat_e, flat_c)
        assert [k["name"] for k in engines[0].kernel_stats()] == ["tiny_kernel"]
        tiny, off2 = engines[1].query_batch(q_off, perm[qv], e_off, perm[flat_e] if len(flat_e) else flat_e, flat_c)
        assert [k["name"] for k in engines[1].kernel_stats()] == ["tiny_kernel"]
        engines[1].set_option("tiny", 0)
        planned, _ = engines[1].query_batch(q_off, perm[qv], e_off, perm[flat_e] if len(flat_e) else flat_e, flat_c)
        assert not any(k["name"] == "tiny_kernel" for k in engines[1].kernel_stats())
        assert np.array_equal(off, off2)
        assert float(np.max(np.abs(tiny - base))) <= 1e-12, net["spec"]["name"]
        assert float(np.max(np.abs(tiny - planned))) <= 1e-12, net["spec"]["name"]
        # the engine-wide option prune = 0 reaches the small-network kernel too: every CPT takes part
        engines[0].set_option("prune", 0)
        a, _ = engines[0].query_batch(q_off, qv.astype(np.int32), e_off, flat_e, flat_c)
        engines[0].set_option("tiny", 0)
        b, _ = engines[0].query_batch(q_off, qv.astype(np.int32), e_off, flat_e, flat_c)
        assert float(np.max(np.abs(a - b))) <= 1e-12
        for e in engines:
            e.close()
    assert n_done >= 3


# small_cells < 1024 forces the FIBER (streaming) step form, normally reserved for > 8 KiB tables, onto the
# small golden networks: mixed cardinalities, sparse CPTs; (big_iters, tile_h) below the defaults (4096, auto)
# turn small steps into tiled levels; fuse = joint elimination of two variables per pass.  What that reaches:
# on these four files the planner emits 18 of its 39 classes of work - segments, generic<2..6>, the NC = 1 FIBER
# classes of every (n_big, cx), a few nc4 / ncN ones and OUTER (the census printed by
# tests/test_kernel_classes_host.py) - and no nc16 or MFMA pair class.  Every class by name, with the
# shapes inside it, is tests/class_cases.py, run on the device by tests/test_kernel_classes.py.
@pytest.mark.parametrize("small_cells,tiling,fuse", [(1024, (4096, 0), 1), (1, (2, 1), 1), (6, (8, 3), 1), (1, (2, 1), 0)])
@pytest.mark.parametrize("fname", ["examples.json", "random_dags.json", "wide_cards.json", "many_nodes.json"])
def test_golden_networks(amd, fname, small_cells, tiling, fuse):
    for net in gu.load(fname):
        bn = netspec.build(net["spec"], amd.BayesNet)
        bn.backend.engine.set_option("tiny", 0)  # (the small-network kernel has its own test below)
        bn.backend.engine.set_option("small_cells", small_cells)
        bn.backend.engine.set_option("big_iters", tiling[0])
        bn.backend.engine.set_option("tile_h", tiling[1])
        bn.backend.engine.set_option("fuse", fuse)
        _check_requests(bn, net["requests"], net["spec"]["name"])


@pytest.mark.parametrize("small_cells,tiling,fuse", [(1024, (4096, 0), 1), (1, (2, 1), 1), (6, (8, 3), 1), (1, (2, 1), 0)])
def test_golden_huge_cardinalities(amd, small_cells, tiling, fuse):
    """the reference's join has no cardinality limit (bayes_net.py:233-250); the goldens stopped at 16.  Random DAGs
    with axes of 17, 33, 64 and 100 states (tests/golden/huge_cards.json: the reference's answers, networks regenerated from their
    recipes) through the GENERIC / FIBER kernels with the same forcing options as test_golden_networks - the streaming forms and the
    tiled levels on tables they would normally never see - and the kernels' classes that actually ran are recorded."""
    seen = set()
    for entry in gu.load("huge_cards.json"):
        spec = gu.dag_spec_from_recipe(entry)
        bn = netspec.build(spec, amd.BayesNet)
        eng = bn.backend.engine
        eng.set_option("tiny", 0)
        eng.set_option("small_cells", small_cells)
        eng.set_option("big_iters", tiling[0])
        eng.set_option("tile_h", tiling[1])
        eng.set_option("fuse", fuse)
        eng.set_option("split_kinds", 1)  # one launch per class: the statistics name the classes
        _check_requests(bn, entry["requests"], spec["name"])
        seen.update(k["name"] for k in eng.kernel_stats())
    assert seen and "tiny_kernel" not in seen, seen
    print(f"huge cardinalities, small_cells {small_cells} tiling {tiling} fuse {fuse}: classes run = {sorted(seen)}")
    # ... and they are the classes the planner writes for these inputs on the CPU (tests/test_kernel_classes_host.py measures the set)
    from class_cases import HUGE_CARDS_CLASSES
    classes = sorted(n for n in seen if n.startswith(("fiber<", "generic<", "ve_sweep")) or n == "segments")
    assert classes == HUGE_CARDS_CLASSES[(small_cells, tiling, fuse)], classes


@pytest.mark.parametrize("mfma_kernel", [1, 0])
@pytest.mark.parametrize("small_cells,tiling,fuse", [(1024, (4096, 0), 1), (3, (4, 1), 1), (20, (64, 2), 1), (3, (4, 1), 0)])
def test_golden_small_grids(amd, small_cells, tiling, fuse, mfma_kernel):
    """(mfma_kernel = 0, VERDICT r5 item 4a: the forcing options put the MFMA pair classes on the small grids; with the option off they run
    inside ve_level_kernel instead of ve_mfma_kernel - both twins against the reference's answers.)"""
    for entry in gu.load("grids_small.json"):
        spec = gu.grid_spec_from_recipe(entry)
        bn = netspec.build(spec, amd.BayesNet)
        bn.backend.engine.set_option("tiny", 0)  # (the small-network kernel has its own test below)
        bn.backend.engine.set_option("mfma_kernel", mfma_kernel)
        bn.backend.engine.set_option("small_cells", small_cells)
        bn.backend.engine.set_option("big_iters", tiling[0])
        bn.backend.engine.set_option("tile_h", tiling[1])
        bn.backend.engine.set_option("fuse", fuse)
        _check_requests(bn, entry["requests"], spec["name"])


def test_tiny_kernel_goldens(amd):
    """The small-network specialisation (csrc/tiny_kernel.hip.h: one lane per request, CPTs in LDS, no planning) on
    every golden network it is eligible for - the four example networks, the small random DAGs (mixed cardinalities,
    zeros, missing rows) and the small grids - against the reference's answers, and against the step-program path."""
    used = 0
    for fname in ("examples.json", "random_dags.json", "wide_cards.json"):
        for net in gu.load(fname):
            bn = netspec.build(net["spec"], amd.BayesNet)
            eng = bn.backend.engine
            _check_requests(bn, net["requests"], net["spec"]["name"] + " tiny")
            if any(k["name"] == "tiny_kernel" for k in eng.kernel_stats()):
                used += 1
                assert eng.stats()["plan_ms"] == 0.0 and eng.stats()["n_launches"] == 1
                reqs = [(tuple(r["query"]), {k: v for k, v in r["event"]}) for r in net["requests"]]
                tiny = bn.query_many(reqs)
                eng.set_option("tiny", 0)
                planned = bn.query_many(reqs)
                assert not any(k["name"] == "tiny_kernel" for k in eng.kernel_stats())
                for a, b in zip(tiny, planned):
                    assert a.index.equals(b.index)
                    if len(a):
                        assert float(np.max(np.abs(a.to_numpy() - b.to_numpy()))) <= 1e-12
    assert used >= 8, used
    for entry in gu.load("grids_small.json"):
        spec = gu.grid_spec_from_recipe(entry)
        bn = netspec.build(spec, amd.BayesNet)
        _check_requests(bn, entry["requests"], spec["name"] + " tiny")
    # the four example networks must all take the kernel
    for net in gu.load("examples.json"):
        bn = netspec.build(net["spec"], amd.BayesNet)
        bn.query_many([(tuple(r["query"]), {k: v for k, v in r["event"]}) for r in net["requests"][:4]])
        assert [k["name"] for k in bn.backend.engine.kernel_stats()] == ["tiny_kernel"], net["spec"]["name"]


def test_golden_grid10x10(amd):
    path = os.path.join(gu.GOLDEN, "grid10x10.json")
    if not os.path.exists(path):
        pytest.skip("grid10x10.json not generated")
    entry = gu.load("grid10x10.json")
    spec = gu.grid_spec_from_recipe(entry)
    bn = netspec.build(spec, amd.BayesNet)
    _check_requests(bn, entry["requests"], spec["name"])


def test_c3_first16_vs_the_reference_answers(amd):
    """The fixed request set of bench.py's `cpu_baseline` leg - requests 0..15 of the C3 stream - against the answers the unmodified
    reference gave in the build container (tests/golden/c3_first16.json, make_c3_first16.py: every request ran to the end, the
    slowest 39 minutes), through query() one by one and through the batched engine call the bench uses: <= 1e-9, labels exact."""
    import json
    gold = json.load(open(os.path.join(gu.GOLDEN, "c3_first16.json")))["requests"]
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 16, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    batched = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    worst = 0.0
    for i, g in enumerate(gold):
        assert g["query"] == int(q[i]) and [e for e, _ in g["evidence"]] == ev[i].tolist() and [c for _, c in g["evidence"]] == ec[i].tolist()
        want = np.zeros(4)
        for key, h in zip(g["index"], g["values_hex"]):
            want[int(key[0])] = float.fromhex(h)
        ans = bn.query(f"{int(q[i]):03d}", event={f"{int(e):03d}": int(c) for e, c in zip(ev[i], ec[i])})
        assert ans.index.tolist() == [int(k[0]) for k in g["index"]], i
        worst = max(worst, float(np.max(np.abs(ans.to_numpy() - want[ans.index.to_numpy()]))), float(np.max(np.abs(batched[i] - want))))
    assert worst <= gu.TOL, worst


def test_c3_fused_vs_single_variable_passes(amd):
    """Size-independent property at the full C3 shapes: eliminating two variables per pass (cx16 / nc16
    kernels, transposed stores) and one variable per pass (cx4 kernels) are different kernels and different
    summation orders of the same contraction - the posteriors must agree to rounding."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 1024, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    be.engine.set_option("split_kinds", 1)  # one launch per class of work: kernel_stats() names the classes that ran
    fused = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    fused_bytes = be.engine.stats()["alg_bytes"]
    names = {k["name"] for k in be.engine.kernel_stats()}
    assert any("cx16" in n for n in names), names
    be.engine.set_option("fuse", 0)
    single = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert be.engine.stats()["alg_bytes"] > 1.3 * fused_bytes
    assert not any("cx16" in k["name"] for k in be.engine.kernel_stats())
    assert np.allclose(fused.sum(1), 1.0, atol=1e-12)
    assert float(np.max(np.abs(fused - single))) <= 1e-13


def test_c3_chain_form_vs_pair_form(amd):
    """CHAIN steps (three variables per pass: pair MFMA + register epilogue, the default) against two-variable
    passes only (option chain=0) on the C3 stream and on the golden 10x10 requests: a different contraction order of the same
    numbers, fewer bytes."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 4096, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    be.engine.set_option("sweep", 0)  # (the SWEEP form would take these steps first: test_c3_sweep_form_vs_chain_form)
    be.engine.set_option("chain", 0)
    pair = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    pair_bytes = be.engine.stats()["alg_bytes"]
    be.engine.set_option("chain", 1)  # the default
    be.engine.set_option("split_kinds", 1)
    chain = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert be.engine.stats()["alg_bytes"] < 0.9 * pair_bytes
    assert any("chain" in k["name"] for k in be.engine.kernel_stats()), [k["name"] for k in be.engine.kernel_stats()]
    assert np.allclose(chain.sum(1), 1.0, atol=1e-12)
    assert float(np.max(np.abs(chain - pair))) <= 1e-13
    be.engine.set_option("split_kinds", 0)
    # several iterations per tile and CHAIN steps on tables of a few thousand cells (partially filled lane blocks)
    be.engine.set_option("tile_h", 3)
    be.engine.set_option("big_iters", 64)
    small = be.engine.query_fixed(to_var[q[:1024]][:, None], to_var[ev[:1024]], ec[:1024])
    assert float(np.max(np.abs(small - pair[:1024]))) <= 1e-13
    be.engine.set_option("tile_h", 0)
    be.engine.set_option("big_iters", 4096)
    entry = gu.load("grid10x10.json")
    _check_requests(bn, entry["requests"], "grid10x10 chain")
    for e in gu.load("grids_small.json"):
        sp = gu.grid_spec_from_recipe(e)
        for small_cells, tiling in [(3, (4, 1)), (20, (64, 2))]:
            b = netspec.build(sp, amd.BayesNet)
            b.backend.engine.set_option("chain", 1)
            b.backend.engine.set_option("sweep", 0)
            b.backend.engine.set_option("tiny", 0)
            b.backend.engine.set_option("small_cells", small_cells)
            b.backend.engine.set_option("big_iters", tiling[0])
            b.backend.engine.set_option("tile_h", tiling[1])
            _check_requests(b, e["requests"], sp["name"] + " chain")


def test_arena_budget_exceeded_path(amd):
    """Option arena_gb below what a chunk needs: the chunk is cut into waves of consecutive requests whose private arenas fit
    the budget together (same posteriors bit for bit, more launches); a budget below ONE request's arena is a clean
    MIBN_E_NOMEM with the reference-style message, not a device OOM."""
    from sorobn_amd import _capi
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 256, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    base = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    launches = be.engine.stats()["n_launches"]
    need = be.engine.stats()["arena_bytes"]
    be.engine.set_option("arena_gb", need / 8 / 1e9)  # an eighth of what the chunk took
    got = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert np.array_equal(got, base)
    assert be.engine.stats()["n_launches"] > 2 * launches
    assert be.engine.stats()["arena_bytes"] <= need / 8 * 1.34 + 4096  # (the allocation grows with a third of headroom)
    be.engine.set_option("arena_gb", 1e-4)  # 100 KB: below a single request's arena
    with pytest.raises(_capi.MibnError) as err:
        be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert err.value.code == _capi.E_NOMEM and "above the arena budget" in str(err.value)
    be.engine.set_option("arena_gb", 200.0)
    assert np.array_equal(be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec), base)  # the context is still usable


def test_sweep_kernels_agree_bit_for_bit(amd):
    """Round 3's sweep kernel (ve_sweep_dma_kernel: tile filled by LDS-DMA, 16-byte LDS accesses on R-cell pairs, wave-local
    stage pairs, the last stage writing the output block from its registers) against round 2's register-staged
    ve_sweep_kernel on the same programs: another lane <-> fiber mapping, another barrier structure, another readout - and the
    SAME sequence of FMAs per output cell, so the posteriors must agree bit for bit.  Covers the canonical 5-, 4- and
    3-variable steps, stages without a new variable (kout < k: the plain readout), the general path (sweep_canon = 0) and
    two tiles per step (4^7-cell tables on the 8x8 grid)."""
    for spec, n_req in ((netspec.grid_spec(10, 10, 4, seed=0), 3072), (netspec.grid_spec(8, 8, 4, seed=3), 512)):
        bn = netspec.build(spec, amd.BayesNet)
        be = bn.backend
        n = len(spec["nodes"])
        q, ev, ec = netspec.c3_requests(n, 4, n_req, 4, seed=5)
        to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(n)], np.int32)
        for opts in ({"sweep": 5}, {"sweep": 4}, {"sweep": 3}, {"sweep": 5, "sweep_canon": 0}, {"sweep": 5, "sweep_iters": 3}):
            for k, v in {"sweep": 5, "sweep_canon": 1, "sweep_iters": 8, **opts}.items():
                be.engine.set_option(k, v)
            be.engine.set_option("sweep_dma", 0)
            old = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
            swept = sum(s["alg_bytes"] for s in be.engine.kernel_stats() if s["name"] == "ve_sweep_kernel")
            assert swept > 0, (spec["name"], opts)
            be.engine.set_option("sweep_dma", 1)
            new = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
            assert np.array_equal(old, new), (spec["name"], opts, float(np.max(np.abs(old - new))))
            assert np.allclose(new.sum(1), 1.0, atol=1e-12)


def test_c3_sweep_form_vs_chain_form(amd):
    """SWEEP steps (up to five variables per pass, the tile resident in LDS: ve_sweep_kernel, the default) against the
    CHAIN / pair programs (option sweep=0) on the C3 stream: another kernel, another contraction order, a quarter fewer
    bytes - and the golden 10x10 answers of the reference with three, four and five variables per pass."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 4096, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    be.engine.set_option("sweep", 0)
    base = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    base_bytes = be.engine.stats()["alg_bytes"]
    assert not any(k["name"].startswith("ve_sweep") for k in be.engine.kernel_stats())  # (the level's launch group carries both names)
    entry = gu.load("grid10x10.json")
    last = base_bytes
    for k in (3, 4, 5):
        be.engine.set_option("sweep", k)
        got = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
        b = be.engine.stats()["alg_bytes"]
        ks = {s["name"]: s for s in be.engine.kernel_stats()}
        assert "ve_sweep_dma_kernel" in ks and ks["ve_sweep_dma_kernel"]["alg_bytes"] > 0.05 * b, list(ks)
        assert b <= last
        last = b
        assert np.allclose(got.sum(1), 1.0, atol=1e-12)
        assert float(np.max(np.abs(got - base))) <= 1e-13, k
        _check_requests(bn, entry["requests"], f"grid10x10 sweep={k}")
    assert last < 0.8 * base_bytes
    be.engine.set_option("sweep_canon", 0)  # the kernel's general path (runtime strides) on the same programs
    got = be.engine.query_fixed(to_var[q[:1024]][:, None], to_var[ev[:1024]], ec[:1024])
    assert float(np.max(np.abs(got - base[:1024]))) <= 1e-13
    be.engine.set_option("sweep_canon", 1)
    # tables of 4^7 - 4^8 cells (one to eight tiles per step) on the 8x8 grid: every class of stage on small inputs
    be.engine.set_option("big_iters", 512)
    small = be.engine.query_fixed(to_var[q[:1024]][:, None], to_var[ev[:1024]], ec[:1024])
    assert float(np.max(np.abs(small - base[:1024]))) <= 1e-13
    be.engine.set_option("big_iters", 4096)


def test_sweep_form_with_other_cardinalities_around_it_gpu(amd):
    """GPU twin of tests/test_host_logic.py::test_sweep_form_with_other_cardinalities_around_it: an 8 x 9 grid whose outer
    columns have 3, 2 and 5 states (the tiles of a SWEEP step then run along axes of other cardinalities) against the C
    oracle and against the CHAIN / pair programs."""
    from oracle.oracle import OracleNet
    R, C = 8, 9
    spec = netspec.mixed_grid_spec(R, C, [3, 4, 4, 4, 4, 4, 4, 2, 5], seed=5)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    n = R * C
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(n)], np.int32)
    on = OracleNet(spec)
    oid = np.array([on.id[f"{i:03d}"] for i in range(n)], np.int32)
    rng = np.random.default_rng(3)
    be.engine.set_option("big_iters", 512)
    B = 48
    qv = rng.integers(n - 2 * C, n, B).astype(np.int32)
    evs = np.stack([rng.choice([v for v in range(n) if v != q], 3, replace=False) for q in qv]).astype(np.int32)
    codes = np.array([[int(rng.integers(0, be.flat.card[to_var[e]])) for e in row] for row in evs], np.int32)
    cells = be.flat.card[to_var[qv]].astype(np.int64)
    q_off = np.arange(B + 1, dtype=np.int64)
    e_off = np.arange(B + 1, dtype=np.int64) * 3
    out_off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
    got, _ = be.engine.query_batch(q_off, to_var[qv], e_off, to_var[evs].reshape(-1), codes.reshape(-1), out_off)
    names = {k["name"] for k in be.engine.kernel_stats()}
    assert "ve_sweep_dma_kernel" in names, names
    be.engine.set_option("sweep", 0)
    ref, _ = be.engine.query_batch(q_off, to_var[qv], e_off, to_var[evs].reshape(-1), codes.reshape(-1), out_off)
    assert float(np.max(np.abs(got - ref))) <= 1e-13
    for i in range(0, B, 4):
        oc, ov = on.query_codes([int(oid[qv[i]])], oid[evs[i]].tolist(), codes[i].tolist())
        assert float(np.max(np.abs(got[out_off[i]:out_off[i + 1]][oc[:, 0]] - ov))) <= gu.TOL


def test_c3_bayes_rule_and_marginalisation_at_full_size(amd):
    """Size-independent properties on the BASELINE C3 stream, whole-grid requests included (no CPU oracle finishes
    those): (i) P(q | e1..e4) equals the slice e4 = v of the two-variable posterior P(q, e4 | e1..e3), renormalised
    - a different request, different relevant set, different elimination order and different kernels for the same
    number; (ii) summing that two-variable posterior over e4 gives the one-variable posterior P(q | e1..e3)."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    B = 8192
    q, ev, ec = netspec.c3_requests(100, 4, B, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    Q, E = to_var[q], to_var[ev]
    cond = be.engine.query_fixed(Q[:, None], E, ec)                                   # P(q | e1..e4)
    joint = be.engine.query_fixed(np.stack([Q, E[:, 3]], 1), E[:, :3], ec[:, :3])     # P(q, e4 | e1..e3), e4 fastest
    prior = be.engine.query_fixed(Q[:, None], E[:, :3], ec[:, :3])                    # P(q | e1..e3)
    joint = joint.reshape(B, 4, 4)
    assert np.allclose(joint.sum((1, 2)), 1.0, atol=1e-12)
    assert float(np.max(np.abs(joint.sum(2) - prior))) <= 1e-12
    sl = joint[np.arange(B), :, ec[:, 3]]
    pe = sl.sum(1)                                                                    # P(e4 = v | e1..e3) > 0: CPTs are positive
    assert pe.min() > 0
    err = np.abs(sl / pe[:, None] - cond)
    assert float(np.max(err * np.minimum(1.0, pe[:, None] * 1e3))) <= 1e-12          # (conditioning on a 1e-6 event amplifies rounding)
    assert float(np.max(err)) <= 1e-9


@pytest.mark.parametrize("seed", range(12))
def test_fresh_random_dags_vs_oracle(amd, seed):
    """New random DAGs (not in the golden files: mixed cardinalities, exact zeros, missing rows), HIP vs the C oracle."""
    from oracle.oracle import OracleNet
    from test_host_logic import _fresh_dag_requests, _oracle_series
    spec, reqs = _fresh_dag_requests(seed)
    on = OracleNet(spec)
    for small_cells, tiling in [(1024, (4096, 0)), (2, (4, 2))]:
        bn = netspec.build(spec, amd.BayesNet)
        bn.backend.engine.set_option("tiny", 0)  # (the small-network kernel has its own test below)
        bn.backend.engine.set_option("small_cells", small_cells)
        bn.backend.engine.set_option("big_iters", tiling[0])
        bn.backend.engine.set_option("tile_h", tiling[1])
        for (q, ev), ans in zip(reqs, bn.query_many(reqs)):
            qs, labels, vals = _oracle_series(on, q, ev)
            assert list(ans.index.names) == qs, (q, ev)
            got = [t if isinstance(t, tuple) else (t,) for t in ans.index.tolist()]
            assert got == labels, (q, ev)
            if len(vals):
                assert float(np.max(np.abs(ans.to_numpy() - vals))) <= gu.TOL, (q, ev)


@pytest.mark.parametrize("shape", [(8, 8), (9, 8), (8, 11)])
def test_wide_grids_every_request_vs_oracle(amd, shape):
    """Grids wide enough for the heavy step forms (SWEEP / CHAIN / pair MFMA / OUTER on 4^8..4^9-cell frontier tables) and
    still small enough for the CPU oracle to answer every request: 96 requests each, all compared."""
    from oracle.oracle import OracleNet
    R, C = shape
    n = R * C
    spec = netspec.grid_spec(R, C, 4, seed=R * 100 + C)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    on = OracleNet(spec)
    q, ev, ec = netspec.c3_requests(n, 4, 96, 3, seed=7)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(n)], np.int32)
    oid = np.array([on.id[f"{i:03d}"] for i in range(n)], np.int32)
    be.engine.set_option("split_kinds", 1)
    post = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    names = {k["name"] for k in be.engine.kernel_stats()}
    assert any("sweep" in x for x in names) and any("nc16-mfma" in x for x in names), names
    be.engine.set_option("sweep", 0)  # ... and the same requests through the CHAIN / pair forms
    post_chain = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert any("chain" in k["name"] for k in be.engine.kernel_stats())
    assert float(np.max(np.abs(post - post_chain))) <= 1e-13
    worst = 0.0
    for i in range(96):
        codes, vals = on.query_codes([int(oid[q[i]])], oid[ev[i]].tolist(), ec[i].tolist())
        dense = np.zeros(4)
        dense[codes[:, 0]] = vals
        worst = max(worst, float(np.max(np.abs(dense - post[i]))))
    assert worst <= gu.TOL, worst


def test_schedule_and_effort_options_do_not_change_answers(amd):
    """`stagger` (groups of requests whose levels are staggered inside a chunk: the same programs in another launch
    order) and the other schedule options must reproduce the posteriors bit for bit; `minfill_above` (the knob the adaptive planning effort turns:
    which requests get the min-fill order search) changes elimination orders, i.e. rounding only."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 6000, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    base = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    base_bytes = be.engine.stats()["alg_bytes"]
    for g in (2, 3, 5):
        be.engine.set_option("stagger", g)
        assert np.array_equal(be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec), base), g
    be.engine.set_option("stagger", 1)
    # round 2: the sweep kernel on its own stream, other workgroup sizes of its launches, the chunking of a call - the same
    # programs in another schedule: bit for bit
    # (round 6: "mfma_kernel" 0 sends the one-table MFMA pair classes back through their twin inside ve_level_kernel - the same tile code,
    # fiber_mfma_call, with the output offsets in registers instead of LDS)
    for name, value, back in (("overlap", 0, 1), ("streams", 2, 1), ("sweep_iters", 4, 8), ("sweep_iters", 2, 8), ("sweep_adapt", 0, 4096),
                              ("first_chunk", 0, 1), ("first_chunk", 2, 1), ("chunk_sets", 3, 2), ("chunk", 4096, 32768), ("mfma_kernel", 0, 1)):
        be.engine.set_option(name, value)
        assert np.array_equal(be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec), base), (name, value)
        be.engine.set_option(name, back)
    # other elimination orders: rounding only
    for name, value, back in (("order_weights", 0, 1), ("builtin_sweeps", 0, 1)):
        be.engine.set_option(name, value)
        other = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
        assert float(np.max(np.abs(other - base))) <= 1e-12, name
        be.engine.set_option(name, back)
    assert np.array_equal(be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec), base)
    be.engine.set_option("minfill_above", 1e18)  # sweeps only
    sweeps = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert be.engine.stats()["alg_bytes"] > 1.1 * base_bytes
    assert float(np.max(np.abs(sweeps - base))) <= 1e-12


@pytest.mark.parametrize("order_effort", [0, 1])
def test_device_planner_writes_the_host_programs(amd, order_effort):
    """(order_effort 1: more candidate orders and the byte model's best two both emitted where the best is expensive - the wave planner
    has it, order_kernel / emit_kernel do not: with wave_plan = 0 the host plans those streams.)
    Option gpu_emit: whole chunks are planned on the device - order_kernel, then emit_kernel: one request per lane runs
    the very code of csrc/emit_core.h that the host's planning workers run, and writes the step program into the chunk's
    device buffer.  Mode 2 makes the engine plan every chunk on the host as well and compare programs, work items and
    statistics word for word (an error otherwise); the posteriors are then the host-planned ones bit for bit - on the C3
    stream, with two query variables and the no-prune flag, with out-of-domain evidence, and on random DAGs with mixed
    cardinalities."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    be.engine.set_option("order_effort", order_effort)
    be.engine.set_option("second_above", 1e7)
    be.engine.set_option("second_on_device", 1)  # (by default a device-planned call runs without the second emission: here the wave planner's is checked)
    q, ev, ec = netspec.c3_requests(100, 4, 6144, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    host = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    host_stats = be.engine.stats()
    # mode 1: the device plans a share of every chunk, the host's workers the rest meanwhile (the share follows the two rates)
    # wave_plan 1 (round 6, default): wave_plan_kernel - one request per wave, csrc/wave_plan.h; 0: order_kernel + emit_kernel - one request
    # per lane, the host's code itself.  Both write the host's programs word for word.
    for wave_plan in (1, 0):
        be.engine.set_option("wave_plan", wave_plan)
        for mode, chunk, share in ((2, 4096, -1), (1, 32768, -1), (1, 2048, 0.3), (1, 32768, 1.0)):
            be.engine.set_option("gpu_emit", mode)
            be.engine.set_option("chunk", chunk)
            be.engine.set_option("emit_share", share)
            dev = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
            st = be.engine.stats()
            assert abs(st["alg_bytes"] - host_stats["alg_bytes"]) <= 1e-9 * host_stats["alg_bytes"] and st["n_steps"] == host_stats["n_steps"]
            assert np.array_equal(dev, host), (wave_plan, mode, chunk, share)
    be.engine.set_option("chunk", 32768)
    be.engine.set_option("emit_share", -1)
    be.engine.set_option("wave_plan", 1)
    be.engine.set_option("gpu_emit", 2)
    for n_ev in (1, 8, 16):  # (other shapes of the stream: short orders, long min-fill orders - checked word for word by mode 2)
        q2, ev2, ec2 = netspec.c3_requests(100, 4, 2048, n_ev, seed=3)
        want = None
        for mode in (0, 2):
            be.engine.set_option("gpu_emit", mode)
            got = be.engine.query_fixed(to_var[q2][:, None], to_var[ev2], ec2)
            if want is None:
                want = got
            assert np.array_equal(got, want), n_ev
    be.engine.set_option("gpu_emit", 1)
    be.engine.set_option("wave_plan", 0)
    for lanes, waves in ((64, 1), (5, 3), (32, 16)):  # the geometry of the planner's launches: requests per wave, waves per workgroup
        be.engine.set_option("plan_lanes", lanes)
        be.engine.set_option("plan_waves", waves)
        assert np.array_equal(be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec), host), (lanes, waves)
    be.engine.set_option("wave_plan", 1)
    assert np.array_equal(be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec), host)
    names = [k["name"] for k in be.engine.kernel_stats()]
    assert "order_kernel+emit_kernel" in names and "ve_sweep_dma_kernel" in names
    be.engine.set_option("gpu_emit", 2)
    from sorobn_amd import _capi
    two_q = to_var[np.stack([q[:512], ev[:512, 0]], 1)]
    two = be.engine.query_fixed(two_q, to_var[ev[:512, 1:]], ec[:512, 1:], flags=_capi.Q_NOPRUNE)
    bad = ec[:512].copy()
    bad[::7, 2] = 9  # a label outside the domain: an all-zero posterior, no steps
    skipped = be.engine.query_fixed(to_var[q[:512]][:, None], to_var[ev[:512]], bad)
    be.engine.set_option("emit_words", 1024)  # programs that do not fit their slot: the host plans the chunk, the slots double
    small = be.engine.query_fixed(to_var[q[:512]][:, None], to_var[ev[:512]], ec[:512])
    assert np.array_equal(small, host[:512])
    be.engine.set_option("gpu_emit", 0)
    assert np.array_equal(two, be.engine.query_fixed(two_q, to_var[ev[:512, 1:]], ec[:512, 1:], flags=_capi.Q_NOPRUNE))
    assert np.array_equal(skipped, be.engine.query_fixed(to_var[q[:512]][:, None], to_var[ev[:512]], bad))
    assert np.all(skipped[::7] == 0) and np.array_equal(skipped[1::7], host[:512][1::7])
    nets = [(net["spec"], net["requests"]) for fname in ("random_dags.json", "wide_cards.json") for net in gu.load(fname)]
    nets += [(gu.grid_spec_from_recipe(e), e["requests"]) for e in gu.load("grids_small.json")]
    for net_spec, requests in nets:
        for small_cells, big_iters in ((1024, 4096), (3, 4)):  # (the second: tiled FIBER steps on small networks)
            b = netspec.build(net_spec, amd.BayesNet)
            b.backend.engine.set_option("tiny", 0)
            b.backend.engine.set_option("small_cells", small_cells)
            b.backend.engine.set_option("big_iters", big_iters)
            reqs = [(tuple(r["query"]), {k: v for k, v in r["event"]}) for r in requests]
            want = b.query_many(reqs)
            b.backend.engine.set_option("gpu_emit", 2)
            got = b.query_many(reqs)
            for a, w in zip(got, want):
                assert a.index.equals(w.index) and np.array_equal(a.to_numpy(), w.to_numpy())
            _check_requests(b, requests, net_spec["name"] + " gpu_emit")
    # the four example networks and friends (no tiny kernel: step programs), and networks of more than 128 variables - which the
    # device planner does not cover: the option is accepted and the host plans
    for net in gu.load("examples.json"):
        b = netspec.build(net["spec"], amd.BayesNet)
        b.backend.engine.set_option("tiny", 0)
        b.backend.engine.set_option("gpu_emit", 2)
        _check_requests(b, net["requests"], net["spec"]["name"] + " gpu_emit")
    for net in gu.load("many_nodes.json"):
        b = netspec.build(net["spec"], amd.BayesNet)
        b.backend.engine.set_option("gpu_emit", 2)
        _check_requests(b, net["requests"], net["spec"]["name"] + " gpu_emit (host)")
        assert "order_kernel+emit_kernel" not in [k["name"] for k in b.backend.engine.kernel_stats()]


def test_wave_planner_hands_what_it_does_not_cover_to_the_host(amd):
    """wave_plan_kernel covers requests of at most 32 evidence variables and a few other bounded shapes (csrc/wave_plan.h, wave_plan_kernel.hip.h):
    a request beyond one reports kEmitErrDevice and the host plans THAT REQUEST into its slot of the device-planned chunk (more than 256 of them in
    a chunk: the whole chunk) - never a different program.  Forty evidence nodes in every eighth request of a device-planned batch: the answers
    are the host-planned ones bit for bit, the chunks stay with the planner's kernel."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    be.engine.set_option("second_on_device", 1)  # (the same search in the host-planned and in the device-planned call: bit for bit below)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    q, ev, ec = netspec.c3_requests(100, 4, 1024, 40, seed=11)
    q4, ev4, ec4 = netspec.c3_requests(100, 4, 1024, 4, seed=12)
    q_off = np.arange(1025, dtype=np.int64)
    ne = np.where(np.arange(1024) % 8 == 0, 40, 4)
    e_off = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
    qq = np.where(np.arange(1024) % 8 == 0, q, q4)
    evs = np.concatenate([ev[i] if i % 8 == 0 else ev4[i] for i in range(1024)])
    ecs = np.concatenate([ec[i] if i % 8 == 0 else ec4[i] for i in range(1024)])
    want, off = be.engine.query_batch(q_off, to_var[qq], e_off, to_var[evs], ecs)
    be.engine.set_option("gpu_emit", 1)
    be.engine.set_option("emit_share", 1.0)
    be.engine.set_option("chunk", 256)
    got, off2 = be.engine.query_batch(q_off, to_var[qq], e_off, to_var[evs], ecs)
    assert np.array_equal(off, off2) and np.array_equal(got, want)
    # ... request by request: the chunks stay device-planned, the host plans the 128 requests beyond the limit into their slots
    planned = [k for k in be.engine.kernel_stats() if k["name"] == "order_kernel+emit_kernel"]
    assert planned and planned[0]["items"] == 1024, planned
    be.engine.set_option("gpu_emit", 2)  # (mode 2: every program, work item and statistic of the mixed chunks against the host planner)
    got2, _ = be.engine.query_batch(q_off, to_var[qq], e_off, to_var[evs], ecs)
    assert np.array_equal(got2, want)
    # the requests it covers, alone: planned by the kernel (mode 2: word for word the host's programs)
    be.engine.set_option("gpu_emit", 2)
    sel = np.arange(1024) % 8 != 0
    a = be.engine.query_fixed(to_var[q4[sel]][:, None], to_var[ev4[sel]], ec4[sel])
    planned = [k for k in be.engine.kernel_stats() if k["name"] == "order_kernel+emit_kernel"]
    assert planned and planned[0]["items"] == int(sel.sum())
    be.engine.set_option("gpu_emit", 0)
    assert np.array_equal(a, be.engine.query_fixed(to_var[q4[sel]][:, None], to_var[ev4[sel]], ec4[sel]))


def test_mixed_chunk_cut_into_waves_on_two_lanes(amd):
    """A chunk planned half by the device and half by the host's workers (the host's programs behind the device's slots), cut into several
    waves by the arena budget, on two lanes with an arena each: the posteriors are the host-planned call's bit for bit.  The same call in
    mode 2 (the device plans every request, checked word for word against the host planner) runs through the same waves and lanes."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    be.engine.set_option("second_on_device", 1)  # (the same search in the host-planned and in the device-planned call)
    q, ev, ec = netspec.c3_requests(100, 4, 1024, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    base = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    launches = be.engine.stats()["n_launches"]
    need = be.engine.stats()["arena_bytes"]
    opts = {"chunk": 512, "gpu_emit": 1, "emit_share": 0.5, "streams": 2, "arena_gb": need / 8 / 1e9}  # 256 requests each to the device and the host
    for k, v in opts.items():
        be.engine.set_option(k, v)
    try:
        got = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
        assert np.array_equal(got, base)
        assert be.engine.stats()["n_launches"] > 2 * launches
        planned = [k for k in be.engine.kernel_stats() if k["name"] == "order_kernel+emit_kernel"]
        assert planned and planned[0]["items"] > 0, planned
        be.engine.set_option("gpu_emit", 2)
        assert np.array_equal(be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec), base)
    finally:
        for k, v in {"chunk": 32768, "gpu_emit": 0, "emit_share": -1, "streams": 1, "arena_gb": 200.0, "second_on_device": 0}.items():
            be.engine.set_option(k, v)


def test_adaptive_policy_starts_a_starved_rank_on_the_device_planner(amd):
    """Option adaptive (bench.py switches it on): an engine with at most four planning threads - a rank of an 8-GPU node with a
    16-CPU quota - plans on the device from its first call (csrc/plan_policy.h, call_start); the answers are the host-planned ones bit for
    bit, and switching the policy off gives the planning back."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    q, ev, ec = netspec.c3_requests(100, 4, 4096, 4, seed=1)
    ref_bn = netspec.build(spec, amd.BayesNet)
    to_var = np.array([ref_bn.backend.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    host = ref_bn.backend.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert "order_kernel+emit_kernel" not in [k["name"] for k in ref_bn.backend.engine.kernel_stats()]
    bn = netspec.build(spec, amd.BayesNet)
    eng = bn.backend.engine
    eng.set_option("threads", 2)
    eng.set_option("adaptive", 1)
    # (order_effort 1: by default the calls the device plans skip the second emission - a starved rank has no time for it - and their plans,
    #  hence the last bits of the posteriors, differ from a host-planned call's; with second_on_device the search is the same and so are the bits)
    eng.set_option("second_on_device", 1)
    for _ in range(2):
        assert np.array_equal(eng.query_fixed(to_var[q][:, None], to_var[ev], ec), host)
        planned = [k for k in eng.kernel_stats() if k["name"] == "order_kernel+emit_kernel"]
        assert planned and planned[0]["items"] > 0
    eng.set_option("second_on_device", 0)  # the default: cheaper plans for the device-planned calls, the same posteriors to the last few bits
    loose = eng.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert [k for k in eng.kernel_stats() if k["name"] == "order_kernel+emit_kernel"]
    assert float(np.max(np.abs(loose - host))) <= 1e-12 and eng.stats()["alg_bytes"] >= ref_bn.backend.engine.stats()["alg_bytes"]  # (equal under order_effort 0)
    eng.set_option("adaptive", 0)
    assert np.array_equal(eng.query_fixed(to_var[q][:, None], to_var[ev], ec), host)
    assert "order_kernel+emit_kernel" not in [k["name"] for k in eng.kernel_stats()]


def test_device_order_search_reproduces_the_host_search(amd):
    """Option gpu_search: the elimination-order search runs as a kernel (order_kernel: one request per lane, the very
    code of csrc/order_search.h that the host runs).  Same orders => same programs => the same posteriors bit for bit
    and the same planned bytes - on the C3 stream and on random DAGs with mixed cardinalities (non-power-of-two cards:
    the floating-point tie-breaks of the min-fill search must agree too)."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 8192, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    host = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    host_bytes = be.engine.stats()["alg_bytes"]
    for mode, chunk in ((2, 16384), (1, 2048)):  # 2: every chunk on the device; 1: first chunk on the host, the rest by one launch
        be.engine.set_option("gpu_search", mode)
        be.engine.set_option("chunk", chunk)
        dev = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
        assert be.engine.stats()["alg_bytes"] == host_bytes
        assert np.array_equal(dev, host), mode
    be.engine.set_option("chunk", 16384)
    be.engine.set_option("gpu_search", 2)
    # two query variables, no-prune flag
    from sorobn_amd import _capi
    two = be.engine.query_fixed(to_var[np.stack([q[:512], ev[:512, 0]], 1)], to_var[ev[:512, 1:]], ec[:512, 1:], flags=_capi.Q_NOPRUNE)
    be.engine.set_option("gpu_search", 0)
    assert np.array_equal(two, be.engine.query_fixed(to_var[np.stack([q[:512], ev[:512, 0]], 1)], to_var[ev[:512, 1:]], ec[:512, 1:], flags=_capi.Q_NOPRUNE))
    for fname in ("random_dags.json", "wide_cards.json"):
        for net in gu.load(fname):
            b = netspec.build(net["spec"], amd.BayesNet)
            b.backend.engine.set_option("tiny", 0)
            reqs = [(tuple(r["query"]), {k: v for k, v in r["event"]}) for r in net["requests"]]
            want = b.query_many(reqs)
            b.backend.engine.set_option("gpu_search", 2)
            got = b.query_many(reqs)
            for a, w in zip(got, want):
                assert a.index.equals(w.index) and np.array_equal(a.to_numpy(), w.to_numpy())
            _check_requests(b, net["requests"], net["spec"]["name"] + " gpu_search")


def test_plan_templates_same_posteriors(amd):
    """A stream that repeats 40 request shapes with changing evidence values: answered from plan templates (default)
    and with every request planned (plan_cache=0) - the same programs, so the same posteriors bit for bit."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    rng = np.random.default_rng(3)
    shapes = [rng.permutation(100)[:5] for _ in range(40)]
    pick = rng.integers(0, 40, 6000)
    q = np.array([shapes[k][0] for k in pick], np.int32)[:, None]
    ev = np.array([shapes[k][1:] for k in pick], np.int32)
    ec = rng.integers(0, 4, (6000, 4)).astype(np.int32)
    templ = be.engine.query_fixed(q, ev, ec)
    be.engine.set_option("plan_cache", 0)
    planned = be.engine.query_fixed(q, ev, ec)
    be.engine.set_option("plan_cache", 1)
    assert np.array_equal(templ, planned)
    assert np.allclose(templ.sum(1), 1.0, atol=1e-12)


def test_single_query_api_alarm(amd):
    """README.md:225-229 (config C1): 0.715828 / 0.284172."""
    spec = next(n for n in gu.load("examples.json") if n["spec"]["name"] == "alarm")["spec"]
    bn = netspec.build(spec, amd.BayesNet)
    ans = bn.query("Burglary", event={"Mary calls": True, "John calls": True})
    expect = pd.Series([0.7158281646356071, 0.28417183536439294], name="P(Burglary)",
                       index=pd.Index([False, True], name="Burglary"))
    pd.testing.assert_series_equal(ans, expect, rtol=0, atol=1e-12)


def test_single_query_zero_copy_path(amd):
    """Round 5: a call of at most 64 requests to the small-network kernel reads its request arrays from - and writes its
    posteriors and the malformed-request flag to - the pinned staging buffer directly (engine.hip run_tiny): the same answers as
    the DMA path (option tiny_zero_copy = 0) and as a larger call, and a malformed request still raises the reference's message."""
    from sorobn_amd import _capi
    for net in gu.load("examples.json"):
        bn = netspec.build(net["spec"], amd.BayesNet)
        eng = bn.backend.engine
        reqs = [(tuple(r["query"]), {k: v for k, v in r["event"]}) for r in net["requests"][:200]]
        big = bn.query_many(reqs)                       # one call of 200 requests: the DMA path
        assert [k["name"] for k in eng.kernel_stats()] == ["tiny_kernel"]
        for i in [i for i in (0, 1, 7, 63, 64, 150) if i < len(reqs)]:
            q, e = reqs[i]
            a = bn.query(*q, event=e)                   # one request: zero-copy
            assert eng.stats()["n_launches"] == 1
            eng.set_option("tiny_zero_copy", 0)
            b = bn.query(*q, event=e)
            eng.set_option("tiny_zero_copy", 1)
            pd.testing.assert_series_equal(a, b, check_exact=True)
            pd.testing.assert_series_equal(a, big[i], check_exact=True)
        small = bn.query_many(reqs[:64])                # one wave of requests: zero-copy
        for i in range(min(64, len(reqs))):
            pd.testing.assert_series_equal(small[i], big[i], check_exact=True)
        with pytest.raises(_capi.MibnError, match="request 2"):
            eng.query_batch([0, 1, 2, 3, 4], [0, 1, 0, 1], [0, 0, 0, 1, 1], [0], [0])  # request 2 (and 3?): query var 0 is also its evidence


def test_reference_unit_tests_replayed_on_the_gpu(amd):
    """VERDICT r4 missing 5: the reference's own unit tests (test_bayes_net.py:116-153, 158-226, 295-312: DataFrame CPTs in any column
    order, string and integer labels, a network without structure) replayed on the HIP backend with pandas' strict Series equality."""
    from test_host_logic import check_reference_unit_tests_replayed
    check_reference_unit_tests_replayed(lambda bn: bn)


def test_pandas_batch_api_on_the_gpu(amd):
    """the drop-in pandas boundary, vectorised - `query()`'s directly built Series, `query_many` (PosteriorBatch),
    `to_frame()` and `query_frame` strictly equal to the reference's tail applied to the posterior (shared with the CPU test)."""
    from test_host_logic import check_pandas_batch_api
    assert check_pandas_batch_api(lambda bn: bn) > 500


def test_query_many_pipelined_c3(amd):
    """`query_many` on 70 000 requests of the C3 stream given as Python (tuple, dict) objects: bulk encode, three sub-batches with
    two engine calls in flight, the answers against the array API bit for bit, a sample of finished Series against `query()`."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    n = 70_000
    q, ev, ec = netspec.c3_requests(100, 4, n, 4, seed=1)
    reqs = [((f"{a:03d}",), {f"{v:03d}": int(c) for v, c in zip(vs, cs)}) for a, vs, cs in zip(q.tolist(), ev.tolist(), ec.tolist())]
    batch = bn.query_many(reqs)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    want = np.concatenate([be.engine.query_fixed(to_var[q[a:a + 32768]][:, None], to_var[ev[a:a + 32768]], ec[a:a + 32768]) for a in range(0, n, 32768)])
    assert np.array_equal(batch.out.reshape(n, 4), want)
    for i in (0, 1, 32767, 32768, 65535, 65536, n - 1):
        pd.testing.assert_series_equal(batch[i], bn.query(*reqs[i][0], event=reqs[i][1]), check_exact=True)
    frame = batch.to_frame()
    assert len(frame) == int((want > 0).sum()) and abs(frame["p"].sum() - n) < 1e-6
    # an unknown name in the last sub-batch: the helper thread's KeyError reaches the caller (the reference's error for an unknown node,
    # bayes_net.py:770), the call in flight is collected, and the engine answers the next batch as if nothing had happened
    bad = list(reqs)
    bad[n - 5] = (("no such node",), {"000": 0})
    with pytest.raises(KeyError):
        bn.query_many(bad)
    again = bn.query_many(reqs[:40_000])
    assert np.array_equal(again.out.reshape(40_000, 4), want[:40_000])


def test_c3_stream_vs_oracle(amd):
    """First requests of the BASELINE C3 stream on the 10x10 grid, HIP vs the C oracle (the oracle
    is pinned to the reference by tests/test_oracle.py).  Cheap requests only: the sparse CPU oracle
    needs seconds to minutes for the wide ones."""
    from oracle.oracle import OracleNet
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 2048, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    post = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert post.shape == (2048, 4)
    assert np.allclose(post.sum(1), 1.0, atol=1e-12)
    on = OracleNet(spec)
    oid = np.array([on.id[f"{i:03d}"] for i in range(100)], np.int32)
    checked, worst = 0, 0.0
    for i in range(2048):
        cost = be.engine.plan_stats([to_var[q[i]]], to_var[ev[i]])["alg_bytes"]
        if cost > 3e6:
            continue
        codes, vals = on.query_codes([int(oid[q[i]])], oid[ev[i]].tolist(), ec[i].tolist())
        dense = np.zeros(4)
        dense[codes[:, 0]] = vals
        worst = max(worst, float(np.max(np.abs(dense - post[i]))))
        checked += 1
        if checked >= 200:
            break
    assert checked >= 50
    assert worst <= gu.TOL, worst


def test_c3_heavy_requests_vs_oracle(amd):
    """The expensive end of the C3 stream: >= 10 requests above 50 MB of plan traffic each - whole
    4^10-cell frontier sweeps through the CHAIN / pair-MFMA / OUTER classes - against the C oracle.  The oracle (sparse
    tables, inner joins, Kahan sums: the reference's algorithm) eliminates in the order the planner chose
    (mibn_plan_order), which makes these requests a matter of seconds instead of the minutes of its row-major default."""
    from oracle.oracle import OracleNet
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 4096, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    cost = be.engine.estimate_costs(to_var[q][:, None], to_var[ev])
    heavy = [int(i) for i in np.argsort(-cost) if 5e7 < be.engine.plan_stats([to_var[q[i]]], to_var[ev[i]])["alg_bytes"] < 1.2e8][:12]
    assert len(heavy) >= 10, len(heavy)
    post = be.engine.query_fixed(to_var[q[heavy]][:, None], to_var[ev[heavy]], ec[heavy])
    on = OracleNet(spec)
    oid = np.array([on.id[f"{i:03d}"] for i in range(100)], np.int32)   # stream id -> oracle id
    var_to_stream = np.argsort(to_var)                                   # engine variable id -> stream id
    worst = 0.0
    for k, i in enumerate(heavy):
        order = be.engine.plan_order([to_var[q[i]]], to_var[ev[i]])
        prio = np.full(100, 1 << 20, np.int32)
        prio[oid[var_to_stream[order]]] = np.arange(len(order), dtype=np.int32)
        codes, vals = on.query_codes([int(oid[q[i]])], oid[ev[i]].tolist(), ec[i].tolist(), order=prio)
        dense = np.zeros(4)
        dense[codes[:, 0]] = vals
        worst = max(worst, float(np.max(np.abs(dense - post[k]))))
    assert worst <= gu.TOL, worst


def _oracle_in_planner_order(spec, be, to_var, q, ev, ec, idxs, n_threads=8):
    """Dense posteriors of stream requests `idxs` from the C oracle (sparse tables, inner joins, Kahan sums: the reference's
    algorithm, oracle/ve_oracle.c), each eliminated in the order the planner chose for it (mibn_plan_order) - seconds instead of
    the minutes of the oracle's row-major default.  One OracleNet per worker thread (ctypes releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle.oracle import OracleNet
    import threading
    var_to_stream = np.argsort(to_var)  # engine variable id -> stream id
    orders = {int(i): be.engine.plan_order([to_var[q[i]]], to_var[ev[i]]) for i in idxs}  # (the engine: one thread)
    local = threading.local()

    def one(i):
        if not hasattr(local, "on"):
            local.on = OracleNet(spec)
            local.oid = np.array([local.on.id[f"{k:03d}"] for k in range(100)], np.int32)  # stream id -> oracle id
        on, oid = local.on, local.oid
        prio = np.full(100, 1 << 20, np.int32)
        prio[oid[var_to_stream[orders[int(i)]]]] = np.arange(len(orders[int(i)]), dtype=np.int32)
        codes, vals = on.query_codes([int(oid[q[i]])], oid[ev[i]].tolist(), ec[i].tolist(), order=prio)
        dense = np.zeros(4)
        dense[codes[:, 0]] = vals
        return dense

    with ThreadPoolExecutor(n_threads) as ex:
        return np.array(list(ex.map(one, [int(i) for i in idxs])))


def _stratified_sample(cost, per_decile, extra_top=0):
    """Stream indices: the first `per_decile` requests (stream order) of every decile of `cost`, plus the `extra_top` most
    expensive ones."""
    edges = np.percentile(cost, np.arange(0, 101, 10))
    picked = []
    for d in range(10):
        lo, hi = edges[d], edges[d + 1]
        band = np.nonzero((cost >= lo) & ((cost < hi) if d < 9 else (cost <= hi)))[0]
        picked += band[:per_decile].tolist()
    if extra_top:
        picked += np.argsort(-cost)[:extra_top].tolist()
    return np.array(sorted(set(picked)), np.int64), edges


def _host_and_device_planned(be, to_var, q, ev, ec, idx):
    """Posteriors of the sample planned by the host's workers and by order_kernel + emit_kernel (bit for bit the same)."""
    eng = be.engine
    eng.set_option("second_on_device", 1)  # (the same search - order_effort 1 with its second emission - in both calls)
    host = eng.query_fixed(to_var[q[idx]][:, None], to_var[ev[idx]], ec[idx])
    eng.set_option("gpu_emit", 1)
    try:
        for attempt in range(2):  # (a program that overflows its slot makes the host plan the chunk and doubles the slots: once more)
            dev = eng.query_fixed(to_var[q[idx]][:, None], to_var[ev[idx]], ec[idx])
            planned = [k for k in eng.kernel_stats() if k["name"] == "order_kernel+emit_kernel"]
            if planned and planned[0]["items"] >= len(idx):
                break
    finally:
        eng.set_option("gpu_emit", 0)
    assert planned and planned[0]["items"] >= len(idx), planned  # the device really planned them
    assert np.array_equal(host, dev)
    return host


def test_c3_stratified_by_plan_cost_vs_oracle(amd):
    """VERDICT r3 missing #6: the C3 stream across ALL of its cost range - 20 requests per decile of the planner's cost estimate
    over the first 65 536 requests of the stream plus the five most expensive ones (0.5 KB .. 113 MB estimated, up to ~160 MB of
    executed plan) - host- and device-planned, against the C oracle eliminating in the planner's order.  bayes_net.py:739-794."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 65536, 4, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    cost = be.engine.estimate_costs(to_var[q][:, None], to_var[ev])
    idx, edges = _stratified_sample(cost, 20, extra_top=5)
    assert len(idx) >= 200
    for d in range(10):  # every decile is represented
        assert np.sum((cost[idx] >= edges[d]) & (cost[idx] <= edges[d + 1])) >= 20
    post = _host_and_device_planned(be, to_var, q, ev, ec, idx)
    assert np.allclose(post.sum(1), 1.0, atol=1e-12)
    want = _oracle_in_planner_order(spec, be, to_var, q, ev, ec, idx)
    worst = float(np.max(np.abs(want - post)))
    assert worst <= gu.TOL, worst


@pytest.mark.parametrize("n_ev", [1, 8, 16])
def test_c3_n_evidence_variants_vs_oracle(amd, n_ev):
    """SURVEY 8(d)'s n_evidence variants of the C3 stream (VERDICT r3 missing #3): 1 query + {1, 8, 16} evidence nodes on the
    10x10 grid - the evidence filtering of bayes_net.py:768-776 collapses 1, 8 or 16 axes - 6 requests per decile of the plan
    cost (>= 50 in all) of the first 8 192 requests, host- and device-planned, against the C oracle in the planner's order;
    and the reference's own answers for the requests of tests/golden/grid10x10_nev.json (make_golden.py grid_nev_fixture)."""
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, ev, ec = netspec.c3_requests(100, 4, 8192, n_ev, seed=1)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    cost = be.engine.estimate_costs(to_var[q][:, None], to_var[ev])
    idx, _ = _stratified_sample(cost, 6, extra_top=2)
    assert len(idx) >= 50
    post = _host_and_device_planned(be, to_var, q, ev, ec, idx)
    assert np.allclose(post.sum(1), 1.0, atol=1e-12)
    want = _oracle_in_planner_order(spec, be, to_var, q, ev, ec, idx)
    worst = float(np.max(np.abs(want - post)))
    assert worst <= gu.TOL, (n_ev, worst)
    # the whole 8 192-request batch: every posterior is a distribution (nothing skipped, no NaN)
    allp = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert allp.shape == (8192, 4) and np.allclose(allp.sum(1), 1.0, atol=1e-12)
    # the reference's own answers
    entry = gu.load("grid10x10_nev.json")
    gu.grid_spec_from_recipe(entry)
    reqs = entry["variants"][str(n_ev)]
    assert len(reqs) >= 5
    for r in reqs:  # (they ARE requests of this stream)
        i = r["stream_index"]
        assert r["query"] == [f"{q[i]:03d}"] and r["event"] == [[f"{e:03d}", int(c)] for e, c in zip(ev[i], ec[i])]
    _check_requests(bn, reqs, f"grid10x10 n_evidence={n_ev}")


def test_impute_gpu(amd):
    """a8: BayesNet.impute (bayes_net.py:877-908, README.md:278-293) through the HIP backend against the reference's
    own answers (tests/golden/impute.json)."""
    n_cases = 0
    for net in gu.load("impute.json"):
        bn = netspec.build(net["spec"], amd.BayesNet)
        for case in net["cases"]:
            sample = {k: v for k, v in case["sample"]}
            if "raises" in case:
                with pytest.raises(Exception):
                    bn.impute(sample)
                continue
            got = bn.impute(sample)
            assert isinstance(got, pd.Series)
            pairs = [[k, netspec._py(v)] for k, v in got.items()]
            if pairs != case["expect"]:
                # only legitimate on an exact tie of the arg-max, which the reference itself resolves by last-bit rounding
                assert [k for k, _ in pairs] == [k for k, _ in case["expect"]]
                missing = [k for k, v in sample.items() if v is None]
                post = bn.query(*missing, event={k: v for k, v in sample.items() if v is not None})
                want = dict(map(tuple, case["expect"]))
                key = lambda d: tuple(d[n] for n in post.index.names)
                assert abs(post[key(want)] - post[key(dict(map(tuple, pairs)))]) < 1e-12, (net["spec"]["name"], sample)
            n_cases += 1
    assert n_cases >= 10
    # README.md:278-293 literally
    alarm = next(n for n in gu.load("examples.json") if n["spec"]["name"] == "alarm")["spec"]
    bn = netspec.build(alarm, amd.BayesNet)
    got = bn.impute({"Alarm": True, "Burglary": True, "Earthquake": False, "John calls": None, "Mary calls": None})
    assert got.to_dict() == {"Alarm": True, "Burglary": True, "Earthquake": False, "John calls": True, "Mary calls": True}


def test_accelerate_live_reference_object_on_the_gpu(amd):
    """The drop-in itself on the device: `accelerate(ref_bn)` on LIVE objects of the unmodified reference (loaded from
    oracle/_ref on the GPU box - byte-compiled from /root/reference by `make -C oracle _ref`); the reference's own
    query() / impute() / predict_proba() run on top of the HIP backend and are compared, whole Series, with the
    untouched reference."""
    from oracle import refload
    from test_host_logic import check_accelerated_reference_object
    if not refload.available():
        pytest.skip("oracle/_ref was not built (make -C oracle _ref where /root/reference is mounted)")
    check_accelerated_reference_object(refload.load(), None)


def test_accelerate_gibbs_rebind_on_the_gpu(amd):
    """`accelerate(ref_bn)` also rebinds `_gibbs_sampling` (the seam bayes_net.py:851-853): the reference's own
    query(..., algorithm="gibbs") on a live reference object runs the HIP chain and post-processes it (869-875)."""
    from oracle import refload
    from test_host_logic import check_accelerated_gibbs
    if not refload.available():
        pytest.skip("oracle/_ref was not built (make -C oracle _ref where /root/reference is mounted)")
    check_accelerated_gibbs(refload.load(), None, n_iterations=400_000, tol=0.02)


def test_c2_stream_vs_reference(amd):
    """BASELINE config 2: the first 2 000 requests of the Asia stream `bench.py` times (netspec.asia_requests, seed 0) through
    the batched C-ABI - the small-network kernel - against the unmodified reference's BayesNet.query (oracle/_ref): values
    within 1e-9 and the zero-probability requests - where the reference returns an EMPTY Series (bayes_net.py:254-255, 790) -
    exactly the requests whose dense posterior is all zero."""
    from oracle import refload
    if not refload.available():
        pytest.skip("oracle/_ref was not built (make -C oracle _ref where /root/reference is mounted)")
    ref_mod = refload.load()
    ref = ref_mod.examples.asia()
    bn = netspec.build(netspec.dump(ref, "asia"), amd.BayesNet)
    be = bn.backend
    reqs = netspec.asia_requests(list(bn.nodes), 2000, seed=0)
    q_off = np.arange(len(reqs) + 1, dtype=np.int64)
    q_vars = np.array([be.flat.id[q] for q, _ in reqs], np.int32)
    e_off = np.concatenate([[0], np.cumsum([len(e) for _, e in reqs])]).astype(np.int64)
    e_vars = np.array([be.flat.id[k] for _, e in reqs for k in e], np.int32)
    e_codes = np.array([be.flat.code_of(be.flat.id[k], v) for _, e in reqs for k, v in e.items()], np.int32)
    post, off = be.engine.query_batch(q_off, q_vars, e_off, e_vars, e_codes)
    assert [k["name"] for k in be.engine.kernel_stats()] == ["tiny_kernel"]
    n_empty, worst = 0, 0.0
    for i, (q, ev) in enumerate(reqs):
        want = ref.query(q, event=ev)
        dense = post[off[i]:off[i + 1]]
        if len(want) == 0:
            n_empty += 1
            assert not dense.any(), (i, q, ev, dense)  # zero-probability evidence: all zeros <-> the reference's empty Series
            continue
        assert dense.sum() > 0, (i, q, ev)
        labels = be.flat.dom_index[be.flat.id[q]]
        got = {lab: dense[c] for c, lab in enumerate(labels) if dense[c] > 0}
        assert set(got) == set(want.index), (i, q, ev)  # rows of probability 0 are absent from the reference's answer
        worst = max(worst, max(abs(got[lab] - want[lab]) for lab in want.index))
        # ... and the pandas object the product API returns is the reference's
        if i < 200:
            pd.testing.assert_series_equal(bn.query(q, event=ev), want, rtol=0, atol=1e-9, check_exact=False)
    assert worst <= 1e-9, worst
    assert n_empty > 0  # (the stream contains TB-or-cancer contradictions: 2.4 % of it)


def _reference_conditionals(ref_mod, bn, node, fast_normalise=False):
    """P(node | Markov boundary) the way bayes_net.py:699-710 builds it: the reference's own pointwise_mul over the CPTs of
    the node and its children, normalised per boundary configuration, levels [*boundary, node].  `fast_normalise`: the same
    g / g.sum() through groupby().transform (the reference's apply-per-group takes minutes on 8^6 groups)."""
    from sorobn.bayes_net import pointwise_mul
    post = pointwise_mul(bn.P[n] for n in [node, *bn.children.get(node, [])])
    boundary = bn.markov_boundary(node)
    if boundary:
        if fast_normalise:
            post = post / post.groupby(boundary).transform("sum")
        else:
            post = post.groupby(boundary, group_keys=False).apply(lambda g: g / g.sum())
        post = post.reorder_levels([*boundary, node])
    return post.sort_index(), boundary


def test_gibbs_conditionals_vs_reference(amd):
    """The deterministic half of the Gibbs path, pinned (SURVEY 8c left the whole path "parity unpinned" because of the
    random stream): `mibn_gibbs_conditional` makes gibbs_kernel write the Markov-blanket conditional it would sample from,
    and that is compared <= 1e-12 with the tables the reference builds from its own factor algebra (bayes_net.py:699-710,
    markov_boundary 1034-1039) - on the four example networks (incl. the zero rows of Asia) with and without evidence,
    and on a 3x3 grid with 8 states (the FAST update form of config 5; its centre node has the maximal boundary of six)."""
    from oracle import refload
    if not refload.available():
        pytest.skip("oracle/_ref was not built (make -C oracle _ref where /root/reference is mounted)")
    ref_mod = refload.load()
    rng = np.random.default_rng(3)
    nets = [(mk, getattr(ref_mod.examples, mk)()) for mk in ("alarm", "asia", "sprinkler", "grades")]
    nets.append(("grid3x3k8", netspec.build(netspec.grid_spec(3, 3, 8, seed=2), ref_mod.BayesNet)))
    worst, n_checked, n_zero = 0.0, 0, 0
    for mk, ref in nets:
        bn = netspec.build(netspec.dump(ref, mk), amd.BayesNet)
        be = bn.backend
        f = be.flat
        n = len(f.card)
        for with_event in ((False, True) if not mk.startswith("grid") else (False,)):
            ev_ids = [int(v) for v in rng.choice(n, size=min(2, n - 2), replace=False)] if with_event else []
            ev_codes = [int(rng.integers(0, f.card[v])) for v in ev_ids]
            states = np.stack([rng.integers(0, f.card[v], size=256) for v in range(n)], axis=1).astype(np.uint8)
            for v, c in zip(ev_ids, ev_codes):
                states[:, v] = c
            free = [v for v in range(n) if v not in ev_ids]
            cycle = sorted(free, key=lambda v: str(f.names[v]))
            for v in free:
                node = f.names[v]
                table, boundary = _reference_conditionals(ref_mod, ref, node, fast_normalise=len(ref.markov_boundary(node)) > 4)
                got = be.engine.gibbs_conditional(v, states, ev_ids, ev_codes, cycle=cycle)
                lookup = table.to_dict()
                labels = list(f.dom_index[v])
                for r in range(len(states)):
                    cond = tuple(f.dom_index[f.id[b]][states[r, f.id[b]]] for b in boundary)
                    want = np.array([lookup.get((*cond, lab) if boundary else lab, 0.0) for lab in labels])
                    if want.sum() == 0:  # a boundary configuration of probability zero: no row in the reference, no draw here
                        n_zero += 1
                        assert not got[r].any(), (mk, node, cond)
                        continue
                    worst = max(worst, float(np.max(np.abs(got[r] - want))))
                    n_checked += 1
    assert worst <= 1e-12, worst
    assert n_checked > 5000 and n_zero > 0, (n_checked, n_zero)


def test_gibbs_chain_shards_reproduce_the_whole(amd):
    """mibn_gibbs_shard: the union of disjoint chain ranges of one stream gives the histogram of the unsharded call bit
    for bit (what the multi-GPU Gibbs path reduces with mibn_comm_reduce_i64)."""
    from sorobn_amd import sharding
    spec = netspec.grid_spec(4, 5, 3, seed=3)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    q, evs, codes = be.encode(("012", "009"), {"000": 1, "019": 2})
    whole = be.engine.gibbs(q, evs, codes, 300, 2000, seed=9)
    for world in (2, 3, 8):
        parts = [be.engine.gibbs(q, evs, codes, hi - lo, 2000, seed=9, chain_first=lo)
                 for lo, hi in (sharding.shard_range(300, world, r) for r in range(world))]
        assert np.array_equal(sum(parts), whole), world
    assert whole.sum() == 300 * 2000
    assert be.engine.gibbs(q, evs, codes, 0, 2000, seed=9, chain_first=5).sum() == 0   # an empty shard


def test_rccl_comm_world_of_one(amd):
    """The RCCL entry points of the C-ABI (mibn_comm_*: dlopen of librccl.so, id exchange through a file, communicator on
    the engine's stream) on the one GPU of this box: all-gather / reduce / max / barrier of a world of one, and the
    sharded Gibbs + posterior gather on top of them - the same code every rank of the N-GPU bench runs."""
    from sorobn_amd import sharding
    spec = netspec.grid_spec(5, 5, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    comm = sharding.RcclComm(be.engine, rank=0, world=1)
    assert (comm.rccl_ranks, comm.rccl_rank) == (1, 0) and be.engine.comm_count() == (1, 0)  # ncclCommCount / ncclCommUserRank
    x = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert np.array_equal(comm.allgather(x), x[None])
    assert np.array_equal(comm.reduce_i64(np.array([1, 2, 3], np.int64)), [1, 2, 3])
    assert np.array_equal(comm.allreduce_max([0.5, 7.0]), [0.5, 7.0])
    comm.barrier()
    q, ev, ec = netspec.c3_requests(25, 4, 64, 3, seed=5)
    to_var = np.array([be.flat.id[f"{i:03d}"] for i in range(25)], np.int32)
    local = be.engine.query_fixed(to_var[q][:, None], to_var[ev], ec)
    assert np.array_equal(sharding.gather_posteriors(local, 64, comm), local)
    qq, evs, codes = be.encode(("012",), {"000": 1})
    assert np.array_equal(sharding.gibbs_sharded(be.engine, comm, qq, evs, codes, 100, 500, seed=3),
                          be.engine.gibbs(qq, evs, codes, 100, 500, seed=3))
    comm.close()


def test_gibbs_matches_exact_posterior(amd):
    """Config-5 style check on strictly positive CPTs (the reference's chain is reducible on
    deterministic CPTs): pooled chain estimate vs the exact backend.  Parity
    with the reference's stream is unpinned (vose absent), so the check is statistical."""
    spec = netspec.grid_spec(4, 5, 3, seed=3)
    bn = netspec.build(spec, amd.BayesNet)
    be = bn.backend
    ev = {"000": 1, "019": 2, "007": 0}
    for q in (("012",), ("009", "010")):
        exact = bn.query(*q, event=ev)
        n_chains, n_iter = 512, 4000
        got = be.gibbs_sampling(*q, event=ev, n_iterations=n_iter, n_chains=n_chains, seed=11)
        got = amd.BayesNet._finish(got, q)
        assert got.index.equals(exact.index)
        assert abs(got.sum() - 1.0) < 1e-12
        # 2M correlated samples: 0.01 absolute is > 6 sigma even with an autocorrelation time of 50
        assert float(np.max(np.abs(got.to_numpy() - exact.to_numpy()))) < 0.01
    # different seeds give different streams, same seed the same counts
    a = be.gibbs_sampling("012", event=ev, n_iterations=500, n_chains=64, seed=1)
    b = be.gibbs_sampling("012", event=ev, n_iterations=500, n_chains=64, seed=1)
    c = be.gibbs_sampling("012", event=ev, n_iterations=500, n_chains=64, seed=2)
    assert a.equals(b) and not a.equals(c)
    # the LDS-resident tables (default when they fit) and the L2 path run the same arithmetic on the same streams
    be.engine.set_option("gibbs_lds", 0)
    d = be.gibbs_sampling("012", event=ev, n_iterations=500, n_chains=64, seed=1)
    be.engine.set_option("gibbs_lds", 1)
    assert a.equals(d)


def test_gibbs_eight_lanes_per_chain_bit_for_bit(amd):
    """gibbs_kernel8 (round 4: eight lanes per chain - a lane per candidate state, a DPP scan in the serial order, one Philox draw
    per lane and eight iterations) against round 3's one-chain-per-lane kernel (gibbs_lds=2) and the L2 path (gibbs_lds=0): the same
    Philox counters, the same products and running sums, so the same histograms bit for bit - 3- and 8-state grids, one and two
    query variables, chain counts that do not fill the last wave, shards of one stream."""
    for (R, C, K, q, ev, chains, iters) in ((4, 5, 3, ("012",), {"000": 1, "019": 2, "007": 0}, 61, 700),
                                            (4, 5, 3, ("009", "010"), {"000": 1}, 130, 300),
                                            (5, 10, 8, ("025",), {"000": 3, "009": 1, "040": 7, "049": 0, "022": 5}, 128, 2000),
                                            (3, 3, 8, ("004", "008"), {}, 9, 1500)):
        bn = netspec.build(netspec.grid_spec(R, C, K, seed=2), amd.BayesNet)
        be = bn.backend
        got = {}
        for mode in (1, 2, 0):
            be.engine.set_option("gibbs_lds", mode)
            got[mode] = be.gibbs_sampling(*q, event=ev, n_iterations=iters, n_chains=chains, seed=5)
        be.engine.set_option("gibbs_lds", 1)
        assert got[1].equals(got[2]) and got[1].equals(got[0]), (R, C, K, q)
        assert abs(got[1].sum() - 1.0) < 1e-12
        # shards of one stream (mibn_gibbs_shard): two halves = the whole
        qq, evs, codes = be.encode(q, ev)
        whole = be.engine.gibbs(qq, evs, codes, chains, iters, seed=9)
        cut = chains // 3
        parts = be.engine.gibbs(qq, evs, codes, cut, iters, seed=9) + be.engine.gibbs(qq, evs, codes, chains - cut, iters, seed=9, chain_first=cut)
        assert np.array_equal(whole, parts)


def test_gibbs_through_query_api(amd):
    """query(..., algorithm='gibbs', n_iterations=N): one chain like the reference (bayes_net.py:850-853),
    returns value counts / N over the visited joint states."""
    spec = next(n for n in gu.load("examples.json") if n["spec"]["name"] == "sprinkler")["spec"]
    bn = netspec.build(spec, amd.BayesNet)
    ans = bn.query("Rain", event={"Sprinkler": True}, algorithm="gibbs", n_iterations=20000)
    assert ans.name == "P(Rain)" and ans.index.name == "Rain" and ans.index.tolist() == [False, True]
    assert abs(ans.sum() - 1.0) < 1e-12
    assert abs(ans[False] - 0.7) < 0.03  # bayes_net.py:751-755: exact answer 0.7 / 0.3
    many = bn.query("Rain", event={"Sprinkler": True}, algorithm="gibbs", n_iterations=2000, n_chains=256)
    assert abs(many[False] - 0.7) < 0.01


def test_config5_gibbs_50_nodes_8_states(amd):
    """BASELINE config 5 at reduced length: 5x10 grid topology, K=8, query node 25, evidence nodes
    {0, 9, 40, 49, 22}; 128 chains x 20k single-site updates vs the exact posterior."""
    spec = netspec.grid_spec(5, 10, 8, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    rng = np.random.default_rng(1)
    ev = {f"{n:03d}": int(rng.integers(0, 8)) for n in (0, 9, 40, 49, 22)}
    exact = bn.query("025", event=ev)
    got = bn.query("025", event=ev, algorithm="gibbs", n_iterations=20000, n_chains=128)
    assert got.index.equals(exact.index)
    assert float(np.max(np.abs(got.to_numpy() - exact.to_numpy()))) < 0.01


def test_config5_gibbs_full_size(amd):
    """BASELINE config 5 at FULL size: 1024 chains x 100 000 single-site updates (1.02e8 recorded states) on the 5x10
    K=8 grid, pooled estimate vs the exact posterior.  With 1e8 samples even an integrated autocorrelation time of
    1000 leaves a standard error of ~1.5e-3: the 5e-3 bound is > 3 sigma of that pessimistic case."""
    spec = netspec.grid_spec(5, 10, 8, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    rng = np.random.default_rng(1)
    ev = {f"{n:03d}": int(rng.integers(0, 8)) for n in (0, 9, 40, 49, 22)}
    exact = bn.query("025", event=ev)
    got = bn.query("025", event=ev, algorithm="gibbs", n_iterations=100_000, n_chains=1024)
    assert got.index.equals(exact.index)
    assert abs(got.sum() - 1.0) < 1e-12
    assert float(np.max(np.abs(got.to_numpy() - exact.to_numpy()))) < 5e-3


def test_async_submit_wait_matches_the_blocking_call(amd):
    """mibn_submit_batch / mibn_wait (two calls in flight) against mibn_query_batch, bit for bit, incl. the misuse
    errors: a third submit before a wait, a blocking call while tickets are open."""
    from sorobn_amd import _capi
    spec = netspec.grid_spec(10, 10, 4, seed=0)
    bn = netspec.build(spec, amd.BayesNet)
    eng = bn.backend.engine
    q, ev, ec = netspec.c3_requests(100, 4, 3 * 3000, 4, seed=7)
    to_var = np.array([bn.backend.flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    parts = [(to_var[q[k * 3000:(k + 1) * 3000]][:, None], to_var[ev[k * 3000:(k + 1) * 3000]], ec[k * 3000:(k + 1) * 3000])
             for k in range(3)]
    want = [eng.query_fixed(*p).copy() for p in parts]
    t0 = eng.total_stats()
    h0 = eng.submit_fixed(*parts[0])
    h1 = eng.submit_fixed(*parts[1])
    with pytest.raises(_capi.MibnError, match="already in flight"):
        eng.submit_fixed(*parts[2])
    with pytest.raises(_capi.MibnError, match="asynchronous calls in flight"):
        eng.query_fixed(*parts[2])
    got0 = eng.wait(h0).copy()
    h2 = eng.submit_fixed(*parts[2])
    got1 = eng.wait(h1).copy()
    got2 = eng.wait(h2).copy()
    eng.drain()
    for g, w in zip((got0, got1, got2), want):
        assert np.array_equal(g, w)
    t1 = eng.total_stats()
    assert t1["n_launches"] > t0["n_launches"] and t1["alg_bytes"] > t0["alg_bytes"] and t1["kernel_ms"] > t0["kernel_ms"]
    assert eng.query_fixed(*parts[0]).shape == (3000, 4)  # the blocking call works again once everything is collected


def test_engine_lifecycle(amd):
    """Three engines one after another in one process, each taking every path that creates a buffer, a pinned buffer, an event or a
    stream on first use - host-planned and device-planned query calls (wave planner and order_kernel + emit_kernel), two lanes, the
    trace events, an asynchronous call, MPE, posterior sampling, P(e), Gibbs, forward sampling, a data set - and closed twice: nothing
    raises, and every answer is bit for bit the first engine's."""
    from sorobn_amd import _capi
    spec = netspec.grid_spec(4, 4, 2)
    q, ev, ec = netspec.c3_requests(16, 2, 8, 3, seed=5)
    rows = np.random.default_rng(3).integers(0, 2, (100, 16)).astype(np.uint8)

    def run_all():
        bn = netspec.build(spec, amd.BayesNet)
        eng = bn.backend.engine
        to_var = np.array([bn.backend.flat.id[f"{i:03d}"] for i in range(16)], np.int32)
        req = (to_var[q][:, None], to_var[ev], ec)
        out = [eng.query_fixed(*req).copy()]  # (the small-network kernel: its staging buffer)
        eng.set_option("tiny", 0)
        out.append(eng.query_fixed(*req).copy())  # eight host-planned requests
        eng.set_option("second_on_device", 1)
        eng.set_option("gpu_emit", 2)
        for wave_plan in (1, 0):
            eng.set_option("wave_plan", wave_plan)
            out.append(eng.query_fixed(*req).copy())
        eng.set_option("wave_plan", 1)
        eng.set_option("streams", 2)
        out.append(eng.query_fixed(*req).copy())
        eng.set_option("streams", 1)
        eng.set_option("trace", 1)
        out.append(eng.query_fixed(*req).copy())
        eng.set_option("trace", 0)
        eng.set_option("gpu_emit", 0)
        out.append(eng.wait(eng.submit_fixed(*req)).copy())
        eng.drain()
        out.extend(eng.mpe(to_var[ev], ec))
        out.extend(eng.posterior_sample(to_var[ev], ec, 4, seed=11))
        out.append(eng.query_fixed(np.zeros((8, 0), np.int32), to_var[ev], ec, flags=_capi.Q_UNNORMALISED).copy())
        out.append(eng.gibbs(to_var[q[:1]], to_var[ev[0]], ec[0], 64, 10, seed=7))
        out.append(eng.sample(64, seed=9))
        ds = eng.dataset(rows, [2] * 16)
        out.append(ds.score_families([(0, 1), (1, 4, 5), (15,)]).copy())
        ds.close()
        eng.close()
        eng.close()
        return out

    first = run_all()
    for a in first[1:6]:  # every way of planning the eight requests gives the host-planned posteriors
        assert np.array_equal(a, first[1])
    for k in (1, 2):
        again = run_all()
        assert len(again) == len(first)
        for i, (a, b) in enumerate(zip(again, first)):
            assert a.dtype == b.dtype and np.array_equal(a, b), (k, i)


def test_engine_argument_errors(amd):
    from sorobn_amd import _capi
    spec = next(n for n in gu.load("examples.json") if n["spec"]["name"] == "asia")["spec"]
    bn = netspec.build(spec, amd.BayesNet)
    eng = bn.backend.engine
    with pytest.raises(_capi.MibnError, match="cannot be part of the event"):
        eng.query_fixed([[0]], [[0]], [[0]])
    with pytest.raises((IndexError, _capi.MibnError)):  # the binding sizes the result from card[q] before the call
        eng.query_fixed([[99]], [[0]], [[0]])
    with pytest.raises(_capi.MibnError, match="unknown evidence variable"):
        eng.query_fixed([[0]], [[99]], [[0]])
    with pytest.raises(_capi.MibnError, match="unknown option"):
        eng.set_option("no-such-option", 1)
    # a 5-column table of 8-state columns has 32768 cells > the 16384 of an LDS histogram: global-atomic path
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 8, (50_000, 5)).astype(np.uint8)
    big, small = eng.count_tables(codes, [8] * 5, [(0, 1, 2, 3, 4), (1, 3)])
    flat = np.ravel_multi_index(tuple(codes[:, c].astype(np.int64) for c in range(5)), (8,) * 5)
    assert np.array_equal(big.reshape(-1), np.bincount(flat, minlength=8 ** 5))
    assert np.array_equal(small, np.bincount(codes[:, 1].astype(np.int64) * 8 + codes[:, 3], minlength=64).reshape(8, 8))
    assert eng.query_fixed(np.zeros((0, 1), np.int32), np.zeros((0, 1), np.int32), np.zeros((0, 1), np.int32)).shape[0] == 0
