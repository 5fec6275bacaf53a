"""The class matrix on the CPU: tests/class_cases.py holds what it claims.  The planner's own kernel_id_of_step / step_is_tiled /
kernel_name (oracle/plan_sim.cpp plan_sim_step_classes) name the class of every step of every pinned request; the simulator
executes the same programs against the C oracle.  The device run of the same cases is tests/test_kernel_classes.py."""
import os
import sys

import numpy as np
import pytest

import class_cases as cc
import golden_util as gu
import netspec
import simengine
import sorobn_amd
from sorobn_amd.flatten import flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dump_plan as dp  # noqa: E402


@pytest.fixture(autouse=True)
def _product_defaults_afterwards():
    """The simulator's planner options are process-wide: every test here leaves the product's defaults behind."""
    yield
    cc.reset_sim_options()


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_case_holds_its_classes_and_edges_and_matches_the_oracle(case):
    from oracle.oracle import OracleNet
    spec = cc.build_spec(case)
    max_nodes, max_cells = cc.size_cap(case)
    assert len(spec["nodes"]) == case["nodes"] <= max_nodes
    flat = flatten(netspec.build(spec, sorobn_amd.BayesNet))
    opt = cc.options(case)
    assert set(case["options"]) <= set(cc.OPTION_NAMES)
    cc.set_sim_options(opt)
    classes, edges, cells = cc.planned(flat, case["requests"])
    assert sorted(classes) == case["classes"], sorted(classes ^ set(case["classes"]))
    assert sorted(edges) == case["edges"], sorted(edges ^ set(case["edges"]))
    assert cells == case["max_cells"] <= max_cells
    # the same programs, executed: every request, every cell, work item by work item of the schedule
    eng = simengine.SimEngine(flat, opt["small_cells"], (opt["big_iters"], opt["tile_h"]), opt["fuse"])
    for name in ("chain", "sweep", "sweep_min", "outer", "sweep_iters", "sweep_canon"):
        eng.set_option(name, opt[name])
    eng.set_option("sweep_adapt", cc.MATRIX_SWEEP_ADAPT)
    on = OracleNet(spec)
    worst = 0.0
    for q, ev, ec in case["requests"]:
        got = eng._one(cc.flat_ids(flat, [q]), cc.flat_ids(flat, ev), np.asarray(ec, np.int32))
        want = cc.oracle_dense(on, len(got), q, ev, ec)
        assert abs(want.sum() - 1.0) < 1e-9, (q, ev, ec)  # (a request of the table has evidence of positive probability)
        worst = max(worst, float(np.max(np.abs(got - want))))
    assert worst <= gu.TOL, worst


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_level_groups_partition_the_launches_by_route(case):
    """planner.h level_groups - the rule by which the engine turns the Launch entries of a schedule into kernel launches - on the
    schedule of every case, under all 16 settings of the options that route a class to a kernel."""
    flat = flatten(netspec.build(cc.build_spec(case), sorobn_amd.BayesNet))
    cc.set_sim_options(cc.options(case))
    for routing in range(16):
        split, seg_kernel, mfma_kernel, sweep_dma = [bool(routing >> k & 1) for k in range(4)]
        launches, groups = cc.level_groups(flat, case["requests"], routing)
        assert {la["cls"] for la in launches} == set(case["classes"])
        # every class goes where the options send it (the tests' notion of the MFMA1 classes is the planner's)
        for la in launches:
            want = ("sweep_dma" if sweep_dma else "sweep_reg") if la["cls"] == cc.SWEEP else "level" if split else \
                "segment" if seg_kernel and la["cls"] == cc.SEGMENTS else "mfma" if mfma_kernel and la["cls"] in cc.MFMA1 else "level"
            assert la["route"] == want, (routing, la)
        # the groups partition the launches in order
        assert [g["first_launch"] for g in groups] == [0] + list(np.cumsum([g["n_launches"] for g in groups])[:-1])
        assert sum(g["n_launches"] for g in groups) == len(launches) and all(g["n_launches"] >= 1 for g in groups)
        for g in groups:
            mine = launches[g["first_launch"]:g["first_launch"] + g["n_launches"]]
            assert all(la["route"] == g["route"] and la["level"] == g["level"] for la in mine), (routing, g)
            assert g["grid"] == sum(la["grid"] for la in mine)
            assert g["alg_bytes"] == sum(la["alg_bytes"] for la in mine)  # (added in the same order: the same double)
            assert (g["wg_level"], g["wg_first"]) == (mine[0]["wg_level"], mine[0]["wg_first"])
            assert g["stat_cls"] == (mine[0]["cls"] if split else None)
        if split:
            assert len(groups) == len(launches)
        else:  # contiguity: a level has at most one launch of a kernel
            keys = [(g["level"], g["route"]) for g in groups]
            assert len(set(keys)) == len(keys), (routing, keys)


def test_the_routing_cases_reach_every_kernel_of_a_level():
    """cc.ROUTING_CASES (the device test test_level_routing_table runs them under every option setting): segments, a level-kernel
    class, an MFMA1 class and SWEEP between them, and no smaller pair of the table does."""
    def reach(case):
        return {"segment": cc.SEGMENTS in case["classes"], "mfma": bool(set(cc.MFMA1) & set(case["classes"])), "sweep": cc.SWEEP in case["classes"],
                "level": bool(set(case["classes"]) - {cc.SEGMENTS, cc.SWEEP, *cc.MFMA1})}
    by_name = {c["name"]: c for c in cc.CASES}
    pair = [by_name[n] for n in cc.ROUTING_CASES]
    assert all(any(reach(c)[k] for c in pair) for k in ("segment", "mfma", "sweep", "level"))
    size = lambda cs: (sum(c["nodes"] for c in cs), sum(c["max_cells"] for c in cs))
    for c in cc.CASES:  # (no single case of the small table does; the ones of the sweep matrix that do are larger than the pair)
        if all(reach(c).values()):
            assert cc.in_sweep_matrix(c) and size(pair) <= size([c]), c["name"]
    for i, a in enumerate(cc.CASES):
        for b in cc.CASES[i + 1:]:
            if all(reach(a)[k] or reach(b)[k] for k in ("segment", "mfma", "sweep", "level")):
                assert size(pair) <= size([a, b]), (a["name"], b["name"])
    # and the schedule says the same: under the engine's defaults the pair's launch groups go to all four kernels
    routes = set()
    for case in pair:
        flat = flatten(netspec.build(cc.build_spec(case), sorobn_amd.BayesNet))
        cc.set_sim_options(cc.options(case))
        routes |= {g["route"] for g in cc.level_groups(flat, case["requests"], cc.ROUTING_DEFAULT)[1]}
    assert routes == {"level", "sweep_dma", "segment", "mfma"}, routes


def test_the_table_covers_every_class_the_planner_can_emit():
    """All names of kernel_name() minus the ones proved unreachable: a class added to emit_core.h fails here until it has a case, and
    so does a case removed from the table if it was the only one of a class."""
    names = dp.class_names()
    assert len(names) == len(set(names)) == 44
    unreachable = [n for n, _ in cc.UNREACHABLE if n is not None]
    assert set(unreachable) <= set(names) and len(set(unreachable)) == len(unreachable)
    assert all(why for _, why in cc.UNREACHABLE)
    have = set().union(*[set(c["classes"]) for c in cc.CASES])
    assert have == set(names) - set(unreachable), sorted(have ^ (set(names) - set(unreachable)))
    assert len({c["name"] for c in cc.CASES}) == len(cc.CASES)


def test_the_table_covers_every_edge_in_every_family_where_it_can_occur():
    have = set().union(*[set(c["edges"]) for c in cc.CASES])
    want = {f"{fam}:{e}" for fam, es in cc.REQUIRED_EDGES.items() for e in es} | set(cc.REQUIRED_ROW_STRIDES)
    assert want <= have, sorted(want - have)
    for c in cc.MFMA1:  # both classes of ve_mfma_kernel at all three row strides
        assert {f"{c}:rs{r}" for r in (1, 4, 16)} <= set(cc.REQUIRED_ROW_STRIDES)
    # (every family of tiled FIBER classes is in REQUIRED_EDGES, and what it lacks there is accounted for in IMPOSSIBLE_EDGES)
    fams = {cc.family(n) for n in dp.class_names()} - {"segments"}
    assert fams == set(cc.REQUIRED_EDGES), fams ^ set(cc.REQUIRED_EDGES)
    for fam in fams - {"generic", "sweep"}:
        assert set(cc.REQUIRED_EDGES[fam]) | set(cc.IMPOSSIBLE_EDGES.get(fam, {})) == set(cc.FIBER_EDGES), fam
    # the sweep matrix: every tag of sweep_edges is required or accounted for, and nothing is both
    assert set(cc.REQUIRED_EDGES["sweep"]) | set(cc.IMPOSSIBLE_EDGES["sweep"]) == set(cc.SWEEP_EDGES)
    assert not set(cc.REQUIRED_EDGES["sweep"]) & set(cc.IMPOSSIBLE_EDGES["sweep"]) and all(cc.IMPOSSIBLE_EDGES["sweep"].values())
    assert len(cc.REQUIRED_EDGES["sweep"]) == len(set(cc.REQUIRED_EDGES["sweep"])) == 50 and len(set(cc.SWEEP_EDGES)) == 57
    assert not {e for e in have if e.startswith("sweep:")} - {f"sweep:{e}" for e in cc.SWEEP_EDGES}  # (no tag outside the list)
    # k2 and k3 name the pass length AND the canonical specialisations <2,false> / <3,false>: a witness of each that is not on the general path
    for k in ("sweep:k2", "sweep:k3"):
        assert any(k in c["edges"] and "sweep:any" not in c["edges"] for c in cc.CASES), k
    # each wave-owned tail with a last work item shorter than the others, with work items of one tile and with several tiles per item
    for t in cc.SWEEP_TAILS:
        assert {f"sweep:{t}+{e}" for e in ("partial_tile", "one_tile_item", "multi_tile", "items2+")} <= have, t
    assert sum(cc.in_sweep_matrix(c) for c in cc.CASES) == 18


def test_the_c3_census_of_sweep_shapes():
    """The sweep shapes the flagship workload runs - the first 300 requests of the C3 stream under the engine's defaults (order_effort 1,
    second_above 2e7, eight tiles per work item) - are all in the sweep matrix: a shape the workload runs and the table lacks fails
    here.  And why the matrix is the only place the ragged shapes of the tile loop run: every SWEEP step of C3 has 8, 32 or 128 tiles,
    whole work items at sweep_iters = 8 and at the 4 and 2 that build_schedule's sweep_adapt may halve it to - no work item of one
    tile, no shorter last one."""
    cc.set_sim_options(cc.DEFAULTS, cc.PRODUCT_SWEEP_ADAPT)
    simengine.lib().plan_sim_set_order_effort(1, 2e7)
    steps = cc.c3_sweep_steps(300)
    assert len(steps) > 500 and {s["cls"] for s in steps} == {cc.SWEEP} and {s["tile_h"] for s in steps} == {8}
    census = {}
    for s in steps:
        for e in cc.sweep_edges(s):
            census[e] = census.get(e, 0) + 1
    for e in sorted(census):
        print(f"  {e:28s} {census[e]:4d} steps")
    table = {e for c in cc.CASES for e in c["edges"] if e.startswith("sweep:")}
    print("C3 never runs:", sorted(table - set(census)))
    assert set(census) <= table, sorted(set(census) - table)
    assert not [e for e in census if "partial_tile" in e or "one_tile_item" in e or "one_tile_step" in e or "odd_tiles" in e]
    assert {s["hi"] for s in steps} <= {8, 32, 128}  # (so a halved work item - 4 or 2 tiles - divides the step too)


def _census_of(flat, reqs):
    """Classes of the programs of (query ids, evidence ids) pairs - the evidence codes do not change a program's shapes."""
    seen = set()
    for q, ev in sorted(set(reqs)):
        seen.update(dp.step_classes(dp.program(flat, np.array(q, np.int32), np.array(ev, np.int32), np.zeros(len(ev), np.int32))))
    return seen


def _golden_requests(bn, requests):
    be = simengine.sim_backend(bn)
    out = []
    for r in requests:
        try:
            q, ev, ec = be.encode(tuple(r["query"]), {k: v for k, v in r["event"]})
        except KeyError:
            continue  # (a name the network does not have: the reference's KeyError, nothing is planned)
        if all(0 <= c < be.flat.card[v] for v, c in zip(ev, ec)):  # (a label outside the domain: empty answer, nothing is planned)
            out.append((tuple(q), tuple(ev)))
    return be.flat, out


def test_census_of_the_golden_gpu_inputs():
    """What the golden GPU tests put on the device, by class, under the engine's defaults (order_effort 1, second_above 2e7): the
    files and option sets of test_golden_networks, test_golden_huge_cardinalities and test_golden_small_grids and the first 300
    requests of the C3 stream.  Printed; every reachable class the census lacks is in the table, and the classes of the
    huge-cardinality networks are the sets test_golden_huge_cardinalities asserts on the device."""
    L = simengine.lib()
    forcing = [(1024, (4096, 0), 1), (1, (2, 1), 1), (6, (8, 3), 1), (1, (2, 1), 0)]
    census = {}

    def run(label, nets, option_sets):
        for small_cells, tiling, fuse in option_sets:
            cc.set_sim_options(dict(cc.DEFAULTS, small_cells=small_cells, big_iters=tiling[0], tile_h=tiling[1], fuse=fuse))
            L.plan_sim_set_order_effort(1, 2e7)
            seen = set()
            for spec, requests in nets:
                flat, reqs = _golden_requests(netspec.build(spec, sorobn_amd.BayesNet), requests)
                seen |= _census_of(flat, reqs)
            census[(label, small_cells, tiling, fuse)] = seen

    for fname in ("examples.json", "random_dags.json", "wide_cards.json", "many_nodes.json"):
        run(fname, [(n["spec"], n["requests"]) for n in gu.load(fname)], forcing)
    run("huge_cards.json", [(gu.dag_spec_from_recipe(e), e["requests"]) for e in gu.load("huge_cards.json")], forcing)
    run("grids_small.json", [(gu.grid_spec_from_recipe(e), e["requests"]) for e in gu.load("grids_small.json")],
        [(1024, (4096, 0), 1), (3, (4, 1), 1), (20, (64, 2), 1), (3, (4, 1), 0)])
    cc.set_sim_options(cc.DEFAULTS)
    L.plan_sim_set_order_effort(1, 2e7)
    flat = flatten(netspec.build(netspec.grid_spec(10, 10, 4, seed=0), sorobn_amd.BayesNet))
    to_var = np.array([flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    q, ev, ec = netspec.c3_requests(100, 4, 300, 4, seed=1)
    census[("C3 first 300", 1024, (4096, 0), 1)] = _census_of(flat, [((int(to_var[q[i]]),), tuple(int(v) for v in to_var[ev[i]])) for i in range(300)])
    for key, seen in census.items():
        print(key, sorted(seen))
    everything = set().union(*census.values())
    names = set(dp.class_names())
    reachable = names - {n for n, _ in cc.UNREACHABLE if n is not None}
    lacking = reachable - everything
    print("the golden inputs never emit:", sorted(lacking))
    table = set().union(*[set(c["classes"]) for c in cc.CASES])
    assert lacking <= table, sorted(lacking - table)
    assert everything <= reachable, sorted(everything - reachable)  # (a class on the unreachable list that IS emitted would show here)
    for (label, small_cells, tiling, fuse), seen in census.items():
        if label == "huge_cards.json":
            assert sorted(seen) == cc.HUGE_CARDS_CLASSES[(small_cells, tiling, fuse)], (small_cells, tiling, fuse, sorted(seen))
