"""The step matrix on the CPU: tests/step_cases.py holds what it claims.  The planner's own programs of every pinned request, planned
as an engine with the case's options plans them (oracle/plan_sim.cpp plan_sim_program_kind), carry exactly the recorded edges; the
host twin tools/prog_sim.cpp runs the same programs with its own checks on; its answers agree with the dense numpy twins; and where a
case is not an exact-tie case the dense twin shows a strict winner, so that the device run of the same cases,
tests/test_step_classes.py, compares codes exactly and has no tie branch."""
import numpy as np
import pytest

import draw_check as dc
import golden_util as gu
import map_check as mp
import mpe_check as mc
import netspec
import sim_tools
import sorobn_amd
import step_cases as sc
from sorobn_amd.flatten import flatten

STRICT = 1e-9  # the project's margin of a strict winner: p1 - p2 > 1e-9 * p1 (mpe_check.check_against_brute, map_check.check)


@pytest.fixture(scope="module")
def prog_sim():
    return sim_tools.build_prog_sim()


@pytest.fixture(autouse=True)
def _product_defaults_afterwards():
    """The simulator's planner options are process-wide: every test here leaves the product's defaults behind."""
    yield
    sc.reset_sim_options()


def proved_edges(case, prog_sim, tmp_path):
    """Every tag of the case, from the planner's programs (step_cases.planned) and from the twins' numbers (tie, zero_mass and
    step_cases.NUMERIC_STEP_TAGS), with every assertion the module's docstring names made on the way."""
    spec = sc.build_spec(case)
    flat = flatten(netspec.build(spec, sorobn_amd.BayesNet))
    n = len(flat.card)
    small = np.prod([float(c) for c in flat.card]) <= sc.MAX_JOINT
    assert len(spec["nodes"]) == n == case["nodes"] and not flat.missing
    assert small or n >= 70, "a network too big for the dense twins is one of the 70-variable cases"
    assert set(case["options"]) <= set(sc.OPTION_NAMES)
    opt, kind, reqs = sc.options(case), case["kind"], case["requests"]
    assert len({rq.get("prune", 0) for rq in reqs}) == 1, "one prune flag per case: the device runs a case in one call"
    sc.set_sim_options(opt)
    edges = sc.planned(flat, kind, reqs)
    steps = [s for rq in reqs for s in sc.steps_of(flat, kind, rq)]
    if any(e.startswith("tile:") for e in edges):
        # (the device test asserts workgroups > launches on the level kernel: some tiled step has more than one workgroup)
        assert any(s["tiled"] and -(-s["hi"] // s["tile_h"]) >= 2 for s in steps), "every tiled step is a single workgroup"
    wide = {("tile" if s["tiled"] else "seg") for s in steps if s["max"] and s["cx"] > 255}
    evs = [sc.evidence(flat, rq) for rq in reqs]
    is_tie = "tie" in case["edges"]
    on_path, largest_code = 0, -1

    def against(lp, codes, p1, p2, best, ctx):
        """One answer of prog_sim against a dense twin's (best, runner-up, argmax); -> whether the mass is zero."""
        if p1 <= 0:
            assert lp == -np.inf and all(int(c) == -1 for c in codes), ctx
            return True
        assert abs(lp - np.log(p1)) <= 1e-12, (ctx, lp, np.log(p1))
        if not is_tie:
            assert p1 - p2 > STRICT * p1, (ctx, "no strict winner", p1, p2)
            assert [int(c) for c in codes] == [int(c) for c in best], (ctx, list(codes), list(best))
        return False

    if kind == "max":
        lp, codes, ties = mc.run_max_sim(prog_sim, tmp_path, flat, [(list(ev), list(ev.values())) for ev in evs], options=opt, ties=True)
        on_path = sum(t[2] for t in ties)
        for rq, ev, l, c in zip(reqs, evs, lp, codes):
            free = [v for v in range(n) if v not in ev]
            assert all(c[v] == x for v, x in ev.items())
            if small:
                lp_star, best, p1, p2 = mc.brute(flat, ev)
                if against(float(l), c[free], p1, p2, best[free], (case["name"], rq)):
                    edges.add("zero_mass")
                elif is_tie:  # of the assignments that attain the maximum exactly, the twin's is the one the lowest-x rule decodes
                    vs, joint = mc._mul(mc._sliced(flat, ev))
                    want = sc.first_maximiser(np.asarray(joint), vs, sc.traceback_order(flat, kind, rq))
                    assert {v: int(c[v]) for v in vs} == want, (case["name"], "not the lowest maximising x", c, want)
            else:
                assert abs(float(l) - mc.ve_max(flat, ev, sc.ids(flat, sorted(int(x) for x in spec["nodes"])))) <= 1e-12, case["name"]
                assert abs(mc.log_joint(flat, c) - float(l)) <= 1e-12, case["name"]
            largest_code = max(largest_code, int(np.max(c[free], initial=-1)))
    elif kind == "map":
        for prune in (0, 1):
            rows = [(not prune, sc.ids(flat, rq["M"]), list(ev), list(ev.values())) for rq, ev in zip(reqs, evs)]
            lp, codes, ties = mp.run_map_sim(prog_sim, tmp_path, flat, rows, options=opt, ties=True)
            if all(prune == rq["prune"] for rq in reqs):
                on_path = sum(t[2] for t in ties)
            for rq, ev, row, l, c in zip(reqs, evs, rows, lp, codes):
                if small:
                    p1, p2, best, table, axes = mp.brute(flat, row[1], ev, prune=bool(prune))
                    if against(float(l), c, p1, p2, best, (case["name"], rq, prune)):
                        edges.add("zero_mass")
                    elif is_tie:
                        want = sc.first_maximiser(table, axes, sc.traceback_order(flat, kind, dict(rq, prune=prune)))
                        assert dict(zip(row[1], (int(x) for x in c))) == want, (case["name"], "not the lowest maximising x", c, want)
                else:  # M is every free variable: the answer is the most probable explanation
                    full = np.zeros(n, np.int64)
                    full[row[1]] = c
                    full[list(ev)] = list(ev.values())
                    assert sorted(row[1] + list(ev)) == list(range(n)), "M is every free variable"
                    assert abs(float(l) - mc.ve_max(flat, ev, sc.ids(flat, sorted(int(x) for x in spec["nodes"])))) <= 1e-12, case["name"]
                    assert abs(mc.log_joint(flat, full) - float(l)) <= 1e-12, case["name"]
                    _, mpe_codes = mc.run_max_sim(prog_sim, tmp_path, flat, [(list(ev), list(ev.values()))], options=opt)
                    assert np.array_equal(mpe_codes[0], full), case["name"]
                largest_code = max(largest_code, max([int(x) for x in c], default=-1))
    else:
        rows, g = [], 0
        for rq, ev in zip(reqs, evs):
            rows.append((list(ev), list(ev.values()), rq["n"], g))
            g += rq["n"]
        res = dc.run_draw_sim(prog_sim, tmp_path, flat, case["seed"], reqs[0].get("prune", 0), rows, options=opt)
        for rq, ev, r in zip(reqs, evs, res):
            vs, post, mass = dc.dense_posterior(flat, ev)
            if mass <= 0:
                assert r["p_e"] == 0.0 and all((r["codes"][:, v] == -1).all() for v in range(n) if v not in ev), case["name"]
                edges.add("zero_mass")
                continue
            assert abs(r["p_e"] - mass) <= 1e-12 * mass, (case["name"], r["p_e"], mass)
            assert not r["low"] and r["min_margin"] > 1e-12, (case["name"], "a draw within 1e-12 of a boundary", r["low"])
            assert (post[tuple(r["codes"][:, v] for v in vs)] > 0).all(), (case["name"], "a row of probability zero")
            assert all((r["codes"][:, v] == x).all() for v, x in ev.items())
    if is_tie:
        assert on_path >= 1, "no traceback of an exact-tie case reads a cell whose maximum two values of x attain"
        edges.add("tie")
    if largest_code > 255:  # (only the variable a wide MAX step eliminates has such codes in the table's networks)
        edges |= {f"{p}:argmax_gt_255" for p in wide}
    return edges


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_case_holds_its_edges_and_the_twins_agree(case, prog_sim, tmp_path):
    edges = proved_edges(case, prog_sim, tmp_path)
    assert sorted(edges) == case["edges"], sorted(edges ^ set(case["edges"]))


def test_the_table_covers_every_edge_or_says_why_not():
    """REQUIRED is met, IMPOSSIBLE is disjoint from what the table shows, and between them the two name every (kind, path, tag)
    combination and every case-level tag of every kind: nothing is silently dropped."""
    assert len({c["name"] for c in sc.CASES}) == len(sc.CASES)
    for kind in sc.KINDS:
        seen = set().union(*[set(c["edges"]) for c in sc.CASES if c["kind"] == kind])
        everything = {f"{p}:{t}" for p in sc.PATHS for t in sc.STEP_TAGS + sc.PATH_TAGS[p] + sc.NUMERIC_STEP_TAGS} | set(sc.CASE_TAGS)
        assert seen <= everything, sorted(seen - everything)
        assert set(sc.REQUIRED[kind]) <= seen, (kind, sorted(set(sc.REQUIRED[kind]) - seen))
        assert not set(sc.IMPOSSIBLE[kind]) & seen, (kind, sorted(set(sc.IMPOSSIBLE[kind]) & seen))
        assert all(why for why in sc.IMPOSSIBLE[kind].values())
        assert set(sc.REQUIRED[kind]) | set(sc.IMPOSSIBLE[kind]) == everything, (kind, sorted(everything ^ (set(sc.REQUIRED[kind]) | set(sc.IMPOSSIBLE[kind]))))
        assert not set(sc.REQUIRED[kind]) & set(sc.IMPOSSIBLE[kind])
    # every case the device test holds to "workgroups > launches" on the tile path names that path
    assert all(isinstance(c["edges"], list) and c["edges"] == sorted(c["edges"]) for c in sc.CASES)


def test_census_of_n_in_on_the_golden_inputs():
    """Which generic_call<NIN> bodies the three kinds reach on the networks the existing device tests of MPE, MAP and posterior
    sampling run (examples.json, random_dags.json; the engine's defaults), as (kind, path, n_in): printed, and every one of them is
    in the table - the table's cases are what pins each of them to a reference."""
    sc.set_sim_options(sc.DEFAULTS)
    rng = np.random.default_rng(3)
    census = set()
    for fname in ("examples.json", "random_dags.json"):
        for entry in gu.load(fname):
            flat = flatten(netspec.build(entry["spec"], sorobn_amd.BayesNet))
            n = len(flat.card)
            if flat.missing or np.prod([float(c) for c in flat.card]) > sc.MAX_JOINT:
                continue
            import dump_plan as dp
            for k in range(3):
                evn = [] if k == 0 else sorted(rng.choice(n, size=int(rng.integers(1, max(2, n // 2) + 1)), replace=False).tolist())
                ec = [int(rng.integers(0, flat.card[v])) for v in evn]
                free = [v for v in range(n) if v not in evn]
                for kind, q in (("max", []), ("draw", []), ("map", free[:max(1, len(free) // 2)])):
                    w, th = dp.program_kind(flat, kind, q, evn, ec, no_prune=kind != "max")
                    census |= {(kind, "tile" if t else "seg", min(max(s["n_in"], 1), 6)) for s, t in zip(dp.decode(w), th)}
    print(sorted(census))
    table = {(c["kind"], e.split(":")[0], int(e[-1])) for c in sc.CASES for e in c["edges"] if ":n_in" in e}
    assert {k for k, _, _ in census} == set(sc.KINDS)
    assert census <= table, sorted(census - table)
    assert table == {(k, p, i) for k in sc.KINDS for p in sc.PATHS for i in range(1, 7)}


def test_the_twin_plans_with_the_engines_own_settings():
    """sim_tools.ENGINE_PLANNING repeats what mibn_create gives an engine's Network beyond a bare one: read back from the sources,
    so that a retuned default shows here and not as a twin whose program is no longer the engine's."""
    import os
    import re
    csrc = os.path.join(sc.ROOT, "sorobn_amd", "csrc")
    policy = open(os.path.join(csrc, "plan_policy.h")).read()
    engine = open(os.path.join(csrc, "engine.hip")).read()
    assert float(re.search(r"double base_minfill = ([0-9.e+]+)", policy).group(1)) == sim_tools.ENGINE_PLANNING["minfill_above"]
    assert float(re.search(r"double base_second_above = ([0-9.e+]+)", policy).group(1)) == sim_tools.ENGINE_PLANNING["second_above"]
    efforts = set(re.findall(r"h->net\.order_effort = (\d+); h->net\.second_above = h->pol\.base_second_above;", engine))
    assert efforts == {str(sim_tools.ENGINE_PLANNING["order_effort"])}, efforts
    assert "h->net.minfill_above = h->pol.base_minfill;" in engine
