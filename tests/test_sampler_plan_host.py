"""The host side of the sampling family (sorobn_amd/csrc/sampler_plan.h: gibbs_plan, sample_plan and the two LDS layout functions the
kernels share with them) on a CPU: tools/sampler_plan_sim.cpp includes the header gibbs_run and sample_run include and prints what a call
would launch.  Expected forms, sizes and words are worked out here from the rules in the header's comments - none is copied from the tool."""
import itertools
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import gibbs_cases as gc
import sample_check as sc
import sim_tools

ROOT = sim_tools.ROOT
E_ARG, E_LIMIT = -1, -6
KIB = 1024
GIBBS_TOO_LARGE = "gibbs: network/query too large for the LDS-resident chain state"
SAMPLING_TOO_LARGE = "sampling: network/query too large for the LDS-resident state"
SAMPLE, REJECTION, LIKELIHOOD, PROBE = 0, 1, 2, 3

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def a16(x):
    return (x + 15) // 16 * 16


def _prefix(net):
    card, scope_off, scope_vars, value_off, values = net.engine_args()
    return sim_tools.network_prefix(types.SimpleNamespace(card=card.tolist(), scope_off=scope_off.tolist(), scope_vars=scope_vars.tolist(),
                                                          value_off=value_off.tolist(), values=values))


def _parse(line):
    if line.startswith("error="):
        code, msg = line.split(" ", 1)
        return {"error": int(code[6:]), "msg": msg[4:]}
    out = {}
    for kv in line.split():
        k, v = kv.split("=")
        out[k] = v if k == "form" else [int(x) for x in v.split(",") if x] if k in ("vars", "pack") else int(v)
    return out


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sampler") / "sampler_plan_sim")
    r = subprocess.run(["g++", "-O2", "-mpopcnt", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "sampler_plan_sim.cpp"),
                        os.path.join(ROOT, "sorobn_amd", "csrc", "planner.cpp"), "-lpthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(net, lines):
        """net: a sample_check.Net or the prefix lines themselves -> one dict per command line"""
        prefix = net if isinstance(net, list) else _prefix(net)
        out = subprocess.run([exe], input="\n".join(prefix + list(lines)) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        res = [_parse(ln) for ln in out.stdout.splitlines()]
        assert len(res) == len(lines)
        return res
    return run


def gibbs_line(mode, chains, q, ev=None, cycle=None, cond=-1):
    ev = dict(ev or {})
    words = [mode, chains, cond, len(q), *q, len(ev), *ev, *ev.values()] + ([-1] if cycle is None else [len(cycle), *cycle])
    return "gibbs " + " ".join(map(str, words))


def sample_line(mode, n_samples, q=(), clamp=None, ev=None, cdf_stride=0):
    clamp, ev = dict(clamp or {}), dict(ev or {})
    words = [mode, n_samples, cdf_stride, len(q), *q, len(clamp), *clamp, *clamp.values(), len(ev), *ev, *ev.values()]
    return "sample " + " ".join(map(str, words))


# ---------------------------------------------------------------------------------------------- the GPU cases and their forms

GPU_CHAIN_COUNTS = (1, 8, 9, 61, 65)  # test_gibbs_chain_counts, and the sizes of gibbs_cases.SIZES among them


@pytest.fixture(scope="module")
def case_plans(sim):
    """{(case, gibbs_lds, chains | "cond"): plan} of every launch tests/test_sampling_twin.py makes of gibbs_cases.GIBBS_CASES"""
    plans = {}
    for name, (make, q, ev, cycle, _, sizes) in gc.GIBBS_CASES.items():
        net = make()
        cyc = gc.cycle_of(net, ev, cycle)
        chains = sorted({c for c, _ in sizes} | (set(GPU_CHAIN_COUNTS) if name == "grid3x3k8" else set()))
        keys = [(name, mode, c) for mode in gc.LDS_MODES for c in chains] + [(name, mode, "cond") for mode in gc.LDS_MODES]
        lines = [gibbs_line(mode, gc.CONDITIONAL_ROWS, [q[0]], ev, cyc, cond=q[0]) if c == "cond" else gibbs_line(mode, c, q, ev, cyc) for _, mode, c in keys]
        plans.update(zip(keys, sim(net, lines)))
    return plans


def test_every_gpu_case_takes_the_form_its_table_names(case_plans):
    for (name, mode, chains), plan in case_plans.items():
        assert plan["form"] == gc.GIBBS_CASES[name][4][mode], (name, mode, chains)
    assert {len(c[5]) for c in gc.GIBBS_CASES.values()} == {2}


def test_every_form_is_reached_drawing_and_conditional(case_plans):
    reached = {(plan["form"], chains == "cond") for (_, _, chains), plan in case_plans.items()}
    assert reached == set(itertools.product(gc.FORMS, (False, True)))


def test_grid_and_blocks_of_the_gpu_cases(case_plans):
    for (name, mode, chains), plan in case_plans.items():
        n = gc.CONDITIONAL_ROWS if chains == "cond" else chains
        assert plan["blocks"] == ((n + 7) // 8 if plan["form"] == "Fast8" else (n + 63) // 64), (name, mode, chains)


# ------------------------------------------------------------------------------------------------------------- packed words

def _programs(net, cycle, q, fast):
    """The update programs as sampler_plan.h describes them.  Generic: card, n_factors, then per factor (the variable's own CPT, then
    its children's in ascending id) table offset, stride of v, n_other, (other variable, stride)*.  FAST: v, card, n_factors, is-query,
    then four slots of (table offset, stride of v, other 0, its stride, other 1, its stride); an unused slot = (pool cells, 0 x 5)."""
    words, offs = [], []
    for v in cycle:
        offs.append(len(words))
        factors = [v] + net.children[v]
        words += [v, int(net.card[v]), len(factors), int(v in q)] if fast else [int(net.card[v]), len(factors)]
        for c in factors:
            sv = net.stride[c][net.scope[c].index(v)]
            others = [(u, s) for u, s in zip(net.scope[c], net.stride[c]) if u != v]
            flat = [x for pair in others for x in pair]
            words += [int(net.value_off[c]), sv] + (flat + [0] * (4 - len(flat)) if fast else [len(others)] + flat)
        if fast:
            words += [len(net.values), 0, 0, 0, 0, 0] * (4 - len(factors))
    return words, offs


@pytest.mark.parametrize("name", ["grid4x5k3", "dag-reverse-cycle", "tree-17-255", "asia-five-queries-evidence"])
def test_packed_words(case_plans, name):
    make, q, ev, cycle, _, sizes = gc.GIBBS_CASES[name]
    net = make()
    V = len(net.card)
    cyc = gc.cycle_of(net, ev, cycle) or [v for v in range(V) if v not in ev]
    qstride = [int(np.prod([net.card[u] for u in q[i + 1:]], dtype=np.int64)) for i in range(len(q))]
    _, generic_offs = _programs(net, cyc, q, False)
    for mode in gc.LDS_MODES:
        p = case_plans[name, mode, sizes[0][0]]
        fast = p["form"] in ("Fast", "Fast8")
        prog, _ = _programs(net, cyc, q, fast)
        pack = p["pack"]
        part = lambda key, n: pack[p[key]:p[key] + n]
        n_scope = sum(len(s) for s in net.scope)
        assert part("o_sv", n_scope) == [u for s in net.scope for u in s] and part("o_ss", n_scope) == [x for s in net.stride for x in s]
        assert part("o_ch", n_scope - V) == [c for ch in net.children for c in ch]
        assert part("o_cy", len(cyc)) == cyc and part("o_q", len(q)) == q and part("o_qs", len(q)) == qstride
        assert part("o_up", len(prog)) == prog and p["uprog_words"] == len(prog) and part("o_uo", len(cyc)) == generic_offs
        assert p["prog_words"] == (0 if p["form"] in ("L2", "PoolLds") else len(prog) if fast else len(prog) + 2 * len(cyc))
        assert len(pack) == 2 * n_scope + (n_scope - V) + 2 * len(cyc) + 2 * len(q) + len(prog)
        want_vars, sb, cb = [], 0, 0
        for v in range(V):
            want_vars += [int(net.card[v]), int(net.value_off[v]), sb, len(net.scope[v]), cb, len(net.children[v]), int(v in ev), ev.get(v, 0)]
            sb, cb = sb + len(net.scope[v]), cb + len(net.children[v])
        assert p["vars"] == want_vars
        assert (p["n_cycle"], p["hist_cells"], p["pool_cells"]) == (len(cyc), qstride[0] * int(net.card[q[0]]), len(net.values))


def test_conditional_position(sim):
    net = gc.grid_net(3, 3, 2, 53)
    cyc = [8, 7, 6, 4, 3, 2, 1, 0]
    a, b, c = sim(net, [gibbs_line(1, 70, [6], {5: 1}, cyc, cond=6), gibbs_line(1, 70, [0], {5: 1}, None, cond=0), gibbs_line(1, 70, [7], {5: 1}, None, cond=7)])
    assert (a["cond_pos"], b["cond_pos"], c["cond_pos"]) == (2, 0, 6)


# ------------------------------------------------------------------------------------------------------------------- layout

def _old_gibbs_total(n, cells, pool, fast, prog):
    """The sums of the driver this header replaced, restated: state + histogram; the tables behind them, 16-byte aligned; FAST: 8 bytes
    more; the programs behind that, 16-byte aligned."""
    lds = a16(n * 64) + cells * 4
    if pool:
        lds = a16(lds) + pool * 8
    if fast:
        lds += 8
    if prog:
        lds = a16(lds) + prog * 4
    return lds


def test_gibbs_layout_over_a_grid_of_sizes(sim):
    grid = [(n, cells, pool, fast, prog) for n in (1, 3, 50, 1024) for cells in (1, 2, 3, 255, 4913, 38400) for pool in (0, 1, 7, 469, 7938, 20000)
            for fast in (0, 1) for prog in (0, 1, 28, 1001, 28 * 1024) if not fast or (pool and prog)]
    trivial = sc.make_net([2], [[]], [np.array([0.5, 0.5])])
    res = sim(trivial, [f"glayout {n} {cells} {pool} {fast} {prog}" for n, cells, pool, fast, prog in grid])
    for (n, cells, pool, fast, prog), L in zip(grid, res):
        ctx = (n, cells, pool, fast, prog)
        assert L["total"] == _old_gibbs_total(n, cells, pool, fast, prog), ctx
        assert L["hist"] % 16 == 0 and L["pool"] % 16 == 0 and L["prog"] % (16 if fast else 8) == 0, ctx  # (u32, f64, four-word / one-word reads)
        assert n * 64 <= L["hist"] and L["hist"] + cells * 4 <= L["pool"], ctx
        assert L["hist"] + cells * 4 <= L["total"], ctx
        if pool:  # (an empty region has a start and needs no room)
            assert L["pool"] + (pool + fast) * 8 <= min(L["prog"], L["total"]), ctx
        if prog:
            assert L["pool"] <= L["prog"] and L["prog"] + prog * 4 <= L["total"], ctx


def test_sample_layout_over_a_grid_of_sizes(sim):
    grid = [(n, cells) for n in (1, 3, 50, 1024) for cells in (0, 1, 2, 255, 4913, 12768, 12800)]
    trivial = sc.make_net([2], [[]], [np.array([0.5, 0.5])])
    for (n, cells), L in zip(grid, sim(trivial, [f"slayout {n} {cells}" for n, cells in grid])):
        assert L["total"] == a16(n * 64) + cells * 12, (n, cells)  # the old driver's sum
        assert L["hsum"] % 16 == 0 and L["hcnt"] % 4 == 0 and n * 64 <= L["hsum"] and L["hsum"] + cells * 8 <= L["hcnt"] and L["hcnt"] + cells * 4 == L["total"]


def _roots(card):
    return gc.random_net(card, [[] for _ in card], 3, zeros=False)


def test_the_150_kib_limit_of_state_and_histogram(sim):
    """Gibbs: 6 variables = 384 bytes of state + 252 x 152 cells x 4 bytes = exactly 150 KiB runs - with its 412 table cells and its
    programs (6 x (2 + 3) words, + 2 x 6 for offsets and cycle) in LDS; a seventh variable (64 bytes more) is refused.  Sampling: 12 bytes a cell."""
    card = [252, 152, 2, 2, 2, 2, 2]
    assert 6 * 64 + 252 * 152 * 4 == 150 * KIB
    fits, = sim(_roots(card[:6]), [gibbs_line(1, 9, [0, 1])])
    assert fits["form"] == "PoolProgLds" and (fits["hist"], fits["pool"], fits["prog"]) == (384, 150 * KIB, 150 * KIB + 412 * 8)
    assert fits["total"] == 150 * KIB + 412 * 8 + 42 * 4 and fits["hist_cells"] == 252 * 152
    over, = sim(_roots(card), [gibbs_line(1, 9, [0, 1])])
    assert over == {"error": E_LIMIT, "msg": GIBBS_TOO_LARGE}
    card = [32, 21, 19, 2, 2, 2, 2]
    assert 6 * 64 + 32 * 21 * 19 * 12 == 150 * KIB
    for mode in (REJECTION, LIKELIHOOD):
        fits, = sim(_roots(card[:6]), [sample_line(mode, 100, [0, 1, 2])])
        assert (fits["hsum"], fits["hcnt"], fits["total"], fits["hist_cells"]) == (384, 384 + 12768 * 8, 150 * KIB, 12768)
        over, = sim(_roots(card), [sample_line(mode, 100, [0, 1, 2])])
        assert over == {"error": E_LIMIT, "msg": SAMPLING_TOO_LARGE}


def test_the_160_kib_limit_of_the_tables(sim):
    """A chain a -> b -> c of 5, 127 and 156 states, query a: 192 bytes of state, 20 of histogram (the tables start at 224), tables of
    5 + 5 x 127 + 127 x 156 = 20 452 cells = 163 616 bytes: state + histogram + tables are exactly 160 KiB - the tables are in LDS and
    nothing fits beside them (PoolLds); one more state of c and they stay in L2, with the programs in LDS (ProgLds)."""
    def chain(card):
        return gc.random_net(card, [[], [0], [1]], 4, zeros=False)
    a, b, c = 5, 127, 156
    cells = a + a * b + b * c
    assert a16(a16(192) + 4 * a) + 8 * cells == 160 * KIB
    exact, = sim(chain([a, b, c]), [gibbs_line(1, 9, [0])])
    assert (exact["form"], exact["total"], exact["prog_words"]) == ("PoolLds", 160 * KIB, 0)
    over, = sim(chain([a, b, c + 1]), [gibbs_line(1, 9, [0])])
    words = (2 + 3 + 5) + (2 + 5 + 5) + (2 + 5) + 2 * 3  # a: its CPT and b's; b: its own and c's; c: its own; offsets and cycle
    assert (over["form"], over["pool"], over["prog"], over["total"]) == ("ProgLds", a16(192 + 4 * a), a16(192 + 4 * a), a16(192 + 4 * a) + 4 * words)


def test_a_histogram_of_one_cell(sim):
    net = gc.random_net([1, 3], [[], [0]], 5, zeros=False)
    p, s = sim(net, [gibbs_line(1, 9, [0]), sample_line(REJECTION, 9, [0])])
    assert (p["hist_cells"], p["hist"], p["pool"]) == (1, 128, 144) and p["form"] == "Fast8"
    assert (s["hist_cells"], s["hsum"], s["hcnt"], s["total"]) == (1, 128, 136, 140)


# ------------------------------------------------------------------------------------------------------------ FAST and Fast8

def test_fast_needs_every_condition(sim):
    """At most 8 states, at most 4 factors, at most two other variables per factor - of the variables of the CYCLE."""
    form = lambda net, ev=None: sim(net, [gibbs_line(1, 9, [len(net.card) - 1], ev)])[0]["form"]
    chain = lambda card: gc.random_net(card, [[], [0], [1]], 6)
    assert form(chain([8, 2, 2])) == "Fast8" and form(chain([9, 2, 2])) == "PoolProgLds"
    assert form(chain([9, 2, 2]), {0: 8}) == "Fast8"  # the nine-state variable is evidence: no update, no record
    star = lambda k: gc.random_net([2] * (k + 1), [[]] + [[0]] * k, 7)
    assert form(star(3)) == "Fast8" and form(star(4)) == "PoolProgLds" and form(star(4), {0: 1}) == "Fast8"
    collider = lambda k: gc.random_net([2] * (k + 1), [[] for _ in range(k)] + [list(range(k))], 8)
    assert form(collider(2)) == "Fast8" and form(collider(3)) == "PoolProgLds"


def test_eight_lanes_a_chain_up_to_512_workgroups(sim):
    net = gc.grid_net(3, 3, 8, 51)
    res = sim(net, [gibbs_line(m, c, [4]) for m, c in ((1, 4096), (1, 4097), (2, 8), (2, 4096), (1, 32768), (1, 32769), (2, 32769), (0, 8))])
    assert [(r["form"], r["blocks"]) for r in res] == [("Fast8", 512), ("Fast", 65), ("Fast", 1), ("Fast", 64), ("Fast", 512), ("L2", 513), ("L2", 513), ("L2", 1)]


# ------------------------------------------------------------------------------------------------------------- forward sampling

def test_sample_plans(sim):
    gc_mixed_card = [3, 2, 5, 4, 2, 3]
    net = gc.random_net(gc_mixed_card, [[], [0], [0, 1], [2], [1, 3], [2, 4]], 21)
    n_scope = sum(len(s) for s in net.scope)
    lines = [sample_line(SAMPLE, 1), sample_line(SAMPLE, 262_144 + 65, clamp={2: 4, 0: 1}), sample_line(REJECTION, 65, [2, 0], ev={4: 1}),
             sample_line(LIKELIHOOD, 65, [0, 2], clamp={4: 1}), sample_line(PROBE, 5, cdf_stride=5), sample_line(SAMPLE, 0)]
    one, many, rej, lik, probe, none = sim(net, lines)
    assert (one["blocks"], many["blocks"], rej["blocks"], none["blocks"]) == (1, 4096, 2, 1)  # capped at 256 x 16, at least one
    for p in (one, many, probe):
        assert (p["hist_cells"], p["total"]) == (0, 384)
    assert (one["out_bytes"], many["out_bytes"]) == (6, (262_144 + 65) * 6)
    assert (probe["probe_states"], probe["out_bytes"]) == (32, 32 + 5 * 8 * (1 + 6 * 5))
    for p, q in ((rej, [2, 0]), (lik, [0, 2])):
        assert (p["hist_cells"], p["cells"], p["hsum"], p["hcnt"], p["total"], p["out_bytes"]) == (15, 15, 384, 384 + 120, 384 + 180, 240)
        assert p["pack"][p["o_q"]:p["o_q"] + 2] == q and p["pack"][p["o_qs"]:p["o_qs"] + 2] == [gc_mixed_card[q[1]], 1]
    assert rej["pack"][rej["o_ev"]:rej["o_ev"] + 1] == [4] and rej["pack"][rej["o_ec"]:rej["o_ec"] + 1] == [1]
    assert rej["pack"][:n_scope] == [u for s in net.scope for u in s] and rej["pack"][n_scope:2 * n_scope] == [x for s in net.stride for x in s]
    clamped = lambda p: [(v, p["vars"][8 * v + 7]) for v in range(6) if p["vars"][8 * v + 6]]
    assert clamped(many) == [(0, 1), (2, 4)] and clamped(lik) == [(4, 1)] and clamped(rej) == []  # rejection clamps nothing


# ------------------------------------------------------------------------------------------------------------------ errors

def test_error_paths(sim):
    net = gc.grid_net(2, 2, 3, 9)
    cycle_msg = "gibbs: cycle must list every non-evidence variable once"
    res = sim(net, [gibbs_line(1, 9, [3], {0: 1}, [1, 2, 2]),             # a repeat
                    gibbs_line(1, 9, [3], {0: 1}, [1, 0, 3]),             # names the evidence
                    gibbs_line(1, 9, [3], {0: 1}, [1, 2, 4]),             # an unknown id
                    gibbs_line(1, 9, [3], {0: 1, 1: 0, 2: 2, 3: 1}),      # nothing left to update
                    gibbs_line(1, 9, [0], {0: 1}, cond=0),                # the conditional of an evidence variable
                    gibbs_line(1, 9, [3], {0: 3}), gibbs_line(1, 9, [3], {0: -1}),
                    sample_line(SAMPLE, 9, clamp={1: 3}), sample_line(LIKELIHOOD, 9, [0], clamp={1: -1}), sample_line(SAMPLE, 9, clamp={4: 0})])
    assert res == [{"error": E_ARG, "msg": m} for m in (
        cycle_msg, cycle_msg, cycle_msg, "gibbs: every variable is evidence", "gibbs conditional: the variable is evidence or unknown",
        "gibbs: evidence label outside the domain", "gibbs: evidence label outside the domain",
        "sampling: clamped label outside the domain", "sampling: clamped label outside the domain", "sampling: unknown clamped variable")]


def test_sampling_needs_topological_ids(sim):
    """Variable 0 is the child of variable 1: forward sampling, which walks the variables in id order, refuses the network; the Gibbs
    plan never checked the order and still does not."""
    prefix = ["2", "2 2", "0 2 3", "1 0 1", "0 4 6", " ".join(float(x).hex() for x in (0.1, 0.9, 0.4, 0.6, 0.5, 0.5))]
    s, g = sim(prefix, [sample_line(SAMPLE, 9), gibbs_line(1, 9, [0])])
    assert s == {"error": E_ARG, "msg": "sampling: variable ids are not in topological order"}
    assert g["form"] == "Fast8"


def test_a_cell_product_beyond_int64_is_refused_not_wrapped(sim):
    """255^8 > 2^63: nine 255-state query variables.  The product stops above the largest histogram a launch holds."""
    assert 255 ** 8 > 2 ** 63
    net = _roots([255] * 9 + [2])
    g, r, l, ok = sim(net, [gibbs_line(1, 9, list(range(9))), sample_line(REJECTION, 9, list(range(9))), sample_line(LIKELIHOOD, 9, list(range(9))),
                            gibbs_line(1, 9, [9, 0])])
    assert g == {"error": E_LIMIT, "msg": GIBBS_TOO_LARGE} and r == l == {"error": E_LIMIT, "msg": SAMPLING_TOO_LARGE}
    assert ok["hist_cells"] == 510


def test_cardinality_above_255(sim):
    net = gc.random_net([256, 2], [[], [0]], 4)
    g, s = sim(net, [gibbs_line(1, 8, [1]), sample_line(SAMPLE, 4)])
    assert g == {"error": E_LIMIT, "msg": "gibbs: cardinality above 255"} and s == {"error": E_LIMIT, "msg": "sampling: cardinality above 255"}
