"""The class matrix: pinned small inputs that make the planner emit every class of work it can emit (emit_core.h kKid*, named by
kernel_name()), and inside each class the shapes at which the kernels differ.  Data and small helpers - no test lives here.
tests/test_kernel_classes_host.py proves every case on the planner's own programs (CPU); tests/test_kernel_classes.py runs them on
the device.

A case is
    recipe    (netspec function name, keyword arguments) - CPTs with p_zero = 0 and p_missing = 0, so every state code exists
    options   the engine options that shape the programs (OPTION_NAMES); the same values go to the simulator and to the engine
    requests  [(query node, [evidence nodes], [evidence codes])] - nodes by the integer of their name ("007" -> 7)
    nodes, max_cells   the size of the network and of the largest step (output cells x eliminated combinations) - the table stays
              at networks of at most 30 nodes and steps of at most 2^16 cells (MAX_NODES, MAX_CELLS); the cases of the sweep matrix
              (a sweep_iters or sweep_canon option, or the roof_grid_spec recipe) at 37 nodes and 2^20 cells = 8 MiB (SWEEP_MAX_NODES,
              SWEEP_MAX_CELLS): a wave-owned tail wants a table over seven four-state variables, several work items of several
              tiles one over eight, and whole work items of eight tiles one over nine
    classes   the class names the programs of those requests contain, all of them
    edges     the edge tags (see step_edges) those programs contain, all of them
The cases are the cheapest witnesses a random search over netspec recipes and option sets found, chosen greedily so that every class
and every (family, edge) pair is covered, plus a second witness per class; the host test proves each, whatever found it.

The sweep matrix (the cases from 39 on, and sweep_edges): the paths of ve_sweep_dma_kernel and ve_sweep_kernel by name.  A grid small
enough for the table is eliminated along its short side and never carries the frontier of seven or more four-state variables the
wave-owned tails need, so these cases use netspec.roof_grid_spec - a grid whose first row is tied together by one more node, which
is always in the evidence - at 7, 8 and 9 columns (2, 8 and 32 tiles per step).  Each base (recipe, request) comes with sweep_iters
3 (work items of three tiles and a shorter last one) and 1 (work items of one tile: no next-tile fetch), one of them again with
sweep_canon 0 (the kernel's general path on the same programs), one with the engine's eight tiles per work item on 32-tile steps.
Two more have a two- and a three-state column: steps of three tiles, run as work items of two tiles and one.
"""
import os
import sys

import numpy as np

import netspec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))  # dump_plan

OPTION_NAMES = ("small_cells", "big_iters", "tile_h", "fuse", "chain", "sweep", "sweep_min", "outer", "order_effort", "sweep_iters", "sweep_canon")
DEFAULTS = dict(small_cells=1024, big_iters=4096, tile_h=0, fuse=1, chain=1, sweep=5, sweep_min=2, outer=1, order_effort=0, sweep_iters=8, sweep_canon=1)
# Not an option of a case: build_schedule halves the work items of a small sweep launch (sweep_adapt, 4096 workgroups by default), down to
# two tiles and, from three, to one - every launch of this table is small.  The matrix runs with it off, on the simulator and on the
# device, so that a SWEEP step's work items are the sweep_iters tiles its case names.
MATRIX_SWEEP_ADAPT, PRODUCT_SWEEP_ADAPT = 0, 4096
# The two thresholds of the order search, in modelled bytes: the simulator plans with these (a bare Network's minfill_above, and the
# second_above set_sim_options passes), the engine's own defaults are 5e6 and 2e7 - the device tests set them, so that the engine
# writes the programs the host test proved.
MATRIX_MINFILL_ABOVE, MATRIX_SECOND_ABOVE = 2e7, 1e7

MAX_NODES, MAX_CELLS = 30, 1 << 16
SWEEP_MAX_NODES, SWEEP_MAX_CELLS = 37, 1 << 20

MFMA1 = ("fiber<1,cx4,nc16-mfma>", "fiber<1,cx16,nc16-mfma>")  # the classes ve_mfma_kernel takes in the product's launch shape
CHAIN = "fiber<1,cx64,chain-mfma>"
SWEEP = "ve_sweep_kernel"
SEGMENTS = "segments"


def family(cls):
    """The kernel body a class shares with its siblings: the store / contraction form of a FIBER class (its NC part: fiber_call,
    fiber_mfma_call, outer_mfma_call of ve_kernel.hip.h are specialised on it), "chain", "generic", "sweep", "segments"."""
    if cls.startswith("generic<"):
        return "generic"
    if cls == CHAIN:
        return "chain"
    if cls == SWEEP:
        return "sweep"
    if cls.startswith("fiber<"):
        return cls[:-1].split(",")[2]
    return cls


def step_edges(s):
    """Edge tags of one decoded step (tools/dump_plan.py decode): "<family>:<edge>", and "<class>:rs<n>" for the row stride of the MFMA forms."""
    if not s["tile_h"]:
        return set()
    fam, out = family(s["cls"]), set()
    add = lambda e: out.add(f"{fam}:{e}")
    if s["kind"] == "SWEEP":
        return sweep_edges(s)
    if s["hi"] % s["tile_h"]:
        add("partial_tile")           # the last workgroup of the step takes fewer hi iterations than the others
    if s["lo"] % 64 or s["lo"] < 64:
        add("lane_ragged")            # the last (or only) wave of the lane block has idle lanes
    if s["kind"] == "GENERIC":
        return out
    rs = (s["w1"] >> 20) & 0xff
    if fam in ("nc16-mfma", "outer-mfma", "chain"):
        out.add(f"{s['cls']}:rs{rs}")
    add("nctrl0" if s["nctrl"] == 0 else "nctrl+")
    add("ns0" if s["ns"] == 0 else "ns1" if s["ns"] == 1 else "ns2+")
    if s["cls"].split(",")[1] == "cxN":
        if s["cx"] % 4:
            add("cx_not_mult4")
        if s["cx"] != s["c1"] and s["cx"] // s["c1"] != s["c1"]:
            add("c1_ne_c2")           # a fused pair of two different cardinalities
    if fam == "ncN" and s["NC"] & (s["NC"] - 1):
        add("nc_not_pow2")
    if any(t == "C" for t, _ in s["big"]):
        add("big_in_consts")          # a big input read from the constants pool (a CPT), not from the arena
    return out


SWEEP_DEAD_PACKS = {0x4321: 0, 0x4320: 1, 0x4310: 2, 0x4210: 3, 0x3210: 4}  # w8 of a five-variable pass in which digit d alone dies
SWEEP_SHAPES = ("own5", "dead0", "dead1", "dead2", "dead3", "dead4", "readout5", "own4", "readout4", "k3", "k2", "any")
SWEEP_ITEMS = ("items2+", "multi_tile", "one_tile_item", "partial_tile", "one_tile_step")
SWEEP_STAGES = ("par", "par_tail", "rbits", "nctrl2+", "ns2+")
SWEEP_STEP = ("odd_tiles",)
SWEEP_TAILS = ("own5", "dead0", "dead1", "dead2", "dead3", "dead4")  # the wave-owned tails the ragged shapes of the tile loop are crossed with


def sweep_shape(s):
    """The specialisation of sweep_tiles_dma that ve_sweep_dma_kernel (sweep_kernel.hip.h) sends a decoded SWEEP step to - its
    dispatch restated on the step's header: the canonical flag (w1), k, kout (w7) and the surviving digits (w8)."""
    k, kout, surv = s["k"], s["kout"], s["surv"]
    if not s["canon"]:
        return "any"                                     # <0,false>: runtime strides
    if k == 5 and kout == 5 and surv == 0x43210:
        return "own5"                                    # <5,true>: the wave-owned tail
    if k == 5 and kout == 4 and surv in SWEEP_DEAD_PACKS:
        return f"dead{SWEEP_DEAD_PACKS[surv]}"           # <5,true,true>: the wave-owned tail with one dying digit
    if k == 5:
        return "readout5"                                # <5,false>
    if k == 4:
        return "own4" if kout == 4 and surv == 0x3210 else "readout4"  # <4,true> / <4,false>
    return f"k{k}"                                       # <3,false> / <2,false>


def sweep_edges(s):
    """Edge tags of one decoded SWEEP step.  hi = tiles of 8192 cells, tile_h = tiles per work item (the option sweep_iters; the
    matrix runs with sweep_adapt 0, so the schedule does not change it): work item i takes the tiles [i tile_h, min(hi, (i + 1) tile_h)).
      k<k>, kout0 / kout+      variables per pass; none / some of them replaced by a new axis
      the shape                one of SWEEP_SHAPES (sweep_shape)
      par, rbits               a stage whose T offset takes a ctrl value from bits 0-1 of r (source 8 + 0: the PAR form of a stage,
                               two T columns per lane pair) / from any bits of r (source >= 8)
      par_tail                 the LAST stage of a wave-owned tail (own5, dead<d>, own4) is of the PAR form: sweep_last_stage_out<K, true>
      nctrl2+, ns2+            a stage with two or three ctrl values / with two or more small inputs
      odd_tiles                an odd number of tiles: the R cells of the table - the stride between the tile's combinations in
                               memory - are no power of two (a two- or three-state axis among them)
      items2+                  more than one work item
      multi_tile               a work item of two or more tiles: the next tile is fetched while the current one is finished
      one_tile_item            a work item of exactly one tile: no next-tile fetch behind the (only, or last) tail
      partial_tile             the last work item takes fewer tiles than the others
      one_tile_step            a step of one tile (the planner emits none: IMPOSSIBLE_EDGES)
      <shape>+<item tag>       both on the same step, for the wave-owned tails (SWEEP_TAILS)"""
    out = set()
    add = lambda e: out.add(f"sweep:{e}")
    hi, th = s["hi"], s["tile_h"]
    add(f"k{s['k']}")
    add("kout0" if s["kout"] == 0 else "kout+")
    shape = sweep_shape(s)
    add(shape)
    srcs = [c for g in s["stages"] for c in g["ctrl"]]
    if 8 in srcs:
        add("par")
    if any(c >= 8 for c in srcs):
        add("rbits")
    if shape in SWEEP_TAILS + ("own4",) and 8 in s["stages"][-1]["ctrl"]:
        add("par_tail")
    if any(len(g["ctrl"]) >= 2 for g in s["stages"]):
        add("nctrl2+")
    if any(g["ns"] >= 2 for g in s["stages"]):
        add("ns2+")
    if hi % 2:
        add("odd_tiles")
    items = set()
    if hi > th:
        items.add("items2+")
    if min(hi, th) >= 2:
        items.add("multi_tile")
    if th == 1 or hi % th == 1:
        items.add("one_tile_item")
    if hi % th:
        items.add("partial_tile")
    if hi == 1:
        items.add("one_tile_step")
    for e in items:
        add(e)
        if shape in SWEEP_TAILS:
            add(f"{shape}+{e}")
    return out


def in_sweep_matrix(case):
    """A case of the sweep matrix: the larger size cap holds for these alone."""
    return case["recipe"][0] == "roof_grid_spec" or "sweep_iters" in case["options"] or "sweep_canon" in case["options"]


def size_cap(case):
    return (SWEEP_MAX_NODES, SWEEP_MAX_CELLS) if in_sweep_matrix(case) else (MAX_NODES, MAX_CELLS)


_roof_specs = {}  # (the roof's CPT has up to 2 x 4^9 rows, and a base of the sweep matrix is used by two or three cases: built once, read only)


def build_spec(case):
    fn, kw = case["recipe"]
    kw = dict(kw)
    if fn == "random_dag_spec":
        kw.update(p_zero=0.0, p_missing=0.0)
    if fn == "roof_grid_spec":
        key = repr(sorted(kw.items()))
        if key not in _roof_specs:
            _roof_specs[key] = netspec.roof_grid_spec(**kw)
        return _roof_specs[key]
    return getattr(netspec, fn)(**kw)


def options(case):
    return {**DEFAULTS, **case["options"]}


def set_sim_options(opt, sweep_adapt=MATRIX_SWEEP_ADAPT):
    """The case's options on the simulator (process-wide)."""
    import simengine
    L = simengine.lib()
    L.plan_sim_set_small_cells(opt["small_cells"]); L.plan_sim_set_tiling(opt["big_iters"], opt["tile_h"]); L.plan_sim_set_fuse(opt["fuse"])
    L.plan_sim_set_chain(opt["chain"]); L.plan_sim_set_sweep(opt["sweep"]); L.plan_sim_set_sweep_min(opt["sweep_min"])
    L.plan_sim_set_outer(opt["outer"]); L.plan_sim_set_prune(1); L.plan_sim_set_order_effort(opt["order_effort"], MATRIX_SECOND_ABOVE)
    L.plan_sim_set_sweep_iters(opt["sweep_iters"]); L.plan_sim_set_sweep_canon(opt["sweep_canon"]); L.plan_sim_set_sweep_adapt(sweep_adapt)


def reset_sim_options():
    """The product's defaults (a bare Network's: order_effort 0)."""
    set_sim_options(DEFAULTS, PRODUCT_SWEEP_ADAPT)


def flat_ids(flat, nodes):
    return np.array([flat.id[f"{int(v):03d}"] for v in nodes], np.int32)


def planned(flat, requests):
    """(classes, edges, largest step table in cells) of the programs the planner writes for `requests` under the simulator's options."""
    import dump_plan as dp
    classes, edges, cells = set(), set(), 0
    for q, ev, ec in requests:
        steps = dp.decode(dp.program(flat, flat_ids(flat, [q]), flat_ids(flat, ev), np.asarray(ec, np.int32)), classes=True)
        for s in steps:
            classes.add(s["cls"])
            edges |= step_edges(s)
            cells = max(cells, s["lo"] * s["hi"] * (s["cx"] if s["kind"] != "SWEEP" else 1) * s.get("NC", 1))
    return classes, edges, cells


def c3_sweep_steps(n_requests=300):
    """The decoded SWEEP steps (with cls and tile_h) of the first requests of the C3 stream - the 10 x 10 grid of four-state nodes, four
    evidence nodes per request - under the simulator's options."""
    import dump_plan as dp
    import sorobn_amd
    from sorobn_amd.flatten import flatten
    flat = flatten(netspec.build(netspec.grid_spec(10, 10, 4, seed=0), sorobn_amd.BayesNet))
    to_var = np.array([flat.id[f"{i:03d}"] for i in range(100)], np.int32)
    q, ev, ec = netspec.c3_requests(100, 4, n_requests, 4, seed=1)
    return [s for i in range(n_requests) for s in dp.decode(dp.program(flat, [to_var[q[i]]], to_var[ev[i]], ec[i]), classes=True) if s["kind"] == "SWEEP"]


ROUTES = ("level", "sweep_dma", "sweep_reg", "segment", "mfma")  # planner.h LevelRoute, in order: the kernel a launch group goes to
ROUTING_OPTIONS = ("split_kinds", "seg_kernel", "mfma_kernel", "sweep_dma")  # bit k of a routing setting; the engine's defaults: 0, 1, 1, 1
ROUTING_DEFAULT = 0b1110
# the smallest pair of cases whose classes reach all four kernels of a level between them: segments, a level-kernel class and an MFMA1
# class in the first; segments, level-kernel classes and SWEEP in the second (test_kernel_classes_host.py proves it)
ROUTING_CASES = ("34-dag84812n9-sc16-bi256x0", "35-dag87864n12-sc256-bi64x2")


def level_groups(flat, requests, routing):
    """(launches, groups) of the schedule of `requests` as one batch under the simulator's options and the routing setting `routing`
    (bits: ROUTING_OPTIONS) - oracle/plan_sim.cpp plan_sim_level_groups, the planner's own level_groups.  Dictionaries with the fields
    of planner.h Launch (+ route) and LaunchGroup; routes by name, classes by name (cls; stat_cls: None unless split_kinds)."""
    import ctypes as C
    import dump_plan as dp
    import simengine
    L = simengine.lib()
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    L.plan_sim_level_groups.argtypes = [C.c_int32, i32p, i64p, i32p, i64p, f64p, C.c_int32, i32p, C.c_int64, i64p, i32p, i64p, i32p, i32p,
                                        C.c_int32, f64p, C.c_int64, f64p, C.c_int64, i64p]
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    qv = flat_ids(flat, [q for q, _, _ in requests])
    ev = np.ascontiguousarray(np.concatenate([flat_ids(flat, e) for _, e, _ in requests] + [np.zeros(1, np.int32)]), np.int32)
    ec = np.array([c for _, _, cs in requests for c in cs] + [0], np.int32)
    q_off = np.arange(len(requests) + 1, dtype=np.int64)
    e_off = np.concatenate([[0], np.cumsum([len(e) for _, e, _ in requests])]).astype(np.int64)
    hints = np.ascontiguousarray(np.stack(flat.hints).reshape(-1) if flat.hints else [0], np.int32)
    cap = 4096
    la, gr, n = np.zeros((cap, 7)), np.zeros((cap, 9)), np.zeros(2, np.int64)
    rc = L.plan_sim_level_groups(len(flat.card), p(flat.card, C.c_int32), p(flat.scope_off, C.c_int64), p(flat.scope_vars, C.c_int32),
                                 p(flat.value_off, C.c_int64), p(flat.values, C.c_double), len(flat.hints), p(hints, C.c_int32),
                                 len(requests), p(q_off, C.c_int64), p(qv, C.c_int32), p(e_off, C.c_int64), p(ev, C.c_int32), p(ec, C.c_int32),
                                 routing, p(la, C.c_double), cap, p(gr, C.c_double), cap, p(n, C.c_int64))
    assert rc == 0, (rc, L.plan_sim_error().decode())
    names = dp.class_names()
    launches = [dict(level=int(r[0]), cls=names[int(r[1])], route=ROUTES[int(r[2])], grid=int(r[3]), wg_level=int(r[4]), wg_first=int(r[5]),
                     alg_bytes=float(r[6])) for r in la[:n[0]]]
    groups = [dict(route=ROUTES[int(r[0])], level=int(r[1]), stat_cls=names[int(r[2])] if r[2] >= 0 else None, wg_level=int(r[3]),
                   wg_first=int(r[4]), grid=int(r[5]), alg_bytes=float(r[6]), first_launch=int(r[7]), n_launches=int(r[8])) for r in gr[:n[1]]]
    return launches, groups


def oracle_dense(on, card, q, ev, ec):
    """The oracle's posterior of one request as a dense vector over the query node's codes."""
    codes, vals = on.query_codes([on.id[f"{q:03d}"]], [on.id[f"{v:03d}"] for v in ev], list(ec))
    dense = np.zeros(card)
    dense[codes[:, 0]] = vals
    return dense


CASES = [
    dict(name='00-grid3x6s21249-sc20-bi8x3',
         recipe=('grid_spec', {'R': 3, 'C': 6, 'K': 4, 'seed': 21249}),
         options={'big_iters': 8, 'small_cells': 20, 'sweep_min': 3, 'tile_h': 3},
         requests=[(3, [10, 17], [2, 0])],
         nodes=18, max_cells=1024,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx16,ncN>', 'fiber<2,cx16,nc1>', 'fiber<2,cx16,nc4>', 'fiber<2,cx16,ncN>',
                  'fiber<2,cx16,outer-mfma>', 'fiber<2,cx4,nc1>', 'generic<3>', 'segments'],
         edges=['fiber<1,cx16,nc16-mfma>:rs1', 'fiber<2,cx16,outer-mfma>:rs16', 'generic:lane_ragged', 'generic:partial_tile',
                'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile', 'nc1:big_in_consts', 'nc1:nctrl+',
                'nc1:nctrl0', 'nc1:ns0', 'nc1:ns2+', 'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:lane_ragged', 'nc4:nctrl0', 'nc4:ns1',
                'nc4:partial_tile', 'ncN:big_in_consts', 'ncN:lane_ragged', 'ncN:nctrl0', 'ncN:ns1', 'ncN:ns2+', 'ncN:partial_tile',
                'outer-mfma:big_in_consts', 'outer-mfma:lane_ragged', 'outer-mfma:nctrl0', 'outer-mfma:ns1', 'outer-mfma:partial_tile']),
    dict(name='01-grid5x4s28056-sc16-bi4x1',
         recipe=('grid_spec', {'R': 5, 'C': 4, 'K': 4, 'seed': 28056}),
         options={'big_iters': 4, 'small_cells': 16, 'sweep': 0, 'tile_h': 1},
         requests=[(10, [1, 19], [3, 0])],
         nodes=20, max_cells=4096,
         classes=['fiber<2,cx16,nc1>', 'fiber<2,cx16,ncN>', 'fiber<2,cx16,outer-mfma>', 'fiber<2,cx4,outer-mfma>', 'generic<1>', 'generic<3>',
                  'segments'],
         edges=['fiber<2,cx16,outer-mfma>:rs1', 'fiber<2,cx16,outer-mfma>:rs4', 'fiber<2,cx4,outer-mfma>:rs1', 'fiber<2,cx4,outer-mfma>:rs16',
                'fiber<2,cx4,outer-mfma>:rs4', 'generic:lane_ragged', 'nc1:big_in_consts', 'nc1:lane_ragged', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1',
                'ncN:big_in_consts', 'ncN:nctrl0', 'ncN:ns1', 'outer-mfma:big_in_consts', 'outer-mfma:lane_ragged', 'outer-mfma:nctrl+',
                'outer-mfma:nctrl0', 'outer-mfma:ns0', 'outer-mfma:ns1', 'outer-mfma:ns2+']),
    dict(name='02-grid5x5s32624-sc20-bi64x2',
         recipe=('grid_spec', {'R': 5, 'C': 5, 'K': 4, 'seed': 32624}),
         options={'big_iters': 64, 'fuse': 0, 'small_cells': 20, 'sweep': 0, 'sweep_min': 3, 'tile_h': 2},
         requests=[(3, [14, 17], [1, 2])],
         nodes=25, max_cells=1024,
         classes=['fiber<1,cx4,nc4>', 'fiber<1,cx4,ncN>', 'fiber<2,cx4,nc1>', 'fiber<2,cx4,nc4>', 'fiber<2,cx4,ncN>', 'fiber<2,cx4,outer-mfma>',
                  'segments'],
         edges=['fiber<2,cx4,outer-mfma>:rs4', 'nc1:big_in_consts', 'nc1:nctrl0', 'nc1:ns0', 'nc1:partial_tile', 'nc4:big_in_consts',
                'nc4:lane_ragged', 'nc4:nctrl0', 'nc4:ns1', 'nc4:partial_tile', 'ncN:big_in_consts', 'ncN:lane_ragged', 'ncN:nctrl+', 'ncN:nctrl0',
                'ncN:ns1', 'ncN:ns2+', 'ncN:partial_tile', 'outer-mfma:big_in_consts', 'outer-mfma:lane_ragged', 'outer-mfma:nctrl0',
                'outer-mfma:ns0', 'outer-mfma:partial_tile']),
    dict(name='03-grid5x5s53556-sc64-bi64x3',
         recipe=('grid_spec', {'R': 5, 'C': 5, 'K': 4, 'seed': 53556}),
         options={'big_iters': 64, 'small_cells': 64, 'sweep_min': 3, 'tile_h': 3},
         requests=[(9, [13, 24], [3, 2])],
         nodes=25, max_cells=4096,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx16,nc4>', 'fiber<1,cx4,nc16-mfma>', 'fiber<1,cx4,nc1>', 'fiber<1,cx64,chain-mfma>',
                  'generic<2>', 'generic<3>', 'segments'],
         edges=['chain:lane_ragged', 'chain:nctrl+', 'chain:ns2+', 'chain:partial_tile', 'fiber<1,cx16,nc16-mfma>:rs16',
                'fiber<1,cx16,nc16-mfma>:rs4', 'fiber<1,cx4,nc16-mfma>:rs16', 'fiber<1,cx64,chain-mfma>:rs16', 'generic:partial_tile',
                'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl+', 'nc16-mfma:nctrl0', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile', 'nc1:nctrl0', 'nc1:ns0',
                'nc1:partial_tile', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile']),
    dict(name='04-grid5x5s91875-sc64-bi2x1',
         recipe=('grid_spec', {'R': 5, 'C': 5, 'K': 4, 'seed': 91875}),
         options={'big_iters': 2, 'small_cells': 64, 'sweep': 0, 'sweep_min': 3, 'tile_h': 1},
         requests=[(24, [13, 21], [1, 3])],
         nodes=25, max_cells=4096,
         classes=['fiber<1,cx16,nc4>', 'fiber<1,cx4,nc1>', 'fiber<1,cx64,chain-mfma>', 'generic<1>', 'generic<3>', 'segments'],
         edges=['chain:lane_ragged', 'chain:nctrl+', 'chain:nctrl0', 'chain:ns1', 'chain:ns2+', 'fiber<1,cx64,chain-mfma>:rs1',
                'fiber<1,cx64,chain-mfma>:rs16', 'generic:lane_ragged', 'nc1:nctrl+', 'nc1:ns1', 'nc4:nctrl+', 'nc4:ns2+']),
    dict(name='05-mixed3x3s7475-sc6-bi2x1',
         recipe=('mixed_grid_spec', {'R': 3, 'C': 3, 'cards': [2, 2, 3], 'seed': 7475}),
         options={'big_iters': 2, 'chain': 0, 'outer': 0, 'small_cells': 6, 'sweep_min': 3, 'tile_h': 1},
         requests=[(7, [5, 6], [2, 0])],
         nodes=9, max_cells=32,
         classes=['fiber<1,cxN,nc1>', 'fiber<1,cxN,nc4>', 'generic<2>', 'segments'],
         edges=['generic:lane_ragged', 'nc1:cx_not_mult4', 'nc1:lane_ragged', 'nc1:nctrl+', 'nc1:ns2+', 'nc4:big_in_consts', 'nc4:lane_ragged',
                'nc4:nctrl0', 'nc4:ns2+']),
    dict(name='06-mixed3x3s57275-sc4-bi4x1',
         recipe=('mixed_grid_spec', {'R': 3, 'C': 3, 'cards': [3, 2, 2], 'seed': 57275}),
         options={'big_iters': 4, 'chain': 0, 'fuse': 0, 'outer': 0, 'small_cells': 4, 'sweep': 0, 'sweep_min': 3, 'tile_h': 1},
         requests=[(8, [0, 1], [1, 0])],
         nodes=9, max_cells=24,
         classes=['fiber<1,cxN,nc1>', 'fiber<2,cxN,nc1>', 'fiber<2,cxN,ncN>', 'segments'],
         edges=['nc1:big_in_consts', 'nc1:cx_not_mult4', 'nc1:lane_ragged', 'nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'ncN:big_in_consts',
                'ncN:cx_not_mult4', 'ncN:lane_ragged', 'ncN:nctrl0', 'ncN:ns1']),
    dict(name='07-mixed3x3s62633-sc16-bi2x1',
         recipe=('mixed_grid_spec', {'R': 3, 'C': 3, 'cards': [5, 4, 4], 'seed': 62633}),
         options={'big_iters': 2, 'chain': 0, 'fuse': 0, 'outer': 0, 'small_cells': 16, 'tile_h': 1},
         requests=[(5, [2, 7], [1, 0])],
         nodes=9, max_cells=100,
         classes=['fiber<1,cxN,nc1>', 'fiber<2,cx4,nc1>', 'fiber<2,cx4,nc4>', 'fiber<2,cxN,nc1>', 'segments'],
         edges=['nc1:big_in_consts', 'nc1:cx_not_mult4', 'nc1:lane_ragged', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc4:big_in_consts',
                'nc4:lane_ragged', 'nc4:nctrl0', 'nc4:ns1']),
    dict(name='08-mixed3x5s24154-sc16-bi2x1',
         recipe=('mixed_grid_spec', {'R': 3, 'C': 5, 'cards': [5, 4, 3, 4, 4], 'seed': 24154}),
         options={'big_iters': 2, 'chain': 0, 'small_cells': 16, 'sweep_min': 3, 'tile_h': 1},
         requests=[(13, [], []), (10, [8, 11], [0, 2])],
         nodes=15, max_cells=576,
         classes=['fiber<1,cxN,nc1>', 'fiber<2,cx16,nc1>', 'fiber<2,cx4,ncN>', 'fiber<2,cxN,nc1>', 'fiber<2,cxN,nc4>', 'generic<1>', 'generic<2>',
                  'generic<3>', 'segments'],
         edges=['generic:lane_ragged', 'nc1:big_in_consts', 'nc1:c1_ne_c2', 'nc1:cx_not_mult4', 'nc1:lane_ragged', 'nc1:nctrl+', 'nc1:nctrl0',
                'nc1:ns0', 'nc1:ns1', 'nc4:big_in_consts', 'nc4:c1_ne_c2', 'nc4:lane_ragged', 'nc4:nctrl0', 'nc4:ns1', 'ncN:big_in_consts',
                'ncN:lane_ragged', 'ncN:nc_not_pow2', 'ncN:nctrl0', 'ncN:ns1']),
    dict(name='09-mixed4x3s56360-sc20-bi64x3',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 3, 'cards': [5, 4, 4], 'seed': 56360}),
         options={'big_iters': 64, 'small_cells': 20, 'sweep': 0, 'tile_h': 3},
         requests=[(11, [4, 10], [3, 3])],
         nodes=12, max_cells=400,
         classes=['fiber<1,cx4,ncN>', 'fiber<1,cxN,nc16>', 'segments'],
         edges=['nc16:big_in_consts', 'nc16:cx_not_mult4', 'nc16:lane_ragged', 'nc16:nctrl0', 'nc16:ns2+', 'nc16:partial_tile', 'ncN:big_in_consts',
                'ncN:lane_ragged', 'ncN:nctrl0', 'ncN:ns1', 'ncN:partial_tile']),
    dict(name='10-mixed4x4s36655-sc16-bi2x1',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 4, 'cards': [4, 2, 4, 4], 'seed': 36655}),
         options={'big_iters': 2, 'small_cells': 16, 'sweep_min': 3, 'tile_h': 1},
         requests=[(11, [6, 12], [3, 1])],
         nodes=16, max_cells=512,
         classes=['fiber<1,cx16,nc16>', 'fiber<1,cx4,nc1>', 'fiber<1,cxN,ncN>', 'generic<1>', 'generic<2>', 'generic<3>', 'segments'],
         edges=['generic:lane_ragged', 'nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc1:big_in_consts', 'nc1:lane_ragged', 'nc1:nctrl+',
                'nc1:ns1', 'ncN:c1_ne_c2', 'ncN:lane_ragged', 'ncN:nctrl0', 'ncN:ns2+']),
    dict(name='11-mixed4x4s31374-sc64-bi256x0',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 4, 'cards': [5, 4, 4, 4], 'seed': 31374}),
         options={'big_iters': 256, 'chain': 0, 'small_cells': 64, 'sweep_min': 3},
         requests=[(11, [9, 14], [1, 2])],
         nodes=16, max_cells=1280,
         classes=['fiber<1,cx4,nc16>', 'segments'],
         edges=['nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc16:partial_tile']),
    dict(name='12-mixed4x4s75766-sc64-bi8x3',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 4, 'cards': [5, 4, 4, 4], 'seed': 75766}),
         options={'big_iters': 8, 'fuse': 0, 'outer': 0, 'small_cells': 64, 'sweep_min': 3, 'tile_h': 3},
         requests=[(14, [0, 7], [3, 3])],
         nodes=16, max_cells=1280,
         classes=['fiber<1,cx4,nc16-mfma>', 'fiber<1,cx4,nc1>', 'fiber<1,cx4,nc4>', 'fiber<1,cx4,ncN>', 'fiber<1,cxN,nc1>', 'fiber<1,cxN,ncN>',
                  'fiber<2,cx4,nc1>', 'segments'],
         edges=['fiber<1,cx4,nc16-mfma>:rs1', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile',
                'nc1:big_in_consts', 'nc1:cx_not_mult4', 'nc1:lane_ragged', 'nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc1:partial_tile',
                'nc4:lane_ragged', 'nc4:nctrl+', 'nc4:ns1', 'nc4:partial_tile', 'ncN:big_in_consts', 'ncN:cx_not_mult4', 'ncN:lane_ragged',
                'ncN:nc_not_pow2', 'ncN:nctrl0', 'ncN:ns1', 'ncN:ns2+', 'ncN:partial_tile']),
    dict(name='13-mixed4x5s29490-sc20-bi256x5',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 5, 'cards': [2, 4, 4, 4, 4], 'seed': 29490}),
         options={'big_iters': 256, 'chain': 0, 'outer': 0, 'small_cells': 20, 'sweep': 0, 'sweep_min': 3, 'tile_h': 5},
         requests=[(19, [7, 9], [0, 3])],
         nodes=20, max_cells=8192,
         classes=['fiber<1,cxN,nc1>', 'fiber<2,cx16,nc16-mfma>', 'segments'],
         edges=['fiber<2,cx16,nc16-mfma>:rs4', 'nc16-mfma:big_in_consts', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+',
                'nc16-mfma:partial_tile', 'nc1:cx_not_mult4', 'nc1:nctrl0', 'nc1:ns0', 'nc1:partial_tile']),
    dict(name='14-mixed4x5s80785-sc64-bi2x1',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 5, 'cards': [4, 3, 5, 4, 4], 'seed': 80785}),
         options={'big_iters': 2, 'fuse': 0, 'outer': 0, 'small_cells': 64, 'tile_h': 1},
         requests=[(5, [3, 19], [1, 3])],
         nodes=20, max_cells=1600,
         classes=['fiber<1,cx4,nc16-mfma>', 'fiber<1,cx4,nc1>', 'fiber<1,cx4,ncN>', 'fiber<1,cxN,nc4>', 'fiber<1,cxN,ncN>', 'fiber<2,cx4,nc1>',
                  'fiber<2,cxN,nc1>', 'generic<2>', 'generic<3>', 'segments'],
         edges=['fiber<1,cx4,nc16-mfma>:rs16', 'generic:lane_ragged', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl0', 'nc16-mfma:ns1',
                'nc1:big_in_consts', 'nc1:cx_not_mult4', 'nc1:lane_ragged', 'nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc4:cx_not_mult4',
                'nc4:lane_ragged', 'nc4:nctrl+', 'nc4:ns1', 'ncN:big_in_consts', 'ncN:cx_not_mult4', 'ncN:lane_ragged', 'ncN:nc_not_pow2',
                'ncN:nctrl+', 'ncN:nctrl0', 'ncN:ns1']),
    dict(name='15-mixed4x5s27126-sc256-bi4x1',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 5, 'cards': [4, 4, 4, 4, 16], 'seed': 27126}),
         options={'big_iters': 4, 'small_cells': 256, 'tile_h': 1},
         requests=[(17, [8, 14], [2, 6])],
         nodes=20, max_cells=4096,
         classes=['fiber<1,cx16,ncN>', 'fiber<1,cx64,chain-mfma>', 'generic<2>', 'generic<3>', 'segments'],
         edges=['chain:lane_ragged', 'chain:nctrl0', 'chain:ns2+', 'fiber<1,cx64,chain-mfma>:rs4', 'generic:lane_ragged', 'ncN:nctrl+', 'ncN:ns2+']),
    dict(name='16-mixed4x5s87846-sc20-bi256x5',
         recipe=('mixed_grid_spec', {'R': 4, 'C': 5, 'cards': [4, 4, 4, 4, 4], 'seed': 87846}),
         options={'big_iters': 256, 'small_cells': 20, 'sweep': 0, 'sweep_min': 3, 'tile_h': 5},
         requests=[(7, [14, 18], [0, 3])],
         nodes=20, max_cells=4096,
         classes=['fiber<2,cx16,nc16-mfma>', 'fiber<2,cx16,nc4>', 'fiber<2,cx16,ncN>', 'fiber<2,cx16,outer-mfma>', 'fiber<2,cx4,outer-mfma>',
                  'segments'],
         edges=['fiber<2,cx16,nc16-mfma>:rs16', 'fiber<2,cx16,outer-mfma>:rs1', 'fiber<2,cx4,outer-mfma>:rs1', 'fiber<2,cx4,outer-mfma>:rs4',
                'nc16-mfma:big_in_consts', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl0', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile',
                'nc4:big_in_consts', 'nc4:nctrl0', 'nc4:ns1', 'nc4:partial_tile', 'ncN:big_in_consts', 'ncN:nctrl0', 'ncN:ns2+', 'ncN:partial_tile',
                'outer-mfma:big_in_consts', 'outer-mfma:lane_ragged', 'outer-mfma:nctrl+', 'outer-mfma:nctrl0', 'outer-mfma:ns0', 'outer-mfma:ns1',
                'outer-mfma:partial_tile']),
    dict(name='17-mixed5x4s7376-sc20-bi2x1',
         recipe=('mixed_grid_spec', {'R': 5, 'C': 4, 'cards': [4, 2, 4, 4], 'seed': 7376}),
         options={'big_iters': 2, 'chain': 0, 'outer': 0, 'small_cells': 20, 'sweep_min': 3, 'tile_h': 1},
         requests=[(3, [6, 17], [3, 1])],
         nodes=20, max_cells=512,
         classes=['fiber<1,cx16,nc16>', 'fiber<1,cxN,nc1>', 'fiber<1,cxN,ncN>', 'generic<1>', 'generic<3>', 'segments'],
         edges=['generic:lane_ragged', 'nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc1:cx_not_mult4', 'nc1:lane_ragged', 'nc1:nctrl+',
                'nc1:ns1', 'ncN:c1_ne_c2', 'ncN:lane_ragged', 'ncN:nctrl0', 'ncN:ns2+']),
    dict(name='18-mixed5x4s64633-sc16-bi64x2',
         recipe=('mixed_grid_spec', {'R': 5, 'C': 4, 'cards': [5, 4, 2, 8], 'seed': 64633}),
         options={'big_iters': 64, 'chain': 0, 'small_cells': 16, 'tile_h': 2},
         requests=[(11, [], [])],
         nodes=20, max_cells=3200,
         classes=['fiber<1,cxN,nc1>', 'fiber<2,cx4,nc1>', 'fiber<2,cxN,nc16>', 'fiber<2,cxN,ncN>', 'segments'],
         edges=['nc16:big_in_consts', 'nc16:c1_ne_c2', 'nc16:cx_not_mult4', 'nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc16:partial_tile',
                'nc1:big_in_consts', 'nc1:cx_not_mult4', 'nc1:nctrl0', 'nc1:ns0', 'nc1:partial_tile', 'ncN:big_in_consts', 'ncN:c1_ne_c2',
                'ncN:lane_ragged', 'ncN:nctrl+', 'ncN:ns1', 'ncN:partial_tile']),
    dict(name='19-mixed5x5s36169-sc256-bi4x1',
         recipe=('mixed_grid_spec', {'R': 5, 'C': 5, 'cards': [16, 4, 4, 16, 16], 'seed': 36169}),
         options={'big_iters': 4, 'fuse': 0, 'small_cells': 256, 'sweep': 0, 'sweep_min': 3, 'tile_h': 1},
         requests=[(18, [0, 7], [11, 0])],
         nodes=25, max_cells=16384,
         classes=['fiber<1,cx4,nc16>', 'fiber<1,cx4,nc4>', 'fiber<1,cxN,nc16>', 'fiber<1,cxN,nc1>', 'fiber<1,cxN,ncN>', 'generic<1>', 'generic<2>',
                  'generic<3>', 'segments'],
         edges=['generic:lane_ragged', 'nc16:nctrl+', 'nc16:nctrl0', 'nc16:ns1', 'nc16:ns2+', 'nc1:big_in_consts', 'nc1:nctrl+', 'nc1:nctrl0',
                'nc1:ns0', 'nc1:ns1', 'nc4:nctrl+', 'nc4:ns1', 'ncN:big_in_consts', 'ncN:nctrl+', 'ncN:ns1']),
    dict(name='20-dag19898n6-sc1-bi2x1',
         recipe=('random_dag_spec', {'seed': 19898, 'n_nodes': 6, 'max_parents': 2, 'cards': (2, 4), 'max_cells': 4096}),
         options={'big_iters': 2, 'outer': 0, 'small_cells': 1, 'tile_h': 1},
         requests=[(1, [2, 3], [0, 2])],
         nodes=6, max_cells=8,
         classes=['generic<4>', 'segments'],
         edges=['generic:lane_ragged']),
    dict(name='21-dag20994n21-sc20-bi2x1',
         recipe=('random_dag_spec', {'seed': 20994, 'n_nodes': 21, 'max_parents': 4, 'cards': (4,), 'max_cells': 4096}),
         options={'big_iters': 2, 'small_cells': 20, 'tile_h': 1},
         requests=[(14, [9, 15], [3, 1])],
         nodes=21, max_cells=65536,
         classes=['fiber<1,cx16,nc1>', 'fiber<1,cx4,nc1>', 'fiber<2,cx16,nc1>', 'generic<1>', 'generic<4>', 'generic<5>', 'segments',
                  've_sweep_kernel'],
         edges=['generic:lane_ragged', 'nc1:big_in_consts', 'nc1:lane_ragged', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'sweep:k2', 'sweep:kout0',
                'sweep:multi_tile', 'sweep:partial_tile', 'sweep:rbits']),
    dict(name='22-dag253604n23-sc32-bi8x3',
         recipe=('random_dag_spec', {'seed': 253604, 'n_nodes': 23, 'max_parents': 3, 'cards': (4, 4, 4, 4, 16, 2, 3), 'max_cells': 4096}),
         options={'big_iters': 8, 'fuse': 0, 'outer': 0, 'small_cells': 32, 'sweep': 0, 'tile_h': 3},
         requests=[(11, [4, 10, 12], [0, 0, 2])],
         nodes=23, max_cells=2048,
         classes=['fiber<1,cx4,ncN>', 'fiber<1,cxN,nc1>', 'fiber<2,cx4,nc16>', 'fiber<2,cxN,nc1>', 'generic<1>', 'generic<3>', 'segments'],
         edges=['generic:lane_ragged', 'generic:partial_tile', 'nc16:big_in_consts', 'nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+',
                'nc16:partial_tile', 'nc1:big_in_consts', 'nc1:lane_ragged', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc1:partial_tile',
                'ncN:big_in_consts', 'ncN:lane_ragged', 'ncN:nctrl0', 'ncN:ns1', 'ncN:ns2+', 'ncN:partial_tile']),
    dict(name='23-dag253604n23-sc32-bi2x1',
         recipe=('random_dag_spec', {'seed': 253604, 'n_nodes': 23, 'max_parents': 3, 'cards': (4, 4, 4, 4, 16, 2, 3), 'max_cells': 4096}),
         options={'big_iters': 2, 'chain': 0, 'fuse': 0, 'small_cells': 32, 'tile_h': 1},
         requests=[(11, [4, 10, 12], [0, 0, 2])],
         nodes=23, max_cells=2048,
         classes=['fiber<1,cx4,ncN>', 'fiber<1,cxN,nc1>', 'fiber<2,cx4,nc16>', 'fiber<2,cxN,nc1>', 'generic<1>', 'generic<3>', 'segments'],
         edges=['generic:lane_ragged', 'nc16:big_in_consts', 'nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc1:big_in_consts', 'nc1:lane_ragged',
                'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'ncN:big_in_consts', 'ncN:lane_ragged', 'ncN:nctrl0', 'ncN:ns1', 'ncN:ns2+']),
    dict(name='24-dag28702n6-sc4-bi2x1',
         recipe=('random_dag_spec', {'seed': 28702, 'n_nodes': 6, 'max_parents': 4, 'cards': (4,), 'max_cells': 4096}),
         options={'big_iters': 2, 'small_cells': 4, 'sweep_min': 3, 'tile_h': 1},
         requests=[(5, [2, 3], [0, 0])],
         nodes=6, max_cells=64,
         classes=['fiber<1,cx16,nc1>', 'fiber<1,cx4,nc1>', 'segments'],
         edges=['nc1:big_in_consts', 'nc1:lane_ragged', 'nc1:nctrl0', 'nc1:ns1', 'nc1:ns2+']),
    dict(name='25-dag295289n10-sc64-bi256x5',
         recipe=('random_dag_spec', {'seed': 295289, 'n_nodes': 10, 'max_parents': 4, 'cards': (4, 4, 4, 2, 3, 5, 8), 'max_cells': 4096}),
         options={'big_iters': 256, 'chain': 0, 'small_cells': 64, 'sweep': 0, 'tile_h': 5},
         requests=[(9, [], []), (9, [4], [1])],
         nodes=10, max_cells=6144,
         classes=['fiber<1,cx4,nc1>', 'fiber<2,cx16,nc16>', 'segments'],
         edges=['nc16:big_in_consts', 'nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc16:partial_tile', 'nc1:big_in_consts', 'nc1:lane_ragged',
                'nc1:nctrl+', 'nc1:ns2+', 'nc1:partial_tile']),
    dict(name='26-dag31647n17-sc16-bi256x5',
         recipe=('random_dag_spec', {'seed': 31647, 'n_nodes': 17, 'max_parents': 4, 'cards': (4,), 'max_cells': 4096}),
         options={'big_iters': 256, 'small_cells': 16, 'sweep': 0, 'tile_h': 5},
         requests=[(6, [3, 12], [1, 3])],
         nodes=17, max_cells=16384,
         classes=['fiber<1,cx4,nc1>', 'fiber<2,cx16,nc16-mfma>', 'fiber<2,cx4,nc1>', 'segments'],
         edges=['fiber<2,cx16,nc16-mfma>:rs1', 'nc16-mfma:big_in_consts', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile',
                'nc1:big_in_consts', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc1:partial_tile']),
    dict(name='27-dag34881n10-sc20-bi4x1',
         recipe=('random_dag_spec', {'seed': 34881, 'n_nodes': 10, 'max_parents': 3, 'cards': (2, 4), 'max_cells': 4096}),
         options={'big_iters': 4, 'outer': 0, 'small_cells': 20, 'tile_h': 1},
         requests=[(8, [4, 5], [2, 1])],
         nodes=10, max_cells=64,
         classes=['fiber<1,cx4,nc1>', 'fiber<2,cx4,nc1>', 'generic<1>', 'generic<6>', 'segments'],
         edges=['generic:lane_ragged', 'nc1:big_in_consts', 'nc1:lane_ragged', 'nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1']),
    dict(name='28-dag45045n24-sc20-bi4x1',
         recipe=('random_dag_spec', {'seed': 45045, 'n_nodes': 24, 'max_parents': 3, 'cards': (2, 3, 4, 5), 'max_cells': 4096}),
         options={'big_iters': 4, 'chain': 0, 'small_cells': 20, 'tile_h': 1},
         requests=[(15, [], []), (10, [], [])],
         nodes=24, max_cells=1536,
         classes=['fiber<1,cx4,nc1>', 'fiber<2,cxN,nc16>', 'fiber<2,cxN,nc1>', 'fiber<2,cxN,nc4>', 'generic<1>', 'segments'],
         edges=['generic:lane_ragged', 'nc16:big_in_consts', 'nc16:c1_ne_c2', 'nc16:cx_not_mult4', 'nc16:lane_ragged', 'nc16:nctrl0', 'nc16:ns2+',
                'nc1:big_in_consts', 'nc1:c1_ne_c2', 'nc1:lane_ragged', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc4:big_in_consts', 'nc4:c1_ne_c2',
                'nc4:cx_not_mult4', 'nc4:lane_ragged', 'nc4:nctrl0', 'nc4:ns2+']),
    dict(name='29-dag60455n6-sc6-bi2x1',
         recipe=('random_dag_spec', {'seed': 60455, 'n_nodes': 6, 'max_parents': 4, 'cards': (2, 4), 'max_cells': 4096}),
         options={'big_iters': 2, 'fuse': 0, 'small_cells': 6, 'sweep_min': 3, 'tile_h': 1},
         requests=[(5, [2, 4], [0, 2])],
         nodes=6, max_cells=16,
         classes=['generic<1>', 'generic<2>', 'generic<5>', 'segments'],
         edges=['generic:lane_ragged']),
    dict(name='30-dag63624n6-sc16-bi64x3',
         recipe=('random_dag_spec', {'seed': 63624, 'n_nodes': 6, 'max_parents': 4, 'cards': (2, 4), 'max_cells': 4096}),
         options={'big_iters': 64, 'fuse': 0, 'small_cells': 16, 'sweep': 0, 'tile_h': 3},
         requests=[(4, [3, 5], [3, 0])],
         nodes=6, max_cells=256,
         classes=['generic<6>', 'segments'],
         edges=['generic:partial_tile']),
    dict(name='31-dag6691n20-sc64-bi4x1',
         recipe=('random_dag_spec', {'seed': 6691, 'n_nodes': 20, 'max_parents': 4, 'cards': (4,), 'max_cells': 4096}),
         options={'big_iters': 4, 'chain': 0, 'fuse': 0, 'outer': 0, 'small_cells': 64, 'tile_h': 1},
         requests=[(17, [6, 18], [3, 2])],
         nodes=20, max_cells=65536,
         classes=['fiber<1,cx4,nc1>', 'fiber<1,cx4,nc4>', 'fiber<1,cx4,ncN>', 'fiber<2,cx4,nc16-mfma>', 'generic<1>', 'generic<3>', 'segments'],
         edges=['fiber<2,cx4,nc16-mfma>:rs1', 'generic:lane_ragged', 'nc16-mfma:big_in_consts', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+',
                'nc1:big_in_consts', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc4:nctrl+', 'nc4:ns1', 'ncN:nctrl+', 'ncN:ns2+']),
    dict(name='32-dag74633n21-sc64-bi2x1',
         recipe=('random_dag_spec', {'seed': 74633, 'n_nodes': 21, 'max_parents': 3, 'cards': (4,), 'max_cells': 4096}),
         options={'big_iters': 2, 'small_cells': 64, 'sweep': 0, 'tile_h': 1},
         requests=[(13, [14, 19], [2, 2])],
         nodes=21, max_cells=1024,
         classes=['fiber<1,cx16,ncN>', 'fiber<1,cx64,chain-mfma>', 'generic<2>', 'segments'],
         edges=['chain:big_in_consts', 'chain:lane_ragged', 'chain:nctrl0', 'chain:ns2+', 'fiber<1,cx64,chain-mfma>:rs16', 'generic:lane_ragged',
                'ncN:lane_ragged', 'ncN:nctrl+', 'ncN:ns2+']),
    dict(name='33-dag81918n15-sc20-bi64x2',
         recipe=('random_dag_spec', {'seed': 81918, 'n_nodes': 15, 'max_parents': 4, 'cards': (2, 4), 'max_cells': 4096}),
         options={'big_iters': 64, 'chain': 0, 'fuse': 0, 'outer': 0, 'small_cells': 20, 'sweep_min': 3, 'tile_h': 2},
         requests=[(11, [5, 7], [2, 1])],
         nodes=15, max_cells=512,
         classes=['fiber<2,cx4,nc16-mfma>', 'segments'],
         edges=['fiber<2,cx4,nc16-mfma>:rs16', 'nc16-mfma:big_in_consts', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl0', 'nc16-mfma:ns2+',
                'nc16-mfma:partial_tile']),
    dict(name='34-dag84812n9-sc16-bi256x0',
         recipe=('random_dag_spec', {'seed': 84812, 'n_nodes': 9, 'max_parents': 4, 'cards': (4,), 'max_cells': 4096}),
         options={'big_iters': 256, 'small_cells': 16, 'sweep_min': 3},
         requests=[(1, [6, 8], [2, 1])],
         nodes=9, max_cells=1024,
         classes=['fiber<1,cx4,nc16-mfma>', 'fiber<1,cx4,nc1>', 'segments'],
         edges=['fiber<1,cx4,nc16-mfma>:rs4', 'nc16-mfma:big_in_consts', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+',
                'nc16-mfma:partial_tile', 'nc1:big_in_consts', 'nc1:nctrl+', 'nc1:ns1', 'nc1:partial_tile']),
    dict(name='35-dag87864n12-sc256-bi64x2',
         recipe=('random_dag_spec', {'seed': 87864, 'n_nodes': 12, 'max_parents': 4, 'cards': (4,), 'max_cells': 4096}),
         options={'big_iters': 64, 'chain': 0, 'outer': 0, 'small_cells': 256, 'tile_h': 2},
         requests=[(10, [], [])],
         nodes=12, max_cells=65536,
         classes=['fiber<1,cx4,nc4>', 'generic<4>', 'segments', 've_sweep_kernel'],
         edges=['nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:k5', 'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+',
                'sweep:partial_tile', 'sweep:rbits', 'sweep:readout5']),
    dict(name='36-mixed5x5s664334-sc32-bi2x1',
         recipe=('mixed_grid_spec', {'R': 5, 'C': 5, 'cards': [4, 2, 4, 4, 4], 'seed': 664334}),
         options={'small_cells': 32, 'big_iters': 2, 'tile_h': 1, 'sweep': 0, 'outer': 0},
         requests=[(9, [0, 3, 24], [3, 3, 1])],
         nodes=25, max_cells=8192,
         classes=['fiber<1,cx4,nc1>', 'fiber<1,cxN,ncN>', 'fiber<2,cx16,nc16>', 'fiber<2,cx16,nc1>', 'fiber<2,cx16,ncN>', 'fiber<2,cx4,nc1>',
                  'generic<1>', 'generic<2>', 'generic<3>', 'segments'],
         edges=['generic:lane_ragged', 'nc16:big_in_consts', 'nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc1:big_in_consts', 'nc1:lane_ragged',
                'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'ncN:big_in_consts', 'ncN:c1_ne_c2', 'ncN:lane_ragged', 'ncN:nctrl+', 'ncN:nctrl0', 'ncN:ns1',
                'ncN:ns2+']),
    dict(name='37-dag684196n21-sc32-bi64x2',
         recipe=('random_dag_spec', {'seed': 684196, 'n_nodes': 21, 'max_parents': 3, 'cards': (4, 4, 4, 16), 'max_cells': 4096}),
         options={'small_cells': 32, 'big_iters': 64, 'tile_h': 2, 'fuse': 0, 'sweep': 0, 'outer': 0},
         requests=[(15, [4, 9, 18], [7, 3, 2])],
         nodes=21, max_cells=1024,
         classes=['fiber<1,cx4,nc1>', 'fiber<1,cxN,nc1>', 'fiber<2,cx4,nc16-mfma>', 'segments'],
         edges=['fiber<2,cx4,nc16-mfma>:rs4', 'nc16-mfma:big_in_consts', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+',
                'nc16-mfma:partial_tile', 'nc1:big_in_consts', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc1:partial_tile']),
    dict(name='38-dag882825n13-sc16-bi8x3',
         recipe=('random_dag_spec', {'seed': 882825, 'n_nodes': 13, 'max_parents': 4, 'cards': (4, 4, 4, 2), 'max_cells': 4096}),
         options={'small_cells': 16, 'big_iters': 8, 'tile_h': 3, 'fuse': 0, 'sweep': 0, 'outer': 0},
         requests=[(12, [3, 6, 9], [1, 3, 1])],
         nodes=13, max_cells=1024,
         classes=['fiber<1,cx4,nc1>', 'fiber<2,cx4,nc16-mfma>', 'fiber<2,cx4,nc1>', 'segments'],
         edges=['fiber<2,cx4,nc16-mfma>:rs4', 'nc16-mfma:big_in_consts', 'nc16-mfma:lane_ragged', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+',
                'nc16-mfma:partial_tile', 'nc1:big_in_consts', 'nc1:lane_ragged', 'nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1',
                'nc1:partial_tile']),
    # the sweep matrix (see the module docstring): roofed grids, sweep_iters and sweep_canon set
    dict(name='39-roof2x7s12857-sc256-bi1024x0-si8',
         recipe=('roof_grid_spec', {'R': 2, 'C': 7, 'cards': [4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 12857}),
         options={'small_cells': 256, 'big_iters': 1024, 'chain': 0, 'outer': 0, 'order_effort': 1},
         requests=[(12, [14], [1])],
         nodes=15, max_cells=65536,
         classes=['fiber<1,cx16,ncN>', 'fiber<1,cx4,ncN>', 'segments', 've_sweep_kernel'],
         edges=['ncN:big_in_consts', 'ncN:nctrl+', 'ncN:ns2+', 'ncN:partial_tile', 'sweep:k3', 'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+',
                'sweep:ns2+', 'sweep:partial_tile', 'sweep:rbits']),
    dict(name='40-roof3x8s54579-sc1024-bi512x0-si1',
         recipe=('roof_grid_spec', {'R': 3, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 54579}),
         options={'big_iters': 512, 'sweep_iters': 1},
         requests=[(22, [24, 18, 10], [1, 1, 3])],
         nodes=25, max_cells=262144,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx16,nc4>', 'fiber<1,cx4,nc4>', 'segments', 've_sweep_kernel'],
         edges=['fiber<1,cx16,nc16-mfma>:rs1', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+',
                'nc4:ns1', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:dead3', 'sweep:dead3+items2+', 'sweep:dead3+one_tile_item', 'sweep:items2+',
                'sweep:k5', 'sweep:kout+', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:one_tile_item', 'sweep:par', 'sweep:rbits']),
    dict(name='41-roof3x8s54579-sc1024-bi512x0-si3',
         recipe=('roof_grid_spec', {'R': 3, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 54579}),
         options={'big_iters': 512, 'sweep_iters': 3},
         requests=[(22, [24, 18, 10], [1, 1, 3])],
         nodes=25, max_cells=262144,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx16,nc4>', 'fiber<1,cx4,nc4>', 'segments', 've_sweep_kernel'],
         edges=['fiber<1,cx16,nc16-mfma>:rs1', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+',
                'nc4:ns1', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:dead3', 'sweep:dead3+items2+', 'sweep:dead3+multi_tile', 'sweep:dead3+partial_tile',
                'sweep:items2+', 'sweep:k5', 'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:par', 'sweep:partial_tile',
                'sweep:rbits']),
    dict(name='42-roof3x8s74180-sc64-bi64x2-si1',
         recipe=('roof_grid_spec', {'R': 3, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 74180}),
         options={'small_cells': 64, 'big_iters': 64, 'tile_h': 2, 'sweep_iters': 1},
         requests=[(16, [24, 18, 23], [0, 1, 1])],
         nodes=25, max_cells=262144,
         classes=['fiber<1,cx16,nc1>', 'fiber<1,cx4,nc4>', 'segments', 've_sweep_kernel'],
         edges=['nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'sweep:dead4',
                'sweep:dead4+items2+', 'sweep:dead4+one_tile_item', 'sweep:items2+', 'sweep:k4', 'sweep:k5', 'sweep:kout+', 'sweep:nctrl2+',
                'sweep:ns2+', 'sweep:one_tile_item', 'sweep:own4', 'sweep:own5', 'sweep:own5+items2+', 'sweep:own5+one_tile_item', 'sweep:par',
                'sweep:rbits']),
    dict(name='43-roof3x8s74180-sc64-bi64x2-si2-any',
         recipe=('roof_grid_spec', {'R': 3, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 74180}),
         options={'small_cells': 64, 'big_iters': 64, 'tile_h': 2, 'sweep_iters': 2, 'sweep_canon': 0},
         requests=[(16, [24, 18, 23], [0, 1, 1])],
         nodes=25, max_cells=262144,
         classes=['fiber<1,cx16,nc1>', 'fiber<1,cx4,nc4>', 'segments', 've_sweep_kernel'],
         edges=['nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'sweep:any',
                'sweep:items2+', 'sweep:k4', 'sweep:k5', 'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:par', 'sweep:rbits']),
    dict(name='44-roof3x8s74180-sc64-bi64x2-si3',
         recipe=('roof_grid_spec', {'R': 3, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 74180}),
         options={'small_cells': 64, 'big_iters': 64, 'tile_h': 2, 'sweep_iters': 3},
         requests=[(16, [24, 18, 23], [0, 1, 1])],
         nodes=25, max_cells=262144,
         classes=['fiber<1,cx16,nc1>', 'fiber<1,cx4,nc4>', 'segments', 've_sweep_kernel'],
         edges=['nc1:nctrl+', 'nc1:nctrl0', 'nc1:ns0', 'nc1:ns1', 'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'sweep:dead4',
                'sweep:dead4+items2+', 'sweep:dead4+multi_tile', 'sweep:dead4+partial_tile', 'sweep:items2+', 'sweep:k4', 'sweep:k5', 'sweep:kout+',
                'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:own4', 'sweep:own5', 'sweep:own5+items2+', 'sweep:own5+multi_tile',
                'sweep:own5+partial_tile', 'sweep:par', 'sweep:partial_tile', 'sweep:rbits']),
    dict(name='45-roof3x8s84521-sc1024-bi64x0-si1',
         recipe=('roof_grid_spec', {'R': 3, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 84521}),
         options={'big_iters': 64, 'outer': 0, 'sweep_iters': 1},
         requests=[(21, [24, 12, 22], [0, 0, 2])],
         nodes=25, max_cells=262144,
         classes=['fiber<1,cx4,nc1>', 'fiber<1,cx4,nc4>', 'fiber<1,cx64,chain-mfma>', 'generic<1>', 'segments', 've_sweep_kernel'],
         edges=['chain:nctrl+', 'chain:ns2+', 'chain:partial_tile', 'fiber<1,cx64,chain-mfma>:rs1', 'generic:partial_tile', 'nc1:nctrl0', 'nc1:ns0',
                'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:dead1', 'sweep:dead1+items2+',
                'sweep:dead1+one_tile_item', 'sweep:dead3', 'sweep:dead3+items2+', 'sweep:dead3+one_tile_item', 'sweep:items2+', 'sweep:k5',
                'sweep:kout+', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:one_tile_item', 'sweep:par', 'sweep:rbits']),
    dict(name='46-roof3x8s84521-sc1024-bi64x0-si3',
         recipe=('roof_grid_spec', {'R': 3, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 84521}),
         options={'big_iters': 64, 'outer': 0, 'sweep_iters': 3},
         requests=[(21, [24, 12, 22], [0, 0, 2])],
         nodes=25, max_cells=262144,
         classes=['fiber<1,cx4,nc1>', 'fiber<1,cx4,nc4>', 'fiber<1,cx64,chain-mfma>', 'generic<1>', 'segments', 've_sweep_kernel'],
         edges=['chain:nctrl+', 'chain:ns2+', 'chain:partial_tile', 'fiber<1,cx64,chain-mfma>:rs1', 'generic:partial_tile', 'nc1:nctrl0', 'nc1:ns0',
                'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:dead1', 'sweep:dead1+items2+',
                'sweep:dead1+multi_tile', 'sweep:dead1+partial_tile', 'sweep:dead3', 'sweep:dead3+multi_tile', 'sweep:dead3+partial_tile',
                'sweep:items2+', 'sweep:k5', 'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:par', 'sweep:partial_tile',
                'sweep:rbits']),
    dict(name='47-roof4x7s74590-sc16-bi64x2-si8',
         recipe=('roof_grid_spec', {'R': 4, 'C': 7, 'cards': [4, 4, 4, 4, 4, 4, 3], 'roof_card': 4, 'seed': 74590}),
         options={'small_cells': 16, 'big_iters': 64, 'tile_h': 2, 'sweep': 3},
         requests=[(24, [28, 10, 16], [2, 1, 2])],
         nodes=29, max_cells=65536,
         classes=['fiber<1,cx4,nc1>', 'fiber<1,cx4,nc4>', 'fiber<1,cxN,nc1>', 'fiber<2,cx16,nc1>', 'fiber<2,cx16,ncN>', 'generic<3>', 'segments',
                  've_sweep_kernel'],
         edges=['nc1:big_in_consts', 'nc1:c1_ne_c2', 'nc1:nctrl+', 'nc1:ns1', 'nc1:ns2+', 'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:lane_ragged',
                'nc4:nctrl0', 'nc4:ns1', 'nc4:partial_tile', 'ncN:big_in_consts', 'ncN:nctrl+', 'ncN:ns2+', 'ncN:partial_tile', 'sweep:k2',
                'sweep:kout0', 'sweep:multi_tile', 'sweep:partial_tile', 'sweep:rbits']),
    dict(name='48-roof4x8s4165-sc64-bi1024x0-si2',
         recipe=('roof_grid_spec', {'R': 4, 'C': 8, 'cards': [4, 4, 4, 4, 3, 2, 4, 4], 'roof_card': 2, 'seed': 4165}),
         options={'big_iters': 1024, 'small_cells': 64, 'order_effort': 1, 'chain': 0, 'outer': 0, 'sweep_iters': 2},
         requests=[(30, [32, 26], [1, 0])],
         nodes=33, max_cells=294912,
         classes=['fiber<1,cx16,nc16>', 'fiber<1,cx16,nc4>', 'fiber<1,cx4,nc4>', 'fiber<1,cxN,ncN>', 'segments', 've_sweep_kernel'],
         edges=['nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc16:partial_tile', 'nc4:big_in_consts', 'nc4:lane_ragged', 'nc4:nctrl+', 'nc4:ns2+',
                'nc4:partial_tile', 'ncN:c1_ne_c2', 'ncN:cx_not_mult4', 'ncN:nc_not_pow2', 'ncN:nctrl+', 'ncN:nctrl0', 'ncN:ns2+', 'ncN:partial_tile',
                'sweep:dead4', 'sweep:dead4+items2+', 'sweep:dead4+multi_tile', 'sweep:dead4+one_tile_item', 'sweep:dead4+partial_tile',
                'sweep:items2+', 'sweep:k5', 'sweep:kout+', 'sweep:multi_tile', 'sweep:odd_tiles', 'sweep:one_tile_item', 'sweep:partial_tile']),
    dict(name='49-roof4x8s4187-sc256-bi256x0-si2',
         recipe=('roof_grid_spec', {'R': 4, 'C': 8, 'cards': [4, 2, 3, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 4187}),
         options={'big_iters': 256, 'small_cells': 256, 'order_effort': 1, 'chain': 0, 'outer': 0, 'sweep_iters': 2},
         requests=[(25, [32, 31], [1, 3])],
         nodes=33, max_cells=393216,
         classes=['fiber<1,cx16,nc16>', 'fiber<1,cx16,ncN>', 'fiber<1,cx4,nc4>', 'fiber<1,cxN,nc1>', 'fiber<1,cxN,ncN>', 'segments', 've_sweep_kernel'],
         edges=['nc16:lane_ragged', 'nc16:nctrl+', 'nc16:ns2+', 'nc16:partial_tile', 'nc1:cx_not_mult4', 'nc1:nctrl0', 'nc1:ns0', 'nc1:partial_tile',
                'nc4:big_in_consts', 'nc4:lane_ragged', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile', 'ncN:c1_ne_c2', 'ncN:cx_not_mult4',
                'ncN:lane_ragged', 'ncN:nc_not_pow2', 'ncN:nctrl+', 'ncN:ns2+', 'ncN:partial_tile', 'sweep:items2+', 'sweep:k4', 'sweep:k5',
                'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:odd_tiles', 'sweep:one_tile_item', 'sweep:own4',
                'sweep:own5', 'sweep:own5+items2+', 'sweep:own5+multi_tile', 'sweep:own5+one_tile_item', 'sweep:own5+partial_tile', 'sweep:par',
                'sweep:partial_tile', 'sweep:rbits', 'sweep:readout4']),
    dict(name='50-roof4x8s6089-sc1024-bi64x0-si1',
         recipe=('roof_grid_spec', {'R': 4, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 4, 'seed': 6089}),
         options={'big_iters': 64, 'chain': 0, 'outer': 0, 'order_effort': 1, 'sweep_iters': 1},
         requests=[(30, [32, 11], [2, 3])],
         nodes=33, max_cells=262144,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx4,nc4>', 'generic<1>', 'segments', 've_sweep_kernel'],
         edges=['fiber<1,cx16,nc16-mfma>:rs1', 'generic:partial_tile', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile',
                'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:dead2', 'sweep:dead2+items2+', 'sweep:dead2+one_tile_item',
                'sweep:dead3', 'sweep:dead3+items2+', 'sweep:dead3+one_tile_item', 'sweep:items2+', 'sweep:k5', 'sweep:kout+', 'sweep:nctrl2+',
                'sweep:ns2+', 'sweep:one_tile_item', 'sweep:own5', 'sweep:own5+items2+', 'sweep:own5+one_tile_item', 'sweep:par', 'sweep:rbits',
                'sweep:readout5']),
    dict(name='51-roof4x8s6089-sc1024-bi64x0-si3',
         recipe=('roof_grid_spec', {'R': 4, 'C': 8, 'cards': [4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 4, 'seed': 6089}),
         options={'big_iters': 64, 'chain': 0, 'outer': 0, 'order_effort': 1, 'sweep_iters': 3},
         requests=[(30, [32, 11], [2, 3])],
         nodes=33, max_cells=262144,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx4,nc4>', 'generic<1>', 'segments', 've_sweep_kernel'],
         edges=['fiber<1,cx16,nc16-mfma>:rs1', 'generic:partial_tile', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile',
                'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:dead2', 'sweep:dead2+items2+', 'sweep:dead2+multi_tile',
                'sweep:dead2+partial_tile', 'sweep:dead3', 'sweep:dead3+multi_tile', 'sweep:dead3+partial_tile', 'sweep:items2+', 'sweep:k5',
                'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:own5', 'sweep:own5+multi_tile', 'sweep:own5+partial_tile',
                'sweep:par', 'sweep:partial_tile', 'sweep:rbits', 'sweep:readout5']),
    dict(name='52-roof5x7s3039-sc1024-bi1024x0-si1',
         recipe=('roof_grid_spec', {'R': 5, 'C': 7, 'cards': [4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 3039}),
         options={'big_iters': 1024, 'sweep_iters': 1},
         requests=[(34, [35], [1])],
         nodes=36, max_cells=65536,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx16,nc4>', 'fiber<1,cx4,ncN>', 'fiber<1,cx64,chain-mfma>', 'generic<2>', 'segments',
                  've_sweep_kernel'],
         edges=['chain:nctrl+', 'chain:nctrl0', 'chain:ns2+', 'fiber<1,cx16,nc16-mfma>:rs16', 'fiber<1,cx64,chain-mfma>:rs1',
                'fiber<1,cx64,chain-mfma>:rs16', 'generic:partial_tile', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile', 'nc4:nctrl0',
                'nc4:ns1', 'nc4:partial_tile', 'ncN:big_in_consts', 'ncN:nctrl+', 'ncN:ns2+', 'ncN:partial_tile', 'sweep:dead1',
                'sweep:dead1+items2+', 'sweep:dead1+one_tile_item', 'sweep:items2+', 'sweep:k5', 'sweep:kout+', 'sweep:nctrl2+', 'sweep:ns2+',
                'sweep:one_tile_item', 'sweep:par', 'sweep:par_tail', 'sweep:rbits']),
    dict(name='53-roof5x7s3039-sc1024-bi1024x0-si2',
         recipe=('roof_grid_spec', {'R': 5, 'C': 7, 'cards': [4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 3039}),
         options={'big_iters': 1024, 'sweep_iters': 2},
         requests=[(34, [35], [1])],
         nodes=36, max_cells=65536,
         classes=['fiber<1,cx16,nc16-mfma>', 'fiber<1,cx16,nc4>', 'fiber<1,cx4,ncN>', 'fiber<1,cx64,chain-mfma>', 'generic<2>', 'segments',
                  've_sweep_kernel'],
         edges=['chain:nctrl+', 'chain:nctrl0', 'chain:ns2+', 'fiber<1,cx16,nc16-mfma>:rs16', 'fiber<1,cx64,chain-mfma>:rs1',
                'fiber<1,cx64,chain-mfma>:rs16', 'generic:partial_tile', 'nc16-mfma:nctrl+', 'nc16-mfma:ns2+', 'nc16-mfma:partial_tile', 'nc4:nctrl0',
                'nc4:ns1', 'nc4:partial_tile', 'ncN:big_in_consts', 'ncN:nctrl+', 'ncN:ns2+', 'ncN:partial_tile', 'sweep:dead1',
                'sweep:dead1+multi_tile', 'sweep:k5', 'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:par', 'sweep:par_tail',
                'sweep:rbits']),
    dict(name='54-roof4x9s2002-sc1024-bi512x0-si8',
         recipe=('roof_grid_spec', {'R': 4, 'C': 9, 'cards': [4, 4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 2002}),
         options={'big_iters': 512, 'order_effort': 1},
         requests=[(27, [36, 35], [0, 1])],
         nodes=37, max_cells=1048576,
         classes=['fiber<1,cx16,nc1>', 'fiber<1,cx4,nc1>', 'fiber<1,cx4,nc4>', 'segments', 've_sweep_kernel'],
         edges=['nc1:nctrl0', 'nc1:ns0', 'nc1:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns2+', 'nc4:partial_tile', 'sweep:items2+',
                'sweep:k2', 'sweep:k4', 'sweep:k5', 'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:own4', 'sweep:own5',
                'sweep:own5+items2+', 'sweep:own5+multi_tile', 'sweep:par', 'sweep:rbits']),
    dict(name='55-roof4x9s2002-sc256-bi64x0-si1',
         recipe=('roof_grid_spec', {'R': 4, 'C': 9, 'cards': [4, 4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 2002}),
         options={'big_iters': 64, 'small_cells': 256, 'sweep_iters': 1},
         requests=[(31, [36, 5], [1, 2])],
         nodes=37, max_cells=262144,
         classes=['fiber<1,cx16,nc4>', 'fiber<1,cx4,nc4>', 'fiber<1,cx64,chain-mfma>', 'generic<1>', 'segments', 've_sweep_kernel'],
         edges=['chain:lane_ragged', 'chain:nctrl+', 'chain:ns2+', 'chain:partial_tile', 'fiber<1,cx64,chain-mfma>:rs1',
                'fiber<1,cx64,chain-mfma>:rs4', 'generic:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns1', 'nc4:ns2+', 'nc4:partial_tile',
                'sweep:dead0', 'sweep:dead0+items2+', 'sweep:dead0+one_tile_item', 'sweep:items2+', 'sweep:k5', 'sweep:kout+', 'sweep:nctrl2+',
                'sweep:ns2+', 'sweep:one_tile_item', 'sweep:par', 'sweep:rbits', 'sweep:readout5']),
    dict(name='56-roof4x9s2002-sc256-bi64x0-si3',
         recipe=('roof_grid_spec', {'R': 4, 'C': 9, 'cards': [4, 4, 4, 4, 4, 4, 4, 4, 4], 'roof_card': 2, 'seed': 2002}),
         options={'big_iters': 64, 'small_cells': 256, 'sweep_iters': 3},
         requests=[(31, [36, 5], [1, 2])],
         nodes=37, max_cells=262144,
         classes=['fiber<1,cx16,nc4>', 'fiber<1,cx4,nc4>', 'fiber<1,cx64,chain-mfma>', 'generic<1>', 'segments', 've_sweep_kernel'],
         edges=['chain:lane_ragged', 'chain:nctrl+', 'chain:ns2+', 'chain:partial_tile', 'fiber<1,cx64,chain-mfma>:rs1',
                'fiber<1,cx64,chain-mfma>:rs4', 'generic:partial_tile', 'nc4:big_in_consts', 'nc4:nctrl+', 'nc4:ns1', 'nc4:ns2+', 'nc4:partial_tile',
                'sweep:dead0', 'sweep:dead0+items2+', 'sweep:dead0+multi_tile', 'sweep:dead0+partial_tile', 'sweep:items2+', 'sweep:k5',
                'sweep:kout+', 'sweep:multi_tile', 'sweep:nctrl2+', 'sweep:ns2+', 'sweep:par', 'sweep:partial_tile', 'sweep:rbits', 'sweep:readout5']),
]

# The edges of step_edges every family of tiled FIBER classes must show somewhere in the table ...
FIBER_EDGES = ("partial_tile", "lane_ragged", "nctrl0", "nctrl+", "ns0", "ns1", "ns2+", "cx_not_mult4", "c1_ne_c2", "nc_not_pow2", "big_in_consts")
REQUIRED_EDGES = {
    "generic": ["lane_ragged", "partial_tile"],
    "nc1": ["big_in_consts", "c1_ne_c2", "cx_not_mult4", "lane_ragged", "nctrl+", "nctrl0", "ns0", "ns1", "ns2+", "partial_tile"],
    "nc4": ["big_in_consts", "c1_ne_c2", "cx_not_mult4", "lane_ragged", "nctrl+", "nctrl0", "ns1", "ns2+", "partial_tile"],
    "nc16": ["big_in_consts", "c1_ne_c2", "cx_not_mult4", "lane_ragged", "nctrl+", "nctrl0", "ns1", "ns2+", "partial_tile"],
    "ncN": ["big_in_consts", "c1_ne_c2", "cx_not_mult4", "lane_ragged", "nc_not_pow2", "nctrl+", "nctrl0", "ns1", "ns2+", "partial_tile"],
    "nc16-mfma": ["big_in_consts", "lane_ragged", "nctrl+", "nctrl0", "ns1", "ns2+", "partial_tile"],
    "outer-mfma": ["big_in_consts", "lane_ragged", "nctrl+", "nctrl0", "ns0", "ns1", "ns2+", "partial_tile"],
    "chain": ["big_in_consts", "lane_ragged", "nctrl+", "nctrl0", "ns1", "ns2+", "partial_tile"],
    # SWEEP: the sweep matrix.  Every specialisation ve_sweep_dma_kernel dispatches to (SWEEP_SHAPES), every form of a stage
    # (SWEEP_STAGES) and every shape of the tile loop (SWEEP_ITEMS), and each wave-owned tail (SWEEP_TAILS) crossed with the shapes of
    # the tile loop: work items of one, two and three tiles, several of them, the last one shorter.  The C3 tests run most of the
    # shapes as well, on whole work items only (test_the_c3_census_of_sweep_shapes).
    "sweep": ["k4", "k5", "kout0", "kout+", *SWEEP_SHAPES, *SWEEP_STAGES, *SWEEP_STEP, *[e for e in SWEEP_ITEMS if e != "one_tile_step"],
              *[f"{t}+{e}" for t in SWEEP_TAILS for e in SWEEP_ITEMS if e != "one_tile_step"]],
}
SWEEP_EDGES = ("k4", "k5", "kout0", "kout+", *SWEEP_SHAPES, *SWEEP_STAGES, *SWEEP_STEP, *SWEEP_ITEMS, *[f"{t}+{e}" for t in SWEEP_TAILS for e in SWEEP_ITEMS])
# ... and why a family lacks the others (the condition of emit_core.h that excludes the shape)
_NO_NS0 = "N axes are output axes no big input depends on, so only a small input brings them: ns = 0 means nN = 0 and NC = 1 (emit_fiber)"
_CX_4_16 = "fiber_cx_class(w) < 2 / `if (!((cx == 4 && c1 == 4) || (cx == 16 && c1 == 4))) return false;`: cx is 4 or 4 x 4"
_POW2 = "NC is 1, 4 or 16 by the definition of the class (fiber_nc_class)"
_TWO_TILES = ("emit_core.h, the SWEEP candidates of emit_program: `if (nbig == 1 && !(bigf->off & kConstFlag) && bigf->cells >= 16 * (int64_t)net.big_iters && "
              "bigf->cells >= 2 * kSweepTileCells) {` - the big input of a SWEEP step has at least two tiles")
IMPOSSIBLE_EDGES = {
    "nc1": {"nc_not_pow2": _POW2},
    "nc4": {"ns0": _NO_NS0, "nc_not_pow2": _POW2},
    "nc16": {"ns0": _NO_NS0, "nc_not_pow2": _POW2},
    "ncN": {"ns0": _NO_NS0},
    "nc16-mfma": {"ns0": _NO_NS0, "cx_not_mult4": _CX_4_16, "c1_ne_c2": _CX_4_16, "nc_not_pow2": _POW2},
    "outer-mfma": {"cx_not_mult4": _CX_4_16, "c1_ne_c2": _CX_4_16, "nc_not_pow2": _POW2},
    "chain": {"ns0": "emit_chain_as: `if (nn12 != 2 || nax3 < 0) return false;` - the two N axes of the pair table are axes a pair-group small input depends on",
              "cx_not_mult4": "emit_chain_as: `if (net.card[out.vars[a]] != 4) return false;` and three 4-state variables: cx = 64",
              "c1_ne_c2": "the same: all three eliminated variables have four states", "nc_not_pow2": "NC = 16 (x 4 in registers)"},
    "sweep": {e: _TWO_TILES for e in ("one_tile_step", *[f"{t}+one_tile_step" for t in SWEEP_TAILS])},
}
# The row stride of the MFMA forms (w1 bits 20..27): both classes of ve_mfma_kernel, CHAIN, both two-table pair classes and both
# OUTER classes at 1, 4 and 16.
REQUIRED_ROW_STRIDES = [f"{c}:rs{r}" for c in (*MFMA1, CHAIN, "fiber<2,cx4,nc16-mfma>", "fiber<2,cx16,nc16-mfma>", "fiber<2,cx4,outer-mfma>",
                                              "fiber<2,cx16,outer-mfma>") for r in (1, 4, 16)]

# Names of kernel_name() no program can carry, each with the line of emit_core.h that rules it out.  (A sixth specialisation,
# <2,cxN,outer-mfma>, is ruled out by the same line of emit_outer as below; it has no name - CHAIN took its id, kKidChain = 36.)
_OUTER_2 = "emit_outer: `if (nbig != 2 || ns > kMaxSmall) return false;` - kFlagOuter is only ever set by emit_outer, which writes n_big = 2 (`w[7] = 2u | ...`)"
_MFMA_CX = "fiber_nc_class: `if (NC == 16 && ((w[1] >> kRowStrideShift) & 0xff) && fiber_cx_class(w) < 2) return 4;` - the row form needs cx 4 or 4 x 4"
UNREACHABLE = [
    ("fiber<1,cx4,outer-mfma>", _OUTER_2),
    ("fiber<1,cx16,outer-mfma>", _OUTER_2),
    ("fiber<1,cxN,outer-mfma>", _OUTER_2),
    ("fiber<1,cxN,nc16-mfma>", _MFMA_CX),
    ("fiber<2,cxN,nc16-mfma>", _MFMA_CX),
    (None, "<2,cxN,outer-mfma>: emit_outer `if (!((cx == 4 && c1 == 4) || (cx == 16 && c1 == 4))) return false;`"),
]
# The three classes fiber<2,cx4,nc16>, fiber<2,cx16,nc16> and fiber<2,cxN,nc16> ARE emitted, with OUTER on as well as off: emit_outer
# wants two 4-state output axes that ONE of the big tables owns, emit_fiber takes N axes that NEITHER big table depends on, and the VALU
# nc16 class is what remains when the MFMA row form is refused (`if (inside > 1 || !ok) row_stride = 0;` - a ctrl axis of another
# cardinality than 4, or two of them, inside a wave's 64 cells) or cx is neither 4 nor 4 x 4.  Mixed cardinalities (4 with 2 or 16)
# reach them on tables of 2 048 to 6 144 cells; the cases below hold two witnesses of each.

# The classes the planner writes for tests/golden/huge_cards.json under the option sets of test_golden_huge_cardinalities and the
# engine's defaults, as (small_cells, tiling, fuse) -> sorted names: asserted on the CPU by test_census_of_the_golden_gpu_inputs and
# on the device by test_golden_huge_cardinalities.
HUGE_CARDS_CLASSES = {
    (1024, (4096, 0), 1): ['generic<4>', 'segments'],
    (1, (2, 1), 1): ['fiber<2,cxN,nc1>', 'generic<1>', 'generic<2>', 'generic<3>', 'generic<4>', 'segments'],
    (6, (8, 3), 1): ['fiber<1,cxN,nc1>', 'fiber<2,cxN,nc1>', 'fiber<2,cxN,ncN>', 'generic<1>', 'generic<2>', 'generic<3>', 'generic<4>', 'segments'],
    (1, (2, 1), 0): ['fiber<2,cxN,nc1>', 'generic<1>', 'generic<2>', 'generic<3>', 'generic<4>', 'segments'],
}
