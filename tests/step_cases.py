"""The step matrix: pinned small inputs that take the level kernels of the step-wise program kinds - ve_max_kernel, ve_sum_kernel
(draw programs) and ve_map_kernel of csrc/elim_kernel.hip.h, all of them elim_level<M> over generic_body<NIN, MAXC, 0, LANES, MAX>
of ve_kernel.hip.h - and their tracebacks through every shape of step at which that body differs.  Data and small helpers - no test
lives here.  tests/test_step_classes_host.py proves every case on the planner's own programs and on the host twin tools/prog_sim.cpp
(CPU); tests/test_step_classes.py runs them on the device.  The sum path's table of the same kind is tests/class_cases.py.

A case is
    recipe    (netspec function name, keyword arguments)
    options   small_cells, big_iters, tile_h: the engine options that shape the schedule (and, through the order search, the
              program); the same values go to the simulator, to prog_sim and to the engine
    kind      "max" (mibn_mpe_batch), "map" (mibn_map_batch) or "draw" (mibn_posterior_sample_batch)
    requests  dictionaries: ev, ec - evidence nodes and codes; M, prune - a map request's variables and whether the case's programs
              are the pruned ones (MIBN_MAP_PRUNE; the device test runs both); n - a draw request's samples.  Nodes by the integer
              of their name ("007" -> 7).
    seed      draw: the seed of the call
    edges     the tags its programs contain, all of them: per step "<path>:<edge>" (step_edges; NUMERIC_STEP_TAGS from the answers),
              per case CASE_TAGS
The cases are the cheapest witnesses a random search over netspec recipes, option sets and requests found, chosen greedily so that
every tag of REQUIRED is covered; the host test proves each, whatever found it.  Every network but the two of 70 variables has a joint
of at most 2^20 states: the dense twins enumerate it.
"""
import os
import sys

import numpy as np

import class_cases as cc
import netspec
import sim_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))  # dump_plan

OPTION_NAMES = ("small_cells", "big_iters", "tile_h")
DEFAULTS = dict(small_cells=1024, big_iters=4096, tile_h=0)
KINDS = ("max", "map", "draw")
PATHS = ("seg", "tile")
MAX_JOINT = 2 ** 20  # the limit of test_mpe.py's brute-force cases

# what step_edges can say of a step, per path ...
STEP_TAGS = ("n_in1", "n_in2", "n_in3", "n_in4", "n_in5", "n_in6", "hi1", "lo1", "cx1", "cx2", "cx4", "cx_not_pow2", "cx_gt_255",
             "max", "sum", "max_unflagged", "const_in")
PATH_TAGS = {"tile": ("partial_tile", "lane_ragged", "lo_le_256"), "seg": ("passes2+", "hi_gt_64")}
# ... and what a case as a whole can show
# ... what the numbers add to a step: a MAX step of cx > 255 on that path, and a code above 255 in the answer (the traceback read an
# argmax entry whose second byte is not zero)
NUMERIC_STEP_TAGS = ("argmax_gt_255",)
CASE_TAGS = ("tie", "zero_mass", "map_seg_mixed", "map_tile_sum", "map_tile_max", "gather_gt_64", "nvars_gt_64")


def step_edges(step, tiled, tile_h, flagged, kind="max"):
    """Edge tags "<path>:<edge>" of one decoded GENERIC step (tools/dump_plan.py decode) of a `kind` program: path "tile" (a level of
    its own, `tile_h` hi iterations per workgroup: generic_body with LANES = kWG = 256) or "seg" (a step of a segment, one wave:
    LANES = 64); flagged: the step carries kFlagMax."""
    path, out = ("tile" if tiled else "seg"), set()
    add = lambda e: out.add(f"{path}:{e}")
    lo, hi, n_in, cx = step["lo"], step["hi"], step["n_in"], step["cx"]
    add(f"n_in{min(max(n_in, 1), 6)}")        # generic_dispatch: one body per n_in, two cells per lane up to 3 inputs (M3), one beyond (M6)
    if tiled:
        if hi % tile_h:
            add("partial_tile")               # the last workgroup of the step takes fewer hi iterations than the others
        if lo % 256:
            add("lane_ragged")                # lanes of the workgroup without a cell in their last (or only) row of 256
        if lo <= 256:
            add("lo_le_256")                  # at two cells per lane the second cell of every lane is idle
    else:
        if lo > (128 if n_in <= 3 else 64):
            add("passes2+")                   # one wave covers the lane block in more than one pass
        if hi > 64:
            add("hi_gt_64")                   # the h0 loop of generic_body repeats: more than kTileMax offsets
    if step["nlo"] == step["na"]:
        add("hi1")                            # no wave-uniform axis at all
    if lo == 1:
        add("lo1")
    if cx <= 1:
        add("cx1")                            # product only
    elif cx in (2, 4):
        add(f"cx{cx}")                        # (the sum body has compile-time loops for these; the max body has one loop)
    elif cx & (cx - 1):
        add("cx_not_pow2")
    if cx > 255:
        add("cx_gt_255")                      # an argmax entry needs its second byte
    add("max" if flagged else "max_unflagged" if kind == "max" else "sum")  # max_unflagged: MAX = true, amp null
    if any(t == "C" for t, _ in step["ins"]):
        add("const_in")                       # an input in the constants pool (a CPT), not in the arena
    return out


def build_spec(case):
    fn, kw = case["recipe"]
    kw = dict(kw)
    if fn == "random_dag_spec":
        kw.setdefault("p_zero", 0.0)
        kw.update(p_missing=0.0)
    return getattr(netspec, fn)(**kw)


def options(case):
    return {**DEFAULTS, **case["options"]}


def set_sim_options(opt):
    """The case's options on the simulator (process-wide), on top of what an engine plans with (sim_tools.ENGINE_PLANNING)."""
    import ctypes as C
    import simengine
    L = simengine.lib()
    cc.set_sim_options({**cc.DEFAULTS, **opt, "order_effort": sim_tools.ENGINE_PLANNING["order_effort"]})
    L.plan_sim_set_order_effort(sim_tools.ENGINE_PLANNING["order_effort"], sim_tools.ENGINE_PLANNING["second_above"])
    L.plan_sim_set_minfill_above.argtypes = [C.c_double]
    L.plan_sim_set_minfill_above(sim_tools.ENGINE_PLANNING["minfill_above"])


def reset_sim_options():
    import ctypes as C
    import simengine
    L = simengine.lib()
    L.plan_sim_set_minfill_above.argtypes = [C.c_double]
    L.plan_sim_set_minfill_above(-1.0)
    cc.reset_sim_options()


def ids(flat, nodes):
    return [int(flat.id[f"{int(v):03d}"]) for v in nodes]


def steps_of(flat, kind, rq):
    """The decoded steps of one request's program under the simulator's options, each with `tiled` and `tile_h` from the schedule."""
    import dump_plan as dp
    w, th = dp.program_kind(flat, kind, ids(flat, rq.get("M", [])), ids(flat, rq["ev"]), rq["ec"], no_prune=(kind != "max" and not rq.get("prune", 0)))
    steps = dp.decode(w)
    assert all(s["kind"] == "GENERIC" for s in steps)
    for s, t in zip(steps, th):
        s["tile_h"], s["tiled"] = t, t > 0
    return steps


def planned(flat, kind, requests):
    """The structural tags of the programs of `requests` under the simulator's options: step_edges of every step, and of CASE_TAGS
    those that follow from the programs alone (the others - tie, zero_mass - need the numbers)."""
    edges = set()
    for rq in requests:
        steps = steps_of(flat, kind, rq)
        seg = set()  # what the segment the walk is in has held so far
        for s in steps:
            edges |= step_edges(s, s["tiled"], s["tile_h"], bool(s["max"]), kind)
            if kind == "map":
                what = "max" if s["max"] else "sum" if s["cx"] > 1 else None
                if s["tiled"]:
                    seg = set()
                    if what:
                        edges.add(f"map_tile_{what}")
                elif what:
                    seg.add(what)
                    if seg == {"max", "sum"}:
                        edges.add("map_seg_mixed")
        if kind == "map" and len(rq["M"]) > 64:
            edges.add("gather_gt_64")   # map_traceback_kernel: the k += kTracebackWG loop over the gather list takes a second trip
        if kind == "max" and len(flat.card) > 64:
            edges.add("nvars_gt_64")    # mpe_traceback_kernel: the same of its store loop over n_vars
    return edges


def traceback_order(flat, kind, rq):
    """The variables the MAX steps of one request's max / map program eliminate, last eliminated first: the x of the entries of its
    traceback record (planner.h: n_rec, n_ev, (variable, code) x n_ev, then per entry argmax off lo, hi, x, n_out, (variable, stride) x
    n_out).  "The lowest maximising x" of every step makes the decoded assignment the first of all maximisers in the lexicographic
    order that ranks these variables in this order - what the exact-tie cases hold the twin to."""
    import dump_plan as dp
    w, _ = dp.program_kind(flat, kind, ids(flat, rq.get("M", [])), ids(flat, rq["ev"]), rq["ec"], no_prune=(kind != "max" and not rq.get("prune", 0)))
    p = 1
    for _ in range(int(w[0])):
        p += int(w[p + 6])
    n_rec, n_ev = int(w[p]), int(w[p + 1])
    p += 2 + 2 * n_ev
    order = []
    for _ in range(n_rec):
        order.append(int(w[p + 2]))
        p += 4 + 2 * int(w[p + 3])
    return order


def first_maximiser(table, axes, order):
    """Of the cells of `table` (axes: its variables) that hold its maximum exactly, the first in the lexicographic order that ranks the
    variables as `order` does (variables of `axes` that `order` lacks have one state) -> {variable: code}."""
    cells = np.argwhere(table == table.max())
    rank = [axes.index(v) for v in order if v in axes] + [i for i, v in enumerate(axes) if v not in order]
    best = min(cells.tolist(), key=lambda c: [c[i] for i in rank])
    return dict(zip(axes, best))


def evidence(flat, rq):
    return dict(zip(ids(flat, rq["ev"]), (int(c) for c in rq["ec"])))


CASES = [
    dict(name='00-map-hub93924-bi8x3',
         recipe=('hub_spec', {'seed': 93924, 'hub_card': 5, 'parent_cards': [2, 2], 'child_cards': [5, 5, 4, 3, 4, 4]}),
         options={'big_iters': 8, 'tile_h': 3}, kind='map', nodes=9,
         requests=[{'ev': [], 'ec': [], 'M': [4, 3, 7, 1, 5], 'prune': 0}],
         edges=['map_tile_max', 'map_tile_sum', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx4', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1',
                'seg:n_in2', 'seg:sum', 'tile:const_in', 'tile:cx1', 'tile:cx2', 'tile:cx4', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256',
                'tile:max', 'tile:n_in1', 'tile:n_in2', 'tile:n_in6', 'tile:partial_tile', 'tile:sum']),
    dict(name='01-max-hub32556-bi2x3',
         recipe=('hub_spec', {'seed': 32556, 'hub_card': 600, 'parent_cards': [4, 2], 'child_cards': [2, 3]}),
         options={'big_iters': 2, 'tile_h': 3}, kind='max', nodes=5,
         requests=[{'ev': [], 'ec': []}, {'ev': [0], 'ec': [2]}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'seg:n_in2', 'tile:argmax_gt_255',
                'tile:const_in', 'tile:cx2', 'tile:cx4', 'tile:cx_gt_255', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo1', 'tile:lo_le_256',
                'tile:max', 'tile:n_in1', 'tile:n_in2', 'tile:n_in3', 'tile:partial_tile']),
    dict(name='02-draw-hub32556-bi2x3',
         recipe=('hub_spec', {'seed': 32556, 'hub_card': 600, 'parent_cards': [4, 2], 'child_cards': [2, 3]}),
         options={'big_iters': 2, 'tile_h': 3}, kind='draw', seed=1, nodes=5,
         requests=[{'ev': [], 'ec': [], 'n': 300}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:n_in2', 'seg:sum', 'tile:const_in', 'tile:cx2', 'tile:cx4',
                'tile:cx_gt_255', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo1', 'tile:lo_le_256', 'tile:n_in1', 'tile:n_in2', 'tile:n_in3',
                'tile:partial_tile', 'tile:sum']),
    dict(name='03-max-hub53878-bi4096x0',
         recipe=('hub_spec', {'seed': 53878, 'hub_card': 300, 'parent_cards': [4, 2], 'child_cards': [3, 2]}),
         options={}, kind='max', nodes=5,
         requests=[{'ev': [], 'ec': []}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx4', 'seg:cx_gt_255', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged',
                'seg:n_in1', 'seg:n_in2', 'seg:n_in3', 'seg:passes2+']),
    dict(name='04-draw-hub53878-bi4096x0',
         recipe=('hub_spec', {'seed': 53878, 'hub_card': 300, 'parent_cards': [4, 2], 'child_cards': [3, 2]}),
         options={}, kind='draw', seed=1, nodes=5,
         requests=[{'ev': [], 'ec': [], 'n': 300}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx4', 'seg:cx_gt_255', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:n_in2', 'seg:n_in3',
                'seg:passes2+', 'seg:sum']),
    dict(name='05-map-hub62973-bi65536x0',
         recipe=('hub_spec', {'seed': 62973, 'hub_card': 320, 'parent_cards': [2, 3], 'child_cards': [3, 3, 2]}),
         options={'big_iters': 65536}, kind='map', nodes=6,
         requests=[{'ev': [], 'ec': [], 'M': [0, 3, 2], 'prune': 0}],
         edges=['map_seg_mixed', 'seg:argmax_gt_255', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_gt_255', 'seg:cx_not_pow2', 'seg:hi1', 'seg:hi_gt_64', 'seg:lo1',
                'seg:max', 'seg:n_in1', 'seg:n_in2', 'seg:n_in4', 'seg:passes2+', 'seg:sum']),
    dict(name='06-map-hub69652-bi2x1-sc16',
         recipe=('hub_spec', {'seed': 69652, 'hub_card': 600, 'parent_cards': [2, 2], 'child_cards': [2, 3]}),
         options={'big_iters': 2, 'tile_h': 1, 'small_cells': 16}, kind='map', nodes=5,
         requests=[{'ev': [], 'ec': [], 'M': [1], 'prune': 0}],
         edges=['map_tile_sum', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:n_in2', 'seg:sum', 'tile:const_in',
                'tile:cx2', 'tile:cx_gt_255', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo1', 'tile:lo_le_256', 'tile:n_in1', 'tile:n_in2',
                'tile:n_in3', 'tile:sum']),
    dict(name='07-map-dag19506-bi64x2',
         recipe=('random_dag_spec', {'seed': 19506, 'n_nodes': 7, 'max_parents': 2, 'cards': [7, 3, 2], 'max_cells': 4096}),
         options={'big_iters': 64, 'tile_h': 2}, kind='map', nodes=7,
         requests=[{'ev': [1, 4], 'ec': [1, 5], 'M': [3, 5], 'prune': 0}],
         edges=['map_seg_mixed', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:n_in3', 'seg:n_in5',
                'seg:sum']),
    dict(name='08-max-dag51182-bi4096x0',
         recipe=('random_dag_spec', {'seed': 51182, 'n_nodes': 8, 'max_parents': 4, 'cards': [2, 3], 'max_cells': 4096}),
         options={}, kind='max', nodes=8,
         requests=[{'ev': [1, 6], 'ec': [2, 0]}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'seg:n_in4', 'seg:n_in5']),
    dict(name='09-draw-hub90864-bi2x1',
         recipe=('hub_spec', {'seed': 90864, 'hub_card': 5, 'parent_cards': [3], 'child_cards': [2, 2, 2, 3, 2, 3, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='draw', seed=1, nodes=9,
         requests=[{'ev': [0, 1], 'ec': [1, 0], 'n': 300}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:n_in4', 'seg:n_in6', 'seg:sum']),
    dict(name='10-map-hub69166-bi64x2',
         recipe=('hub_spec', {'seed': 69166, 'hub_card': 2, 'parent_cards': [5], 'child_cards': [2, 2, 4, 5, 3, 3, 3, 2]}),
         options={'big_iters': 64, 'tile_h': 2}, kind='map', nodes=10,
         requests=[{'ev': [2, 3], 'ec': [1, 1], 'M': [6, 8, 9, 0, 5], 'prune': 0}],
         edges=['map_tile_max', 'map_tile_sum', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx4', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1',
                'seg:n_in6', 'seg:sum', 'tile:const_in', 'tile:cx2', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:max', 'tile:n_in2',
                'tile:n_in4', 'tile:partial_tile', 'tile:sum']),
    dict(name='11-draw-hub76678-bi4096x0',
         recipe=('hub_spec', {'seed': 76678, 'hub_card': 600, 'parent_cards': [3], 'child_cards': [3, 3, 2, 2]}),
         options={}, kind='draw', seed=1, nodes=6,
         requests=[{'ev': [3], 'ec': [0], 'n': 300}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_gt_255', 'seg:cx_not_pow2', 'seg:hi1', 'seg:hi_gt_64', 'seg:lo1', 'seg:n_in1', 'seg:n_in2',
                'seg:n_in5', 'seg:sum']),
    dict(name='12-max-hub34744-bi4096x0',
         recipe=('hub_spec', {'seed': 34744, 'hub_card': 600, 'parent_cards': [2, 2], 'child_cards': [2, 3, 2, 3, 3]}),
         options={}, kind='max', nodes=8,
         requests=[{'ev': [1, 7], 'ec': [0, 0]}],
         edges=['seg:argmax_gt_255', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_gt_255', 'seg:cx_not_pow2', 'seg:hi1', 'seg:hi_gt_64', 'seg:lo1', 'seg:max',
                'seg:max_unflagged', 'seg:n_in1', 'seg:n_in2', 'seg:n_in6']),
    dict(name='13-map-hub28599-bi2x1-sc16',
         recipe=('hub_spec', {'seed': 28599, 'hub_card': 3, 'parent_cards': [3], 'child_cards': [5, 3, 4, 3, 2, 3]}),
         options={'big_iters': 2, 'tile_h': 1, 'small_cells': 16}, kind='map', nodes=8,
         requests=[{'ev': [], 'ec': [], 'M': [2, 5, 0, 6, 3], 'prune': 1}],
         edges=['map_tile_max', 'map_tile_sum', 'seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:sum', 'tile:const_in', 'tile:cx_not_pow2',
                'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:max', 'tile:n_in1', 'tile:n_in2', 'tile:n_in5', 'tile:sum']),
    dict(name='14-max-hub55258-bi2x1',
         recipe=('hub_spec', {'seed': 55258, 'hub_card': 600, 'parent_cards': [3], 'child_cards': [2, 2, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='max', nodes=5,
         requests=[{'ev': [2], 'ec': [1]}, {'ev': [2], 'ec': [0]}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'tile:argmax_gt_255', 'tile:const_in', 'tile:cx2',
                'tile:cx_gt_255', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo1', 'tile:lo_le_256', 'tile:max', 'tile:n_in1', 'tile:n_in2',
                'tile:n_in4']),
    dict(name='15-draw-hub55258-bi2x1',
         recipe=('hub_spec', {'seed': 55258, 'hub_card': 600, 'parent_cards': [3], 'child_cards': [2, 2, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='draw', seed=1, nodes=5,
         requests=[{'ev': [], 'ec': [], 'n': 300}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:sum', 'tile:const_in', 'tile:cx2', 'tile:cx_gt_255', 'tile:cx_not_pow2', 'tile:hi1',
                'tile:lane_ragged', 'tile:lo1', 'tile:lo_le_256', 'tile:n_in1', 'tile:n_in2', 'tile:n_in4', 'tile:sum']),
    dict(name='16-max-dag36099-bi2x1',
         recipe=('random_dag_spec', {'seed': 36099, 'n_nodes': 9, 'max_parents': 4, 'cards': [6, 2], 'max_cells': 4096}),
         options={'big_iters': 2, 'tile_h': 1}, kind='max', nodes=9,
         requests=[{'ev': [], 'ec': []}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'tile:const_in', 'tile:cx2', 'tile:cx_not_pow2', 'tile:hi1',
                'tile:lane_ragged', 'tile:lo_le_256', 'tile:max', 'tile:n_in1', 'tile:n_in2', 'tile:n_in3', 'tile:n_in5']),
    dict(name='17-draw-dag36099-bi2x1',
         recipe=('random_dag_spec', {'seed': 36099, 'n_nodes': 9, 'max_parents': 4, 'cards': [6, 2], 'max_cells': 4096}),
         options={'big_iters': 2, 'tile_h': 1}, kind='draw', seed=1, nodes=9,
         requests=[{'ev': [], 'ec': [], 'n': 300}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:sum', 'tile:const_in', 'tile:cx2', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged',
                'tile:lo_le_256', 'tile:n_in1', 'tile:n_in2', 'tile:n_in3', 'tile:n_in5', 'tile:sum']),
    dict(name='18-draw-hub14291-bi2x1',
         recipe=('hub_spec', {'seed': 14291, 'hub_card': 300, 'parent_cards': [4, 2], 'child_cards': [2, 3, 2, 2, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='draw', seed=1, nodes=8,
         requests=[{'ev': [], 'ec': [], 'n': 300}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:sum', 'tile:const_in', 'tile:cx2', 'tile:cx4', 'tile:cx_gt_255', 'tile:cx_not_pow2',
                'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:n_in1', 'tile:n_in2', 'tile:n_in6', 'tile:sum']),
    dict(name='19-max-hub54199-bi2x1',
         recipe=('hub_spec', {'seed': 54199, 'hub_card': 300, 'parent_cards': [2, 3], 'child_cards': [2, 2, 3, 3, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='max', nodes=8,
         requests=[{'ev': [], 'ec': []}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'tile:const_in', 'tile:cx2', 'tile:cx_gt_255',
                'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:max', 'tile:n_in1', 'tile:n_in2', 'tile:n_in6']),
    dict(name='20-map-hub38310-bi4096x0',
         recipe=('hub_spec', {'seed': 38310, 'hub_card': 7, 'parent_cards': [4, 2], 'child_cards': [4, 4, 4, 2, 4, 3, 4, 2]}),
         options={}, kind='map', nodes=11,
         requests=[{'ev': [], 'ec': [], 'M': [10, 9, 0, 8, 5, 6, 7, 1, 4, 3], 'prune': 1}],
         edges=['map_tile_max', 'map_tile_sum', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx4', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1',
                'seg:n_in2', 'seg:passes2+', 'seg:sum', 'tile:const_in', 'tile:cx1', 'tile:cx4', 'tile:cx_not_pow2', 'tile:lane_ragged', 'tile:lo_le_256',
                'tile:max', 'tile:n_in1', 'tile:n_in2', 'tile:n_in4', 'tile:n_in6', 'tile:partial_tile', 'tile:sum']),
    dict(name='21-max-dag93680-bi4096x0',
         recipe=('random_dag_spec', {'seed': 93680, 'n_nodes': 6, 'max_parents': 3, 'cards': [4], 'max_cells': 4096}),
         options={}, kind='max', nodes=6,
         requests=[{'ev': [5], 'ec': [1]}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx4', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'seg:n_in3', 'seg:n_in4', 'seg:passes2+']),
    dict(name='22-draw-hub54313-bi4096x0',
         recipe=('hub_spec', {'seed': 54313, 'hub_card': 4, 'parent_cards': [2, 3], 'child_cards': [2, 2, 2, 2, 5, 3, 3, 4]}),
         options={}, kind='draw', seed=1, nodes=11,
         requests=[{'ev': [0, 1], 'ec': [1, 1], 'n': 300}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx4', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:n_in3', 'seg:n_in4', 'seg:n_in6',
                'seg:sum']),
    dict(name='23-map-hub45076-bi65536x0',
         recipe=('hub_spec', {'seed': 45076, 'hub_card': 600, 'parent_cards': [2, 2], 'child_cards': [2]}),
         options={'big_iters': 65536}, kind='map', nodes=4,
         requests=[{'ev': [0, 1], 'ec': [0, 1], 'M': [2], 'prune': 0}],
         edges=['map_seg_mixed', 'seg:argmax_gt_255', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_gt_255', 'seg:cx_not_pow2', 'seg:hi1', 'seg:hi_gt_64', 'seg:lo1',
                'seg:max', 'seg:n_in1', 'seg:n_in2', 'seg:n_in3', 'seg:sum']),
    dict(name='24-map-hub32556-bi2x3',
         recipe=('hub_spec', {'seed': 32556, 'hub_card': 600, 'parent_cards': [4, 2], 'child_cards': [2, 3]}),
         options={'big_iters': 2, 'tile_h': 3}, kind='map', nodes=5,
         requests=[{'ev': [], 'ec': [], 'M': [3, 2], 'prune': 0}],
         edges=['map_tile_max', 'map_tile_sum', 'seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:sum', 'tile:argmax_gt_255', 'tile:const_in',
                'tile:cx2', 'tile:cx4', 'tile:cx_gt_255', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo1', 'tile:lo_le_256', 'tile:max', 'tile:n_in1',
                'tile:n_in2', 'tile:n_in3', 'tile:partial_tile', 'tile:sum']),
    dict(name='25-max-hub87646-bi2x1',
         recipe=('hub_spec', {'seed': 87646, 'hub_card': 4, 'parent_cards': [6, 4, 6, 6], 'child_cards': [2, 2, 2, 2, 2, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='max', nodes=11,
         requests=[{'ev': [], 'ec': []}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'tile:const_in', 'tile:cx1', 'tile:cx2', 'tile:cx4',
                'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:max', 'tile:max_unflagged', 'tile:n_in1', 'tile:n_in2', 'tile:n_in6']),
    dict(name='26-map-hub87820-bi2x1',
         recipe=('hub_spec', {'seed': 87820, 'hub_card': 4, 'parent_cards': [4, 6, 5], 'child_cards': [2, 2, 2, 2, 2, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='map', nodes=10,
         requests=[{'ev': [], 'ec': [], 'M': [5, 4, 8, 1, 0, 7, 2], 'prune': 0}],
         edges=['map_tile_max', 'map_tile_sum', 'seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:sum', 'tile:const_in', 'tile:cx1',
                'tile:cx2', 'tile:cx4', 'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:max', 'tile:n_in1', 'tile:n_in2', 'tile:n_in6',
                'tile:sum']),
    dict(name='27-draw-hub87646-bi2x1',
         recipe=('hub_spec', {'seed': 87646, 'hub_card': 4, 'parent_cards': [6, 4, 6, 6], 'child_cards': [2, 2, 2, 2, 2, 2]}),
         options={'big_iters': 2, 'tile_h': 1}, kind='draw', seed=1, nodes=11,
         requests=[{'ev': [], 'ec': [], 'n': 300}],
         edges=['seg:cx1', 'seg:cx2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:sum', 'tile:const_in', 'tile:cx1', 'tile:cx2', 'tile:cx4', 'tile:cx_not_pow2',
                'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:n_in1', 'tile:n_in2', 'tile:n_in6', 'tile:sum']),
    dict(name='28-max-dyadic88038-bi4096x0',
         recipe=('dyadic_dag_spec', {'seed': 88038, 'n_nodes': 5, 'max_parents': 3, 'cards': [3, 5]}),
         options={}, kind='max', nodes=5,
         requests=[{'ev': [2, 3], 'ec': [2, 2]}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'seg:n_in2', 'seg:n_in3', 'tie']),
    dict(name='29-map-dyadic70798-bi64x2',
         recipe=('dyadic_dag_spec', {'seed': 70798, 'n_nodes': 8, 'max_parents': 3, 'cards': [3, 5]}),
         options={'big_iters': 64, 'tile_h': 2}, kind='map', nodes=8,
         requests=[{'ev': [0, 3], 'ec': [1, 1], 'M': [2, 4, 7, 1, 6], 'prune': 1}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:n_in2', 'seg:n_in3', 'seg:sum', 'tie']),
    dict(name='30-map-dyadic35243-bi8x3',
         recipe=('dyadic_dag_spec', {'seed': 35243, 'n_nodes': 8, 'max_parents': 3, 'cards': [3, 5]}),
         options={'big_iters': 8, 'tile_h': 3}, kind='map', nodes=8,
         requests=[{'ev': [], 'ec': [], 'M': [3, 5, 4, 0, 1, 6], 'prune': 1}],
         edges=['map_tile_max', 'map_tile_sum', 'seg:cx1', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:sum', 'tie', 'tile:const_in',
                'tile:cx_not_pow2', 'tile:hi1', 'tile:lane_ragged', 'tile:lo_le_256', 'tile:max', 'tile:n_in1', 'tile:n_in3', 'tile:n_in5', 'tile:partial_tile',
                'tile:sum']),
    dict(name='31-max-dag27334-bi4096x0',
         recipe=('random_dag_spec', {'seed': 27334, 'n_nodes': 6, 'max_parents': 3, 'cards': [2, 3], 'p_zero': 0.35, 'max_cells': 4096}),
         options={}, kind='max', nodes=6,
         requests=[{'ev': [1, 2, 3], 'ec': [1, 0, 0]}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1', 'seg:n_in3', 'seg:n_in4',
                'zero_mass']),
    dict(name='32-map-dag27334-bi4096x0',
         recipe=('random_dag_spec', {'seed': 27334, 'n_nodes': 6, 'max_parents': 3, 'cards': [2, 3], 'p_zero': 0.35, 'max_cells': 4096}),
         options={}, kind='map', nodes=6,
         requests=[{'ev': [1, 2, 3], 'ec': [1, 0, 0], 'M': [0, 4], 'prune': 0}],
         edges=['map_seg_mixed', 'seg:const_in', 'seg:cx1', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:n_in3', 'seg:n_in4', 'seg:sum',
                'zero_mass']),
    dict(name='33-draw-dag27334-bi4096x0',
         recipe=('random_dag_spec', {'seed': 27334, 'n_nodes': 6, 'max_parents': 3, 'cards': [2, 3], 'p_zero': 0.35, 'max_cells': 4096}),
         options={}, kind='draw', seed=1, nodes=6,
         requests=[{'ev': [1, 2, 3], 'ec': [1, 0, 0], 'n': 300}],
         edges=['seg:const_in', 'seg:cx1', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:n_in1', 'seg:n_in3', 'seg:n_in4', 'seg:sum', 'zero_mass']),
    dict(name='34-max-chain7-bi4096x0',
         recipe=('chain_spec', {'n': 70, 'cards': [2, 3], 'seed': 7}),
         options={}, kind='max', nodes=70,
         requests=[{'ev': [5, 40], 'ec': [1, 0]}],
         edges=['nvars_gt_64', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:max_unflagged', 'seg:n_in1',
                'seg:n_in2', 'seg:n_in3']),
    dict(name='35-map-chain7-bi4096x0',
         recipe=('chain_spec', {'n': 70, 'cards': [2, 3], 'seed': 7}),
         options={}, kind='map', nodes=70,
         requests=[{'ev': [5, 40], 'ec': [1, 0], 'M': [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69], 'prune': 0}],
         edges=['gather_gt_64', 'seg:const_in', 'seg:cx1', 'seg:cx2', 'seg:cx_not_pow2', 'seg:hi1', 'seg:lo1', 'seg:max', 'seg:n_in1', 'seg:n_in2', 'seg:n_in3',
                'seg:sum']),
]

# Why a kind lacks a tag: the line of the planner or of the kernels that excludes it.
_MAX_ALWAYS = ("planner.cpp emit_run_max: `if (se.eliminate(x, &t, &argmax_cells)) recs.push_back(t);` - every elimination step of a max program gets "
               "a trace, so StepEmitter::eliminate flags it (`w[1] |= kFlagMax << 16;`); its product-only steps are max_unflagged by definition")
_MAP_BY_FLAG = ("elim_kernel.hip.h elim_level: `if (M == ElimMode::Max || (M == ElimMode::Map && ((sh_step[1] >> 16) & kFlagMax)))` (and segment_wave "
                "`if ((w_step[1] >> 16) & kFlagMax) generic_dispatch<64, true>`): an unflagged step of a map program takes the sum body, MAX = false")
_DRAW_SUMS = ("planner.cpp emit_run_draw: `if ((r.n_in = se.eliminate(x))) {` - no trace, so no step of a draw program carries kFlagMax, and ve_sum_kernel "
              "is elim_level<ElimMode::Sum>: MAX = false for every step, no argmax table, no traceback")
_MAP_ONLY = "planner.h: `Map   mibn_map_batch: qvars[0..nq) are the MAP variables M` - sum steps next to max steps, and a gather list, exist in map programs only"
_MPE_ONLY = ("elim_kernel.hip.h traceback: `for (int v = lane; v < n; v += kTracebackWG) A.codes[(size_t)r * (size_t)n + v] = sh_code[v];` is the GATHER = false "
             "branch, mpe_traceback_kernel's; the other kinds store through the gather list (map) or not at all (draw)")
IMPOSSIBLE = {
    "max": {"seg:sum": _MAX_ALWAYS, "tile:sum": _MAX_ALWAYS, "map_seg_mixed": _MAP_ONLY, "map_tile_sum": _MAP_ONLY, "map_tile_max": _MAP_ONLY,
            "gather_gt_64": _MAP_ONLY},
    "map": {"seg:max_unflagged": _MAP_BY_FLAG, "tile:max_unflagged": _MAP_BY_FLAG, "nvars_gt_64": _MPE_ONLY},
    "draw": {"seg:max": _DRAW_SUMS, "tile:max": _DRAW_SUMS, "seg:max_unflagged": _DRAW_SUMS, "tile:max_unflagged": _DRAW_SUMS,
             "seg:argmax_gt_255": _DRAW_SUMS, "tile:argmax_gt_255": _DRAW_SUMS, "tie": _DRAW_SUMS, "map_seg_mixed": _MAP_ONLY, "map_tile_sum": _MAP_ONLY,
             "map_tile_max": _MAP_ONLY, "gather_gt_64": _MAP_ONLY, "nvars_gt_64": _MPE_ONLY},
}
# Everything else every kind must show somewhere in the table, on both paths.
REQUIRED = {kind: sorted(({f"{p}:{t}" for p in PATHS for t in STEP_TAGS + PATH_TAGS[p] + NUMERIC_STEP_TAGS} | set(CASE_TAGS)) - set(IMPOSSIBLE[kind]))
            for kind in KINDS}
