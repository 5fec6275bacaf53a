"""The networks and the Gibbs cases that tests/test_sampling_twin.py runs on the GPU and tests/test_sampler_plan_host.py plans on the
host (tools/sampler_plan_sim.cpp): one table, so that the launch form a case is said to pin is the form the plan gives it.

Every case names the form it takes under gibbs_lds 1, 2 and 0.  The forms are worked out here from the rules in the head of
sorobn_amd/csrc/sampler_plan.h, never read off the tool:
  * gibbs_lds 0 is always L2.
  * Every chain count the GPU tests use (1 .. 65, CONDITIONAL_ROWS) is below 4 096, so neither the 512-workgroup rule of the 8-lane form
    nor the 512-wave rule of the LDS forms bites: only sizes and the FAST conditions decide.
  * Grids (parents = top and left neighbour): a variable has at most two children, so at most 3 factors, each with at most two other
    variables; with K <= 8 states they qualify for FAST, and small ones fit: Fast8 under 1, Fast under 2.  Asia likewise (binary, at
    most two children, at most two parents).
  * dag2: variable 4 (never evidence here) has four children = 5 factors: generic programs, all of it in LDS (469 cells): PoolProgLds.
  * The tree has 17 and 255 states: not FAST; 17 + 17*255 + 255*3 + 17*17 + 17*2 = 5 440 cells = 43 KB fit: PoolProgLds.
  * 255 x 255: the 65 025-cell table (508 KB) cannot sit in LDS, the two programs can: ProgLds.
  * The 32 x 32 binary grid: 64 KiB of state + 7 938 cells (62 KB) of tables fit in 160 KiB; the 1 024 FAST records (28 words = 112
    bytes each, 112 KB) do not fit beside them, nor do the generic programs (an interior variable: 2 + 7 + 5 + 5 words, + 2 for its
    offset and cycle entry = 84 bytes, 961 of them alone 79 KB; 126 + 79 KB > 160 KiB): PoolLds."""
import numpy as np

import golden_util as gu
import netspec
import sample_check as sc
import sorobn_amd
from sorobn_amd.flatten import flatten

FORMS = ("L2", "PoolLds", "ProgLds", "PoolProgLds", "Fast", "Fast8")
LDS_MODES = (1, 2, 0)
CONDITIONAL_ROWS = 70  # rows of the mibn_gibbs_conditional test: a wave and six lanes


def tables(rng, card, parents, zeros=True):
    """Unnormalised positive tables; every third row gets a zero at the start, the middle or the end (in turn), some rows two
    trailing zeros - never a whole row."""
    out = []
    for v, p in enumerate(parents):
        k = int(card[v])
        t = rng.random([int(card[u]) for u in p] + [k]) * 2 + 0.05
        rows = t.reshape(-1, k)
        if zeros and k > 1:
            for r in range(0, len(rows), 3):
                rows[r, (0, k // 2, k - 1)[(r // 3) % 3]] = 0.0
                if k > 3 and (r // 3) % 4 == 3:
                    rows[r, -2:] = 0.0
        assert (rows.sum(axis=1) > 0).all()
        out.append(t)
    return out


def random_net(card, parents, seed, zeros=True):
    return sc.make_net(card, parents, tables(np.random.default_rng(seed), card, parents, zeros))


def grid_net(R, C, K, seed):
    """Row-major grid, parents = top and left neighbour."""
    parents = [([v - C] if v >= C else []) + ([v - 1] if v % C else []) for v in range(R * C)]
    return random_net([K] * (R * C), parents, seed)


def chain_net(n, seed):
    return random_net([2] * n, [[v - 1] if v else [] for v in range(n)], seed)


def example(name):
    spec = next(n for n in gu.load("examples.json") if n["spec"]["name"] == name)["spec"]
    return sc.from_flat(flatten(netspec.build(spec, sorobn_amd.BayesNet)))


def dag():
    """A network of tests/golden/random_dags.json with a node of five children and nodes of three parents (normalised rows, exact
    zeros, missing rows = zeros of the dense table)."""
    spec = next(e["spec"] for e in gu.load("random_dags.json") if e["spec"]["name"] == "dag2")
    net = sc.from_flat(flatten(netspec.build(spec, sorobn_amd.BayesNet)))
    assert max(len(c) for c in net.children) >= 4 and max(len(s) for s in net.scope) - 1 >= 3
    return net


def tree_net():
    """Cards 17 and 255: the `card > 16` update form (variables 0, 1, 3), beside two small ones."""
    return random_net([17, 255, 3, 17, 2], [[], [0], [1], [0], [3]], seed=41)


GRID, GENERIC = {1: "Fast8", 2: "Fast", 0: "L2"}, {1: "PoolProgLds", 2: "PoolProgLds", 0: "L2"}
SIZES = ((61, 257), (9, 40))  # (chains, iterations) of the whole-stream run and of the two shard runs

GIBBS_CASES = {
    # name: (network, query, evidence, cycle, form under each gibbs_lds, sizes)
    "grid3x3k8": (lambda: grid_net(3, 3, 8, 51), [4, 8], {}, None, GRID, SIZES),                                  # 8-lane / FAST, no evidence
    "grid4x5k3": (lambda: grid_net(4, 5, 3, 52), [12], {0: 1, 19: 2, 7: 0}, None, GRID, SIZES),                   # three evidence variables
    "grid4x5k3-reverse-cycle": (lambda: grid_net(4, 5, 3, 52), [9, 10], {0: 1}, "reverse", GRID, SIZES),           # a caller's cycle
    "dag-5-children-3-parents": (dag, [4, 9], {1: 1}, None, GENERIC, SIZES),                                       # generic `card <= 16` form
    "dag-reverse-cycle": (dag, [10, 0, 5], {}, "reverse", GENERIC, SIZES),
    "tree-17-255": (tree_net, [1], {4: 1}, None, GENERIC, SIZES),                                                  # `card > 16` form, 255 cells
    "tree-17-255-two-queries": (tree_net, [3, 0], {}, "reverse", GENERIC, SIZES),
    "asia-five-queries": (lambda: example("asia"), [0, 2, 4, 5, 7], {}, None, GRID, SIZES),                        # n_q > 4, a deterministic CPT
    "asia-five-queries-evidence": (lambda: example("asia"), [6, 1, 3, 0, 5], {2: 1, 4: 0, 7: 1}, "reverse", GRID, SIZES),
    "grid-five-queries": (lambda: grid_net(3, 3, 2, 53), [8, 0, 4, 2, 6], {5: 1}, None, GRID, SIZES),              # n_q > 4 in the 8-lane / FAST forms
    # the programs in LDS beside tables that stay in L2
    "two-255-state-variables": (lambda: random_net([255, 255], [[], [0]], 54), [1], {}, None, {1: "ProgLds", 2: "ProgLds", 0: "L2"}, SIZES),
    # the tables in LDS, the programs of 1 024 variables in global memory (9 x 20: the numpy twin walks 1 024 variables per chain; the
    # reverse cycle updates the variables whose tables end the pool)
    "grid32x32k2": (lambda: grid_net(32, 32, 2, 55), [1023, 1005], {512: 1}, "reverse", {1: "PoolLds", 2: "PoolLds", 0: "L2"}, ((9, 20), (9, 20))),
}


def cycle_of(net, ev, cycle):
    """The cycle a case passes to the engine: None, or every non-evidence variable in descending id."""
    return [v for v in range(len(net.card) - 1, -1, -1) if v not in ev] if cycle == "reverse" else cycle
