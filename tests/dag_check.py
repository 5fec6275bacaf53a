"""Twin of mibn_best_dag (exact structure learning by dynamic programming over variable subsets), numpy only: what include/mibn.h
pins, literally - phase A one index bit per pass over the whole table, phase B level by level of popcount, the traceback - and
an enumeration of every DAG as the oracle of the twin itself.  Candidates are three parallel lists: child, parent mask (bit u =
column u is a parent), score."""
import itertools
import math

import numpy as np

from structure_check import has_cycle

NO_MASK = 0xFFFFFFFF
NO_SINK = 255


def squeeze(C, v):
    """Subsets of the columns without v -> indices of child v's table: bit v squeezed out (arrays or ints)."""
    return (C & ((1 << v) - 1)) | ((C >> (v + 1)) << v)


def bps_tables(n, children, masks, scores):
    """Phase A -> (score float64 [n, 2^(n-1)], mask uint32 [n, 2^(n-1)])."""
    m = 1 << (n - 1)
    score = np.full((n, m), -np.inf)
    mask = np.full((n, m), NO_MASK, np.uint32)
    v, pm = np.asarray(children, np.int64).reshape(-1), np.asarray(masks, np.int64).reshape(-1)
    at = squeeze(pm, v)
    score[v, at] = np.asarray(scores, np.float64).reshape(-1)
    mask[v, at] = pm.astype(np.uint32)
    idx = np.arange(m)
    for b in range(n - 1):
        dst = idx[(idx >> b) & 1 == 1]
        src = dst ^ (1 << b)
        better = (score[:, src] > score[:, dst]) | ((score[:, src] == score[:, dst]) & (mask[:, src] < mask[:, dst]))
        score[:, dst] = np.where(better, score[:, src], score[:, dst])
        mask[:, dst] = np.where(better, mask[:, src], mask[:, dst])
    return score, mask


def sink_tables(n, score):
    """Phase B -> (best float64 [2^n], sink uint8 [2^n])."""
    S = np.arange(1 << n, dtype=np.int64)
    pop = np.zeros(1 << n, np.int64)
    for v in range(n):
        pop += (S >> v) & 1
    best = np.full(1 << n, -np.inf)
    sink = np.full(1 << n, NO_SINK, np.uint8)
    best[0] = 0.0
    for level in range(1, n + 1):
        at = S[pop == level]
        top = np.full(len(at), -np.inf)
        who = np.full(len(at), NO_SINK, np.uint8)
        for v in range(n):  # ascending v, strict >: ties go to the smallest v
            has = (at >> v) & 1 == 1
            sub = at[has] ^ (1 << v)
            term = best[sub] + score[v, squeeze(sub, v)]
            win = term > top[has]
            where = np.flatnonzero(has)[win]
            top[where] = term[win]
            who[where] = v
        best[at], sink[at] = top, who
    return best, sink


def best_dag(n, children, masks, scores, tables=False):
    """-> (parents uint32[n], order int32[n], total); with tables: + (bps score, bps mask, best, sink)."""
    score, mask = bps_tables(n, children, masks, scores)
    best, sink = sink_tables(n, score)
    S = (1 << n) - 1
    parents = np.full(n, NO_MASK, np.uint32)
    order = np.full(n, -1, np.int32)
    if sink[S] != NO_SINK:
        for k in range(n - 1, -1, -1):
            v = int(sink[S])
            S ^= 1 << v
            parents[v] = mask[v, squeeze(S, v)]
            order[k] = v
    out = (parents, order, float(best[(1 << n) - 1]))
    return out + (score, mask, best, sink) if tables else out


def all_dags_best(n, children, masks, scores, exclude=None):
    """Every choice of one candidate per child, the acyclic ones kept -> (fsum total of the best, its parent masks as a tuple);
    (-inf, None) without one.  exclude: a tuple of parent masks that does not count (the runner-up of that graph)."""
    per = [[] for _ in range(n)]
    for v, pm, s in zip(children, masks, scores):
        per[int(v)].append((int(pm), float(s)))
    top, arg = -math.inf, None
    for pick in itertools.product(*per):
        pms = tuple(pm for pm, _ in pick)
        if pms == exclude or has_cycle(n, [[u for u in range(n) if (pm >> u) & 1] for pm in pms]):
            continue
        total = math.fsum(s for _, s in pick)
        if total > top:
            top, arg = total, pms
    return top, arg


def tie_candidates(n, seed):
    """Every (child, parent set) with about half absent, integer scores in [-3, 0]: ties and -inf entries everywhere."""
    rng = np.random.default_rng(seed)
    m = 1 << (n - 1)
    i = np.arange(m, dtype=np.int64)
    children, masks = [], []
    for v in range(n):
        children.append(np.full(m, v, np.int32))
        masks.append(((i & ((1 << v) - 1)) | ((i >> v) << (v + 1))).astype(np.uint32))  # bit v put back as 0
    children, masks = np.concatenate(children), np.concatenate(masks)
    keep = rng.random(len(children)) < 0.5
    scores = rng.integers(-3, 1, len(children)).astype(np.float64)
    return children[keep], masks[keep], scores[keep]


def bounded_candidates(n, max_parents, required=(), forbidden=()):
    """The candidate order `exact_search` is pinned to: children in column order, parent sets in ascending (size, mask); a set
    must hold the child's required parents and none of its forbidden ones.  (parent, child) index pairs."""
    out = []
    for v in range(n):
        req = {u for u, c in required if c == v}
        forb = {u for u, c in forbidden if c == v}
        sets = []
        for k in range(max_parents + 1):
            for P in itertools.combinations([u for u in range(n) if u != v], k):
                if req <= set(P) and not forb & set(P):
                    sets.append((k, sum(1 << u for u in P)))
        out += [(v, pm) for _, pm in sorted(sets)]
    return out
