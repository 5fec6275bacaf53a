"""Brute-force twin of the constraint-based structure learner (`structure.ci_tests`, `structure.pc`): Python integers,
`math.log` / `math.log1p` and `math.fsum` only, no engine.  The reference has no such search, so - as for the scores of
structure_check.py - the oracle is this twin: the G2 and X2 statistics term by term, a PC-stable that tests one triple at a
time and rebuilds adjacency, v-structures and Meek's closure naively on a matrix, the CPDAG of a known DAG, and an exact
d-separation oracle.  Codes are a [n_rows, n_cols] integer matrix, columns are positions."""
import itertools
import math

import numpy as np

KINDS = ("g2", "x2")


def ci_table(codes, card, x, y, Z):
    """Dense counts [q, rx, ry]: Z in the given order (first slowest), then x, then y fastest."""
    flat = np.zeros(len(codes), np.int64)
    q = 1
    for c in [*Z, x, y]:
        flat = flat * int(card[c]) + codes[:, c].astype(np.int64)
    for z in Z:
        q *= int(card[z])
    rx, ry = int(card[x]), int(card[y])
    return np.bincount(flat, minlength=q * rx * ry).astype(np.int64).reshape(q, rx, ry)


def ci_stat(codes, card, x, y, Z, kind="g2"):
    """(stat, A, adj_dof, classic_dof): the statistic of x and y given Z, A = fsum(|term|) over the same terms - the scale
    rounding errors of a sum of those terms are measured against - and both degrees of freedom.  Exact integers up to the one
    division (and logarithm) per cell; the logarithm of a quotient near 1 is taken as log1p of the exact integer difference
    over the denominator, so the twin does not carry the rounding of the quotient that the tolerance grants the device."""
    assert kind in KINDS
    t = ci_table(codes, card, x, y, Z)
    q, rx, ry = t.shape
    terms, adj = [], 0
    for stratum in t.tolist():
        rows = [sum(r) for r in stratum]
        cols = [sum(r[k] for r in stratum) for k in range(ry)]
        nz = sum(rows)
        if nz == 0:
            continue
        adj += (sum(1 for v in rows if v) - 1) * (sum(1 for v in cols if v) - 1)
        for i, nx in enumerate(rows):
            for k, ny in enumerate(cols):
                n = stratum[i][k]
                if nx == 0 or ny == 0:
                    continue
                if kind == "x2":
                    d = n * nz - nx * ny
                    terms.append(d * d / (nz * nx * ny))
                elif n:
                    num, den = n * nz, nx * ny
                    ln = math.log1p((num - den) / den) if 2 * abs(num - den) < den else math.log(num / den)
                    terms.append(2.0 * n * ln)
    return math.fsum(terms), math.fsum(abs(v) for v in terms), adj, q * (rx - 1) * (ry - 1)


# ------------------------------------------------------------------------------------------------- graphs, naively
def skeleton_of(n, parents):
    M = np.zeros((n, n), bool)
    for v, ps in enumerate(parents):
        for u in ps:
            M[u, v] = M[v, u] = True
    return M


def meek_closure(M):
    """M[u, v] and M[v, u]: u - v; M[u, v] alone: u -> v.  Rules 1 to 3, ordered pairs ascending, a rule that fires orients at
    once, passes until one changes nothing (the order the product documents)."""
    n = len(M)
    adjacent = lambda u, v: M[u, v] or M[v, u]
    und = lambda u, v: M[u, v] and M[v, u]
    into = lambda u, v: M[u, v] and not M[v, u]
    while True:
        fired = False
        for a in range(n):
            for b in range(n):
                if a == b or not und(a, b):
                    continue
                rule = any(into(c, a) and not adjacent(c, b) for c in range(n) if c not in (a, b))
                rule = rule or any(into(a, c) and into(c, b) for c in range(n) if c not in (a, b))
                spokes = [c for c in range(n) if c not in (a, b) and und(a, c) and into(c, b)]
                rule = rule or any(not adjacent(c, d) for c in spokes for d in spokes if c < d)
                if rule:
                    M[b, a] = False
                    fired = True
        if not fired:
            return M


def split(M):
    """-> (arrows {(u, v)}, undirected {(u, v), u < v})."""
    n = len(M)
    arrows = {(u, v) for u in range(n) for v in range(n) if M[u, v] and not M[v, u]}
    return arrows, {(u, v) for u in range(n) for v in range(u + 1, n) if M[u, v] and M[v, u]}


def cpdag(n, parents):
    """The completed partially directed graph of the DAG given by its parent sets: skeleton, the DAG's v-structures, Meek."""
    M = skeleton_of(n, parents)
    for v, ps in enumerate(parents):
        for a, b in itertools.combinations(sorted(ps), 2):
            if not M[a, b]:
                M[v, a] = M[v, b] = False
    return split(meek_closure(M))


def d_separated(n, parents, x, y, Z):
    """Exact: x and y are d-separated by Z iff Z cuts them in the moral graph of the ancestral set of {x, y} and Z."""
    keep, todo = set(), [x, y, *Z]
    while todo:
        v = todo.pop()
        if v not in keep:
            keep.add(v)
            todo += list(parents[v])
    nb = {v: set() for v in keep}
    for v in keep:
        ps = list(parents[v])
        for p in ps:
            nb[v].add(p)
            nb[p].add(v)
        for a, b in itertools.combinations(ps, 2):
            nb[a].add(b)
            nb[b].add(a)
    seen, todo = {x}, [x]
    while todo:
        v = todo.pop()
        for w in nb[v]:
            if w not in seen and w not in Z:
                seen.add(w)
                todo.append(w)
    return y not in seen


def oracle_tester(n, parents):
    """A batch tester for `_pc_search`: p = 1 where the DAG d-separates, else 0; `asked` keeps every batch."""
    asked = []

    def tester(batch):
        asked.append(list(batch))
        return [1.0 if d_separated(n, parents, x, y, set(S)) else 0.0 for x, y, S in batch]

    tester.asked = asked
    return tester


def pc_brute(n, p_of, alpha, max_cond=3, required=(), forbidden=()):
    """PC-stable one triple at a time.  p_of(x, y, S) with x < y, S ascending -> p-value.  -> (arrows, undirected, sepsets)."""
    forbidden, required = set(forbidden), list(required)
    A = np.ones((n, n), bool) & ~np.eye(n, dtype=bool)
    for u in range(n):
        for v in range(n):
            if (u, v) in forbidden and (v, u) in forbidden:
                A[u, v] = False
    keep = np.zeros((n, n), bool)
    for u, v in required:
        A[u, v] = A[v, u] = keep[u, v] = keep[v, u] = True
    sepsets = {}
    for level in range(max_cond + 1):
        frozen = A.copy()
        any_test = False
        for a in range(n):
            for b in range(a + 1, n):
                if not frozen[a, b] or keep[a, b]:
                    continue
                cand = []
                for end, other in ((a, b), (b, a)):
                    rest = [z for z in range(n) if frozen[end, z] and z != other]
                    cand += [S for S in itertools.combinations(rest, level) if S not in cand]
                for S in cand:
                    any_test = True
                    if p_of(a, b, S) > alpha:
                        A[a, b] = A[b, a] = False
                        sepsets[(a, b)] = S
                        break
        if not any_test:
            break
    M = A.copy()

    def orient(u, v):  # u -> v unless the edge is gone, already points the other way, or may not point this way
        if A[u, v] and M[u, v] and (u, v) not in forbidden:
            M[v, u] = False

    for u, v in required:
        orient(u, v)
    for u, v in sorted(forbidden):
        orient(v, u)
    for x in range(n):
        for y in range(x + 1, n):
            if A[x, y] or (x, y) not in sepsets:
                continue
            for z in range(n):
                if A[x, z] and A[y, z] and z not in sepsets[(x, y)]:
                    orient(x, z)
                    orient(y, z)
    arrows, und = split(meek_closure(M))
    return arrows, und, sepsets


def is_dag_of_class(n, edges, arrows, undirected):
    """`edges` (u, v) is acyclic and its completed partially directed graph is exactly the given one (a CPDAG)."""
    parents = [set() for _ in range(n)]
    for u, v in edges:
        parents[v].add(u)
    order, left = [], set(range(n))
    while left:
        free = [v for v in left if not (parents[v] & left)]
        if not free:
            return False
        order += free
        left -= set(free)
    return cpdag(n, parents) == (set(arrows), {(min(e), max(e)) for e in undirected})


# ------------------------------------------------------------------------- test doubles for the host tests
class TwinDataset:
    """TEST DOUBLE for _capi.Dataset (never on the product path): CI tests by the twin, records what was asked."""

    def __init__(self, codes, card, log):
        self.codes, self.card, self.log = np.asarray(codes), [int(c) for c in card], log

    def ci_tests(self, tests, kind="g2"):
        self.log.append([tuple(t) for t in tests])
        got = [ci_stat(self.codes, self.card, t[-2], t[-1], list(t[:-2]), kind) for t in tests]
        return np.array([g[0] for g in got], np.float64), np.array([g[2] for g in got], np.int64)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


class TwinEngine:
    """TEST DOUBLE for the counting engine: `dataset` -> TwinDataset; `calls` lists the test batches of every call."""

    def __init__(self):
        self.calls = []

    def dataset(self, codes, card):
        return TwinDataset(codes, card, self.calls)
