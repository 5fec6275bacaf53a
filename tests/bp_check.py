"""Plain numpy twin of loopy belief propagation as include/mibn.h pins it for mibn_bp_batch (tests/test_bp.py, tests/test_bp_host.py):
the factor graph of the flattened network (sorobn_amd.flatten: the tables the engine itself is given), the flooding schedule with the
header's multiplication and addition orders - every sum a strict left-to-right scan (np.add.accumulate), never numpy's pairwise
np.sum -, damping, the residual, the zero-mass rules; and brute-force marginals of the full weighted joint
(likelihood_check.weighted_joint) to hold it against where belief propagation is exact.

The twin is vectorised over variables of equal (cardinality, degree) and over factors of equal scope cardinalities, so that a 20 x 20
grid takes a second; within a group every request cell sees exactly the operations, in the order, of the scalar definition.

A request's findings are a list [(variable id, weights float64[card])], its evidence a dict {variable id: code}."""
import numpy as np

import likelihood_check as lc


def seq_sum(a):
    """Sum along the last axis in ascending index order, one addition after the other."""
    return np.add.accumulate(a, axis=-1)[..., -1]


class Graph:
    """The factor graph of a flattened network: edges e = (f, k) by ascending factor, then scope position."""

    def __init__(self, f):
        card = [int(c) for c in f.card]
        n = len(card)
        self.n, self.card = n, card
        self.scope = [[int(u) for u in f.scope_vars[f.scope_off[v]:f.scope_off[v + 1]]] for v in range(n)]
        self.table = [np.asarray(f.values[f.value_off[v]:f.value_off[v + 1]], np.float64).reshape([card[u] for u in self.scope[v]])
                      for v in range(n)]
        self.edge_begin, self.edges, self.moff = [], [], []
        cells = 0
        for v in range(n):
            self.edge_begin.append(len(self.edges))
            for k, u in enumerate(self.scope[v]):
                self.edges.append((v, k, u))
                self.moff.append(cells)
                cells += card[u]
        self.cells = cells
        self.nbr = [[] for _ in range(n)]
        for e, (_, _, u) in enumerate(self.edges):
            self.nbr[u].append(e)
        self.loff = np.concatenate([[0], np.cumsum(card)]).astype(np.int64)
        self.lam_cells = int(self.loff[-1])
        moff = np.asarray(self.moff, np.int64)
        # variables of equal (card, degree): cell indices [n, degree, card] of their neighbours' messages, [n, card] of lambda
        self.var_groups = []
        keys = {}
        for v in range(n):
            keys.setdefault((card[v], len(self.nbr[v])), []).append(v)
        for (c, d), vs in sorted(keys.items()):
            eg = np.array([self.nbr[v] for v in vs], np.int64).reshape(len(vs), d)
            self.var_groups.append((c, d, moff[eg][:, :, None] + np.arange(c), self.loff[vs][:, None] + np.arange(c)))
        # factors of equal scope cardinalities: tables [n, *cards], cell indices [n, card_j] of every position's messages
        self.factor_groups = []
        keys = {}
        for v in range(n):
            keys.setdefault(tuple(card[u] for u in self.scope[v]), []).append(v)
        for cards, vs in sorted(keys.items()):
            tables = np.stack([self.table[v] for v in vs])
            idx = [moff[[self.edge_begin[v] + j for v in vs]][:, None] + np.arange(cards[j]) for j in range(len(cards))]
            self.factor_groups.append((cards, tables, idx))


_graphs = {}


def graph(f):
    g = _graphs.get(id(f))
    if g is None or g[0] is not f:
        g = _graphs[id(f)] = (f, Graph(f))
    return g[1]


def local_vectors(G, ev, findings):
    lam = np.ones(G.lam_cells)
    for v, c in ev.items():
        lam[G.loff[v]:G.loff[v + 1]] = 0.0
        if 0 <= c < G.card[v]:
            lam[G.loff[v] + c] = 1.0
    for v, w in findings:
        assert v not in ev and len(w) == G.card[v]
        lam[G.loff[v]:G.loff[v + 1]] = np.asarray(w, np.float64)
    return lam


def run(f, ev=None, findings=(), max_iterations=100, tol=1e-9, damping=0.0, residuals=None):
    """-> (beliefs [sum card], iterations, residual).  residuals: a list that receives r_1, r_2, .."""
    G = graph(f)
    ev = dict(ev or {})
    lam = local_vectors(G, ev, list(findings))
    zeros = np.zeros(G.lam_cells)
    if any(seq_sum(lam[G.loff[v]:G.loff[v + 1]]) == 0.0 for v in range(G.n)):
        return zeros, 0, 0.0
    mu = np.empty(G.cells)
    for e, (_, _, u) in enumerate(G.edges):
        mu[G.moff[e]:G.moff[e] + G.card[u]] = 1.0 / G.card[u]
    d = float(damping)
    it, r = 0, 0.0
    while True:
        it += 1
        zero = False
        nu = np.empty(G.cells)
        for c, deg, midx, lidx in G.var_groups:
            M = mu[midx]
            for i in range(deg):
                p = lam[lidx].copy()
                for i2 in range(deg):
                    if i2 != i:
                        p = p * M[:, i2, :]
                s = seq_sum(p)
                zero = zero or bool(np.any(s == 0.0))
                nu[midx[:, i, :]] = p / np.where(s == 0.0, 1.0, s)[:, None]
        new = np.empty(G.cells)
        for cards, tables, idx in G.factor_groups:
            m = len(cards)
            N = [nu[ix] for ix in idx]
            for k in range(m):
                t = tables
                for j in range(m):
                    if j != k:
                        shape = [1] * (m + 1)
                        shape[0], shape[j + 1] = len(tables), cards[j]
                        t = t * N[j].reshape(shape)
                acc = seq_sum(np.moveaxis(t, k + 1, 1).reshape(len(tables), cards[k], -1))
                s = seq_sum(acc)
                zero = zero or bool(np.any(s == 0.0))
                hat = acc / np.where(s == 0.0, 1.0, s)[:, None]
                if d > 0.0:
                    hat = (1.0 - d) * hat + d * mu[idx[k]]
                new[idx[k]] = hat
        if zero:
            return zeros, it, 0.0
        r = float(np.max(np.abs(new - mu)))
        if residuals is not None:
            residuals.append(r)
        mu = new
        if r <= tol or it == max_iterations:
            break
    bel = np.empty(G.lam_cells)
    for c, deg, midx, lidx in G.var_groups:
        M = mu[midx]
        p = lam[lidx].copy()
        for i in range(deg):
            p = p * M[:, i, :]
        s = seq_sum(p)
        if np.any(s == 0.0):
            return zeros, it, 0.0
        bel[lidx] = p / s[:, None]
    return bel, it, r


def brute(f, ev=None, findings=()):
    """Every single-variable marginal of the full weighted joint, laid out like `run`'s beliefs (evidence: its one-hot); all zeros
    where nothing has mass."""
    G = graph(f)
    ev = dict(ev or {})
    out = np.zeros(G.lam_cells)
    if any(not 0 <= c < G.card[v] for v, c in ev.items()):
        return out
    vs, a = lc.weighted_joint(f, ev, list(findings))
    a = np.asarray(a, np.float64)
    z = a.sum()
    if not z > 0:
        return out
    for i, v in enumerate(vs):
        out[G.loff[v]:G.loff[v + 1]] = a.sum(axis=tuple(j for j in range(len(vs)) if j != i)) / z
    for v, c in ev.items():
        out[G.loff[v] + c] = 1.0
    return out


def edge_records(f):
    """What bp_plan.h's plan holds, worked out from the rules in its header comment alone: (edges as 8-word records, variables as
    8-word records, neighbour edge numbers, their moffs, message cells, lambda cells)."""
    card = [int(c) for c in f.card]
    n = len(card)
    scope = [[int(u) for u in f.scope_vars[f.scope_off[v]:f.scope_off[v + 1]]] for v in range(n)]
    loff = [sum(card[:v]) for v in range(n)]
    edges, begin, cells = [], [], 0
    for v in range(n):
        begin.append(len(edges))
        for k, u in enumerate(scope[v]):
            stride = int(np.prod([card[w] for w in scope[v][k + 1:]], dtype=np.int64))
            edges.append([v, k, u, card[u], cells, int(f.value_off[v]), stride, loff[u]])
            cells += card[u]
    nbr = [[e for e, rec in enumerate(edges) if rec[2] == u] for u in range(n)]
    flat_nbr = [e for u in range(n) for e in nbr[u]]
    variables, at = [], 0
    for v in range(n):
        variables.append([card[v], loff[v], at, len(nbr[v]), begin[v], len(scope[v]), int(f.value_off[v]),
                          int(np.prod([card[u] for u in scope[v]], dtype=np.int64))])
        at += len(nbr[v])
    return edges, variables, flat_nbr, [edges[e][4] for e in flat_nbr], cells, sum(card)
