"""Plain numpy twin of approximate MPE by max-product belief propagation as include/mibn.h pins it for mibn_bp_mpe_batch
(tests/test_bp_mpe.py, tests/test_bp_mpe_host.py): bp_check's graph, local vectors and left-to-right sums; the maximum where the header
says maximum; the decode on the products before the division; the score in the header's order - terms padded with +0.0 to rows of 64,
summed down the rows, then along the 64 -; the best candidate so far; the greedy colouring of the moral graph and the polish (iterated
conditional modes) colour by colour.  `one_opt` checks the local-optimum property straight from the CPTs, without the twin's polish.

A request's findings are a list [(variable id, weights float64[card])], its evidence a dict {variable id: code}."""
import types

import numpy as np

import bp_check as bc
import mpe_check as mc


def colouring(G):
    """Greedy colouring of the moral graph: ascending v, the smallest colour no already-coloured neighbour has ->
    (colour of each variable, [members of each colour, ascending])."""
    adj = [set() for _ in range(G.n)]
    for sc in G.scope:
        for u in sc:
            adj[u] |= set(sc) - {u}
    colour = []
    for v in range(G.n):
        taken = {colour[u] for u in adj[v] if u < v}
        c = 0
        while c in taken:
            c += 1
        colour.append(c)
    return colour, [[v for v in range(G.n) if colour[v] == c] for c in range(max(colour) + 1)]


def score(G, lam, codes):
    """The header's score: term_v = log f_v[cell] + log lambda_v(x_v); partial_l over v = l mod 64 ascending; the 64 partials ascending."""
    with np.errstate(divide="ignore"):
        term = np.array([np.log(G.table[v][tuple(int(codes[u]) for u in G.scope[v])]) + np.log(lam[G.loff[v] + int(codes[v])])
                         for v in range(G.n)], np.float64)
    rows = -(-G.n // 64)
    padded = np.concatenate([term, np.zeros(rows * 64 - G.n)]).reshape(rows, 64)
    return float(bc.seq_sum(bc.seq_sum(padded.T)))


def local_products(G, lam, codes, v):
    """L(x) = lambda_v(x) * prod over the edges of N(v), ascending, of f[cell of `codes` with v := x]."""
    out = np.empty(G.card[v])
    for x in range(G.card[v]):
        p = lam[G.loff[v] + x]
        for e in G.nbr[v]:
            fac, k, _ = G.edges[e]
            idx = [int(codes[u]) for u in G.scope[fac]]
            idx[k] = x
            p = p * G.table[fac][tuple(idx)]
        out[x] = p
    return out


def polish(G, lam, codes, sweeps_max):
    """-> (codes, sweeps run, moves made)"""
    codes = np.array(codes, np.int64)
    _, members = colouring(G)
    sweeps = moves = 0
    for s in range(1, sweeps_max + 1):
        moved = 0
        for group in members:
            for v in group:
                L = local_products(G, lam, codes, v)
                x = int(np.argmax(L))
                if L[x] > L[codes[v]]:
                    codes[v] = x
                    moved += 1
        sweeps = s
        moves += moved
        if moved == 0:
            break
    return codes, sweeps, moves


def _no_mass(G, ev, it):
    codes = np.full(G.n, -1, np.int64)
    for v, c in ev.items():
        codes[v] = c
    return types.SimpleNamespace(codes=codes, log_p=-np.inf, iterations=it, residual=0.0, best_iteration=0, sweeps=0, moves=0,
                                 trajectory=[], margin=np.inf)


def run(f, ev=None, findings=(), max_iterations=100, tol=1e-9, damping=0.5, polish_sweeps=10):
    """-> namespace(codes [n], log_p, iterations, residual, best_iteration, sweeps, moves, trajectory = the candidates' scores step by
    step, margin = the smallest gap between the best and the second max-marginal product, relative to the best, over the kept decode)."""
    return run_many(f, ev, findings, (max_iterations,), tol, damping, (polish_sweeps,))[(max_iterations, polish_sweeps)]


def run_many(f, ev=None, findings=(), iterations=(100,), tol=1e-9, damping=0.5, polishes=(10,)):
    """{(max_iterations, polish_sweeps): what `run` returns for them}, from ONE pass over the steps: a call with a smaller
    max_iterations is the same call stopped earlier."""
    G = bc.graph(f)
    ev = dict(ev or {})
    lam = bc.local_vectors(G, ev, list(findings))
    out = {}

    def no_mass(it, ms):
        for m in ms:
            for q in polishes:
                out[(m, q)] = _no_mass(G, ev, it)
        return out

    if any(bc.seq_sum(lam[G.loff[v]:G.loff[v + 1]]) == 0.0 for v in range(G.n)):
        return no_mass(0, iterations)
    mu = np.empty(G.cells)
    for e, (_, _, u) in enumerate(G.edges):
        mu[G.moff[e]:G.moff[e] + G.card[u]] = 1.0 / G.card[u]
    d = float(damping)
    it, r = 0, 0.0
    kept, best, best_it, trajectory, kept_margin = None, 0.0, 0, [], np.inf
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
                s = bc.seq_sum(p)
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
                acc = np.max(np.moveaxis(t, k + 1, 1).reshape(len(tables), cards[k], -1), axis=-1)  # (a maximum has no order)
                s = bc.seq_sum(acc)
                zero = zero or bool(np.any(s == 0.0))
                hat = acc / np.where(s == 0.0, 1.0, s)[:, None]
                if d > 0.0:
                    hat = (1.0 - d) * hat + d * mu[idx[k]]
                new[idx[k]] = hat
        if zero:
            return no_mass(it, [m for m in iterations if m >= it])
        r = float(np.max(np.abs(new - mu)))
        mu = new
        # max-marginals, decode
        cur = np.zeros(G.n, np.int64)
        margin = np.inf
        for c, deg, midx, lidx in G.var_groups:
            M = mu[midx]
            p = lam[lidx].copy()
            for i in range(deg):
                p = p * M[:, i, :]
            if np.any(bc.seq_sum(p) == 0.0):
                return no_mass(it, [m for m in iterations if m >= it])
            vs = np.searchsorted(G.loff[:-1], lidx[:, 0])  # (the group's variables, from their first lambda cell)
            cur[vs] = np.argmax(p, axis=1)  # (the first of the maxima: the lowest state)
            if c > 1:
                top = np.sort(p, axis=1)
                live = top[:, -2] > 0  # (evidence and one-hot findings have no runner-up)
                if live.any():
                    margin = min(margin, float(np.min(((top[:, -1] - top[:, -2]) / top[:, -1])[live])))
        sc = score(G, lam, cur)
        trajectory.append(sc)
        if it == 1 or sc > best:
            kept, best, best_it, kept_margin = cur, sc, it, margin
        stop = r <= tol or it == max(iterations)
        for m in iterations:
            if m == it or (stop and m > it):
                for q in polishes:
                    codes, sweeps, moves = polish(G, lam, kept, q)
                    out[(m, q)] = types.SimpleNamespace(codes=codes, log_p=score(G, lam, codes), iterations=it, residual=r,
                                                        best_iteration=best_it, sweeps=sweeps, moves=moves, trajectory=list(trajectory),
                                                        margin=kept_margin)
        if stop:
            return out


def score_gap(trajectory):
    """The distance between the two best DISTINCT candidate scores of a run (inf with one): where it is tiny, the last bit of a
    logarithm may decide which candidate is kept."""
    top = sorted(set(trajectory), reverse=True)
    if len(top) < 2:
        return np.inf
    if np.isinf(top[1]):
        return np.inf
    return top[0] - top[1]


def log_weighted_joint(f, codes, ev=None, findings=()):
    """log of P(codes) times the findings' weights, factor by factor from mpe_check.cpts - no part of the twin."""
    s = mc.log_joint(f, codes)
    for v, w in findings:
        with np.errstate(divide="ignore"):
            s += float(np.log(w[int(codes[v])]))
    return s


def one_opt(f, codes, ev=None, findings=(), rel=1e-12):
    """True when no change of a single non-evidence variable gives a more probable assignment, straight from the CPTs: for every v and
    x the product of the factors that hold v (and v's finding) with v := x is at most the current one, up to `rel` - the products are
    formed here in another order than the polish forms them."""
    ev = dict(ev or {})
    weights = dict((v, np.asarray(w, np.float64)) for v, w in findings)
    tables = mc.cpts(f)
    for v in range(len(f.card)):
        if v in ev:
            continue
        vals = []
        for x in range(int(f.card[v])):
            trial = [int(c) for c in codes]
            trial[v] = x
            p = float(weights[v][x]) if v in weights else 1.0
            for sc, a in tables:
                if v in sc:
                    p *= float(a[tuple(trial[u] for u in sc)])
            vals.append(p)
        if max(vals) > vals[int(codes[v])] * (1.0 + rel):
            return False
    return True
