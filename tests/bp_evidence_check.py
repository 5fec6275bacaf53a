"""Plain numpy twin of the Bethe log Z and the family beliefs as include/mibn.h pins them for mibn_bp_evidence_batch
(tests/test_bp_evidence.py, tests/test_bp_evidence_host.py): bp_check's graph, local vectors and left-to-right sums; the message loop
of mibn_bp_batch; then the final phase - nu* from the final mu, Z_f over every cell of a factor in ascending C-order with the product
over ALL positions, Z_v, Z_e, the terms left to right, the 64 partials and their ascending sum.  Beside it the sequential rule of
`acc`, and a brute-force log mass and family posterior of the full weighted joint (likelihood_check.weighted_joint).

A request's findings are a list [(variable id, weights float64[card])], its evidence a dict {variable id: code}."""
import types

import numpy as np

import bp_check as bc
import likelihood_check as lc


def family_layout(G):
    """(foff [n + 1], fcells): factor v's cells in a family-belief row - the tables back to back in the C-order of (parents.., v)."""
    foff = np.concatenate([[0], np.cumsum([G.table[v].size for v in range(G.n)])]).astype(np.int64)
    return foff, int(foff[-1])


def phase1(G, lam, mu):
    """Step 1 -> (nu, whether a normaliser was 0)."""
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
    return nu, zero


def phase2(G, mu, nu, d):
    """Steps 2 and 3 -> (mu of this step, whether a normaliser was 0)."""
    zero = False
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
            acc = bc.seq_sum(np.moveaxis(t, k + 1, 1).reshape(len(tables), cards[k], -1))
            s = bc.seq_sum(acc)
            zero = zero or bool(np.any(s == 0.0))
            hat = acc / np.where(s == 0.0, 1.0, s)[:, None]
            if d > 0.0:
                hat = (1.0 - d) * hat + d * mu[idx[k]]
            new[idx[k]] = hat
    return new, zero


def partial_sum(term):
    """The score rule's order: partial_l over v = l, l + 64, .. ascending, then the 64 partials ascending."""
    rows = -(-len(term) // 64)
    padded = np.concatenate([term, np.zeros(rows * 64 - len(term))]).reshape(rows, 64)
    return float(bc.seq_sum(bc.seq_sum(padded.T)))


def run(f, ev=None, findings=(), max_iterations=100, tol=1e-9, damping=0.0):
    """-> namespace(log_z, beliefs [sum card], fbeliefs [fcells], iterations, residual)"""
    G = bc.graph(f)
    ev = dict(ev or {})
    lam = bc.local_vectors(G, ev, list(findings))
    foff, fcells = family_layout(G)

    def no_mass(it):
        return types.SimpleNamespace(log_z=-np.inf, beliefs=np.zeros(G.lam_cells), fbeliefs=np.zeros(fcells), iterations=it, residual=0.0)

    if any(bc.seq_sum(lam[G.loff[v]:G.loff[v + 1]]) == 0.0 for v in range(G.n)):
        return no_mass(0)
    mu = np.empty(G.cells)
    for e, (_, _, u) in enumerate(G.edges):
        mu[G.moff[e]:G.moff[e] + G.card[u]] = 1.0 / G.card[u]
    it, r = 0, 0.0
    while True:
        it += 1
        nu, z1 = phase1(G, lam, mu)
        new, z2 = phase2(G, mu, nu, float(damping))
        if z1 or z2:
            return no_mass(it)
        r = float(np.max(np.abs(new - mu)))
        mu = new
        if r <= tol or it == max_iterations:
            break
    # ---- the final phase
    nu, zero = phase1(G, lam, mu)
    if zero:
        return no_mass(it)
    log_zf = np.empty(G.n)
    fbel = np.empty(fcells)
    for cards, tables, idx in G.factor_groups:
        m = len(cards)
        t = tables
        for j in range(m):
            shape = [1] * (m + 1)
            shape[0], shape[j + 1] = len(tables), cards[j]
            t = t * nu[idx[j]].reshape(shape)
        t = t.reshape(len(tables), -1)
        s = bc.seq_sum(t)
        if np.any(s == 0.0):
            return no_mass(it)
        vs = [v for v in range(G.n) if tuple(G.card[u] for u in G.scope[v]) == cards]  # (the group's factors, ascending: Graph's order)
        for i, v in enumerate(vs):
            log_zf[v] = np.log(s[i])
            fbel[foff[v]:foff[v + 1]] = t[i] / s[i]
    bel = np.empty(G.lam_cells)
    for c, deg, midx, lidx in G.var_groups:
        M = mu[midx]
        p = lam[lidx].copy()
        for i in range(deg):
            p = p * M[:, i, :]
        s = bc.seq_sum(p)
        if np.any(s == 0.0):
            return no_mass(it)
        bel[lidx] = p / s[:, None]
    term = np.empty(G.n)
    for v in range(G.n):
        p = lam[G.loff[v]:G.loff[v + 1]].copy()
        for e in G.nbr[v]:
            p = p * mu[G.moff[e]:G.moff[e] + G.card[v]]
        tv = log_zf[v] + np.log(bc.seq_sum(p))
        for j, u in enumerate(G.scope[v]):
            mo = G.moff[G.edge_begin[v] + j]
            ze = bc.seq_sum(mu[mo:mo + G.card[u]] * nu[mo:mo + G.card[u]])
            if ze == 0.0:
                return no_mass(it)
            tv = tv - np.log(ze)
        term[v] = tv
    return types.SimpleNamespace(log_z=partial_sum(term), beliefs=bel, fbeliefs=fbel, iterations=it, residual=r)


def accumulate(acc, rows, weight=None):
    """The header's rule: acc[c] = acc[c] + weight[b] * b_f(c) for b ascending, one addition after the other.  -> a new array"""
    acc = np.array(acc, np.float64)
    for b, row in enumerate(rows):
        acc = acc + (1.0 if weight is None else float(weight[b])) * np.asarray(row, np.float64)
    return acc


def brute(f, ev=None, findings=()):
    """(log of the mass of the full weighted joint, the posterior of every family laid out like `run`'s fbeliefs); -inf and zeros where
    nothing has mass."""
    G = bc.graph(f)
    ev = dict(ev or {})
    foff, fcells = family_layout(G)
    out = np.zeros(fcells)
    if any(not 0 <= c < G.card[v] for v, c in ev.items()):
        return -np.inf, out
    vs, a = lc.weighted_joint(f, ev, list(findings))
    a = np.asarray(a, np.float64)
    z = float(a.sum())
    if not z > 0:
        return -np.inf, out
    vs = list(vs)
    for v in range(G.n):
        free = [u for u in G.scope[v] if u not in ev]
        m = a.sum(axis=tuple(i for i, u in enumerate(vs) if u not in free)) / z  # axes: the free members in the order of vs
        rest = [u for u in vs if u in free]
        m = np.transpose(m, [rest.index(u) for u in free]) if free else m
        full = np.zeros([G.card[u] for u in G.scope[v]])
        full[tuple(ev[u] if u in ev else slice(None) for u in G.scope[v])] = m
        out[foff[v]:foff[v + 1]] = full.reshape(-1)
    return float(np.log(z)), out
