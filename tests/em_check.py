"""Brute-force twin of EM on a small Bayesian network (tests/test_em.py, tests/test_em_host.py) - numpy only, nothing from
sorobn_amd: the full joint from the CPTs, every row conditioned on its observed cells, the posterior of every family added to
its table, the tables renormalised.  Feasible for joints of up to 2^16 states.

A network here is (card [V], scopes, thetas): scopes[v] = variable ids of family v, the parents then v itself; thetas[v] = the
flat C-order table P(v | parents) over that scope (v fastest).  Rows are int codes [n, V], -1 = not observed."""
import numpy as np


def joint(card, scopes, thetas):
    """Dense product of every CPT, axes = variables 0..V-1."""
    V = len(card)
    out = np.ones([1] * V)
    for sc, th in zip(scopes, thetas):
        a = np.asarray(th, np.float64).reshape([int(card[u]) for u in sc])
        perm = sorted(range(len(sc)), key=lambda i: sc[i])
        shape = [1] * V
        for i in perm:
            shape[sc[i]] = a.shape[i]
        out = out * np.transpose(a, perm).reshape(shape)
    return out


def sample_rows(card, scopes, thetas, n, rng):
    """n complete rows drawn from the joint."""
    a = joint(card, scopes, thetas)
    flat = a.reshape(-1) / a.sum()
    cells = rng.choice(len(flat), size=n, p=flat)
    return np.stack(np.unravel_index(cells, a.shape), axis=1).astype(np.int32)


def knock_out(codes, fraction, rng, drop_column=None):
    """Every cell removed independently with probability `fraction`; `drop_column` removed entirely."""
    out = codes.copy()
    out[rng.random(codes.shape) < fraction] = -1
    if drop_column is not None:
        out[:, drop_column] = -1
    return out


def e_step(card, scopes, thetas, codes, table=None):
    """-> (expected counts per family [flat, like thetas], P(observed cells) per row).  A row of probability zero adds nothing."""
    a = joint(card, scopes, thetas) if table is None else table
    counts = [np.zeros([int(card[u]) for u in sc]) for sc in scopes]
    p_row = np.zeros(len(codes))
    for r, row in enumerate(codes):
        hidden = [v for v in range(len(card)) if row[v] < 0]
        sub = a[tuple(slice(None) if row[v] < 0 else int(row[v]) for v in range(len(card)))]
        p = float(sub.sum())
        p_row[r] = p
        if not p > 0:
            continue
        post = sub / p
        for sc, tab in zip(scopes, counts):
            mine = [u for u in sc if row[u] < 0]
            m = post.sum(axis=tuple(i for i, v in enumerate(hidden) if v not in mine)) if hidden else post
            kept = [v for v in hidden if v in mine]  # axes of m, ascending id
            m = np.transpose(m, [kept.index(u) for u in mine]) if mine else m
            tab[tuple(slice(None) if row[u] < 0 else int(row[u]) for u in sc)] += m
    return [c.reshape(-1) for c in counts], p_row


def m_step(counts, thetas, card, prior_count=0.0):
    """theta = (N + prior_count) / row sums; a parent configuration without mass keeps its previous row."""
    out = []
    for v, (n, th) in enumerate(zip(counts, thetas)):
        n = np.asarray(n, np.float64).reshape(-1, int(card[v])) + prior_count
        prev = np.asarray(th, np.float64).reshape(-1, int(card[v]))
        new = prev.copy()
        for i in range(len(n)):
            s = n[i].sum()
            if s > 0:
                new[i] = n[i] / s
        out.append(new.reshape(-1))
    return out


def em(card, scopes, thetas, codes, n_iter, prior_count=0.0):
    """n_iter E/M-steps -> (thetas, [log-likelihood of the parameters every E-step started from], last expected counts)."""
    lls, counts = [], None
    for _ in range(n_iter):
        counts, p = e_step(card, scopes, thetas, codes)
        with np.errstate(divide="ignore"):
            lls.append(float(np.log(p).sum()))
        thetas = m_step(counts, thetas, card, prior_count)
    return thetas, lls, counts


def relabel(card, scopes, thetas, codes, order):
    """The same network with variable `order[i]` renamed i (a library numbers variables in its own topological order): the
    members of a family keep their order, so the tables are unchanged."""
    new = {old: i for i, old in enumerate(order)}
    return ([card[o] for o in order], [[new[u] for u in scopes[o]] for o in order], [thetas[o] for o in order],
            None if codes is None else codes[:, list(order)])
