"""Twin of mibn_arc_posteriors (exact arc posteriors by the sum-product subset DP), numpy only: what include/mibn.h pins,
literally - the centring, the subset sums one index bit per pass over the whole table, L and R level by level of popcount, the
gaps, the superset sums one bit per pass, the outputs - and an enumeration of every (linear order, consistent parent sets) pair
as the oracle of the twin itself.  Candidates are three parallel lists: child, parent mask (bit u = column u is a parent), score."""
import itertools
import math

import numpy as np

from dag_check import squeeze


def logaddexp(a, b):
    """a (+) b as pinned: m + log1p(exp(-|a - b|)), m = max(a, b); m itself where the other operand (or both) is -inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m, o = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(invalid="ignore"):
        d = -np.abs(a - b)
    live = o > -np.inf
    return np.where(live, m + np.log1p(np.exp(np.where(live, d, 0.0))), m)


def unsqueeze(i, v):
    """Indices of child v's table -> the subsets: bit v put back as 0."""
    return (i & ((1 << v) - 1)) | ((i >> v) << (v + 1))


def centres(n, children, scores):
    c = np.zeros(n)
    for v in range(n):
        own = np.asarray(scores, np.float64).reshape(-1)[np.asarray(children).reshape(-1) == v]
        if len(own):
            c[v] = own.max()
    return c


def depth(n, n_fam):
    """D of include/mibn.h: how many roundings deep a result sits at most."""
    return n * n + 2 * n + math.ceil(math.log2(n_fam + 1))


def tolerance(n, n_fam, M):
    return 8 * depth(n, n_fam) * 2.0 ** -53 * (1.0 + M)


def arc_posteriors(n, children, masks, scores, tables=False):
    """-> (log_post float64[n_fam], arc float64[n, n], log_evidence); with tables: + (L, R, centred scores, M) - M the largest
    finite magnitude among them, the scale of the tolerance."""
    v = np.asarray(children, np.int64).reshape(-1)
    pm = np.asarray(masks, np.int64).reshape(-1)
    s = np.asarray(scores, np.float64).reshape(-1)
    c = centres(n, v, s)
    centred = s - c[v] if len(s) else s
    m, full = 1 << (n - 1), (1 << n) - 1
    alpha = np.full((n, m), -np.inf)
    alpha[v, squeeze(pm, v)] = centred
    idx = np.arange(m, dtype=np.int64)
    for b in range(n - 1):
        dst = idx[(idx >> b) & 1 == 1]
        alpha[:, dst] = logaddexp(alpha[:, dst], alpha[:, dst ^ (1 << b)])
    S = np.arange(1 << n, dtype=np.int64)
    pop = np.zeros(1 << n, np.int64)
    for w in range(n):
        pop += (S >> w) & 1
    L, R = np.full(1 << n, -np.inf), np.full(1 << n, -np.inf)
    L[0] = R[0] = 0.0
    for level in range(1, n + 1):
        at = S[pop == level]
        l, r = np.full(len(at), -np.inf), np.full(len(at), -np.inf)
        for w in range(n):  # ascending v
            has = (at >> w) & 1 == 1
            sub = at[has] ^ (1 << w)
            l[has] = logaddexp(l[has], L[sub] + alpha[w, squeeze(sub, w)])
            r[has] = logaddexp(r[has], alpha[w, squeeze(full ^ at[has], w)] + R[sub])
        L[at], R[at] = l, r
    gamma = np.empty((n, m))
    for w in range(n):
        inside = unsqueeze(idx, w)
        gamma[w] = L[inside] + R[full ^ inside ^ (1 << w)]
    for b in range(n - 1):
        src = idx[(idx >> b) & 1 == 1]
        gamma[:, src ^ (1 << b)] = logaddexp(gamma[:, src ^ (1 << b)], gamma[:, src])
    if L[full] == -np.inf:
        log_post, log_evidence = np.full(len(s), -np.inf), -np.inf
    else:
        log_post = (centred + gamma[v, squeeze(pm, v)]) - L[full]
        log_evidence = L[full]
        for w in range(n):
            log_evidence = log_evidence + c[w]
    arc = np.zeros((n, n))
    post = np.exp(log_post)
    for u in range(n):
        inside = (pm >> u) & 1 == 1
        arc[u] = np.bincount(v[inside], weights=post[inside], minlength=n)
    out = (log_post, arc, float(log_evidence))
    if not tables:
        return out
    finite = np.concatenate([L[np.isfinite(L)], R[np.isfinite(R)], centred])
    return out + (L, R, centred, float(np.abs(finite).max()) if len(finite) else 0.0)


def all_orders_posterior(n, children, masks, scores):
    """Every linear order of the columns, every choice of one candidate per child whose parents precede it: the weight of a pair
    is prod exp(score) -> (posterior of each candidate float64[n_fam], arc float64[n, n], log_evidence); (zeros, zeros, -inf)
    without a pair.  Linear domain on centred scores, math.fsum: for small scores only."""
    v = [int(x) for x in children]
    pm = [int(x) for x in masks]
    c = centres(n, np.asarray(v, np.int64), scores)
    w = [math.exp(float(s) - c[x]) for s, x in zip(scores, v)]
    per = [[f for f in range(len(v)) if v[f] == x] for x in range(n)]
    terms, z_terms = [[] for _ in v], []
    for order in itertools.permutations(range(n)):
        before, seen = [0] * n, 0
        for x in order:
            before[x], seen = seen, seen | (1 << x)
        fits = [[f for f in per[x] if pm[f] & ~before[x] == 0] for x in range(n)]
        a = [math.fsum(w[f] for f in fs) for fs in fits]
        if min(a) == 0.0:
            continue
        z_terms.append(math.prod(a))
        for x in range(n):
            rest = math.prod(a[y] for y in range(n) if y != x)
            for f in fits[x]:
                terms[f].append(w[f] * rest)
    Z = math.fsum(z_terms)
    if Z == 0.0:
        return np.zeros(len(v)), np.zeros((n, n)), -math.inf
    post = np.array([math.fsum(t) / Z for t in terms])
    arc = np.zeros((n, n))
    for u in range(n):
        for x in range(n):
            arc[u, x] = math.fsum(post[f] for f in per[x] if (pm[f] >> u) & 1)
    return post, arc, math.log(Z) + math.fsum(c)


def random_candidates(n, max_parents, seed, required=(), forbidden=(), scale=5.0):
    """The bounded candidate list of `exact_search` (tests/dag_check.bounded_candidates) with normal scores."""
    from dag_check import bounded_candidates
    cand = bounded_candidates(n, max_parents, required, forbidden)
    rng = np.random.default_rng(seed)
    return [x for x, _ in cand], [p for _, p in cand], rng.normal(0.0, scale, len(cand))


def dense_candidates(n, seed, keep=0.5, scale=1000.0):
    """Every (child, parent set) with about `keep` of them present - the empty sets always, so that a DAG exists -, scores uniform
    in [-scale, 0]: -inf entries everywhere."""
    rng = np.random.default_rng(seed)
    m = 1 << (n - 1)
    i = np.arange(m, dtype=np.int64)
    children = np.concatenate([np.full(m, x, np.int32) for x in range(n)])
    masks = np.concatenate([unsqueeze(i, x) for x in range(n)]).astype(np.uint32)
    pick = (rng.random(len(children)) < keep) | (masks == 0)
    return children[pick], masks[pick], -scale * rng.random(int(pick.sum()))


def forced_chain(n, seed=0):
    """Child 0 has {}, child v only {v - 1}, integer scores: one DAG, one order."""
    rng = np.random.default_rng(seed)
    return list(range(n)), [0] + [1 << (x - 1) for x in range(1, n)], rng.integers(-50, 50, n).astype(np.float64)
