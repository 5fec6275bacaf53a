"""Brute-force twin of the structure-learning extension (score-based hill climbing): numpy `bincount`, `math.lgamma` /
`math.log` and `math.fsum` only, no engine.  The reference has no such search, so - as for MPE, P(e) and EM - the oracle is
this twin: family scores term by term, and a greedy search that rescores every legal move from scratch at every step (no
cache, acyclicity by a fresh depth-first search).  Codes are a [n_rows, n_cols] integer matrix, columns are positions."""
import math

import numpy as np

KINDS = ("loglik", "bic", "aic", "bdeu", "k2")
MOVES = ("add", "delete", "reverse")


def family_table(codes, card, child, parents):
    """Dense counts [q, r]: parents in the given order (first slowest), child fastest."""
    flat = np.zeros(len(codes), np.int64)
    q = 1
    for p in parents:
        flat = flat * int(card[p]) + codes[:, p].astype(np.int64)
        q *= int(card[p])
    r = int(card[child])
    flat = flat * r + codes[:, child].astype(np.int64)
    return np.bincount(flat, minlength=q * r).astype(np.int64).reshape(q, r)


def family_score(codes, card, child, parents, kind="bic", ess=1.0):
    """(score, S): the family's score in natural logs and S = fsum(|term|) over the same terms - the scale rounding errors
    of a sum of those terms are measured against.  Empty configurations and empty cells are no terms."""
    assert kind in KINDS
    t = family_table(codes, card, child, parents)
    q, r = t.shape
    n = len(codes)
    terms = []
    a_q, a_qr = float(ess) / q, float(ess) / (q * r)
    for row in t.tolist():
        nj = sum(row)
        if nj == 0:
            continue
        if kind == "bdeu":
            terms.append(math.lgamma(a_q) - math.lgamma(a_q + nj))
            terms += [math.lgamma(a_qr + c) - math.lgamma(a_qr) for c in row if c]
        elif kind == "k2":
            terms.append(math.lgamma(r) - math.lgamma(r + nj))
            terms += [math.lgamma(1 + c) for c in row if c]
        else:
            terms += [c * (math.log(c) - math.log(nj)) for c in row if c]
    if kind == "bic":
        terms.append(-0.5 * math.log(max(n, 1)) * q * (r - 1))
    elif kind == "aic":
        terms.append(-float(q * (r - 1)))
    return math.fsum(terms), math.fsum(abs(x) for x in terms)


def scorer(codes, card, kind="bic", ess=1.0):
    """(child, parents) -> score; parents in ascending position, as the product orders a family."""
    return lambda child, parents: family_score(codes, card, child, sorted(parents), kind, ess)[0]


def has_cycle(n, parents):
    """Fresh depth-first search over the parent sets."""
    state = [0] * n

    def visit(v):
        if state[v] == 1:
            return True
        if state[v] == 2:
            return False
        state[v] = 1
        if any(visit(p) for p in parents[v]):
            return True
        state[v] = 2
        return False

    return any(visit(v) for v in range(n))


def apply_move(parents, op, u, v):
    """A copy of the parent sets after `op` on the edge u -> v."""
    new = [set(p) for p in parents]
    if op == "add":
        new[v].add(u)
    elif op == "delete":
        new[v].discard(u)
    else:
        new[v].discard(u)
        new[u].add(v)
    return new


def is_legal(n, parents, op, u, v, max_parents=3, required=(), forbidden=()):
    if u == v:
        return False
    if op == "add":
        if u in parents[v] or (u, v) in forbidden or len(parents[v]) >= max_parents:
            return False
    elif op == "delete":
        if u not in parents[v] or (u, v) in required:
            return False
    elif op == "reverse":
        if u not in parents[v] or (u, v) in required or (v, u) in forbidden or len(parents[u]) >= max_parents:
            return False
    else:
        return False
    return not has_cycle(n, apply_move(parents, op, u, v))


def move_gain(score, parents, op, u, v):
    """The same arithmetic as the product: every family's new score minus its old one, a reversal = the deletion's
    difference plus the addition's."""
    if op == "add":
        return score(v, parents[v] | {u}) - score(v, parents[v])
    if op == "delete":
        return score(v, parents[v] - {u}) - score(v, parents[v])
    return (score(v, parents[v] - {u}) - score(v, parents[v])) + (score(u, parents[u] | {v}) - score(u, parents[u]))


def legal_moves(n, parents, max_parents=3, required=(), forbidden=()):
    """In the order equal gains are preferred: add before delete before reverse, then child, then parent."""
    return [(op, u, v) for op in MOVES for v in range(n) for u in range(n)
            if is_legal(n, parents, op, u, v, max_parents, required, forbidden)]


def best_move(score, n, parents, max_parents=3, required=(), forbidden=()):
    """(gain, op, u, v) of the best legal move - the first of the largest gain in `legal_moves` order - and the gain of
    the runner-up (-inf if there is none); None without a legal move."""
    moves = legal_moves(n, parents, max_parents, required, forbidden)
    if not moves:
        return None, -math.inf
    gains = [move_gain(score, parents, *m) for m in moves]
    k = max(range(len(moves)), key=lambda i: (gains[i], -i))
    second = max([g for i, g in enumerate(gains) if i != k], default=-math.inf)
    return (gains[k], *moves[k]), second


def hill_climb(score, n, max_parents=3, start=(), required=(), forbidden=(), max_iter=None, epsilon=1e-4):
    """-> (parent sets, trace [(op, u, v, gain)], total score, smallest gap between the best two gains of a step)."""
    parents = [set() for _ in range(n)]
    for u, v in [*start, *required]:
        parents[v].add(u)
    assert not has_cycle(n, parents)
    trace, gap = [], math.inf
    while max_iter is None or len(trace) < max_iter:
        best, second = best_move(score, n, parents, max_parents, set(required), set(forbidden))
        if best is None or not best[0] > epsilon:
            break
        gap = min(gap, best[0] - second)
        gain, op, u, v = best
        parents = apply_move(parents, op, u, v)
        trace.append((op, u, v, gain))
    total = math.fsum(score(v, parents[v]) for v in range(n))
    return parents, trace, total, gap


def edges_of(parents):
    return {(u, v) for v, ps in enumerate(parents) for u in ps}


# ------------------------------------------------------------------------- test doubles and data for the host tests
class TwinDataset:
    """TEST DOUBLE for _capi.Dataset (never on the product path): scores by the twin, records what was asked."""

    def __init__(self, codes, card, log):
        self.codes, self.card, self.log = np.asarray(codes), [int(c) for c in card], log

    def score_families(self, families, kind="bic", ess=1.0):
        self.log.append([tuple(f) for f in families])
        return np.array([family_score(self.codes, self.card, f[-1], list(f[:-1]), kind, ess)[0] for f in families], np.float64)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


class TwinEngine:
    """TEST DOUBLE for the counting engine: `dataset` -> TwinDataset; `calls` lists the family batches of every call."""

    def __init__(self):
        self.calls = []

    def dataset(self, codes, card):
        return TwinDataset(codes, card, self.calls)


def forward_sample(spec, n_rows, seed):
    """Rows from a netspec network by a small numpy forward sampler: (column names = spec["nodes"], codes [n_rows, n_vars]
    uint8 over the sorted label domains, cards).  A parent configuration whose CPT rows are all missing or zero is
    sampled uniformly (the rows only have to be data)."""
    import netspec
    rng = np.random.default_rng(seed)
    dom = netspec.domains(spec)
    names = list(spec["nodes"])
    parents = {nm: [c for c in spec["cpts"][nm]["names"][:-1]] for nm in names}
    done, order = set(), []
    while len(order) < len(names):
        for nm in names:
            if nm not in done and all(p in done for p in parents[nm]):
                done.add(nm)
                order.append(nm)
    col = {}
    for nm in order:
        r = len(dom[nm])
        shape = [len(dom[p]) for p in parents[nm]]
        table = np.zeros((int(np.prod(shape)) if shape else 1, r))
        for row in spec["cpts"][nm]["rows"]:
            j = 0
            for p, lab in zip(parents[nm], row[:-2]):
                j = j * len(dom[p]) + dom[p].index(lab)
            table[j, dom[nm].index(row[-2])] = row[-1]
        table[table.sum(axis=1) <= 0] = 1.0
        j = np.zeros(n_rows, np.int64)
        for p in parents[nm]:
            j = j * len(dom[p]) + col[p]
        cdf = np.cumsum(table[j], axis=1)
        x = rng.random(n_rows) * cdf[:, -1]
        col[nm] = np.minimum((x[:, None] >= cdf).sum(axis=1), r - 1)
    codes = np.stack([col[nm] for nm in names], axis=1).astype(np.uint8)
    return names, codes, [len(dom[nm]) for nm in names]
