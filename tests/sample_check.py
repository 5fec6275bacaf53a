"""Exact twin of the project's own Philox stream in the approximate-inference kernels (tests/test_sampling_twin.py,
tests/test_sampling_host.py) - numpy only, nothing from sorobn_amd: forward sampling, rejection sampling, likelihood
weighting (sample_kernel) and Gibbs chains (gibbs_kernel in its three update forms, gibbs_kernel8).  Written from the
documented conventions (include/mibn.h, the kernels' comments) as a specification; the kernels have to reproduce it
bit for bit: the same states, the same histograms.

A network here is a `Net`: card [V], scope[v] = the parents of v then v itself, values = every CPT as a dense C-order
table over its scope (v fastest) starting at value_off[v] - the layout of `flatten()` and of mibn_set_network.  Variable
ids are in topological order (every parent has a smaller id).

Every product and sum below is a plain IEEE double operation in the stated order: numpy's elementwise `*` and `+` on
float64 arrays, running sums accumulated state after state.  No fused operations, no pairwise reductions."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
U64 = np.uint64


# ------------------------------------------------------------------------------------------------------------ network

class Net:
    def __init__(self, card, scope, value_off, values):
        self.card = np.asarray(card, np.int32)
        self.scope = [[int(u) for u in sc] for sc in scope]
        self.value_off = np.asarray(value_off, np.int64)
        self.values = np.ascontiguousarray(values, np.float64)
        n = len(self.card)
        assert len(self.scope) == n and len(self.value_off) == n + 1
        self.stride, self.children = [], [[] for _ in range(n)]
        for v, sc in enumerate(self.scope):
            assert sc[-1] == v and all(u < v for u in sc[:-1]), "parents first, then the variable; ids in topological order"
            st, s = [0] * len(sc), 1
            for k in range(len(sc) - 1, -1, -1):
                st[k] = s
                s *= int(self.card[sc[k]])
            assert s == self.value_off[v + 1] - self.value_off[v]
            self.stride.append(st)
            for u in sc[:-1]:
                self.children[u].append(v)  # ascending id: v grows

    # the arguments of Engine.set_network
    def engine_args(self):
        scope_off = np.concatenate([[0], np.cumsum([len(s) for s in self.scope])]).astype(np.int64)
        return self.card, scope_off, np.array([u for s in self.scope for u in s], np.int32), self.value_off, self.values


def from_flat(f):
    """A `flatten()`ed network (card, scope, value_off, values)."""
    return Net(f.card, f.scope, f.value_off, f.values)


def make_net(card, parents, tables):
    """card[v], parents[v] (ids below v), tables[v] = array of shape [*card of the parents, card[v]]."""
    scope = [list(p) + [v] for v, p in enumerate(parents)]
    flat = [np.asarray(t, np.float64).reshape(-1) for t in tables]
    value_off = np.concatenate([[0], np.cumsum([len(t) for t in flat])])
    return Net(card, scope, value_off, np.concatenate(flat))


def joint(net):
    """Dense product of every CPT, axes = variables 0..V-1 (small networks only)."""
    V = len(net.card)
    out = np.ones([1] * V)
    for v, sc in enumerate(net.scope):
        a = net.values[net.value_off[v]:net.value_off[v + 1]].reshape([int(net.card[u]) for u in sc])
        shape = [1] * V
        for u in sc:  # the scope is ascending: parents have smaller ids, v is last
            shape[u] = int(net.card[u])
        assert sc == sorted(sc)
        out = out * a.reshape(shape)
    return out


# ------------------------------------------------------------------------------------------------------------- Philox

def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., Random123) vectorised over uint32 arrays: counter = 4 words, key = 2 words."""
    c = [np.asarray(x, np.uint64) & M32 for x in counter]
    k0, k1 = (np.asarray(x, np.uint64) & M32 for x in key)
    M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> U64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> U64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + U64(0x9E3779B9)) & M32, (k1 + U64(0xBB67AE85)) & M32
    return [x.astype(np.uint32) for x in c]


def uniform_from_words(c0, c1):
    """53 bits of two output words -> a double in [0, 1)."""
    m = ((np.asarray(c0, np.uint64) << U64(21)) ^ (np.asarray(c1, np.uint64) >> U64(11))) & U64((1 << 53) - 1)
    return m.astype(np.float64) * 2.0 ** -53  # both exact: m < 2^53


def philox_uniform(i, stream, k0, k1):
    i = np.asarray(i, np.uint64)
    zero = np.zeros_like(i)
    c = philox4x32_10((i & M32, i >> U64(32), zero + np.asarray(stream, np.uint64), zero), (k0, k1))
    return uniform_from_words(c[0], c[1])


def _seed_words(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


# ------------------------------------------------------------------------------------------------------- forward walk

def _row_offset(net, v, states):
    """Offset of the conditional row of v in `values` for every row of states [n, V]."""
    off = np.full(len(states), int(net.value_off[v]), np.int64)
    for u, s in zip(net.scope[v][:-1], net.stride[v][:-1]):
        off += states[:, u].astype(np.int64) * s
    return off


def _draw(net, rows, uniform):
    """Inverse-CDF draw from unnormalised rows [n, card]: total = the row summed in ascending state order, u = uniform * total,
    the first x with u < running sum, else card - 1."""
    card = rows.shape[1]
    total = np.zeros(len(rows))
    for x in range(card):
        total = total + rows[:, x]
    u = uniform * total
    val = np.full(len(rows), card - 1, np.int64)
    found = np.zeros(len(rows), bool)
    acc = np.zeros(len(rows))
    for x in range(card):
        acc = acc + rows[:, x]
        hit = ~found & (u < acc)
        val[hit] = x
        found |= hit
    return val


def forward(net, n_samples, seed, clamp=None):
    """-> (states uint8 [n, V], likelihood [n]): variable v of sample s is drawn with philox_uniform(s, 2 + v, k0, k1) from its
    conditional row, or takes its clamped value; the likelihood is the product of P(value | parents) over every variable in id
    order, clamped ones included."""
    clamp = dict(clamp or {})
    lo, hi = _seed_words(seed)
    k0, k1 = lo, hi ^ 0x85EBCA6B
    V = len(net.card)
    for v, c in clamp.items():
        if not (0 <= v < V and 0 <= c < net.card[v]):
            raise ValueError("clamp outside the domain")
    s = np.arange(int(n_samples), dtype=np.uint64)
    states = np.zeros((len(s), V), np.uint8)
    lik = np.ones(len(s))
    for v in range(V):
        off = _row_offset(net, v, states)
        if v in clamp:
            val = np.full(len(s), clamp[v], np.int64)
        else:
            rows = net.values[off[:, None] + np.arange(int(net.card[v]))]
            val = _draw(net, rows, philox_uniform(s, 2 + v, k0, k1))
        states[:, v] = val
        lik = lik * net.values[off + val]
    return states, lik


def _cells(net, q, states):
    stride, cells = [0] * len(q), 1
    for i in range(len(q) - 1, -1, -1):
        stride[i] = cells
        cells *= int(net.card[q[i]])
    cell = np.zeros(len(states), np.int64)
    for v, s in zip(q, stride):
        cell += states[:, v].astype(np.int64) * s
    return cell, cells


def rejection(net, q, ev, n_samples, seed):
    """Nothing is clamped; the samples that agree with `ev` {var: code} are counted per joint query cell (C-order over q)."""
    states, _ = forward(net, n_samples, seed)
    keep = np.ones(len(states), bool)
    for v, c in ev.items():
        keep &= states[:, v] == c
    cell, cells = _cells(net, q, states)
    return np.bincount(cell[keep], minlength=cells).astype(np.int64)


def likelihood(net, q, ev, n_samples, seed):
    """`ev` is clamped -> (counts, wsum): per query cell the number of samples and math.fsum of their likelihoods."""
    states, lik = forward(net, n_samples, seed, clamp=ev)
    cell, cells = _cells(net, q, states)
    counts = np.bincount(cell, minlength=cells).astype(np.int64)
    order = np.argsort(cell, kind="stable")
    edges = np.concatenate([[0], np.cumsum(counts)])
    sorted_lik = lik[order]
    wsum = np.array([math.fsum(sorted_lik[a:b]) for a, b in zip(edges[:-1], edges[1:])])
    return counts, wsum


# -------------------------------------------------------------------------------------------------------------- Gibbs

def gibbs_weights(net, v, states):
    """[n, card[v]]: own CPT value times the children's CPT values, children in ascending id, multiplied left to right."""
    x = np.arange(int(net.card[v]), dtype=np.int64)
    w = net.values[_row_offset(net, v, states)[:, None] + x]
    for c in net.children[v]:
        off = np.full(len(states), int(net.value_off[c]), np.int64)
        sv = 0
        for u, s in zip(net.scope[c], net.stride[c]):
            if u == v:
                sv = s
            else:
                off += states[:, u].astype(np.int64) * s
        w = w * net.values[off[:, None] + x * sv]
    return w


def gibbs(net, q, ev, n_chains, n_iterations, seed, cycle=None, chain_first=0):
    """Histogram (int64, C-order over q) of chains [chain_first, chain_first + n_chains): Philox keyed by (seed, chain), a forward
    draw with stream 1 / counter v as the start (evidence clamped), update `it` on cycle position it mod n_cycle with the
    uniform philox_uniform(it, 0), the joint query cell recorded after every update."""
    V = len(net.card)
    ev = dict(ev)
    for v, c in ev.items():
        if not 0 <= c < net.card[v]:
            raise ValueError("evidence outside the domain")
    if cycle is None:
        cycle = [v for v in range(V) if v not in ev]
    assert sorted(cycle) == [v for v in range(V) if v not in ev]
    lo, hi = _seed_words(seed)
    chain = np.arange(int(chain_first), int(chain_first) + int(n_chains), dtype=np.uint64)
    k0 = U64(lo) ^ ((chain * U64(0x9E3779B1)) & M32)
    k1 = U64(hi) ^ (chain >> U64(32)) ^ U64(0x85EBCA6B)
    states = np.zeros((len(chain), V), np.uint8)
    for v in range(V):
        if v in ev:
            states[:, v] = ev[v]
            continue
        rows = net.values[_row_offset(net, v, states)[:, None] + np.arange(int(net.card[v]))]
        states[:, v] = _draw(net, rows, philox_uniform(np.full(len(chain), v, np.uint64), 1, k0, k1))
    _, cells = _cells(net, q, states)
    counts = np.zeros(cells, np.int64)
    for it in range(int(n_iterations)):
        v = cycle[it % len(cycle)]
        w = gibbs_weights(net, v, states)
        card = w.shape[1]
        acc = np.empty_like(w)  # running sums, state after state
        run = np.zeros(len(w))
        for x in range(card):
            run = run + w[:, x]
            acc[:, x] = run
        total = run
        u = philox_uniform(np.full(len(chain), it, np.uint64), 0, k0, k1) * total
        hit = u[:, None] < acc
        first = np.argmax(hit, axis=1)
        last = card - 1 - np.argmax((w > 0)[:, ::-1], axis=1)  # the last state of positive weight
        new = np.where(hit.any(axis=1), first, last)
        move = total > 0  # a conditional without mass keeps the state
        states[move, v] = new[move]
        cell, _ = _cells(net, q, states)
        counts += np.bincount(cell, minlength=cells)
    return counts
