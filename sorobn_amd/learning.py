"""Parameter and structure learning on grouped counts.

The reference learns CPTs with `X.groupby([*parents, node]).size()` per node (sorobn/bayes_net.py:467-516) and a
Chow-Liu tree from the pairwise `X.groupby([u, v]).size()` (sorobn/structure.py:9-63).  Here the label columns are
factorised once on the host (sorted label domains -> uint8 codes) and *all* contingency tables of a call are counted
by one launch of the count kernel (csrc/count_kernel.hip.h, `mibn_count_tables`); the small tables that come back are
turned into the same pandas objects on the host.  No CPU fallback: counting needs a gfx950 device.
"""
import itertools
import math

import numpy as np
import pandas as pd

from . import _capi
from .events import csr_rows

_engines = {}


def counting_engine(device=None):
    """One engine per device, used only for `count_tables` (no network attached)."""
    from .bayes_net import _default_device
    d = _default_device() if device is None else device
    if d not in _engines:
        _engines[d] = _capi.Engine(d)
    return _engines[d]


def encode_columns(X, columns):
    """Label columns -> (uint8 codes [n_rows, n_cols], sorted label domains, cards).  Missing values (NaN / None / NaT)
    are NOT labels: pandas' `groupby(...).size()` and `value_counts()` drop them (dropna=True), so they get the extra
    code len(domain) - `cards[j]` is then len(domain) + 1 - and `count_tables_dropna` cuts that slice off every table.
    More than 256 codes per column is outside what the count kernel (and any CPT one would learn) handles."""
    codes = np.empty((len(columns), len(X)), np.uint8)  # filled column by column: column-major, as the count kernel reads it
    domains, cards = [], []
    for j, c in enumerate(columns):
        v = X[c].to_numpy()
        col = dom = None
        has_na = False
        if v.dtype.kind in "iub" and len(v):  # small integer range: a lookup table instead of hashing (no NA possible)
            iv = v.view(np.uint8) if v.dtype.kind == "b" else v
            lo, hi = int(iv.min()), int(iv.max())
            if hi - lo < (1 << 16):
                shifted = iv.astype(np.int64) - lo  # (in int64: narrow signed dtypes would wrap, e.g. int8 100 - (-100))
                present = np.zeros(hi - lo + 1, bool)
                present[shifted] = True
                dom = (np.flatnonzero(present) + lo).astype(v.dtype)
                if len(dom) <= 256:
                    col = (np.cumsum(present) - 1).astype(np.uint8)[shifted]
        if col is None:
            col, dom = pd.factorize(v, sort=True, use_na_sentinel=True)  # one hash pass per column; NA -> -1
            has_na = bool((col < 0).any())
            if has_na:
                col = np.where(col < 0, len(dom), col)
        if len(dom) + int(has_na) > 256:
            raise ValueError(f"column {c!r} has {len(dom)} distinct labels (max 256)")
        codes[j] = col
        domains.append(pd.Index(dom, name=c))
        cards.append(len(dom) + int(has_na))
    return codes.T, domains, cards


def count_tables_dropna(engine, codes, domains, cards, tables, **more):
    """Dense contingency tables over the *labels*: rows with a missing value in any of a table's columns are dropped
    (the NA slice, where a column has one, is cut off) - pandas' dropna=True."""
    dense = engine.count_tables(codes, cards, tables, **more)
    out = []
    for d, t in zip(dense, tables):
        cut = tuple(slice(0, len(domains[c])) for c in t)
        out.append(np.ascontiguousarray(d[cut]) if any(cards[c] != len(domains[c]) for c in t) else d)
    return out


def count_series(counts, domains, names):
    """Dense contingency table -> the Series `groupby(names).size()` returns: one row per observed combination."""
    flat = counts.reshape(-1)
    keep = np.flatnonzero(flat)
    if len(names) == 1:
        return pd.Series(flat[keep], index=domains[0][keep].rename(names[0]))
    codes = np.unravel_index(keep, counts.shape)
    idx = pd.MultiIndex(levels=[d.rename(n) for d, n in zip(domains, names)], codes=list(codes), names=list(names),
                        verify_integrity=False)
    return pd.Series(flat[keep], index=idx)


def row_weights(X, weights):
    """The `weights` argument of the learning calls -> (X without the weight column, uint32 weights or None).  A weight vector
    is 1-D, of length len(X), and holds non-negative integers (floats only when integral) whose sum is at most 2^32 - 1: row
    i counts weights[i] times, exactly as if it were written out that often - except that the label domains (and with them
    the cardinalities in BIC / AIC / BDeu) are those of ALL rows of X, weight 0 included.  Alternatively the NAME of a column
    of X: that column is the weight and not a variable (aggregated data: one row per pattern plus a frequency).  Anything
    else is a ValueError.  None -> (X, None): the unweighted path."""
    if weights is None:
        return X, None
    if isinstance(weights, (str, bytes)) or np.isscalar(weights):
        if weights not in X.columns:
            raise ValueError(f"weights: X has no column {weights!r}")
        w, X = X[weights].to_numpy(), X.drop(columns=[weights])
    else:
        w = weights.to_numpy() if hasattr(weights, "to_numpy") else np.asarray(weights)
    if w.ndim != 1 or len(w) != len(X):
        raise ValueError(f"weights must be one-dimensional with one entry per row of X ({len(X)})")
    if w.dtype.kind == "b" or w.dtype.kind not in "iuf":
        raise ValueError("weights must be non-negative integers")
    if w.dtype.kind == "f" and not (np.isfinite(w).all() and (w == np.floor(w)).all()):
        raise ValueError("weights must be integral (real-valued weights are not supported)")
    if len(w) and w.min() < 0:
        raise ValueError("weights must not be negative")
    if math.fsum(w.tolist()) > _capi.MAX_WEIGHT_SUM:
        raise ValueError("weights sum to more than 2^32 - 1")
    return X, w.astype(np.uint32)


def grouped_counts(X, tables, device=None, weights=None):
    """`tables`: list of column-name tuples -> list of `X.groupby(list(t)).size()`-like Series, one GPU launch.  `weights`
    (uint32 per row, from `row_weights`): row i counts weights[i] times."""
    columns = sorted({c for t in tables for c in t}, key=list(X.columns).index)
    codes, domains, cards = encode_columns(X, columns)
    pos = {c: j for j, c in enumerate(columns)}
    more = {} if weights is None else {"weights": weights}
    dense = count_tables_dropna(counting_engine(device), codes, domains, cards, [tuple(pos[c] for c in t) for t in tables], **more)
    return [count_series(d, [domains[pos[c]] for c in t], list(t)) for d, t in zip(dense, tables)]


# ------------------------------------------------------------------------------------------------ rank 3: fit
def partial_fit(bn, X, weights=None):
    """BayesNet.partial_fit (bayes_net.py:467-510): update every CPT with the rows of X.  Exact integer counts are
    kept per node (`bn._counts`), so fitting in chunks gives bit-identical CPTs to fitting at once.  `weights`: see
    `row_weights` - the counts are those of the rows written out weights[i] times."""
    X, weights = row_weights(X, weights)
    if not hasattr(bn, "_counts") or bn._counts is None:
        bn._counts = {}
    tables = [tuple([*bn.parents[c], c]) for c in bn.parents] + [(r,) for r in bn.roots]
    fresh = grouped_counts(X, tables, device=getattr(bn, "_device", None), weights=weights)
    for names, new in zip(tables, fresh):
        node = names[-1]
        new = new.astype(np.float64)
        if node in bn._counts:
            counts = bn._counts[node].add(new, fill_value=0.0)
        else:
            counts = new
            if bn.prior_count and len(names) > 1:
                # the reference adds ONE pseudo-count for every combination of the values seen in this chunk, whatever
                # prior_count is (bayes_net.py:480-488)
                combos = pd.MultiIndex.from_tuples(list(itertools.product(*[X[v].unique() for v in names])), names=list(names))
                counts = counts.add(pd.Series(1.0, combos), fill_value=0.0)
        bn._counts[node] = counts
        if len(names) > 1:
            bn.P[node] = counts / counts.groupby(level=list(names[:-1])).transform("sum")
        else:
            # Deliberate deviation for a ROOT column with missing values (NaN / None): the reference divides the counts of
            # the observed labels by the number of ROWS seen so far (`_P_sizes[root] += len(X)`, bayes_net.py:503-508), so
            # its P(root) sums to less than 1 when rows were missing; here the CPT stays a distribution (counts / their
            # sum).  Without missing values in the column the two agree exactly.
            bn.P[node] = counts / counts.sum()
    bn.prepare()
    return bn


def fit(bn, X, weights=None):
    """BayesNet.fit (bayes_net.py:512-516)."""
    X, weights = row_weights(X, weights)
    bn.P = {}
    bn._counts = {}
    return partial_fit(bn, X, weights=weights)


# ------------------------------------------------------------------------------------------- rank 4: Chow-Liu
def mutual_information(X, device=None):
    """All pairwise mutual informations (structure.py:33-45, 55-63) from one counting launch: {(u, v): mi} for u < v."""
    cols = sorted(X.columns)
    codes, domains, cards = encode_columns(X, cols)
    pairs = list(itertools.combinations(range(len(cols)), 2))
    dense = count_tables_dropna(counting_engine(device), codes, domains, cards, [(j,) for j in range(len(cols))] + pairs)
    n = float(len(X))
    # value_counts(normalize=True) divides by the non-missing rows of the column, groupby().size() / len(X) by all rows
    # (structure.py:33-41)
    marg = [d / float(d.sum()) if d.sum() else d.astype(np.float64) for d in dense[:len(cols)]]
    out = {}

    def one(i, j, c):
        puv = c / n
        nz = puv > 0
        ratio = puv[nz] / (marg[j][None, :].repeat(len(marg[i]), 0)[nz] * marg[i][:, None].repeat(len(marg[j]), 1)[nz])
        return float((puv[nz] * np.log(ratio)).sum())

    # pairs whose table has no empty cell (the usual case with many rows) are evaluated together, shape by shape -
    # the same elementwise arithmetic and the same row sums as `one`, bit for bit; the others go through `one`
    by_shape = {}
    for k, (i, j) in enumerate(pairs):
        by_shape.setdefault(dense[len(cols) + k].shape, []).append(k)
    mi = np.empty(len(pairs), np.float64)
    for shape, ks in by_shape.items():
        c = np.stack([dense[len(cols) + k] for k in ks])
        full = (c > 0).reshape(len(ks), -1).all(axis=1)
        if full.any():
            sel = np.flatnonzero(full)
            pi = np.stack([marg[pairs[ks[t]][0]] for t in sel])[:, :, None]
            pj = np.stack([marg[pairs[ks[t]][1]] for t in sel])[:, None, :]
            puv = c[sel] / n
            mi[np.asarray(ks)[sel]] = (puv * np.log(puv / (pj * pi))).reshape(len(sel), -1).sum(axis=1)
        for t in np.flatnonzero(~full):
            k = ks[t]
            mi[k] = one(pairs[k][0], pairs[k][1], dense[len(cols) + k])
    for k, (i, j) in enumerate(pairs):
        out[(cols[i], cols[j])] = float(mi[k])
    return out


def chow_liu(X, root=None, device=None):
    """structure.chow_liu (structure.py:9-52): maximum spanning tree of the mutual-information graph (Kruskal with a
    union-find over the edges in descending MI order, ties in sorted-pair order like the reference's stable sort),
    oriented away from `root` (default: the first column).  Returns (parent, child) tuples.  Like the reference's
    `kruskal` (structure.py:108-117) the scan stops as soon as every vertex has a neighbour - which can be before the
    components are joined: the result is then the part of that forest reachable from `root`.
    The ORDER of the returned edge list is unspecified (the reference orients the tree by iterating Python sets, the order
    depends on the hash seed): compare trees as sets of directed edges.
    """
    mi = mutual_information(X, device=device)
    ranked = sorted(mi, key=lambda e: mi[e], reverse=True)  # stable: equal MI keeps combinations() order
    leader = {v: v for v in X.columns}

    def find(v):
        while leader[v] != v:
            leader[v] = leader[leader[v]]
            v = leader[v]
        return v

    size = {v: 1 for v in X.columns}
    adj = {v: [] for v in X.columns}
    touched = 0  # vertices with at least one neighbour
    for u, v in ranked:
        a, b = find(u), find(v)
        if a != b:
            touched += (not adj[u]) + (not adj[v])
            adj[u].append(v)
            adj[v].append(u)
            if size[a] < size[b]:
                a, b = b, a
            leader[b] = a
            size[a] += size[b]
        if touched == len(X.columns):  # structure.py:116-117
            break
    root = X.columns[0] if root is None else root
    edges, stack, seen = [], [root], {root}
    while stack:
        u = stack.pop()
        for v in adj[u]:
            if v not in seen:
                seen.add(v)
                edges.append((u, v))
                stack.append(v)
    return edges


# ------------------------------------------------------------------- EM: CPTs from rows with missing values
# An extension (the reference's fit drops every row that is incomplete in a family): expectation-maximisation with the
# expected counts accumulated on the device (csrc/expect_kernel.hip.h, `mibn_expect_batch`).
EM_MAX_MISSING = 8  # missing members of one family in one row = query variables of one expect request (kExpectMaxQ)
EM_INITS = ("auto", "current", "counts", "uniform")


def em_family_layout(scopes, card):
    """Families back to back in one accumulation buffer: scopes[v] = variable ids of family v (node last) ->
    (fam_off [V + 1], strides: per family the C-order strides of its members, in cells)."""
    fam_off, strides = [0], []
    for sc in scopes:
        st = np.ones(len(sc), np.int64)
        for k in range(len(sc) - 2, -1, -1):
            st[k] = st[k + 1] * int(card[sc[k + 1]])
        strides.append(st)
        fam_off.append(fam_off[-1] + int(st[0]) * int(card[sc[0]]))
    return np.asarray(fam_off, np.int64), strides


def em_requests(codes, rows, scopes, strides, fam_off):
    """The expect requests of the rows `rows` (indices into `codes` [n_rows, V], -1 = not observed), family-major: for
    every family, in family order, and every row of `rows`, in their order, that misses a member of it - query = the
    missing members (scope order), evidence = every observed column of the row (ascending id), target = the family's
    table with the observed members' codes folded into the base.  Rows without any such family follow with one request
    of no query variable each (it yields the row's P(e)).  Pure numpy on whole columns.
    -> dict: q_off, q_vars, e_off, e_vars, e_codes, acc_base, acc_stride, row (the row of every request)."""
    rows = np.asarray(rows, np.int64)
    sub = codes[rows]
    seen = sub >= 0
    V = codes.shape[1]
    ids = np.arange(V, dtype=np.int32)
    nq, qv, qs, base, who = [], [], [], [], []
    covered = np.zeros(len(rows), bool)
    for v, sc in enumerate(scopes):
        sc = np.asarray(sc, np.int64)
        miss = ~seen[:, sc]
        need = np.flatnonzero(miss.any(axis=1))
        if not len(need):
            continue
        m = miss[need]
        covered[need] = True
        nq.append(m.sum(axis=1))
        qv.append(np.broadcast_to(sc.astype(np.int32), m.shape)[m])
        qs.append(np.broadcast_to(strides[v], m.shape)[m])
        base.append(fam_off[v] + (np.where(m, 0, sub[need][:, sc]) * strides[v]).sum(axis=1))
        who.append(need)
    rest = np.flatnonzero(~covered)
    if len(rest):
        nq.append(np.zeros(len(rest), np.int64))
        base.append(np.zeros(len(rest), np.int64))
        who.append(rest)
    who = np.concatenate(who) if who else np.zeros(0, np.int64)
    nq = np.concatenate(nq) if nq else np.zeros(0, np.int64)
    ev = seen[who]
    return {
        "q_off": np.concatenate([[0], np.cumsum(nq)]).astype(np.int64),
        "q_vars": np.concatenate(qv).astype(np.int32) if qv else np.zeros(0, np.int32),
        "e_off": np.concatenate([[0], np.cumsum(ev.sum(axis=1))]).astype(np.int64),
        "e_vars": np.broadcast_to(ids, ev.shape)[ev],
        "e_codes": sub[who][ev].astype(np.int32),
        "acc_base": np.concatenate(base).astype(np.int64) if base else np.zeros(0, np.int64),
        "acc_stride": np.concatenate(qs).astype(np.int64) if qs else np.zeros(0, np.int64),
        "row": rows[who],
    }


def em_sub_batches(codes, scopes, sub_batch):
    """Rows ordered pattern group by pattern group (rows with the same observed columns together; patterns in the order of
    `np.unique(seen, axis=0)`, column 0 most significant, rows ascending within a pattern) and cut into runs of at most
    `sub_batch` requests (a row makes one request per family it is incomplete in, at least one): list of row-index arrays.
    The order fixes the order in which expected counts are accumulated, and with it the last bits of `fit_em`: it is this
    function's own, not that of `events.pattern_groups`."""
    seen = codes >= 0
    n = len(codes)
    if n == 0:
        return []
    if seen.shape[1]:
        _, inv = np.unique(seen, axis=0, return_inverse=True)
        order = np.argsort(np.asarray(inv).reshape(-1), kind="stable")
    else:
        order = np.arange(n)
    per_row = np.zeros(n, np.int64)
    for sc in scopes:
        per_row += ~seen[:, np.asarray(sc, np.int64)].all(axis=1)
    cum = np.cumsum(np.maximum(per_row, 1)[order])
    out, start, done = [], 0, 0
    while start < n:
        stop = int(np.searchsorted(cum, done + max(1, int(sub_batch)), side="right"))
        stop = max(stop, start + 1)  # (a single row with more families than sub_batch still goes through)
        out.append(order[start:stop])
        done = int(cum[stop - 1])
        start = stop
    return out


def em_mstep(counts, theta, card_node, prior_count=0.0):
    """theta = (N + prior_count) / row sums over the node's states; a parent configuration with zero mass keeps its
    previous row.  counts / theta: flat family tables (node fastest)."""
    n = np.asarray(counts, np.float64).reshape(-1, int(card_node)) + float(prior_count)
    mass = n.sum(axis=1, keepdims=True)
    prev = np.asarray(theta, np.float64).reshape(-1, int(card_node))
    with np.errstate(divide="ignore", invalid="ignore"):
        new = np.where(mass > 0, n / mass, prev)
    return new.reshape(-1)


def _em_series(node, parents, domains, values):
    """Dense family table -> the CPT Series in the layout `prepare()` stores (levels [*parents, node], sorted)."""
    if parents:
        idx = pd.MultiIndex.from_product([*[domains[p] for p in parents], domains[node]], names=[*parents, node])
        name = f"P({node} | {', '.join(map(str, parents))})"
    else:
        idx = pd.Index(domains[node], name=node)
        name = f"P({node})"
    return pd.Series(np.asarray(values, np.float64), index=idx, name=name)


def _em_current(bn, nodes, observed_domains):
    """(domains, thetas) of the net's CPTs as prepared, or a string saying why they cannot start EM: every node needs a
    CPT over [*parents, node] with every row present and summing to 1, whose labels cover the observed ones."""
    from .flatten import flatten
    if not bn.P or any(n not in bn.P for n in nodes):
        return "a node has no CPT"
    try:
        bn.prepare()
        f = flatten(bn)
    except (ValueError, KeyError, TypeError) as e:
        return f"the CPTs do not flatten ({e})"
    if list(f.names) != list(nodes):
        return "the CPTs name variables outside the structure"
    domains, thetas = {}, []
    for v, node in enumerate(nodes):
        if list(f.scope[v]) != [f.id[p] for p in bn.parents.get(node, [])] + [v]:
            return f"the CPT of {node!r} is not over its parents and itself"
        a, b = int(f.value_off[v]), int(f.value_off[v + 1])
        rows = np.asarray(f.values[a:b], np.float64).reshape(-1, int(f.card[v]))
        if not (np.all(f.present[a:b] == 1.0) and np.all(np.abs(rows.sum(axis=1) - 1.0) <= 1e-9)):
            return f"the CPT of {node!r} lacks a row or has a row that does not sum to 1 (EM learns dense CPTs)"
        dom = pd.Index(f.domains[v], name=node)
        seen = observed_domains.get(node)
        if seen is not None and len(seen) and (dom.get_indexer(seen) < 0).any():
            return f"the CPT of {node!r} does not cover the labels observed in its column"
        domains[node] = dom
        thetas.append(rows.reshape(-1).copy())
    return domains, thetas


EM_ALGORITHMS = ("exact", "lbp")


def fit_em(bn, X, n_iter=20, tol=1e-6, prior_count=0.0, init="auto", sub_batch=32768, algorithm="exact", bp_iterations=100, bp_tol=1e-9,
           damping=0.0):
    """CPTs from rows with missing values (NaN / None = not observed in that row) by expectation-maximisation.

    The structure is the net's.  A column's labels are the sorted labels observed in it (with `init="current"`: the
    labels of the CPTs in place, which must cover them); a node whose column is absent from X or entirely missing is a
    latent variable and needs CPTs in place.  Every iteration: the E-step adds, for every row and family, the posterior
    of the family's members given everything the row observes to the family's table - families complete in a row by
    the count kernel (once), the others as exact queries whose posteriors are accumulated on the device
    (`Engine.expect_batch`) - then theta = (N + prior_count) / row sums; a parent configuration without mass keeps its
    previous row.  A row may miss at most EM_MAX_MISSING members of one family.

    init: "current" (bn.P as prepared), "counts" (the available-case counts of `fit` + 1 in every cell), "uniform",
    "auto" ("current" where it applies, else "counts").  Stops after n_iter iterations or when the log-likelihood gains
    less than tol * |ll|.  Leaves bn.em_log_likelihood_ (the observed-data log-likelihood of the parameters each E-step
    STARTED from), bn.em_iterations_ and bn._counts (the last expected counts).  A row of probability zero under the
    current parameters contributes no counts and makes that iteration's entry -inf.

    algorithm="lbp": an APPROXIMATE E-step for networks on which the exact one is refused (a 20 x 20 grid) - one request of loopy
    belief propagation per row (`Engine.bp_evidence_batch`: at most `bp_iterations` flooding sweeps, `bp_tol`, `damping`), rows in
    X's order in engine calls of `sub_batch`; every family of every row receives its belief, so there is no count-kernel pass and
    no limit on the missing members of a family, and bn.em_log_likelihood_ holds the sums of the rows' Bethe log_z.  Exact on
    polytrees.  On a network with loops the E-step has no error bound, and the recorded log-likelihood NEED NOT BE MONOTONE: the
    stopping rule is the same, so it may stop at a decrease."""
    if int(n_iter) < 1:
        raise ValueError("n_iter must be at least 1")
    if algorithm not in EM_ALGORITHMS:
        raise ValueError(f"algorithm must be one of {EM_ALGORITHMS}, not {algorithm!r}")
    lbp = algorithm == "lbp"
    if lbp:
        if int(bp_iterations) != bp_iterations or bp_iterations < 1:
            raise ValueError("bp_iterations must be an integer >= 1")
        if not bp_tol >= 0:
            raise ValueError("bp_tol must be a number >= 0")
        if not 0 <= damping < 1:
            raise ValueError("damping must be in [0, 1)")
    if not float(prior_count) >= 0:
        raise ValueError("prior_count must not be negative")
    if init not in EM_INITS:
        raise ValueError(f"init must be one of {EM_INITS}, not {init!r}")
    nodes = list(bn.nodes)
    for c in X.columns:
        if c not in nodes:
            raise KeyError(c)
    V, n = len(nodes), len(X)
    vid = {node: v for v, node in enumerate(nodes)}
    present = [node for node in nodes if node in X.columns]
    raw, seen_dom, _ = encode_columns(X, present) if present else (np.zeros((n, 0), np.uint8), [], [])
    observed = {node: seen_dom[j] for j, node in enumerate(present)}
    latent = [node for node in nodes if node not in observed or not len(observed[node])]
    current = _em_current(bn, nodes, observed) if init in ("auto", "current") else "not asked for"
    if isinstance(current, str):
        if init == "current":
            raise ValueError(f"init='current': {current}")
        if latent:
            raise ValueError(f"{latent[0]!r} is never observed: a latent variable needs CPTs in place (init='current'; {current})")
        domains = {node: observed[node] for node in nodes}
        thetas = None
    else:
        domains, thetas = current
    card = np.array([len(domains[node]) for node in nodes], np.int32)
    scopes = [[vid[p] for p in bn.parents.get(node, [])] + [v] for v, node in enumerate(nodes)]
    fam_off, strides = em_family_layout(scopes, card)
    # codes in the final domains, -1 = not observed
    codes = np.full((n, V), -1, np.int32)
    for j, node in enumerate(present):
        if not len(observed[node]):
            continue
        lut = np.append(domains[node].get_indexer(observed[node]), -1).astype(np.int32)  # (the NA code: one past the labels)
        codes[:, vid[node]] = lut[raw[:, j]]
    seen = codes >= 0
    for v, sc in enumerate(scopes):
        if not lbp and n and int((~seen[:, sc]).sum(axis=1).max()) > EM_MAX_MISSING:
            raise ValueError(f"a row misses more than {EM_MAX_MISSING} members of the family of {nodes[v]!r} "
                             f"(the engine takes at most {EM_MAX_MISSING} query variables per expect request)")
    # families complete in a row: counted once (they do not change between iterations)
    full = [v for v in range(V) if all(nodes[u] not in latent for u in scopes[v])]
    hard = np.zeros(int(fam_off[-1]), np.float64)
    if n and full and (not lbp or (thetas is None and init != "uniform")):  # (lbp: only the start of init="counts" reads them)
        na = np.where(seen, codes, card[None, :]).astype(np.uint8)
        cards_na = card + (~seen).any(axis=0)
        if int(cards_na.max()) > 256:
            raise ValueError("a column has 256 labels and missing values (max 256 codes)")
        dense = count_tables_dropna(counting_engine(getattr(bn, "_device", None)), np.asfortranarray(na),
                                    [domains[node] for node in nodes], cards_na, [tuple(scopes[v]) for v in full])
        for v, d in zip(full, dense):
            hard[fam_off[v]:fam_off[v + 1]] = d.reshape(-1)
    if thetas is None:
        if init == "uniform":
            thetas = [np.full(int(fam_off[v + 1] - fam_off[v]), 1.0 / int(card[v])) for v in range(V)]
        else:
            thetas = [em_mstep(hard[fam_off[v]:fam_off[v + 1]] + 1.0, np.zeros(int(fam_off[v + 1] - fam_off[v])), card[v])
                      for v in range(V)]
    batches = [] if lbp else em_sub_batches(codes, scopes, sub_batch)
    requests = None if len(batches) > 8 else [em_requests(codes, rows, scopes, strides, fam_off) for rows in batches]
    lls, counts = [], hard
    ids, step = np.arange(V, dtype=np.int32), max(1, int(sub_batch))
    for it in range(int(n_iter)):
        bn.P = {node: _em_series(node, bn.parents.get(node, []), domains, thetas[v]) for v, node in enumerate(nodes)}
        bn.prepare()
        eng = bn.backend.engine
        acc = np.zeros(int(fam_off[-1]), np.float64)
        if lbp:  # one request per row, in X's order: its family beliefs are the expected counts of EVERY family of the row
            log_z = np.zeros(n, np.float64)
            for s in range(0, n, step):
                rows = slice(s, s + step)
                log_z[rows] = eng.bp_evidence_batch(*csr_rows(ids, codes[rows], seen[rows]), int(bp_iterations), bp_tol, damping, acc=acc)[0]
            counts = acc
            lls.append(float(log_z.sum()) if n else 0.0)
        else:
            p_row = np.zeros(n, np.float64)
            for k, rows in enumerate(batches):
                rq = requests[k] if requests is not None else em_requests(codes, rows, scopes, strides, fam_off)
                p = eng.expect_batch(rq["q_off"], rq["q_vars"], rq["e_off"], rq["e_vars"], rq["e_codes"], rq["acc_base"],
                                     rq["acc_stride"], acc)
                p_row[rq["row"][::-1]] = p[::-1]  # (any of a row's requests carries its P(e): the first one stays)
            counts = acc + hard
            dead = np.flatnonzero(~(p_row > 0))
            if len(dead):  # rows of probability zero contribute nothing: their complete families come off again
                for v in full:
                    sc = np.asarray(scopes[v], np.int64)
                    ok = dead[seen[dead][:, sc].all(axis=1)]
                    np.subtract.at(counts, fam_off[v] + (codes[ok][:, sc] * strides[v]).sum(axis=1), 1.0)
            with np.errstate(divide="ignore"):
                lls.append(float(np.log(p_row).sum()) if n else 0.0)
        thetas = [em_mstep(counts[fam_off[v]:fam_off[v + 1]], thetas[v], card[v], prior_count) for v in range(V)]
        if it and np.isfinite(lls[-1]) and np.isfinite(lls[-2]) and lls[-1] - lls[-2] < float(tol) * abs(lls[-1]):
            break
    bn.P = {node: _em_series(node, bn.parents.get(node, []), domains, thetas[v]) for v, node in enumerate(nodes)}
    bn.prepare()
    bn._counts = {node: _em_series(node, bn.parents.get(node, []), domains, counts[fam_off[v]:fam_off[v + 1]]).rename(None)
                  for v, node in enumerate(nodes)}
    bn.em_log_likelihood_ = lls
    bn.em_iterations_ = len(lls)
    return bn


# ------------------------------------------------------ score-based structure learning: greedy hill climbing
# An extension (the reference learns no structure but the Chow-Liu tree).  The rows go to the device once
# (`Engine.dataset`); the search below runs on the host and sends batches of families, one double per family comes back
# (csrc/score_kernel.hip.h, `mibn_score_families`).
SCORES = tuple(_capi.SCORE_KINDS)
MOVES = ("add", "delete", "reverse")  # also the order in which equal gains are preferred


def _check_score(score, ess):
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, not {score!r}")
    if not (float(ess) > 0 and np.isfinite(float(ess))):
        raise ValueError("ess (the equivalent sample size of the bdeu score) must be a finite number above 0")


def encode_complete(X, columns):
    """`encode_columns` for complete data: a missing value in any of `columns` is an error (scores are defined on
    complete rows; `fit_em` learns parameters from incomplete ones)."""
    codes, domains, cards = encode_columns(X, columns)
    for c, dom, card in zip(columns, domains, cards):
        if card != len(dom):
            raise ValueError(f"column {c!r} has missing values: structure scores need complete data "
                             f"(fit_em learns the parameters of a given structure from incomplete rows)")
    return codes, domains, cards


def _weighted(ds, weights):
    """The keyword of `Dataset.score_families` / `ci_tests` for n tables of a call under `weights` - which become set 0 of
    the data set; none without weights: the unweighted calls, exactly as before."""
    if weights is None:
        return lambda n: {}
    ds.set_weights(weights)
    return lambda n: {"wset": np.zeros(n, np.int32)}


def family_scores(X, families, score="bic", ess=1.0, device=None, weights=None):
    """Decomposable scores of families on the rows of X: `families` is a list of (child, parents) name pairs -> float64
    array, one launch pair for all of them.  score: "loglik", "bic", "aic", "bdeu" (equivalent sample size `ess`) or
    "k2", in natural logs (include/mibn.h gives the formulas).  `weights`: see `row_weights`; N is then their sum."""
    _check_score(score, ess)
    X, weights = row_weights(X, weights)
    fams = []
    for child, parents in families:
        parents = [parents] if isinstance(parents, str) or not hasattr(parents, "__iter__") else list(parents)
        for c in [child, *parents]:
            if c not in X.columns:
                raise ValueError(f"unknown column {c!r}")
        if child in parents or len(set(parents)) != len(parents):
            raise ValueError(f"the family of {child!r} names a column twice")
        fams.append((child, parents))
    order = list(X.columns)
    used = sorted({c for child, parents in fams for c in [child, *parents]}, key=order.index)
    codes, _, cards = encode_complete(X, used)
    if not fams:
        return np.zeros(0, np.float64)
    pos = {c: j for j, c in enumerate(used)}
    with counting_engine(device).dataset(codes, cards) as ds:
        return ds.score_families([tuple(sorted(pos[p] for p in parents)) + (pos[child],) for child, parents in fams], score, ess,
                                 **_weighted(ds, weights)(len(fams)))


def _edge_list(edges, columns, what):
    """(parent, child) name pairs -> index pairs, checked."""
    pos = {c: j for j, c in enumerate(columns)}
    out = []
    for e in edges or ():
        if not (isinstance(e, (tuple, list)) and len(e) == 2):
            raise ValueError(f"{what}: {e!r} is not a (parent, child) pair")
        u, v = e
        for c in (u, v):
            if c not in pos:
                raise ValueError(f"{what}: unknown column {c!r}")
        if u == v:
            raise ValueError(f"{what}: {u!r} -> {v!r} is a self-loop")
        if (pos[u], pos[v]) not in out:
            out.append((pos[u], pos[v]))
    return out


class _Graph:
    """Parent sets plus the ancestor relation, kept incrementally: anc[d, a] = a is an ancestor of d."""

    def __init__(self, n, edges):
        self.n = n
        self.pa = [set() for _ in range(n)]
        self.edge = np.zeros((n, n), bool)  # [child, parent]
        self.anc = np.zeros((n, n), bool)
        for u, v in edges:
            if self.anc[u, v] or u == v:
                raise ValueError("start (with the required edges) has a cycle")
            self.add(u, v)

    def add(self, u, v):
        self.pa[v].add(u)
        self.edge[v, u] = True
        up = self.anc[u].copy()
        up[u] = True
        below = self.anc[:, v].copy()  # the descendants of v
        below[v] = True
        self.anc[below] |= up

    def delete(self, u, v):
        self.pa[v].discard(u)
        self.edge[v, u] = False
        below = self.anc[:, v].copy()
        below[v] = True
        todo = set(np.flatnonzero(below).tolist())
        self.anc[below] = False

        def settle(d):
            if d in todo:
                todo.discard(d)
                for p in self.pa[d]:
                    settle(p)
                    self.anc[d] |= self.anc[p]
                    self.anc[d, p] = True

        for d in sorted(todo):
            settle(d)

    def reverse_makes_cycle(self, u, v):
        """After u -> v is replaced by v -> u: a cycle iff u reaches v by another path."""
        return any(self.anc[p, u] for p in self.pa[v] if p != u)


class _Climb:
    """One greedy search as a step-wise object, so that `hill_climb` and the lockstep `bootstrap` drive the same code:
    `needs()` lists the (child, parent set) keys the next step reads and the cache lacks, `feed` stores their scores,
    `advance()` refreshes the gains of the children whose parents changed, then makes the best legal move (or finishes)."""

    def __init__(self, columns, begin, req, forb, max_parents, max_iter, epsilon):
        self.columns, self.n = columns, len(columns)
        n = self.n
        self.g = _Graph(n, begin)
        for v in range(n):
            if len(self.g.pa[v]) > max_parents:
                raise ValueError(f"start gives {columns[v]!r} {len(self.g.pa[v])} parents (max_parents = {max_parents})")
        self.max_parents, self.max_iter, self.epsilon = max_parents, max_iter, float(epsilon)
        self.R = np.zeros((n, n), bool)  # [child, parent]
        self.F = np.zeros((n, n), bool)
        for u, v in req:
            self.R[v, u] = True
        for u, v in forb:
            self.F[v, u] = True
        self.not_self = ~np.eye(n, dtype=bool)
        self.cache, self.trace = {}, []
        # delta[v, u]: what toggling the edge u -> v adds to the score of v's family (NaN: not a candidate)
        self.delta = np.full((n, n), np.nan)
        self.pending = list(range(n))  # children whose row of delta is stale
        self.it, self.done = 0, False

    def candidates(self, v):
        """The families a move into / out of child v needs."""
        pa = frozenset(self.g.pa[v])
        keys = [(v, pa)] + [(v, pa - {p}) for p in sorted(pa)]
        if len(pa) < self.max_parents:
            keys += [(v, pa | {u}) for u in range(self.n) if u != v and u not in pa]
        return keys

    def needs(self):
        return [k for k in dict.fromkeys(k for v in self.pending for k in self.candidates(v)) if k not in self.cache]

    def feed(self, keys, scores):
        for k, s in zip(keys, scores):
            self.cache[k] = float(s)

    def advance(self):
        g, n, delta, cache, max_parents = self.g, self.n, self.delta, self.cache, self.max_parents
        for v in self.pending:
            pa = frozenset(g.pa[v])
            base = cache[(v, pa)]
            delta[v, :] = np.nan
            for p in pa:
                delta[v, p] = cache[(v, pa - {p})] - base
            if len(pa) < max_parents:
                for u in range(n):
                    if u != v and u not in pa:
                        delta[v, u] = cache[(v, pa | {u})] - base
        self.pending = []
        if self.max_iter is not None and self.it >= int(self.max_iter):
            self.done = True
            return
        R, F = self.R, self.F
        npar = np.array([len(p) for p in g.pa])
        room = (npar < max_parents)[:, None]
        E = g.edge
        gains = []
        add_ok = ~E & self.not_self & room & ~F & ~g.anc.T  # (anc.T[v, u]: v is an ancestor of u)
        gains.append(np.where(add_ok, delta, -np.inf))
        gains.append(np.where(E & ~R, delta, -np.inf))
        rev = np.full((n, n), -np.inf)
        for v, u in zip(*np.nonzero(E & ~R & ~F.T & room.T)):  # (room.T[v, u]: u can take another parent)
            if not g.reverse_makes_cycle(u, v):
                rev[v, u] = delta[v, u] + delta[u, v]
        gains.append(rev)
        best = max(float(m.max()) if m.size else -np.inf for m in gains)
        if not best > self.epsilon:
            self.done = True
            return
        op = next(k for k, m in enumerate(gains) if m.size and float(m.max()) == best)
        v, u = np.unravel_index(int(np.argmax(gains[op])), (n, n))  # first maximum in [child, parent] order
        v, u = int(v), int(u)
        if op == 0:
            g.add(u, v)
            changed = [v]
        elif op == 1:
            g.delete(u, v)
            changed = [v]
        else:
            g.delete(u, v)
            g.add(v, u)
            changed = [v, u]
        self.trace.append((MOVES[op], self.columns[u], self.columns[v], best))
        self.pending = changed
        self.it += 1

    def result(self, return_trace):
        g, n, columns = self.g, self.n, self.columns
        total = math.fsum(self.cache[(v, frozenset(g.pa[v]))] for v in range(n))
        result = [(columns[u], columns[v]) for v in range(n) for u in sorted(g.pa[v])]
        linked = {c for e in result for c in e}
        result += [c for c in columns if c not in linked]
        return (result, self.trace, total) if return_trace else result


def _climb_plan(X, score, ess, max_parents, start, required, forbidden, max_iter, epsilon):
    """The argument checks of `hill_climb` -> (columns, a factory of fresh `_Climb` objects); no engine is touched."""
    _check_score(score, ess)
    columns = list(X.columns)
    n = len(columns)
    if len(set(columns)) != n:
        raise ValueError("X has duplicate column names")
    max_parents = int(max_parents)
    if max_parents < 0:
        raise ValueError("max_parents must not be negative")
    if max_iter is not None and int(max_iter) < 0:
        raise ValueError("max_iter must not be negative")
    if not float(epsilon) >= 0:
        raise ValueError("epsilon must not be negative")
    req = _edge_list(required, columns, "required")
    forb = _edge_list(forbidden, columns, "forbidden")
    begin = _edge_list(start, columns, "start")
    for e in req:
        if e in forb:
            raise ValueError(f"the edge {columns[e[0]]!r} -> {columns[e[1]]!r} is both required and forbidden")
        if e not in begin:
            begin.append(e)
    for e in begin:
        if e in forb:
            raise ValueError(f"start contains the forbidden edge {columns[e[0]]!r} -> {columns[e[1]]!r}")

    def fresh():
        return _Climb(columns, begin, req, forb, max_parents, max_iter, epsilon)

    fresh()  # (the checks of the start graph)
    return columns, fresh


def _family_scope(key):
    child, parents = key
    return tuple(sorted(parents)) + (child,)


def hill_climb(X, score="bic", ess=1.0, max_parents=3, start=None, required=(), forbidden=(), max_iter=None, epsilon=1e-4,
               device=None, return_trace=False, weights=None):
    """Greedy hill climbing over DAGs with a decomposable score: from `start` (an edge list, e.g. `chow_liu(X)`; default the
    empty graph) apply the legal move - add u -> v, delete u -> v, reverse u -> v - with the largest gain in score while
    that gain exceeds `epsilon`.  Legal: the graph stays acyclic, no node gets more than `max_parents` parents, a `required`
    edge is never removed or reversed (required edges are part of the start graph), a `forbidden` one never created.  Equal
    gains: add before delete before reverse, then by the position of the edge's child, then of its parent, in X.columns -
    the result is a function of the scores alone.

    Returns what `BayesNet(*result)` accepts: (parent, child) tuples plus the bare names of isolated columns.  With
    `return_trace`: (result, [(op, u, v, gain), ...] - the edge u -> v as it was before the move, for "add" the new edge -
    and the total score of the result).

    The search runs on the host; the rows are uploaded once and every iteration sends the device one batch of the families it
    has not scored yet (scores are cached by (child, parent set): after the first sweep of n + n (n - 1) families only the one
    or two children whose parents changed need new ones).  Complete data only.  `weights`: see `row_weights` - the search on
    the rows written out weights[i] times, bit for bit, without writing them out.

    epsilon: a design choice, not a measured quantity - far above the rounding noise of a score (~1e-9 at a million rows), far
    below any gain that matters (one BIC parameter costs 0.5 ln N >= 0.35)."""
    X, weights = row_weights(X, weights)
    columns, fresh = _climb_plan(X, score, ess, max_parents, start, required, forbidden, max_iter, epsilon)
    codes, _, cards = encode_complete(X, columns)
    climb = fresh()
    with counting_engine(device).dataset(codes, cards) as ds:
        under = _weighted(ds, weights)
        while not climb.done:
            new = climb.needs()
            if new:
                climb.feed(new, ds.score_families([_family_scope(k) for k in new], score, ess, **under(len(new))))
            climb.advance()
    return climb.result(return_trace)


# ------------------------------------------------------ exact structure learning: the best-scoring DAG by subset DP
# An extension, like hill climbing above - and its yardstick: every score here is decomposable, so the globally best DAG
# follows from local scores alone by dynamic programming over variable subsets (csrc/dag_kernel.hip.h, `mibn_best_dag`).
EXACT_MAX_COLUMNS = _capi.BEST_DAG_MAX_VARS
_MAX_TABLE_CELLS = 1 << 28  # of one family's contingency table (mibn_score_families)


def _dag_result(columns, parents):
    """Parent masks -> the result form of `hill_climb`: edges, children in column order and parents ascending, then isolated names."""
    n = len(columns)
    result = [(columns[u], columns[v]) for v in range(n) for u in range(n) if (int(parents[v]) >> u) & 1]
    linked = {c for e in result for c in e}
    return result + [c for c in columns if c not in linked]


def _exact_plan(X, score, ess, max_parents, required, forbidden, max_families, cards, who="exact_search", instead="hill_climb or pc"):
    """The argument checks of `exact_search` (and of `arc_posteriors`: `who`, and what it points to beyond 24 columns) ->
    (columns, candidates [(child, parent mask)]); no engine is touched.  `cards` is a callable (evaluated after the cheaper
    checks) giving the cardinalities."""
    _check_score(score, ess)
    columns = list(X.columns)
    n = len(columns)
    if len(set(columns)) != n:
        raise ValueError("X has duplicate column names")
    if n < 1:
        raise ValueError("X has no columns")
    if n > EXACT_MAX_COLUMNS:
        raise ValueError(f"{who} handles at most {EXACT_MAX_COLUMNS} columns, X has {n} (the tables double with every column): "
                         f"use {instead}")
    max_parents = int(max_parents)
    if max_parents < 0:
        raise ValueError("max_parents must not be negative")
    req = _edge_list(required, columns, "required")
    forb = _edge_list(forbidden, columns, "forbidden")
    for e in req:
        if e in forb:
            raise ValueError(f"the edge {columns[e[0]]!r} -> {columns[e[1]]!r} is both required and forbidden")
    try:
        _Graph(n, req)
    except ValueError:
        raise ValueError("the required edges form a cycle") from None
    need = [sum(1 << u for u, c in req if c == v) for v in range(n)]
    ban = [sum(1 << u for u, c in forb if c == v) for v in range(n)]
    free = []  # the columns a child may or may not take
    for v in range(n):
        k = bin(need[v]).count("1")
        if k > max_parents:
            raise ValueError(f"{columns[v]!r} has {k} required parents (max_parents = {max_parents})")
        free.append([u for u in range(n) if u != v and not ((need[v] | ban[v]) >> u) & 1])
    count = sum(math.comb(len(free[v]), j) for v in range(n) for j in range(max_parents - bin(need[v]).count("1") + 1))
    if count > int(max_families):
        raise ValueError(f"{count} candidate families (max_families = {int(max_families)}): lower max_parents or raise max_families")
    card = cards()
    cand = []
    for v in range(n):
        k0 = bin(need[v]).count("1")
        sets = [(k0 + j, need[v] | sum(1 << u for u in extra)) for j in range(max_parents - k0 + 1) for extra in itertools.combinations(free[v], j)]
        for _, pm in sorted(sets):
            cells = card[v]
            for u in range(n):
                if (pm >> u) & 1:
                    cells *= card[u]
            if cells > _MAX_TABLE_CELLS:
                raise ValueError(f"the family of {columns[v]!r} with parents {[columns[u] for u in range(n) if (pm >> u) & 1]} has a table of "
                                 f"{cells} cells (at most 2^28): lower max_parents")
            cand.append((v, pm))
    return columns, cand


def _mask_scope(child, pm):
    return tuple(u for u in range(pm.bit_length()) if (pm >> u) & 1) + (child,)


def _exact_scores(X, weights, score, ess, max_parents, required, forbidden, max_families, device, **who):
    """The opening `exact_search` and `arc_posteriors` share: the row weights, `_exact_plan` (`who`: its naming arguments), the
    data set and the ONE `score_families` call -> (engine, columns, candidates, scores)."""
    X, weights = row_weights(X, weights)
    encoded = []

    def cards():
        encoded.append(encode_complete(X, list(X.columns)))
        return encoded[0][2]

    columns, cand = _exact_plan(X, score, ess, max_parents, required, forbidden, max_families, cards, **who)
    codes, _, card = encoded[0]
    engine = counting_engine(device)
    with engine.dataset(codes, card) as ds:
        scores = ds.score_families([_mask_scope(v, pm) for v, pm in cand], score, ess, **_weighted(ds, weights)(len(cand)))
    return engine, columns, cand, scores


def exact_search(X, score="bic", ess=1.0, max_parents=3, required=(), forbidden=(), max_families=2_000_000, device=None, return_info=False,
                 weights=None):
    """The globally best DAG under a decomposable score, by dynamic programming over column subsets (Silander and Myllymaki 2006)
    on the device - for up to 24 columns; beyond that `hill_climb` and `pc` remain.  The candidates of child v are every parent
    set P with |P| <= max_parents that holds the `required` parents of v and none of its `forbidden` ones (enumerated per child
    in ascending (|P|, mask) order, children in column order); all of them are scored by ONE `score_families` call, and the scores
    go to `mibn_best_dag` (include/mibn.h pins the tie rules: the result is a function of the scores alone).  More than
    `max_families` candidates is an error that names the count.

    Returns what `hill_climb` returns: (parent, child) tuples, children in column order and parents ascending, then the bare
    names of isolated columns.  With `return_info`: (result, info) - info["total"] the `math.fsum` of the chosen families'
    scores in column order (comparable bit for bit with `hill_climb`'s total of the same graph), info["dp_total"] the call's
    own nested sum, info["order"] a topological order of the column names (roots first), info["n_families"].

    Complete data only.  `weights`: see `row_weights` - the search on the rows written out weights[i] times, bit for bit."""
    engine, columns, cand, scores = _exact_scores(X, weights, score, ess, max_parents, required, forbidden, max_families, device)
    n = len(columns)
    parents, order, dp_total = engine.best_dag(n, [v for v, _ in cand], [pm for _, pm in cand], scores)
    if not dp_total > -math.inf:
        raise RuntimeError("best_dag found no DAG although every child has its required parents as a candidate")
    at = {k: i for i, k in enumerate(cand)}
    result = _dag_result(columns, parents)
    if not return_info:
        return result
    info = {"total": math.fsum(float(scores[at[(v, int(parents[v]))]]) for v in range(n)), "dp_total": dp_total,
            "order": [columns[int(v)] for v in order], "n_families": len(cand)}
    return result, info


def best_dag(columns, candidates, scores, device=None):
    """The best DAG from local scores of the caller's own: `candidates` is a list of (child, parents) name pairs - child may take
    exactly that parent set -, `scores` one number per candidate (higher is better; a child's parent set is always one of its
    candidates).  Returns the result form of `exact_search`.  ValueError when no DAG can be formed from the candidates."""
    columns, children, masks, scores = _named_candidates(columns, candidates, scores, "best_dag")
    n = len(columns)
    parents, _, total = counting_engine(device).best_dag(n, children, masks, scores)
    if not total > -math.inf:
        raise ValueError("no DAG can be formed from these candidates")
    return _dag_result(columns, parents)


# ------------------------------------------------------ exact Bayesian arc posteriors: the sum-product form of the same DP
# `exact_search` returns one graph; with a few thousand rows many DAGs lie within a few units of log score of it.  The same
# subset DP with the maximum replaced by a sum (csrc/dag_post_kernel.hip.h, `mibn_arc_posteriors`; Koivisto and Sood 2004) gives
# the posterior probability of every arc, averaged over ALL DAGs - at about the cost of one `exact_search`.
PARENT_PRIORS = ("uniform", "size")


def _averaged_edges(columns, frame, threshold):
    """The body of `ArcStrength.edges` / `ArcPosterior.edges`: the pairs of `frame` (from, to, strength, direction) with strength
    >= threshold in descending strength (ties by the columns' positions), each oriented by the majority (a tie goes to from ->
    to) and skipped where it would close a cycle; then the bare names of the isolated columns."""
    pos = {c: j for j, c in enumerate(columns)}
    rows = [(-float(s), pos[u], pos[v], float(d)) for u, v, s, d in frame.itertuples(index=False) if s >= threshold]
    g = _Graph(len(columns), [])
    out = []
    for _, i, j, d in sorted(rows):
        u, v = (i, j) if d >= 0.5 else (j, i)
        if g.anc[u, v]:  # v is an ancestor of u
            continue
        g.add(u, v)
        out.append((columns[u], columns[v]))
    linked = {c for e in out for c in e}
    return out + [c for c in columns if c not in linked]


class ArcPosterior:
    """Exact posteriors over all DAGs (`arc_posteriors`), under an ORDER-MODULAR prior: a DAG weighs its number of linear
    extensions times the product of its families' weights - not uniform over DAGs (at two columns the empty graph counts twice).

    `matrix`: DataFrame, row = from, column = to, P(from -> to | data).  `frame`: `ArcStrength.frame`'s four columns - one row
    per unordered pair with `strength` = P(u -> v) + P(v -> u) > 0, `from` before `to` in column order (rows in that order
    too), `direction` = P(from -> to) / strength.  `log_evidence`: the log of the sum over every (order, DAG) pair of the product
    of the weights.  `columns`, `n_families`."""

    def __init__(self, columns, candidates, log_post, arc, log_evidence):
        self.columns = list(columns)
        self.n_families = len(candidates)
        self.log_evidence = float(log_evidence)
        self._candidates = [(int(v), int(pm)) for v, pm in candidates]
        self._log_post = np.asarray(log_post, np.float64).reshape(-1)
        n = len(self.columns)
        arc = np.asarray(arc, np.float64).reshape(n, n)
        self.matrix = pd.DataFrame(arc, index=self.columns, columns=self.columns)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if arc[i, j] + arc[j, i] > 0.0]
        strength = np.array([arc[i, j] + arc[j, i] for i, j in pairs], np.float64)
        self.frame = pd.DataFrame({
            "from": [self.columns[i] for i, _ in pairs], "to": [self.columns[j] for _, j in pairs], "strength": strength,
            "direction": np.array([arc[i, j] for i, j in pairs], np.float64) / strength if pairs else strength})

    def edges(self, threshold=0.5):
        """The averaged DAG as `BayesNet(*edges)` takes it, by `ArcStrength.edges`'s rule: the pairs with strength >= threshold in
        descending strength, each oriented by the majority and skipped where it would close a cycle; then the isolated columns."""
        return _averaged_edges(self.columns, self.frame, threshold)

    def parent_sets(self, child):
        """The posterior of every candidate parent set of `child`: a Series indexed by tuples of parent names (in column
        order), descending (ties in candidate order); it sums to 1."""
        if child not in self.columns:
            raise ValueError(f"unknown column {child!r}")
        v = self.columns.index(child)
        own = [f for f, (c, _) in enumerate(self._candidates) if c == v]
        own.sort(key=lambda f: (-self._log_post[f], f))
        index = [tuple(self.columns[u] for u in range(len(self.columns)) if (self._candidates[f][1] >> u) & 1) for f in own]
        out = pd.Series(np.exp(self._log_post[own]), index=pd.Index(index, tupleize_cols=False), name=child, dtype=np.float64)
        return out


def arc_posteriors(X, score="bdeu", ess=1.0, max_parents=3, required=(), forbidden=(), parent_prior="uniform", max_families=2_000_000, device=None,
                   weights=None):
    """The exact posterior probability of every arc given the rows of X, averaged over every DAG whose families are among the
    candidates, for up to 24 columns (Koivisto and Sood 2004) -> an `ArcPosterior`.  Beyond 24 columns `bootstrap` remains.

    The candidates are `exact_search`'s - every parent set P of child v with |P| <= max_parents that holds the `required` parents
    of v and none of its `forbidden` ones, in the same order -, scored by ONE `score_families` call; the scores go to
    `mibn_arc_posteriors` as log weights.  With `bdeu` or `k2` (log marginal likelihoods) the result is a Bayesian posterior;
    with `bic` or `aic` an approximation of one.  `parent_prior`: "uniform" leaves the scores as they are; "size" adds
    -log C(n - 1, |P|) to each (Koivisto's choice: every parent-set size equally likely a priori).

    The prior over structures is ORDER-MODULAR, not uniform over DAGs: a DAG counts once per linear order it is consistent with
    (see `ArcPosterior`).  Complete data only.  `weights`: see `row_weights`."""
    if parent_prior not in PARENT_PRIORS:
        raise ValueError(f"parent_prior must be one of {PARENT_PRIORS}, not {parent_prior!r}")
    engine, columns, cand, scores = _exact_scores(X, weights, score, ess, max_parents, required, forbidden, max_families, device,
                                                  who="arc_posteriors", instead="bootstrap")
    n = len(columns)
    scores = np.asarray(scores, np.float64)
    if parent_prior == "size":
        scores = scores - np.array([math.log(math.comb(n - 1, bin(pm).count("1"))) for _, pm in cand], np.float64)
    log_post, arc, log_evidence = engine.arc_posteriors(n, [v for v, _ in cand], [pm for _, pm in cand], scores)
    if not log_evidence > -math.inf:
        raise RuntimeError("arc_posteriors found no DAG although every child has its required parents as a candidate")
    return ArcPosterior(columns, cand, log_post, arc, log_evidence)


def _named_candidates(columns, candidates, scores, who):
    """The checks `best_dag` and `arc_posteriors_from_scores` share -> (columns, children, masks, scores)."""
    columns = list(columns)
    n = len(columns)
    if len(set(columns)) != n:
        raise ValueError("duplicate column names")
    if not 1 <= n <= EXACT_MAX_COLUMNS:
        raise ValueError(f"{who} handles 1 to {EXACT_MAX_COLUMNS} columns, not {n}")
    pos = {c: j for j, c in enumerate(columns)}
    scores = np.asarray(scores, np.float64).reshape(-1)
    if len(scores) != len(candidates):
        raise ValueError("scores needs one entry per candidate")
    if not np.isfinite(scores).all():
        raise ValueError("scores must be finite")
    children, masks, seen = [], [], set()
    for child, parents in candidates:
        parents = [parents] if isinstance(parents, str) or not hasattr(parents, "__iter__") else list(parents)
        for c in [child, *parents]:
            if c not in pos:
                raise ValueError(f"unknown column {c!r}")
        if child in parents or len(set(parents)) != len(parents):
            raise ValueError(f"the family of {child!r} names a column twice")
        key = (pos[child], sum(1 << pos[p] for p in parents))
        if key in seen:
            raise ValueError(f"the family of {child!r} with parents {parents} is listed twice")
        seen.add(key)
        children.append(key[0])
        masks.append(key[1])
    return columns, children, masks, scores


def arc_posteriors_from_scores(columns, candidates, scores, device=None):
    """`arc_posteriors` from local log scores of the caller's own - the mirror of `best_dag`: `candidates` is a list of (child,
    parents) name pairs, `scores` one log weight per candidate -> an `ArcPosterior`.  ValueError when no DAG can be formed."""
    columns, children, masks, scores = _named_candidates(columns, candidates, scores, "arc_posteriors_from_scores")
    log_post, arc, log_evidence = counting_engine(device).arc_posteriors(len(columns), children, masks, scores)
    if not log_evidence > -math.inf:
        raise ValueError("no DAG can be formed from these candidates")
    return ArcPosterior(columns, list(zip(children, masks)), log_post, arc, log_evidence)


def net_score(bn, X, score="bic", ess=1.0, weights=None):
    """The sum of the family scores of the net's own structure on the rows of X (`BayesNet.score`)."""
    fams = [(node, list(bn.parents.get(node, []))) for node in bn.nodes]
    return math.fsum(family_scores(X, fams, score=score, ess=ess, device=getattr(bn, "_device", None), weights=weights).tolist())


# ------------------------------------------------------ constraint-based structure learning: CI tests and PC-stable
# An extension, like the score-based search above.  PC in its order-independent form freezes the adjacency sets at the start
# of a level, so every conditional-independence test of a level is known before any runs: a level is ONE batch of tables
# over the resident rows (csrc/citest_kernel.hip.h, `mibn_ci_tests`); the search itself runs on the host.
CI_TESTS = ("g2", "x2", "mi")  # "mi": the G2 test, reported as the conditional mutual information G2 / (2 N) in nats
CI_DOFS = ("classic", "adjusted")


def _gamma_q(a, x):
    """The regularised upper incomplete gamma function Q(a, x), a > 0, x >= 0: the series of P below a + 1, Lentz's
    evaluation of the continued fraction of Q above it."""
    if x <= 0.0:
        return 1.0
    log_front = a * math.log(x) - x - math.lgamma(a)
    if x < a + 1.0:
        term = total = 1.0 / a
        k = a
        for _ in range(100_000):
            k += 1.0
            term *= x / k
            total += term
            if term < total * 1e-17:
                break
        return max(0.0, 1.0 - total * math.exp(log_front))
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for i in range(1, 100_000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h * math.exp(log_front) if log_front > -745.0 else 0.0


def chi2_sf(stat, dof):
    """P(chi-square with `dof` degrees of freedom > stat); 1.0 for dof == 0 (nothing to test)."""
    if dof <= 0:
        return 1.0
    return _gamma_q(0.5 * float(dof), 0.5 * max(float(stat), 0.0))


def _check_ci(test, dof):
    if test not in CI_TESTS:
        raise ValueError(f"test must be one of {CI_TESTS}, not {test!r}")
    if dof not in CI_DOFS:
        raise ValueError(f"dof must be one of {CI_DOFS}, not {dof!r}")


def _ci_batch(ds, cards, n_rows, batch, test, dof, **under):
    """batch: (x, y, Z) column positions -> (stat, dof, p_value) arrays through ONE `Dataset.ci_tests` call (`under`: its
    weight-set keyword, if any; n_rows is then the sets' N)."""
    stat, adj = ds.ci_tests([(*Z, x, y) for x, y, Z in batch], "g2" if test == "mi" else test, **under)
    if dof == "classic":
        d = np.array([math.prod(int(cards[z]) for z in Z) * (int(cards[x]) - 1) * (int(cards[y]) - 1) for x, y, Z in batch], np.int64)
    else:
        d = np.asarray(adj, np.int64)
    p = np.array([chi2_sf(s, k) for s, k in zip(stat.tolist(), d.tolist())], np.float64)
    if test == "mi":
        stat = stat / (2.0 * n_rows) if n_rows else stat
    return np.asarray(stat, np.float64), d.reshape(-1), p


def ci_tests(X, tests, test="g2", dof="classic", device=None, weights=None):
    """Conditional-independence tests on the rows of X: `tests` is a list of (x, y, given) names (`given` a name or a
    sequence of names, possibly empty) -> DataFrame with one row per test: `stat`, `dof`, `p_value`.  test: "g2" (the
    likelihood-ratio statistic), "x2" (Pearson's) or "mi" (G2 / (2 N) as `stat`, the p-value of G2).  dof: "classic" =
    q (rx - 1)(ry - 1) over the cardinalities of the encoded columns, "adjusted" = summed over the strata that occur, from
    the rows and columns that occur in each.  dof == 0 gives p_value 1.  One launch pair for all tests; complete data only.
    `weights`: see `row_weights`; N is then their sum."""
    _check_ci(test, dof)
    X, weights = row_weights(X, weights)
    asked = []
    for t in tests:
        if not (isinstance(t, (tuple, list)) and len(t) == 3):
            raise ValueError(f"{t!r} is not an (x, y, given) triple")
        x, y, given = t
        given = [given] if isinstance(given, str) or not hasattr(given, "__iter__") else list(given)
        for c in [x, y, *given]:
            if c not in X.columns:
                raise ValueError(f"unknown column {c!r}")
        if len({x, y, *given}) != 2 + len(given):
            raise ValueError(f"the test {t!r} names a column twice")
        asked.append((x, y, given))
    order = list(X.columns)
    used = sorted({c for x, y, given in asked for c in [x, y, *given]}, key=order.index)
    codes, _, cards = encode_complete(X, used)
    out = pd.DataFrame({"stat": np.zeros(len(asked)), "dof": np.zeros(len(asked), np.int64), "p_value": np.ones(len(asked))})
    if not asked:
        return out
    pos = {c: j for j, c in enumerate(used)}
    with counting_engine(device).dataset(codes, cards) as ds:
        batch = [(pos[x], pos[y], tuple(sorted(pos[z] for z in given))) for x, y, given in asked]
        n_rows = len(X) if weights is None else int(weights.sum(dtype=np.int64))
        out["stat"], out["dof"], out["p_value"] = _ci_batch(ds, cards, n_rows, batch, test, dof, **_weighted(ds, weights)(len(batch)))
    return out


def _meek(n, adj, arrow):
    """Meek's rules 1 to 3 to closure on the partially directed graph (adj: adjacency sets; arrow: the set of (u, v) with
    u -> v).  Passes over the ordered pairs (a, b) in ascending order, a rule that fires orients a -> b at once; the
    passes repeat until one changes nothing."""
    def undirected(a, b):
        return b in adj[a] and (a, b) not in arrow and (b, a) not in arrow

    changed = True
    while changed:
        changed = False
        for a in range(n):
            for b in sorted(adj[a]):
                if not undirected(a, b):
                    continue
                r1 = any((c, a) in arrow and b not in adj[c] for c in adj[a] if c != b)
                r2 = any((a, c) in arrow and (c, b) in arrow for c in adj[a] if c != b)
                into_b = [c for c in adj[a] if c != b and undirected(a, c) and (c, b) in arrow]
                r3 = any(d not in adj[c] for c, d in itertools.combinations(into_b, 2))
                if r1 or r2 or r3:
                    arrow.add((a, b))
                    changed = True


class _Skeleton:
    """The skeleton phase of PC-stable as a step-wise object (`_pc_search` and the lockstep `bootstrap` drive the same code):
    `next_batch()` gives the tests of the next level - None when the search is over -, `feed` takes their p-values,
    `finish()` orients what is left."""

    def __init__(self, n, alpha, max_cond=3, required=(), forbidden=()):
        self.n, self.alpha, self.max_cond = n, alpha, max_cond
        self.required, self.forbidden = list(required), set(forbidden)
        forbidden = self.forbidden
        self.adj = [{v for v in range(n) if v != u and not ((u, v) in forbidden and (v, u) in forbidden)} for u in range(n)]
        self.fixed = {frozenset(e) for e in self.required}
        for u, v in self.required:
            self.adj[u].add(v)
            self.adj[v].add(u)
        self.sepsets, self.levels, self.trace = {}, [], []
        self.level = 0
        self.batch = self.per_pair = None

    def next_batch(self):
        if self.level > self.max_cond:
            return None
        n, adj, level = self.n, self.adj, self.level
        frozen = [sorted(a) for a in adj]  # the adjacency of the whole level
        batch, index, per_pair = [], {}, {}
        for x in range(n):
            for y in frozen[x]:
                if frozenset((x, y)) in self.fixed:
                    continue
                others = [z for z in frozen[x] if z != y]
                pair = (min(x, y), max(x, y))
                for S in itertools.combinations(others, level):
                    key = (*pair, S)
                    if key not in index:  # (already asked from the other side)
                        index[key] = len(batch)
                        batch.append(key)
                        per_pair.setdefault(pair, []).append(index[key])
        if not batch:
            return None
        self.batch, self.per_pair = batch, per_pair
        return batch

    def feed(self, p_values):
        adj, batch, level = self.adj, self.batch, self.level
        p = [float(v) for v in p_values]
        self.levels.append(len(batch))
        self.trace += [(level, x, y, S, pv) for (x, y, S), pv in zip(batch, p)]
        for (x, y), asked in self.per_pair.items():
            hit = next((i for i in asked if p[i] > self.alpha), None)
            if hit is not None:  # the first separating set in enumeration order
                adj[x].discard(y)
                adj[y].discard(x)
                self.sepsets[(x, y)] = batch[hit][2]
        self.level += 1

    def finish(self):
        """Orientation: background knowledge, v-structures in column order (the first orientation of an edge stays), Meek."""
        n, adj, sepsets, forbidden = self.n, self.adj, self.sepsets, self.forbidden
        arrow = set()

        def orient(u, v):
            if v in adj[u] and (v, u) not in arrow and (u, v) not in forbidden:
                arrow.add((u, v))

        for u, v in self.required:
            orient(u, v)
        for u, v in sorted(forbidden):
            orient(v, u)
        for x in range(n):
            for y in range(x + 1, n):
                if y in adj[x] or (x, y) not in sepsets:
                    continue
                for z in sorted(adj[x] & adj[y]):
                    if z not in sepsets[(x, y)]:
                        orient(x, z)
                        orient(y, z)
        _meek(n, adj, arrow)
        return {"adj": adj, "arrow": arrow, "sepsets": sepsets, "levels": self.levels, "trace": self.trace}


def _pc_search(n, tester, alpha, max_cond=3, required=(), forbidden=()):
    """PC-stable over the columns 0 .. n - 1.  tester: a list of (x, y, S) with x < y and S an ascending tuple -> their
    p-values; it is called ONCE per level.  required / forbidden: (u, v) position pairs for u -> v.  A pair forbidden in both
    directions is never adjacent; a required edge is never tested and starts directed; an edge forbidden one way is directed
    the other way if it survives.  -> dict(adj, arrow, sepsets, levels, trace)."""
    search = _Skeleton(n, alpha, max_cond, required, forbidden)
    while True:
        batch = search.next_batch()
        if batch is None:
            break
        search.feed(tester(batch))
    return search.finish()


class PCResult:
    """What `pc` learned: `directed` [(u, v) for u -> v] and `undirected` [(u, v), u before v in X.columns] - together the
    partially directed graph -, `sepsets` {(u, v): the tuple of columns that separated them}, `tests_per_level`, and `trace`
    ([(level, x, y, given, p_value)] of every test, with return_trace)."""

    def __init__(self, columns, found, keep_trace):
        name = columns.__getitem__
        n = len(columns)
        adj, arrow = found["adj"], found["arrow"]
        self.columns = list(columns)
        self.directed = [(name(u), name(v)) for u, v in sorted(arrow)]
        self.undirected = [(name(u), name(v)) for u in range(n) for v in sorted(adj[u]) if u < v and (u, v) not in arrow and (v, u) not in arrow]
        self.sepsets = {(name(x), name(y)): tuple(name(z) for z in S) for (x, y), S in found["sepsets"].items()}
        self.tests_per_level = list(found["levels"])
        self.trace = [(lv, name(x), name(y), tuple(name(z) for z in S), p) for lv, x, y, S, p in found["trace"]] if keep_trace else None

    def dag(self):
        """A DAG of the learned equivalence class - a consistent extension by Dor and Tarsi's algorithm - as `BayesNet(*edges)`
        takes it: (parent, child) tuples plus the bare names of isolated columns.  ValueError where the partially directed
        graph has none (conflicting test results can produce such a graph)."""
        pos = {c: j for j, c in enumerate(self.columns)}
        arrow = {(pos[u], pos[v]) for u, v in self.directed}
        und = {frozenset((pos[u], pos[v])) for u, v in self.undirected}
        out = set(arrow)
        alive = set(range(len(self.columns)))
        while alive:
            for x in sorted(alive):
                nb = {y for y in alive if frozenset((x, y)) in und}
                adjacent = nb | {y for y in alive if (y, x) in arrow or (x, y) in arrow}
                if any((x, y) in arrow for y in alive):
                    continue  # not a sink
                if all(frozenset((y, z)) in und or (y, z) in arrow or (z, y) in arrow for y in nb for z in adjacent if z != y):
                    break
            else:
                raise ValueError("the partially directed graph has no consistent extension to a DAG")
            out |= {(y, x) for y in nb}
            alive.discard(x)
            und = {e for e in und if x not in e}
            arrow = {(u, v) for u, v in arrow if x not in (u, v)}
        name = self.columns.__getitem__
        result = [(name(u), name(v)) for u, v in sorted(out, key=lambda e: (e[1], e[0]))]
        linked = {c for e in result for c in e}
        return result + [c for c in self.columns if c not in linked]


def _pc_plan(X, alpha, test, dof, max_cond, required, forbidden):
    """The argument checks of `pc` -> (columns, required, forbidden as position pairs); no engine is touched."""
    _check_ci(test, dof)
    if not 0.0 < float(alpha) < 1.0:
        raise ValueError("alpha must lie strictly between 0 and 1")
    if int(max_cond) < 0:
        raise ValueError("max_cond must not be negative")
    columns = list(X.columns)
    if len(set(columns)) != len(columns):
        raise ValueError("X has duplicate column names")
    req = _edge_list(required, columns, "required")
    forb = _edge_list(forbidden, columns, "forbidden")
    for u, v in req:
        if (u, v) in forb:
            raise ValueError(f"the edge {columns[u]!r} -> {columns[v]!r} is both required and forbidden")
        if (v, u) in req:
            raise ValueError(f"{columns[u]!r} and {columns[v]!r} are required in both directions")
    return columns, req, forb


def pc(X, alpha=0.01, test="g2", dof="classic", max_cond=3, required=(), forbidden=(), device=None, return_trace=False, weights=None):
    """The PC algorithm in its order-independent ("stable") form.  Skeleton: from the complete graph, level l = 0, 1, ...,
    max_cond tests every pair still adjacent given every l-subset of either end's other neighbours - the adjacency frozen at
    the start of the level, so ALL tests of a level go to the device as one batch - and drops an edge as soon as one of its
    tests has p > alpha; the separating set is the first such subset (pairs in column order, subsets lexicographic).
    Orientation: v-structures from the separating sets in column order (the first orientation of an edge stays, no
    bidirected edges), then Meek's rules 1 to 3 to closure.  `required` / `forbidden` are (parent, child) pairs: a required
    edge is kept and directed, a forbidden one never directed that way (forbidden both ways: never adjacent).

    test, dof: see `ci_tests`.  Returns a `PCResult`; `PCResult.dag()` gives `BayesNet(*edges).fit(X)` a member of the class.
    Complete data only; the rows are uploaded once.  `weights`: see `row_weights`."""
    X, weights = row_weights(X, weights)
    columns, req, forb = _pc_plan(X, alpha, test, dof, max_cond, required, forbidden)
    codes, _, cards = encode_complete(X, columns)
    with counting_engine(device).dataset(codes, cards) as ds:
        under = _weighted(ds, weights)
        found = _pc_search(len(columns), lambda batch: _ci_batch(ds, cards, len(X), batch, test, dof, **under(len(batch)))[2], float(alpha),
                           int(max_cond), req, forb)
    return PCResult(columns, found, return_trace)


# ------------------------------------------------------ bootstrap arc strengths (Friedman, Goldszmidt and Wyner 1999)
# One search says nothing about which of its arcs to believe; the standard answer is to repeat it on bootstrap resamples and count
# the arcs.  A resample of N rows is a vector of N multiplicities: the rows stay resident once, the device draws the weight sets
# (`Dataset.bootstrap`), and all replicates advance in LOCKSTEP - one `score_families` / `ci_tests` call per search iteration / level
# carries every (table, set) pair any replicate still lacks (csrc/count_weighted_kernel.hip.h).
BOOTSTRAP_LEARNERS = ("hill_climb", "pc")


def _replicate_arcs(rep, pos):
    """A replicate's result - what `hill_climb` returns (with or without its trace) or a `PCResult` - -> (directed position pairs,
    undirected ones)."""
    if hasattr(rep, "directed"):
        return [(pos[u], pos[v]) for u, v in rep.directed], [(pos[u], pos[v]) for u, v in rep.undirected]
    if isinstance(rep, tuple):
        rep = rep[0]
    return [(pos[e[0]], pos[e[1]]) for e in rep if isinstance(e, tuple)], []


class ArcStrength:
    """Arc strengths over the replicates of `bootstrap`.  `frame`: one row per unordered pair of columns adjacent in at least one
    replicate, `from` before `to` in X.columns order (rows in that order too): `strength` = the fraction of replicates holding
    the arc in either direction, `direction` = the share of those with from -> to (an undirected `pc` edge counts half each
    way).  `n_boot`, `columns`."""

    def __init__(self, columns, replicates):
        self.columns = list(columns)
        self.n_boot = len(replicates)
        pos = {c: j for j, c in enumerate(self.columns)}
        seen = {}  # (i, j), i < j -> [i -> j, j -> i, undirected]
        for rep in replicates:
            directed, undirected = _replicate_arcs(rep, pos)
            for kind, arcs in ((None, directed), (2, undirected)):
                for u, v in arcs:
                    seen.setdefault((min(u, v), max(u, v)), [0, 0, 0])[(0 if u < v else 1) if kind is None else 2] += 1
        pairs = sorted(seen)
        total = [sum(seen[p]) for p in pairs]
        self.frame = pd.DataFrame({
            "from": [self.columns[i] for i, _ in pairs], "to": [self.columns[j] for _, j in pairs],
            "strength": np.array([t / self.n_boot for t in total], np.float64),
            "direction": np.array([(seen[p][0] + 0.5 * seen[p][2]) / t for p, t in zip(pairs, total)], np.float64)})

    def edges(self, threshold=0.5):
        """The averaged DAG as `BayesNet(*edges)` takes it: the pairs with strength >= threshold in descending strength (ties by the
        columns' positions), each oriented by the majority (a tie goes to from -> to) and skipped where it would close a cycle;
        then the bare names of the isolated columns."""
        return _averaged_edges(self.columns, self.frame, threshold)


def _lockstep(ds, searches, wanted, scope_of, ask):
    """One round of every unfinished replicate: `wanted(search)` -> the keys it lacks; ONE device call - `ask(scopes, sets)` ->
    one value per pair - carries them all, pairs of one scope next to each other (the count kernel then computes a row's cell
    once per scope); -> {replicate: (keys, values)}."""
    keys = {r: wanted(s) for r, s in enumerate(searches)}
    pairs = sorted((scope_of(k), r, i) for r, ks in keys.items() for i, k in enumerate(ks or ()))
    if not pairs:
        return {}
    values = ask([p[0] for p in pairs], np.array([p[1] for p in pairs], np.int32))
    got = {r: [None] * len(ks) for r, ks in keys.items() if ks}
    for (_, r, i), v in zip(pairs, values):
        got[r][i] = v
    return {r: (keys[r], vs) for r, vs in got.items()}


def bootstrap(X, n_boot=100, learner="hill_climb", seed=0, return_replicates=False, device=None, **learner_args):
    """Bootstrap arc strengths: `learner` ("hill_climb" or "pc", with `learner_args`) on `n_boot` multinomial resamples of the rows
    of X -> an `ArcStrength`; with `return_replicates`: (ArcStrength, [the learner's result per replicate]).

    Replicate r is `learner(X, weights=w_r, **learner_args)`, exactly, where w_r is set r of `Dataset.bootstrap(n_boot, seed)`
    (a function of (seed, r, len(X)) alone: the same seed gives the same strengths, and more replicates extend the list).  The rows
    are encoded and uploaded once and never expanded; the replicates advance in lockstep.  Complete data only."""
    if learner not in BOOTSTRAP_LEARNERS:
        raise ValueError(f"learner must be one of {BOOTSTRAP_LEARNERS}, not {learner!r}")
    if int(n_boot) != n_boot or n_boot < 1:
        raise ValueError("n_boot must be an integer >= 1")
    if int(seed) != seed:
        raise ValueError("seed must be an integer")
    for k in ("weights", "device"):
        if k in learner_args:
            raise ValueError(f"bootstrap: {k!r} is not a learner argument (a weighted frame is not resampled)")
    n_boot = int(n_boot)
    if learner == "hill_climb":
        names = ("score", "ess", "max_parents", "start", "required", "forbidden", "max_iter", "epsilon")
        defaults = ("bic", 1.0, 3, None, (), (), None, 1e-4)
    else:
        names = ("alpha", "test", "dof", "max_cond", "required", "forbidden")
        defaults = (0.01, "g2", "classic", 3, (), ())
    keep_trace = bool(learner_args.pop("return_trace", False))
    for k in learner_args:
        if k not in names:
            raise ValueError(f"bootstrap: {learner} has no argument {k!r}")
    a = {k: learner_args.get(k, d) for k, d in zip(names, defaults)}
    if learner == "hill_climb":
        columns, fresh = _climb_plan(X, *[a[k] for k in names])
    else:
        columns, req, forb = _pc_plan(X, a["alpha"], a["test"], a["dof"], a["max_cond"], a["required"], a["forbidden"])
    codes, _, cards = encode_complete(X, columns)
    with counting_engine(device).dataset(codes, cards) as ds:
        ds.bootstrap(n_boot, seed)
        if learner == "hill_climb":
            searches = [fresh() for _ in range(n_boot)]
            while not all(s.done for s in searches):
                got = _lockstep(ds, searches, lambda s: None if s.done else s.needs(), _family_scope,
                                lambda scopes, sets: ds.score_families(scopes, a["score"], a["ess"], wset=sets))
                for r, s in enumerate(searches):
                    if not s.done:
                        if r in got:
                            s.feed(*got[r])
                        s.advance()
            replicates = [s.result(keep_trace) for s in searches]
        else:
            searches = [_Skeleton(len(columns), float(a["alpha"]), int(a["max_cond"]), req, forb) for _ in range(n_boot)]
            live = list(searches)

            def wanted(s):
                if s in live and s.next_batch() is None:
                    live.remove(s)
                return s.batch if s in live else None

            while live:
                got = _lockstep(ds, searches, wanted, lambda k: k,
                                lambda tests, sets: _ci_batch(ds, cards, len(X), tests, a["test"], a["dof"], wset=sets)[2])
                for r, s in enumerate(searches):
                    if r in got:
                        s.feed(got[r][1])
            replicates = [PCResult(columns, s.finish(), keep_trace) for s in searches]
    strength = ArcStrength(columns, replicates)
    return (strength, replicates) if return_replicates else strength
