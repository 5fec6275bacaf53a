"""Host-side mirror of the reference's `BayesNet` for the exact-inference hot path.

Same constructor, attributes (`P`, `parents`, `children`, `nodes`), `prepare()`, `query()` and
`impute()` as MaxHalford/sorobn (sorobn/bayes_net.py:259-371, 796-908) - names, argument meaning,
return types and error behaviour - but `query(algorithm="exact")` runs on an MI355X: the pandas
CPTs are flattened once (flatten.py) and the variable-elimination loop (bayes_net.py:739-794) is
executed by hand-written gfx950 kernels behind the C-ABI of include/mibn.h.  There is no CPU
fallback: without the HIP extension or without a gfx950 device `query` raises.

`full_joint_dist` / `predict_proba` / `predict_log_proba` (bayes_net.py:398-465, 934-973; SURVEY.md section 8f rank
1) ride on the same kernels: the joint is the posterior of all variables given no evidence, the likelihood of
partially observed rows is the posterior of the observed columns given no evidence (variable elimination of the
rest - so it also works where the reference's full joint would not fit).

`sample`, `query(algorithm="rejection" / "likelihood")` (bayes_net.py:518-663; section 8f rank 2) run on a forward-
sampling kernel (one sample per lane); like Gibbs their parity is statistical (the reference's stream needs `vose`).

`fit` / `partial_fit` (467-516; rank 3) and `sorobn_amd.structure.chow_liu` (structure.py:9-52; rank 4) count their
contingency tables with one launch of the count kernel (learning.py).

`sorobn_amd.examples` offers the reference's four example networks; `is_tree`, `markov_boundary`, `iter_dfs` mirror the
small graph helpers.  Out of scope: graph drawing (`graphviz`), GUI, CLI.

`accelerate(bn)` attaches the same backend to an *existing reference object* by replacing the two
methods `query` dispatches to (bayes_net.py:848, 851-853); see INTEGRATION.md.
"""
import collections
import collections.abc
import graphlib
import itertools
import operator
import os
import sys
import types

import numpy as np
import pandas as pd

from . import _capi
from .events import csr_rows, decode_labels, encode_frame, iter_parts, label_table, part_args, pattern_groups
from .flatten import flatten

__all__ = ["BayesNet", "accelerate", "Backend"]


def _default_device():
    for key in ("MIBN_DEVICE", "LOCAL_RANK"):
        if os.environ.get(key, "") != "":
            return int(os.environ[key])
    return 0


class _Ragged(Exception):
    """exact_many: a request whose arity differs from the first one's (the pipeline takes fixed-arity sub-batches)."""


_get_index = operator.attrgetter("index")
_get_values = operator.attrgetter("_values")  # the Series' own ndarray, no copy (`.values` builds a view object per call)
_get_names = operator.attrgetter("names")
_get_pnames = operator.attrgetter("_names")
_get_pname = operator.attrgetter("_name")


class PosteriorBatch(collections.abc.Sequence):
    """The answers of `BayesNet.query_many`: a read-only sequence whose item i is exactly the Series `query(*q_i, event=e_i)`
    returns (built when asked for: a pandas Series costs ~14 us to construct, a batch of 2^18 of them four seconds - more than
    the kernels), over the dense posteriors as they came back from the device.
      `batch[i]`, `len`, iteration, slices -> Series / lists of Series
      `batch.dense(i)`   the dense C-order posterior over request i's query variables (caller order)
      `batch.to_frame()` every answer in ONE pandas object, built vectorised: a long Series indexed by (request, *labels) when all
                         requests ask for the same variables, else a DataFrame with one row per positive cell"""

    def __init__(self, backend, queries, out, out_off):
        self._b, self._q, self.out, self.out_off = backend, queries, out, out_off

    def __len__(self):
        return len(self._q)

    def dense(self, i):
        return self.out[self.out_off[i]:self.out_off[i + 1]]

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._b.finished_series(self._q[i], self.dense(i))

    def to_frame(self):
        """One pandas object for the whole batch.  Same query variables in every request: a Series `p` with a MultiIndex
        (request, *sorted query names) - level values and row order inside a request exactly those of `batch[i]`, so
        `frame.xs(i, level="request")` equals `batch[i]` (up to the name).  Otherwise (the query variable changes from request to
        request): a DataFrame with columns request, variables (tuple of names), cell (C-order cell of the finished answer's index)
        and p, one row per positive cell."""
        n = len(self)
        sizes = np.diff(self.out_off)
        req = np.repeat(np.arange(n, dtype=np.int64), sizes)
        same = n > 0 and all(q == self._q[0] for q in self._q)
        if same:
            name, order, levels, shape, names = self._b._tail(self._q[0])
            out = self.out
            if shape is None:
                keep = np.flatnonzero(out > 0)
                codes = [req[keep], keep - self.out_off[req[keep]]]
                lv = [pd.RangeIndex(n, name="request"), levels]
                nm = ["request", self._q[0][0]]
            else:
                cells = int(np.prod(shape))
                if order is not None:
                    out = np.ascontiguousarray(out.reshape([n] + shape).transpose([0] + [k + 1 for k in order])).reshape(-1)
                    shape = [shape[k] for k in order]
                keep = np.flatnonzero(out > 0)
                codes = [keep // cells, *np.unravel_index(keep % cells, shape)]
                lv = [pd.RangeIndex(n, name="request"), *levels]
                nm = ["request", *names]
            idx = pd.MultiIndex(levels=lv, codes=codes, names=nm, verify_integrity=False)
            return pd.Series(out[keep], index=idx, name="p")
        keep = np.flatnonzero(self.out > 0)
        r = req[keep]
        # (cells of the caller-order dense table; `batch[i]` gives the finished Series of a request)
        variables = np.empty(n, object)
        variables[:] = self._q
        return pd.DataFrame({"request": r, "variables": variables[r], "cell": keep - self.out_off[r], "p": self.out[keep]})


class CptWatch:
    """Has anything the flattened tables were built from changed?  The reference re-reads `P` on every query (bayes_net.py:770),
    so a CPT replaced (`bn.P['A'] = s`), edited in place (`bn.P['A'][True] = 0.9`, also through a reference the caller kept) or
    re-indexed must reach the device tables.  Round 4 re-hashed every CPT on every `query()` (several hundred
    microseconds on the 100-node grid).  Now: identity of every Series, of its index and of its value array (three id lists
    compared in C), the level names, and ONE bitwise comparison of all CPT numbers against a snapshot (`np.concatenate` of the live
    arrays: 44 KB on the 10x10 grid) - 5 us on a five-node network, 60 us on the grid, and exact: no hashing, no version counter a
    held reference could bypass.  CPTs whose values are not a numeric ndarray fall back to the hashed
    fingerprint."""

    def __init__(self, bn):
        items = list(bn.P.items())
        self.keys = [k for k, _ in items]
        self.series = [v for _, v in items]  # (kept alive: their ids below cannot be recycled by other objects)
        self.exact = True
        try:
            self.index = list(map(_get_index, self.series))
            arrays = list(map(_get_values, self.series))
            self.exact = all(isinstance(a, np.ndarray) and a.dtype != object and a.ndim == 1 for a in arrays)
        except AttributeError:
            self.exact = False
        if self.exact:
            self.ids = (list(map(id, self.series)), list(map(id, self.index)))
            # level names live on the index object and can be re-assigned in place; pandas keeps them in `_names` (MultiIndex: a
            # list) / `_name` (Index) - read directly where present (checked against the public accessor here), the public
            # FrozenList-building `.names` costs ten times as much per CPT
            self.multi = [ix for ix in self.index if isinstance(ix, pd.MultiIndex)]
            self.single = [ix for ix in self.index if not isinstance(ix, pd.MultiIndex)]
            try:
                self.private_names = (all(list(ix._names) == list(ix.names) for ix in self.multi) and
                                      all(ix._name == ix.name or (ix._name is None and ix.name is None) for ix in self.single))
            except AttributeError:
                self.private_names = False
            if self.private_names:
                self.names = ([list(ix._names) for ix in self.multi], [ix._name for ix in self.single])
            else:
                self.names = [list(n) for n in map(_get_names, self.index)]
            self.snap = np.concatenate(arrays).tobytes() if arrays else b""
        else:
            self.slow = Backend.fingerprint_of(bn)

    def changed(self, bn) -> bool:
        P = bn.P
        if len(P) != len(self.keys):
            return True
        if not self.exact:
            return Backend.fingerprint_of(bn) != self.slow
        # (every loop below runs inside map / list comparison: no Python-level work per CPT)
        ids_s, ids_i = self.ids
        if list(map(id, map(P.get, self.keys))) != ids_s or list(map(id, map(_get_index, self.series))) != ids_i:
            return True
        if self.private_names:
            if list(map(_get_pnames, self.multi)) != self.names[0] or list(map(_get_pname, self.single)) != self.names[1]:
                return True
        elif list(map(_get_names, self.index)) != self.names:
            return True
        if not self.series:
            return False
        # the LIVE value arrays (a Series may have replaced its array - an upcast, copy-on-write) against the snapshot, bit for bit
        try:
            return np.concatenate(list(map(_get_values, self.series))).tobytes() != self.snap
        except (ValueError, TypeError):
            return True


class Backend:
    """Flattened network + one mibn engine.  Built lazily from any object exposing the reference's
    `nodes` / `parents` / `P`; rebuilt when the CPT objects change."""

    def __init__(self, bn, device=None, planner_only=False):
        self.flat = flatten(bn)
        self.watch = CptWatch(bn)
        self.engine = _capi.Engine(_default_device() if device is None else device,
                                   planner_only=planner_only)
        f = self.flat
        self.engine.set_network(f.card, f.scope_off, f.scope_vars, f.value_off, f.values)
        if f.hints:
            self.engine.set_order_hints(np.stack(f.hints))
        self._anc = {}
        self._presence = None
        self._device = device
        self._planner_only = planner_only

    def presence_engine(self):
        """A second engine over the same structure whose tables hold 1.0 where the sparse CPT has a row: its joint
        is positive exactly on the rows of the reference's inner join (full_joint_dist(keep_zeros=True))."""
        if self._presence is None:
            f = self.flat
            e = _capi.Engine(_default_device() if self._device is None else self._device, planner_only=self._planner_only)
            e.set_network(f.card, f.scope_off, f.scope_vars, f.value_off, f.present)
            self._presence = e
        return self._presence

    def marginal(self, names, engine=None):
        """Dense C-order table P(names) with no evidence (all other variables eliminated)."""
        q, _, _ = self.encode(names, {})
        eng = self.engine if engine is None else engine
        # every CPT takes part (bayes_net.py:460): no pruning to the ancestors - with sparse CPTs a barren node
        # does not sum to 1.  A per-call flag: nothing engine-wide changes under asynchronous calls in flight.
        return eng.query_fixed([q], np.zeros((1, 0), np.int32), np.zeros((1, 0), np.int32), flags=_capi.Q_NOPRUNE)[0]

    def joint_series(self, names, keep_zeros=False):
        """Series over the sorted `names` like `full_joint_dist` builds it (bayes_net.py:460-465): sorted levels, sorted
        rows, zero rows dropped unless keep_zeros (then: the rows present in every CPT)."""
        f = self.flat
        ids = [f.id[n] for n in names]
        dense = self.marginal(names)
        if keep_zeros:
            mask = self.marginal(names, self.presence_engine()) > 0
        else:
            mask = dense > 0
        keep = np.flatnonzero(mask)
        if len(ids) == 1:
            idx = f.dom_index[ids[0]][keep].rename(names[0])
        else:
            codes = np.unravel_index(keep, [int(f.card[v]) for v in ids])
            idx = pd.MultiIndex(levels=[f.dom_index[v] for v in ids], codes=list(codes), names=list(names),
                                verify_integrity=False)
        return pd.Series(dense[keep], index=idx)

    def stale(self, bn) -> bool:
        """True when `bn.P` no longer is what this backend was flattened from (`CptWatch`)."""
        return self.watch.changed(bn)

    @staticmethod
    def fingerprint_of(bn):
        """Identity AND content of the CPTs by hashing (the slow path of `CptWatch`: CPTs whose values are not numeric
        ndarrays)."""
        fp = []
        for k, v in bn.P.items():
            vals = getattr(v, "values", None)
            try:
                if vals is None:
                    content = None
                elif vals.dtype != object:
                    content = hash(np.ascontiguousarray(vals).tobytes())
                else:
                    content = hash(tuple(vals.tolist()))
            except (TypeError, ValueError, AttributeError):
                content = None
            idx = getattr(v, "index", None)
            if isinstance(idx, pd.MultiIndex):
                ih = hash(tuple(np.ascontiguousarray(c).tobytes() for c in idx.codes)) ^ hash(tuple(len(l) for l in idx.levels))
            elif idx is not None:
                try:
                    ih = hash(tuple(idx.tolist()))
                except TypeError:
                    ih = len(idx)
            else:
                ih = 0
            fp.append((id(k), id(v), len(v), content, ih))
        return tuple(fp)

    # ---- id / code conversion -------------------------------------------------------------------
    def var_id(self, name):
        try:
            return self.flat.id[name]
        except (KeyError, TypeError):
            raise KeyError(name)  # bayes_net.py:770 / 373-375: unknown node -> KeyError(name)

    def _ancestors(self, v):
        if v not in self._anc:
            s = set()
            for p in self.flat.parents[v]:
                s.add(p)
                s |= self._ancestors(p)
            self._anc[v] = s
        return self._anc[v]

    def encode(self, query, event, findings=()):
        """names/labels -> (qvars, evars, ecodes); raises KeyError like the reference when a relevant
        node is unknown or has no CPT.  `findings` (encode_likelihood): their variables are relevant too."""
        q = [self.var_id(n) for n in query]
        ev = [self.var_id(n) for n in event]
        codes = [self.flat.code_of(v, lab) for v, lab in zip(ev, event.values())]
        if self.flat.missing:
            rel = set(q) | set(ev) | {v for v, _ in findings}
            for v in list(rel):
                rel |= self._ancestors(v)
            for v in sorted(rel & self.flat.missing):
                raise KeyError(self.flat.names[v])
        return q, ev, codes

    # ---- likelihood findings (soft evidence) ------------------------------------------------------
    def encode_likelihood(self, likelihood, event=()):
        """{variable: mapping or Series label -> weight} -> [(variable id, float64 weights, one per state)].  A label of the domain
        that is not named gets weight 0 ("X is a or b"); a label outside the domain raises ValueError, an unknown variable the
        reference's KeyError(name), a variable that is also in `event` ValueError - as do weights that are negative or not finite."""
        out = []
        for name, lam in (likelihood or {}).items():
            v = self.var_id(name)
            if name in event:
                raise ValueError("A likelihood variable cannot be part of the event")
            w = np.zeros(int(self.flat.card[v]), np.float64)
            for lab, x in lam.items():
                c = self.flat.code_of(v, lab)
                if c < 0:
                    raise ValueError(f"{lab!r} is not a label of {name!r}")
                x = float(x)
                if not (0.0 <= x < np.inf):
                    raise ValueError(f"the weights of a likelihood finding must be finite and non-negative ({name!r}: {x!r})")
                w[c] = x
            out.append((v, w))
        return out

    @staticmethod
    def likelihood_block(per_request):
        """The findings of a batch, one encode_likelihood list per request -> the CSR block (l_off, l_vars, v_off, values) of
        `Engine.*(likelihoods=...)`, or None when no request has a finding."""
        if not any(per_request):
            return None
        l_off = np.zeros(len(per_request) + 1, np.int64)
        np.cumsum([len(fs) for fs in per_request], out=l_off[1:])
        flat = [f for fs in per_request for f in fs]
        v_off = np.zeros(len(flat) + 1, np.int64)
        np.cumsum([len(w) for _, w in flat], out=v_off[1:])
        return (l_off, np.array([v for v, _ in flat], np.int32), v_off,
                np.concatenate([w for _, w in flat]) if flat else np.zeros(0, np.float64))

    # ---- loopy belief propagation (mibn_bp_batch) -----------------------------------------------------
    def lbp(self, event, likelihood=None, n_iterations=100, tol=1e-9, damping=0.0):
        """One request -> (beliefs [sum(card)] float64 - variable v at sum(card[:v]) -, iterations, residual).  Every CPT takes
        part: a node without one raises the reference's KeyError."""
        findings = self.encode_likelihood(likelihood, event)
        _, ev, codes = self.encode((), event, findings)
        if self.flat.missing:
            raise KeyError(self.flat.names[min(self.flat.missing)])
        more = {"likelihoods": self.likelihood_block([findings])} if findings else {}
        bel, it, res = self.engine.bp(np.array(ev, np.int32).reshape(1, len(ev)), np.array(codes, np.int32).reshape(1, len(ev)),
                                      n_iterations, tol, damping, **more)
        return bel[0], int(it[0]), float(res[0])

    # ---- result construction --------------------------------------------------------------------
    def posterior_series(self, query, dense):
        """Dense C-order posterior over `query` (caller order) -> the Series
        `_variable_elimination` returns (bayes_net.py:789-794): zero rows absent, one level per query
        variable, plain Index for a single variable."""
        f = self.flat
        ids = [f.id[n] for n in query]
        keep = np.flatnonzero(dense > 0)
        vals = dense[keep]
        if len(ids) == 1:
            idx = f.dom_index[ids[0]][keep]
            idx = idx.rename(query[0])
            return pd.Series(vals, index=idx)
        shape = [int(f.card[v]) for v in ids]
        codes = np.unravel_index(keep, shape)
        idx = pd.MultiIndex(levels=[f.dom_index[v] for v in ids], codes=list(codes),
                            names=list(query), verify_integrity=False)
        return pd.Series(vals, index=idx)

    def _tail(self, query):
        """What the tail of `query` (bayes_net.py:869-875: rename, level sort, row sort) amounts to for a given query tuple, worked
        out once: the Series name, and for several variables the level permutation into sorted-name order.  The dense posterior
        is C-order over `query`, the label domains are sorted, so transposing it into sorted-name order and listing its positive
        cells in C-order IS the sorted index - no pandas reorder_levels / sort_index per answer (61 -> 14 us on this host)."""
        try:
            cache = self._tails
        except AttributeError:
            cache = self._tails = {}
        t = cache.get(query)
        if t is None:
            f = self.flat
            ids = [f.id[n] for n in query]
            name = f"P({', '.join(query)})"
            if len(ids) == 1:
                t = (name, None, f.dom_index[ids[0]].rename(query[0]), None, None)
            else:
                names = list(query)
                order = [names.index(n) for n in sorted(names)]
                shape = [int(f.card[v]) for v in ids]
                t = (name, order if order != list(range(len(ids))) else None, [f.dom_index[ids[k]] for k in order],
                     shape, [names[k] for k in order])
            if len(cache) < 4096:
                cache[query] = t
        return t

    def finished_series(self, query, dense):
        """Dense C-order posterior over `query` (caller order) -> exactly the Series `query()` returns: zero rows absent
        (bayes_net.py:789-794), named `P(...)`, levels in sorted-name order, rows sorted (869-875)."""
        name, order, levels, shape, names = self._tail(query)
        if shape is None:
            keep = np.flatnonzero(dense > 0)
            if len(keep) == len(dense):
                # (a view of the cached Index - renaming the answer's index must not reach the cache - and, for an answer that is a
                # slice of a batch's buffer, its own numbers: ADVICE r5)
                return pd.Series(dense if dense.base is None else dense.copy(), index=levels.view(), name=name)
            return pd.Series(dense[keep], index=levels[keep], name=name)
        if order is not None:
            dense = np.ascontiguousarray(dense.reshape(shape).transpose(order)).reshape(-1)
            shape = [shape[k] for k in order]
        keep = np.flatnonzero(dense > 0)
        idx = pd.MultiIndex(levels=levels, codes=list(np.unravel_index(keep, shape)), names=names, verify_integrity=False)
        return pd.Series(dense[keep], index=idx, name=name)

    def exact_query(self, query, event, likelihood=None):
        """`query(*query, event=event)` of the exact path, finished: encode, ONE call into the library, the answer Series."""
        if likelihood:
            findings = self.encode_likelihood(likelihood, event)
            q, ev, codes = self.encode(query, event, findings)
            dense = self.engine.query_fixed([q], [ev], [codes], likelihoods=self.likelihood_block([findings]))[0]
            return self.finished_series(query, dense)
        q, ev, codes = self.encode(query, event)
        one = getattr(self.engine, "query_one", None)
        dense = one(q, ev, codes) if one is not None else self.engine.query_fixed([q], [ev], [codes])[0]
        return self.finished_series(query, dense)

    # ---- the two replaced methods ---------------------------------------------------------------
    def variable_elimination(self, *query, event):
        q, ev, codes = self.encode(query, event)
        out = self.engine.query_fixed([q], [ev], [codes])
        return self.posterior_series(query, out[0])

    def variable_elimination_many(self, requests):
        """requests: iterable of (query tuple, event dict) -> list of Series (one launch)."""
        requests = list(requests)
        q_off, e_off, qv, evs, ecs = self.encode_many(requests)
        out, out_off = self.engine.query_batch(q_off, qv, e_off, evs, ecs)
        return [self.posterior_series(query, out[a:b])
                for (query, _), a, b in zip(requests, out_off[:-1], out_off[1:])]

    def encode_many(self, requests):
        """CSR arrays (q_off, q_vars, e_off, e_vars, e_codes) of a list of (query tuple, event dict).  Names and labels go
        through plain dict lookups in bulk (one pass over the flattened names, one over the flattened labels) instead of one
        `encode` call with its set algebra per request; anything the bulk path cannot answer - an unknown name, an unhashable or
        out-of-domain label, a network with missing CPTs - falls back to `encode` request by request, which raises the
        reference's KeyError or codes the label -1 as before."""
        f = self.flat
        n = len(requests)
        try:
            if f.missing:
                raise KeyError
            ident = f.id
            nq = np.fromiter((len(q) for q, _ in requests), np.int64, n)
            ne = np.fromiter((len(e) for _, e in requests), np.int64, n)
            qv = np.fromiter((ident[name] for q, _ in requests for name in q), np.int32, int(nq.sum()))
            evs = np.fromiter((ident[name] for _, e in requests for name in e), np.int32, int(ne.sum()))
            luts = self._label_luts()
            ecs = np.fromiter((luts[v][lab] for v, lab in zip(evs.tolist(), (lab for _, e in requests for lab in e.values()))),
                              np.int32, len(evs))
            q_off = np.zeros(n + 1, np.int64)
            e_off = np.zeros(n + 1, np.int64)
            np.cumsum(nq, out=q_off[1:])
            np.cumsum(ne, out=e_off[1:])
            return q_off, qv, e_off, evs, ecs
        except (KeyError, TypeError):
            pass
        q_off, e_off, qv, evs, ecs = [0], [0], [], [], []
        for query, event in requests:
            q, ev, codes = self.encode(query, event)
            qv += q
            evs += ev
            ecs += codes
            q_off.append(len(qv))
            e_off.append(len(evs))
        return (np.array(q_off, np.int64), np.array(qv, np.int32), np.array(e_off, np.int64), np.array(evs, np.int32),
                np.array(ecs, np.int32))

    def _label_luts(self):
        """Per variable: label -> code (equal labels hash equally: 1, 1.0 and True share a slot, like the `==` of
        bayes_net.py:774); a variable with unhashable labels has no table (KeyError -> the per-request path)."""
        try:
            return self._luts
        except AttributeError:
            luts = []
            for dom in self.flat.domains:
                t = {}
                try:
                    for i, d in enumerate(dom):
                        t.setdefault(d, i)
                except TypeError:
                    t = {}
                luts.append(t)
            self._luts = luts
            return luts

    def exact_many(self, requests, sub_batch=32768):
        """The exact path over a list of (query tuple, event dict) -> `PosteriorBatch`.  Encoded in bulk, sent to the engine in
        sub-batches of `sub_batch` requests with two calls in flight (mibn_submit_batch / mibn_wait: sub-batch k + 1 is encoded
        and planned while the kernels of k run) when the batch is fixed-arity; a ragged batch goes as one blocking call."""
        def checked(chunk):
            """Query tuples normalised (a bare name is a 1-tuple) and the request checks of `query` (bayes_net.py:840-845)."""
            chunk = [((q,) if isinstance(q, str) else tuple(q), e) for q, e in chunk]
            for q, e in chunk:
                if not q:
                    raise ValueError("At least one query variable has to be specified")
                if not e.keys().isdisjoint(q):
                    raise ValueError("A query variable cannot be part of the event")
            return chunk

        n = len(requests)
        eng = self.engine
        if n == 0:
            return PosteriorBatch(self, [], np.zeros(0), np.zeros(1, np.int64))
        if any(len(r) == 3 for r in requests):
            # requests (query, event, likelihood): sub-batch by sub-batch through the blocking call, which takes the findings
            queries, parts, cells = [], [], []
            for a in range(0, n, sub_batch):
                chunk = [(r[0], r[1], r[2] if len(r) == 3 else None) for r in requests[a:a + sub_batch]]
                plain = checked([(q, e) for q, e, _ in chunk])
                findings = [self.encode_likelihood(lam, e) for _, e, lam in chunk]
                if self.flat.missing:
                    for (q, e), fs in zip(plain, findings):
                        self.encode(q, e, fs)
                q_off, qv, e_off, evs, ecs = self.encode_many(plain)
                out, out_off = eng.query_batch(q_off, qv, e_off, evs, ecs, likelihoods=self.likelihood_block(findings))
                queries.extend(q for q, _ in plain)
                parts.append(out)
                cells.append(np.diff(np.asarray(out_off, np.int64)))
            out_off = np.zeros(n + 1, np.int64)
            np.cumsum(np.concatenate(cells), out=out_off[1:])
            return PosteriorBatch(self, queries, np.concatenate(parts), out_off)
        if not (hasattr(eng, "submit_fixed") and n > sub_batch):
            requests = checked(requests)
            q_off, qv, e_off, evs, ecs = self.encode_many(requests)
            out, out_off = eng.query_batch(q_off, qv, e_off, evs, ecs)
            return PosteriorBatch(self, [q for q, _ in requests], out, np.asarray(out_off, np.int64))
        # a long batch: sub-batches through the two-deep pipeline.  Checked, normalised and encoded sub-batch by sub-batch on a helper
        # thread (a malformed request in sub-batch k raises after the sub-batches before it have run; nothing is returned); the
        # pipeline takes fixed-arity batches - the arity of the first request - and a ragged one falls back to ONE blocking call
        q00 = requests[0][0]
        nq0, ne0 = (1 if isinstance(q00, str) else len(q00)), len(requests[0][1])
        queries = []
        # names / labels -> ids / codes on a helper thread, one sub-batch ahead: the engine calls below release the GIL (ctypes), so
        # the encoding of sub-batch k + 1 runs while the planner works on k and the host waits for the kernels of k - 1
        import queue
        import threading
        todo = queue.Queue(maxsize=2)
        stop = threading.Event()  # set by the consumer when it gives up: the producer does not encode the rest of a 1 M-request batch
        # query tables of different sizes in one fixed-arity batch (a 2-state and a 3-state query variable): the engine's flat
        # wait; an engine without one (the test doubles) takes such a batch through the general CSR call
        wait_flat = getattr(eng, "wait_flat", None)

        def produce():
            try:
                for a in range(0, n, sub_batch):
                    if stop.is_set():
                        break
                    chunk = checked(requests[a:a + sub_batch])
                    if not all(len(q) == nq0 and len(e) == ne0 for q, e in chunk):
                        raise _Ragged()
                    _, qv, _, evs, ecs = self.encode_many(chunk)
                    cells = np.prod(eng.card[qv.reshape(len(chunk), nq0)].astype(np.int64), axis=1)
                    if wait_flat is None and len(cells) and cells.min() != cells.max():
                        raise _Ragged()
                    queries.extend(q for q, _ in chunk)
                    todo.put((len(chunk), qv, evs, ecs, cells))
            except BaseException as e:  # noqa: BLE001 - re-raised on the calling thread (the reference's KeyError for an unknown name)
                todo.put(e)
            todo.put(None)

        def collect(h):
            return (wait_flat(h) if wait_flat is not None else eng.wait(h)).reshape(-1)

        worker = threading.Thread(target=produce, daemon=True)
        worker.start()
        parts, pending, cells = [], None, []
        try:
            while True:
                item = todo.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                b, qv, evs, ecs, c = item
                h = eng.submit_fixed(qv.reshape(b, nq0), evs.reshape(b, ne0), ecs.reshape(b, ne0))
                if pending is not None:
                    prev, pending = pending, h  # (cleared before the wait: an error inside it must not wait on the same ticket again)
                    parts.append(collect(prev))
                pending = h
                cells.append(c)
        except BaseException:
            stop.set()
            last, pending = pending, None
            if last is not None:  # (a call in flight writes into its pinned result buffer: collect it before the error leaves)
                try:
                    eng.wait(last)
                except Exception:  # noqa: BLE001
                    pass
            while worker.is_alive():  # let the producer finish (its queue may be full)
                try:
                    todo.get(timeout=0.05)
                except queue.Empty:
                    pass
            if isinstance(sys.exc_info()[1], _Ragged):  # requests of different arity: the general CSR call, once
                requests = checked(requests)
                q_off, qv, e_off, evs, ecs = self.encode_many(requests)
                out, out_off = eng.query_batch(q_off, qv, e_off, evs, ecs)
                return PosteriorBatch(self, [q for q, _ in requests], out, np.asarray(out_off, np.int64))
            raise
        worker.join()
        parts.append(collect(pending))
        out_off = np.zeros(n + 1, np.int64)
        np.cumsum(np.concatenate(cells), out=out_off[1:])
        return PosteriorBatch(self, queries, np.concatenate(parts), out_off)

    def gibbs_sampling(self, *query, event, n_iterations, n_chains=1, seed=0):
        q, ev, codes = self.encode(query, event)
        f = self.flat
        # the reference cycles through sorted(nodes - event) (bayes_net.py:697,718)
        free = [v for v in range(len(f.names)) if v not in set(ev)]
        try:
            cycle = sorted(free, key=lambda v: f.names[v])
        except TypeError:
            cycle = free
        counts = self.engine.gibbs(q, ev, codes, n_chains, n_iterations, seed=seed, cycle=cycle)
        dense = counts.astype(np.float64) / float(max(1, n_chains * n_iterations))
        return self.posterior_series(query, dense)

    # ---- forward sampling and the algorithms built on it ---------------------------
    def _cells_series(self, query, values, present):
        """Series over the joint query states `present` (flat C-order cell ids), like a pandas groupby builds it."""
        f = self.flat
        ids = [f.id[n] for n in query]
        keep = np.flatnonzero(present)
        if len(ids) == 1:
            idx = f.dom_index[ids[0]][keep].rename(query[0])
        else:
            codes = np.unravel_index(keep, [int(f.card[v]) for v in ids])
            idx = pd.MultiIndex(levels=[f.dom_index[v] for v in ids], codes=list(codes), names=list(query),
                                verify_integrity=False)
        return pd.Series(np.asarray(values, np.float64)[keep], index=idx)

    def rejection_sampling(self, *query, event, n_iterations, seed=0):
        """bayes_net.py:577-619: the share of each query state among the forward samples that agree with the event."""
        q, ev, codes = self.encode(query, event)
        _, counts = self.engine.sampling_query(1, q, ev, codes, n_iterations, seed=seed)
        total = counts.sum()
        return self._cells_series(query, counts / float(total) if total else counts.astype(np.float64), counts > 0)

    def likelihood_weighting(self, *query, event, n_iterations, seed=0):
        """bayes_net.py:621-663: per query state the mean likelihood of the samples drawn with the event clamped,
        normalised (the reference's estimator, product of P(value | parents) over all nodes)."""
        q, ev, codes = self.encode(query, event)
        if any(c < 0 for c in codes):  # P.get(value, 0) == 0 for a label outside the domain: every likelihood is 0
            raise ValueError("likelihood weighting: an event label is outside the variable's domain")
        wsum, counts = self.engine.sampling_query(2, q, ev, codes, n_iterations, seed=seed)
        mean = np.divide(wsum, counts, out=np.zeros_like(wsum), where=counts > 0)
        s = mean.sum()
        return self._cells_series(query, mean / s if s > 0 else mean, counts > 0)

    def forward_samples(self, n, init, seed=0):
        """bayes_net.py:518-575: n joint samples as a DataFrame of labels (columns in variable-id = `nodes` order)."""
        f = self.flat
        iv = [self.var_id(k) for k in init]
        ic = [f.code_of(v, lab) for v, lab in zip(iv, init.values())]
        if any(c < 0 for c in ic):
            raise ValueError("sample: an init label is outside the variable's domain")
        codes = self.engine.sample(n, iv, ic, seed=seed)
        return pd.DataFrame({name: np.asarray(f.dom_index[v])[codes[:, v]] for v, name in enumerate(f.names)})


class BayesNet:
    """Bayesian network with an MI355X exact-inference backend.

    Parameters follow the reference (bayes_net.py:259-289): `structure` is a sequence of
    `(parent(s), child(ren))` tuples (lists are expanded to their cartesian product) and bare node
    names; `prior_count` and `seed` are accepted for signature compatibility (`seed` seeds the Gibbs
    kernel).
    """

    def __init__(self, *structure, prior_count: int = None, seed: int = None):
        self.prior_count = prior_count
        self.seed = seed
        as_list = lambda o: o if isinstance(o, list) else [o]
        parents = collections.defaultdict(set)
        children = collections.defaultdict(set)
        loose = set()
        for item in structure:
            if isinstance(item, tuple):
                ps, cs = item
                for p, c in itertools.product(as_list(ps), as_list(cs)):
                    parents[c].add(p)
                    children[p].add(c)
            else:
                loose.add(item)
        self.parents = {n: sorted(ps) for n, ps in parents.items()}
        self.children = {n: sorted(cs) for n, cs in children.items()}
        # topological order, ties lexicographic - same construction as bayes_net.py:319-322 so that
        # `nodes` (and with it variable ids) are identical to the reference's
        sorter = graphlib.TopologicalSorter()
        for n in sorted({*self.parents, *self.children, *loose}):
            sorter.add(n, *self.parents.get(n, []))
        self.nodes = list(sorter.static_order())
        self.P = {}
        self._backend = None
        self._device = None

    # ---- pickling / copying: device handles are rebuilt lazily -----------
    def __getstate__(self):
        d = dict(self.__dict__)
        d["_backend"] = None
        return d

    # ---- CPT house-keeping (bayes_net.py:327-371) ------------------------------------------------
    def prepare(self) -> "BayesNet":
        """Normalise the user's CPTs: DataFrame with a 'p' column -> Series; name / order the
        index levels as [*parents, node]; sort; name the Series.  Raises the reference's
        ValueErrors (bayes_net.py:341-344, 349-352)."""
        for node in list(self.P):
            P = self.P[node]
            parents = self.parents.get(node, [])
            if isinstance(P, pd.DataFrame):
                if "p" not in P.columns:
                    raise ValueError(f"DataFrame for '{node}' must have a 'p' column "
                                     f"containing probabilities")
                cols = [c for c in P.columns if c != "p"]
                expected = set(parents) | {node}
                if set(cols) != expected:
                    raise ValueError(f"DataFrame for '{node}' has columns {cols}, "
                                     f"but expected {sorted(expected)} (plus 'p')")
                P = P.set_index([*parents, node])["p"]
            wanted = [*parents, node]
            if not parents:
                P = P.copy() if P is self.P[node] else P
                P.index.name = node
            elif set(P.index.names) == set(wanted):
                # NOTE: the reference computes this reordering but never stores it back
                # (SURVEY.md section 3.4); here the reordered, sorted table is what is kept
                P = P.reorder_levels(wanted)
            else:
                P = P.copy() if P is self.P[node] else P
                P.index.names = wanted
            P = P.sort_index()
            P.name = f"P({node} | {', '.join(map(str, parents))})" if parents else f"P({node})"
            self.P[node] = P
        self._backend = None
        return self

    # ---- graph helpers on the hot path ----------------------------------------------------------
    def ancestors(self, node):
        """Set of ancestors (bayes_net.py:373-378), memoised instead of re-walked."""
        memo = {}

        def walk(n):
            if n not in memo:
                s = set()
                for p in self.parents.get(n, ()):
                    s.add(p)
                    s |= walk(p)
                memo[n] = s
            return memo[n]

        return set(walk(node))

    @property
    def roots(self):
        return [n for n in self.nodes if n not in self.parents]

    @property
    def leaves(self):
        return [n for n in self.nodes if n not in self.children]

    @property
    def is_tree(self):
        """No node has more than one parent (bayes_net.py:975-1000)."""
        return all(len(ps) <= 1 for ps in self.parents.values())

    def markov_boundary(self, node):
        """Parents, children and the children's other parents, sorted (bayes_net.py:1002-1039) - the variables the
        Gibbs kernel reads when it resamples `node`."""
        boundary = set(self.parents.get(node, []))
        for child in self.children.get(node, []):
            boundary.add(child)
            boundary.update(self.parents[child])
        boundary.discard(node)
        return sorted(boundary)

    def iter_dfs(self):
        """Depth-first pre-order from every root in `roots` order, children in sorted order (bayes_net.py:1041-1075)."""
        seen = set()
        stack = list(reversed(self.roots))
        while stack:
            node = stack.pop()
            if node in seen:
                continue
            seen.add(node)
            yield node
            stack.extend(c for c in reversed(self.children.get(node, [])) if c not in seen)

    # ---- backend --------------------------------------------------------------------------------
    def use_device(self, device: int):
        """Bind to a HIP device index (default: $MIBN_DEVICE, $LOCAL_RANK, else 0)."""
        self._device = device
        self._backend = None
        return self

    @property
    def backend(self) -> Backend:
        b = self._backend
        if b is None or b.stale(self):
            b = self._backend = Backend(self, device=self._device)
        return b

    def _variable_elimination(self, *query, event):
        return self.backend.variable_elimination(*query, event=event)

    def _gibbs_sampling(self, *query, event, n_iterations, n_chains=1):
        return self.backend.gibbs_sampling(*query, event=event, n_iterations=n_iterations,
                                           n_chains=n_chains, seed=self.seed or 0)

    def _next_seed(self):
        """The reference advances one `random.Random(seed)` per object (bayes_net.py:289): successive sampling
        calls see different streams, the same sequence of calls on an equally seeded object repeats."""
        self._draws = getattr(self, "_draws", 0) + 1
        return ((self.seed or 0) * 0x9E3779B97F4A7C15 + self._draws) & (2**64 - 1)

    def _rejection_sampling(self, *query, event, n_iterations):
        return self.backend.rejection_sampling(*query, event=event, n_iterations=n_iterations, seed=self._next_seed())

    def _llh_weighting(self, *query, event, n_iterations):
        return self.backend.likelihood_weighting(*query, event=event, n_iterations=n_iterations, seed=self._next_seed())

    def sample(self, n=1, init: dict = None, method="forward"):
        """Joint samples: a Series for n == 1, else a DataFrame with sorted columns.

        `method="forward"` (the reference's, bayes_net.py:550-575): forward (ancestral) sampling; `init` forces variables to given
        values, their ancestors are still drawn from the prior.  `method="posterior"` (an extension): exact, independent samples
        of P(x | init) under the normalised joint - `init` is evidence - by elimination and backward sampling on the device
        (mibn_posterior_sample_batch); never a state of probability zero, also with sparse CPTs.  Evidence of probability zero
        raises ValueError."""
        if method == "posterior":
            return self._posterior_sample(n, dict(init or {}))
        if method != "forward":
            raise ValueError("Unknown method, must be one of: forward")
        df = self.backend.forward_samples(max(1, n), init or {}, seed=self._next_seed())
        if n > 1:
            return df.sort_index(axis="columns")
        return df.iloc[0].rename(None)

    # ---- exact posterior sampling (an extension: forward filtering, backward sampling on the device) -------------------------
    def _posterior_sample(self, n, event):
        if n < 1:
            raise ValueError("sample: n must be at least 1")
        be = self._event_backend(event, every_cpt=True)
        f = be.flat
        ev = [f.id[name] for name in event]
        codes = [f.code_of(v, lab) for v, lab in zip(ev, event.values())]
        flags = _capi.DRAW_PRUNE if self._cpts_are_distributions(be) else 0
        out, p_e = be.engine.posterior_sample(np.array([ev], np.int32).reshape(1, len(ev)), np.array([codes], np.int32).reshape(1, len(ev)),
                                              int(n), seed=self._next_seed(), flags=flags)
        if not p_e[0] > 0:
            raise ValueError(f"sample: the evidence of row 0 has probability zero: {event}")
        df = pd.DataFrame(decode_labels(f, self._all_names(), out, event), columns=list(f.names))
        if n > 1:
            return df.sort_index(axis="columns")
        return df.iloc[0].rename(None)

    def sample_frame(self, events: pd.DataFrame, n=1, seed=None, sub_batch=32768, return_proba=False):
        """`n` exact posterior samples for every row of `events`, in the convention of `mpe_frame`: the columns are evidence
        variables, NaN / None = not observed in that row; rows are grouped by their pattern of observed columns, one engine call
        per group (in sub-batches of `sub_batch` rows).  Returns a DataFrame of len(events) * n rows, indexed by (event index,
        draw), one column per variable (sorted names); evidence keeps its label.  A row whose evidence has probability zero (or a
        label outside its domain) gets None for every other variable.  `seed`: the stream of this call (default: the object's next
        seed, as `sample`); the same seed on the same events repeats the frame.  With `return_proba`, (frame, P(evidence) of every
        row of `events` under the normalised joint, as a numpy array)."""
        if n < 1:
            raise ValueError("sample_frame: n must be at least 1")
        cols = list(events.columns)
        be = self._event_backend(cols, every_cpt=True)
        f = be.flat
        ev_ids, codes, observed = encode_frame(be, cols, events)
        n = int(n)
        n_ev = len(events)
        nv = len(f.names)
        out = np.zeros((n_ev, n, nv), np.int32)
        mass = np.zeros(n_ev, np.float64)
        # (the Philox counter of a sample is its position in the order the calls are made, so the grouping is part of what a seed
        # means: a frame too wide for a bit mask keeps the one call per row, in row order, it has always had)
        groups = pattern_groups(observed, wide_by_row=True)
        seed = self._next_seed() if seed is None else int(seed)
        eng = be.engine
        flags = _capi.DRAW_PRUNE if self._cpts_are_distributions(be) else 0
        z = 1.0
        done = 0
        if return_proba and not flags:  # (CPTs that are not distributions: the mass of the empty event normalises)
            z = float(eng.posterior_sample_batch(np.zeros(2, np.int64), [], [], np.zeros(2, np.int64), seed=seed)[1][0])
        for part, on in iter_parts(groups, observed, sub_batch):
            # (global sample rows in the order the calls are made: every sample of the frame has a Philox counter of its own)
            e_off = np.arange(len(part) + 1, dtype=np.int64) * len(on)
            s_off = (done + np.arange(len(part) + 1, dtype=np.int64)) * n
            evars, ecodes = part_args(ev_ids, codes, part, on)
            got, m = eng.posterior_sample_batch(e_off, evars.reshape(-1), ecodes.reshape(-1), s_off, seed=seed, flags=flags)
            out[part] = got.reshape(len(part), n, nv)
            mass[part] = m
            done += len(part)
        names = self._all_names()
        data = decode_labels(f, names, out.reshape(n_ev * n, nv), events, n)
        index = pd.MultiIndex.from_product([events.index, range(n)], names=[events.index.name, "draw"])
        frame = pd.DataFrame(data, index=index, columns=names)
        if return_proba:
            return frame, (mass / z if z > 0 else np.zeros(n_ev, np.float64))
        return frame

    # ---- public API (bayes_net.py:796-908) ------------------------------------------------------
    @staticmethod
    def _check_request(query, event):
        if not query:
            raise ValueError("At least one query variable has to be specified")
        for q in query:
            if q in event:
                raise ValueError("A query variable cannot be part of the event")

    @staticmethod
    def _finish(answer, query):
        """rename + level sort + row sort, exactly the tail of `query` (bayes_net.py:869-875)."""
        answer = answer.rename(f"P({', '.join(query)})")
        if isinstance(answer.index, pd.MultiIndex):
            answer = answer.reorder_levels(sorted(answer.index.names))
        return answer.sort_index()

    def query(self, *query, event: dict, algorithm="exact", n_iterations=100, n_chains=1, likelihood: dict = None) -> pd.Series:
        """Answer a probabilistic query; same contract as the reference (bayes_net.py:796-875).

        `likelihood` (an extension, algorithm "exact" only): likelihood findings - Pearl's virtual evidence, soft evidence - as
        {variable: mapping or Series label -> weight}.  The joint is multiplied by the weight of every finding variable's state
        before it is summed and normalised; a label that is not named weighs 0, so {"X": {"a": 1, "b": 1}} says "X is a or b".
        A finding variable may be queried; it may not be part of `event`.  The reference computes the same on a network with an
        extra binary child V of X, P(V = 1 | X = x) = weight(x) / max weight, observed at 1.

        `algorithm`: "exact" (variable elimination on the GPU), "gibbs" (GPU chains; `n_chains` is an
        extension, default 1 like the reference), "rejection" or "likelihood" (GPU forward sampling, one sample
        per lane), "lbp" (an extension: loopy belief propagation, `marginals(event)[name]` - one query variable only,
        approximate on networks with loops, takes `likelihood` too); anything else raises the reference's ValueError.
        """
        self._check_request(query, event)
        if algorithm == "lbp":
            # loopy belief propagation (an extension, see `marginals`): single-variable posteriors only
            if len(query) != 1:
                raise ValueError("algorithm='lbp' answers one query variable per call: belief propagation yields no joint "
                                 "over several variables (see marginals())")
            return self.marginals(event, algorithm="lbp", n_iterations=n_iterations, likelihood=likelihood)[query[0]]
        if likelihood is not None:
            if algorithm != "exact":
                raise ValueError("likelihood findings need algorithm='exact'")
            return self.backend.exact_query(query, event, likelihood)
        if algorithm == "exact":
            # (the hook the reference's query() dispatches to, bayes_net.py:848, is honoured: not re-bound on this object - e.g. by
            # accelerate() - and not overridden by a subclass)
            if "_variable_elimination" not in self.__dict__ and type(self)._variable_elimination is BayesNet._variable_elimination:
                return self.backend.exact_query(query, event)  # the finished Series, built directly (Backend._tail)
            answer = self._variable_elimination(*query, event=event)
        elif algorithm == "gibbs":
            answer = self._gibbs_sampling(*query, event=event, n_iterations=n_iterations,
                                          n_chains=n_chains)
        elif algorithm == "rejection":
            answer = self._rejection_sampling(*query, event=event, n_iterations=n_iterations)
        elif algorithm == "likelihood":
            answer = self._llh_weighting(*query, event=event, n_iterations=n_iterations)
        else:
            raise ValueError("Unknown algorithm, must be one of: exact, gibbs, likelihood, "
                             + "rejection")
        return self._finish(answer, query)

    def query_many(self, requests, sub_batch=32768):
        """Batched extension: `requests` = iterable of (query tuple, event dict) -> `PosteriorBatch`, a sequence whose item i is
        the Series `query(*q_i, event=e_i)` returns (identical: name, index, level order, row order, values).  A request may be a
        3-tuple (query tuple, event dict, likelihood dict or None), item i then `query(*q_i, event=e_i, likelihood=l_i)`; a batch
        with such a request goes through blocking calls.  Names and labels are
        encoded in bulk, the device works through sub-batches with two calls in flight, and the Series are built on access;
        `.to_frame()` gives every answer as one pandas object."""
        return self.backend.exact_many(requests if isinstance(requests, list) else list(requests), sub_batch=sub_batch)

    def query_frame(self, *query, events: pd.DataFrame) -> pd.DataFrame:
        """The fixed-query batch in pandas' own shape (an extension; the reference answers one event per call, bayes_net.py:796):
        row r of `events` is an event - its columns are evidence variables, NaN / None = not observed in that row - and row r of
        the result is the posterior of `query` given that event: columns = the joint states of the query variables in the order of
        `query()`'s index (sorted names, sorted labels; a MultiIndex for several variables), zeros where `query()` drops the row, so
        that `out.iloc[r][out.iloc[r] > 0]` has the values of `query(*query, event=<row r>)`.  Labels are encoded per column
        (`Index.get_indexer`), rows are grouped by their set of observed columns, every group is one fixed-shape engine call."""
        if not query:
            raise ValueError("At least one query variable has to be specified")
        if any(c in query for c in events.columns):
            raise ValueError("A query variable cannot be part of the event")
        be = self.backend
        f = be.flat
        q = [be.var_id(n) for n in query]
        if f.missing:
            be.encode(query, {c: None for c in events.columns})  # (raises the reference's KeyError for a node without a CPT)
        ev_ids, codes, observed = encode_frame(be, list(events.columns), events)
        n = len(events)
        name, order, levels, shape, names = be._tail(tuple(query))
        cells = int(np.prod([int(f.card[v]) for v in q]))
        out = np.zeros((n, cells), np.float64)
        # one engine call per pattern of observed columns
        qarr = np.array(q, np.int32)
        for rows, on in iter_parts(pattern_groups(observed), observed, None):
            out[rows] = be.engine.query_fixed(np.broadcast_to(qarr, (len(rows), len(q))), *part_args(ev_ids, codes, rows, on))
        if shape is None:
            columns = levels
        else:
            if order is not None:
                out = np.ascontiguousarray(out.reshape([n] + shape).transpose([0] + [k + 1 for k in order])).reshape(n, cells)
                shape = [shape[k] for k in order]
            columns = pd.MultiIndex(levels=levels, codes=list(np.unravel_index(np.arange(cells), shape)), names=names, verify_integrity=False)
        return pd.DataFrame(out, index=events.index, columns=columns)

    def impute(self, sample: dict, **query_params) -> pd.Series:
        """Replace the `None` entries of `sample` by the most probable joint assignment
        (bayes_net.py:877-908).  With a single missing variable the reference zips the *scalar*
        `idxmax()` (TypeError for bool labels, character-zip for strings - SURVEY.md section 3.2);
        here that case simply works.  (It builds the dense posterior over the missing variables; `map_query` / `map_frame`
        answer the same question - also for a sample that names only some of the variables - without that table.)"""
        missing = [k for k, v in sample.items() if v is None]
        event = {k: v for k, v in sample.items() if v is not None}
        posterior = self.query(*missing, event=event, **query_params)
        best = posterior.idxmax()
        if len(missing) == 1:
            best = (best,)
        for k, v in zip(posterior.index.names, best):
            event[k] = v
        return pd.Series(event)

    # ---- most probable explanation (an extension: max-product elimination on the device, mibn_mpe_batch) ----------------------
    def _event_backend(self, names, every_cpt=False):
        """The backend, for a request whose evidence variables are `names` and in which every variable takes part (MPE, posterior
        samples, P(e)): an unknown name raises the reference's KeyError before any engine exists, a node without a CPT the
        KeyError of `query` - with `every_cpt` also before any engine exists, and before the names are looked at."""
        if every_cpt:
            for node in self.nodes:
                if node not in self.P:
                    raise KeyError(node)
        known = set(self._all_names())
        for n in names:
            if n not in known:
                raise KeyError(n)
        be = self.backend
        if be.flat.missing:
            raise KeyError(be.flat.names[min(be.flat.missing)])
        return be

    @staticmethod
    def _mpe_arguments(algorithm, n_iterations, tol, damping, polish):
        """The argument checks of `mpe` / `mpe_frame`, before any engine exists."""
        if algorithm not in ("exact", "lbp"):
            raise ValueError("Unknown algorithm, must be one of: exact, lbp")
        if algorithm == "exact":
            return
        if int(n_iterations) != n_iterations or n_iterations < 1:
            raise ValueError("n_iterations must be an integer >= 1")
        if not tol >= 0:
            raise ValueError("tol must be a number >= 0")
        if not 0 <= damping < 1:
            raise ValueError("damping must be in [0, 1)")
        if int(polish) != polish or polish < 0:
            raise ValueError("polish must be an integer >= 0")

    def mpe(self, event: dict = None, return_log_prob=False, likelihood: dict = None, algorithm="exact", n_iterations=100, tol=1e-9,
            damping=0.5, polish=10, return_info=False):
        """Most probable explanation: the single most probable completion of `event`, argmax_x P(x, event) over every variable
        not in `event`.  Returns a Series of labels indexed by every variable (sorted names); evidence variables keep their
        labels.  Zero-probability or out-of-domain evidence gives None for the other variables (and a log probability of
        -inf).  With `return_log_prob`, returns (series, natural log of P(x*, event)).  Ties go to the lowest label code.
        `likelihood`: likelihood findings as in `query` - the maximum is over P(x, event) times the weights, and so is the log.

        `algorithm="exact"` (default): max-product elimination on the device.
        `algorithm="lbp"`: an APPROXIMATION for networks on which the exact call raises (a 20 x 20 grid) - at most `n_iterations`
        flooding sweeps of max-product belief propagation (stopped when no message moves by more than `tol`), the best decoded
        assignment seen over the sweeps kept, then at most `polish` sweeps of greedy single-variable moves.  Exact on polytrees;
        on a network with loops there is no bound on the gap to the true maximum.  What holds: the log probability returned is that
        of the assignment returned, and when `sweeps < polish` no change of a single variable improves it.  The default `damping`
        is 0.5, not `marginals`' 0.0: max-product messages oscillate where sum-product ones settle, and undamped decodes are poor.
        `return_info=True` appends {"iterations", "residual", "converged", "best_iteration", "sweeps", "moves"} to the result
        (exact: zeros, converged).  Where the assignment found has probability 0 - impossible evidence, or a decode that hit a
        zero of a sparse CPT and was never bettered - the log probability is -inf and the other variables are None."""
        self._mpe_arguments(algorithm, n_iterations, tol, damping, polish)
        event = dict(event or {})
        be = self._event_backend(list(event) + list(likelihood or {}), every_cpt=algorithm == "lbp")
        f = be.flat
        ev = [f.id[name] for name in event]
        codes = [f.code_of(v, lab) for v, lab in zip(ev, event.values())]
        more = {"likelihoods": be.likelihood_block([be.encode_likelihood(likelihood, event)])} if likelihood else {}
        evars, ecodes = np.array([ev], np.int32).reshape(1, len(ev)), np.array([codes], np.int32).reshape(1, len(ev))
        info = {"iterations": 0, "residual": 0.0, "converged": True, "best_iteration": 0, "sweeps": 0, "moves": 0}
        if algorithm == "exact":
            out, log_p = be.engine.mpe(evars, ecodes, **more)
        else:
            out, log_p, it, res, extra = be.engine.bp_mpe(evars, ecodes, int(n_iterations), tol, damping, int(polish), **more)
            out[np.isneginf(log_p)] = -1  # (an assignment of probability 0 is no explanation: None, as for impossible evidence)
            info = {"iterations": int(it[0]), "residual": float(res[0]), "converged": bool(res[0] <= tol),
                    "best_iteration": int(extra[0, 0]), "sweeps": int(extra[0, 1]), "moves": int(extra[0, 2])}
        names = self._all_names()
        data = decode_labels(f, names, out, event)
        series = pd.Series([data[name][0] for name in names], index=pd.Index(names), dtype=object)
        result = (series, float(log_p[0])) if return_log_prob else (series,)
        if return_info:
            result = result + (info,)
        return result if len(result) > 1 else result[0]

    def mpe_frame(self, events: pd.DataFrame, return_log_prob=False, sub_batch=32768, algorithm="exact", n_iterations=100, tol=1e-9,
                  damping=0.5, polish=10, return_info=False):
        """`mpe` for every row of `events`, in the convention of `query_frame`: the columns are evidence variables, NaN / None =
        not observed in that row.  Rows are grouped by their pattern of observed columns, one engine call per group (in
        sub-batches of `sub_batch` rows).  Returns a DataFrame with the index of `events` and one column per variable (sorted
        names); with `return_log_prob`, (frame, log probabilities as a numpy array).

        A row that names every variable - observed values and missing ones (NaN / None) - gets what `impute` returns for it (up
        to ties between equally probable assignments), without `impute`'s posterior table of prod(card(missing)) cells.

        `algorithm`, `n_iterations`, `tol`, `damping`, `polish`: as in `mpe`.  `return_info=True` adds the columns
        ("info", "iterations"), ("info", "residual"), ("info", "converged"), ("info", "best_iteration"), ("info", "sweeps") and
        ("info", "moves"), as `marginals_frame` does; the variables' columns keep their plain names."""
        self._mpe_arguments(algorithm, n_iterations, tol, damping, polish)
        cols = list(events.columns)
        be = self._event_backend(cols, every_cpt=algorithm == "lbp")
        f = be.flat
        ev_ids, codes, observed = encode_frame(be, cols, events)
        n = len(events)
        out = np.zeros((n, len(f.names)), np.int32)
        log_p = np.zeros(n, np.float64)
        its = np.zeros(n, np.int32)
        res = np.zeros(n, np.float64)
        extra = np.zeros((n, 3), np.int32)
        for part, on in iter_parts(pattern_groups(observed), observed, sub_batch):
            if algorithm == "exact":
                out[part], log_p[part] = be.engine.mpe(*part_args(ev_ids, codes, part, on))
            else:
                out[part], log_p[part], its[part], res[part], extra[part] = be.engine.bp_mpe(
                    *part_args(ev_ids, codes, part, on), int(n_iterations), tol, damping, int(polish))
        out[np.isneginf(log_p)] = -1
        names = self._all_names()
        frame = pd.DataFrame(decode_labels(f, names, out, events), index=events.index, columns=names)
        if return_info:
            frame[("info", "iterations")] = its
            frame[("info", "residual")] = res
            frame[("info", "converged")] = res <= tol
            frame[("info", "best_iteration")] = extra[:, 0]
            frame[("info", "sweeps")] = extra[:, 1]
            frame[("info", "moves")] = extra[:, 2]
        return (frame, log_p) if return_log_prob else frame

    # ---- all single-variable posteriors (an extension: loopy belief propagation on the device, mibn_bp_batch) -----------------
    @staticmethod
    def _marginals_algorithm(algorithm):
        if algorithm not in ("lbp", "exact"):
            raise ValueError("Unknown algorithm, must be one of: lbp, exact")

    def marginals(self, event: dict = None, algorithm="lbp", n_iterations=100, tol=1e-9, damping=0.0, likelihood: dict = None,
                  return_info=False):
        """Every single-variable posterior P(X | event) at once: {name: Series} over the variables not in `event`, each Series what
        `query(name, event=event)` returns - name, index, labels, zero rows absent.

        `algorithm="lbp"` (default): loopy belief propagation on the device, one call for all variables - at most `n_iterations`
        flooding sweeps, stopped early when no message moves by more than `tol`; `damping` in [0, 1) mixes each new message with
        its predecessor.  Exact on polytrees.  On a network with loops it is an approximation WITHOUT an error bound and it need
        not converge: pass `return_info=True` and read `converged`.  Its cost is linear in the network, so it answers networks on
        which every exact call raises (a 20 x 20 grid).  Every CPT takes part, as in `mpe`.
        `algorithm="exact"`: one exact `query` per variable through `query_many` - the same spelling, for comparison.
        `likelihood`: likelihood findings as in `query`.
        `return_info=True`: (marginals, {"iterations", "residual", "converged"})."""
        self._marginals_algorithm(algorithm)
        event = dict(event or {})
        if algorithm == "exact":
            names = [n for n in self._all_names() if n not in event]
            answers = self.query_many([((n,), event, likelihood) if likelihood else ((n,), event) for n in names])
            out = {n: answers[i] for i, n in enumerate(names)}
            return (out, {"iterations": 0, "residual": 0.0, "converged": True}) if return_info else out
        be = self._event_backend(list(event) + list(likelihood or {}), every_cpt=True)
        f = be.flat
        names = [n for n in self._all_names() if n not in event]
        bel, it, res = be.lbp(event, likelihood, n_iterations, tol, damping)
        off = np.concatenate([[0], np.cumsum(f.card, dtype=np.int64)])
        out = {n: be.finished_series((n,), bel[off[f.id[n]]:off[f.id[n] + 1]].copy()) for n in names}
        info = {"iterations": it, "residual": res, "converged": bool(res <= tol)}
        return (out, info) if return_info else out

    def marginals_frame(self, events: pd.DataFrame, algorithm="lbp", n_iterations=100, tol=1e-9, damping=0.0, return_info=False,
                        sub_batch=32768):
        """`marginals` for every row of `events`, in the convention of `mpe_frame`: the columns are evidence variables, NaN / None =
        not observed in that row.  Returns a DataFrame with the index of `events` and one column per (variable, state) - sorted
        names, labels in `query()`'s order -, row r holding every posterior given the event of row r (zeros where `query()` drops
        the row; a variable the row observes holds its one-hot).  `return_info=True` adds the columns ("info", "iterations"),
        ("info", "residual") and ("info", "converged")."""
        self._marginals_algorithm(algorithm)
        cols = list(events.columns)
        be = self._event_backend(cols, every_cpt=True)
        f = be.flat
        ev_ids, codes, observed = encode_frame(be, cols, events)
        n = len(events)
        off = np.concatenate([[0], np.cumsum(f.card, dtype=np.int64)])
        dense = np.zeros((n, int(off[-1])), np.float64)
        its = np.zeros(n, np.int32)
        res = np.zeros(n, np.float64)
        for part, on in iter_parts(pattern_groups(observed), observed, sub_batch):
            evars, ecodes = part_args(ev_ids, codes, part, on)
            if algorithm == "lbp":
                dense[part], its[part], res[part] = be.engine.bp(evars, ecodes, n_iterations, tol, damping)
                continue
            seen = set(int(v) for v in ev_ids[on])
            for v in range(len(f.card)):
                if v in seen:
                    continue
                dense[part, off[v]:off[v + 1]] = be.engine.query_fixed(np.full((len(part), 1), v, np.int32), evars, ecodes)
            for j in on:  # the observed variables: their one-hot
                c = codes[part, j]
                ok = (c >= 0) & (c < f.card[ev_ids[j]])
                dense[part[ok], off[ev_ids[j]] + c[ok]] = 1.0
        names = self._all_names()
        order = np.concatenate([np.arange(off[f.id[name]], off[f.id[name] + 1]) for name in names]) if names else np.zeros(0, np.int64)
        columns = pd.MultiIndex.from_tuples([(name, lab) for name in names for lab in f.domains[f.id[name]]], names=["variable", "state"])
        frame = pd.DataFrame(dense[:, order], index=events.index, columns=columns)
        if return_info:
            frame[("info", "iterations")] = its
            frame[("info", "residual")] = res
            frame[("info", "converged")] = res <= tol
        return frame

    # ---- marginal MAP (an extension: sum-then-max elimination on the device, mibn_map_batch) ---------------------------------
    def _map_backend(self, variables, evidence_names):
        """The argument checks of `map_query` / `map_frame`, all before any engine exists, with the exception types of `query`."""
        if len(set(variables)) != len(variables):
            raise ValueError("A MAP variable is named twice")
        for q in variables:
            if q in evidence_names:
                raise ValueError("A query variable cannot be part of the event")
        return self._event_backend(list(variables) + list(evidence_names), every_cpt=True)

    def _map_log_z(self, be):
        """(flags, log Z) of the marginal MAP calls: CPTs that are all distributions prune (Z = 1); otherwise every CPT takes part and
        log max_m P(m, e) is taken under the normalised joint, as `evidence_proba` does - Z is the mass of the empty request."""
        if self._cpts_are_distributions(be):
            return _capi.MAP_PRUNE, 0.0
        none = np.zeros((1, 0), np.int32)
        return 0, float(be.engine.map(none, none, none, flags=0)[1][0])

    def map_query(self, *variables, event: dict = None, return_log_prob=False, likelihood: dict = None):
        """Marginal MAP: the most probable joint assignment of `variables` given `event`, every other variable summed out -
        argmax_m sum_h P(m, h, event).  Unlike `mpe` it does not maximise over the variables the caller did not name, and unlike
        `query(*variables).idxmax()` it never builds the dense table over `variables`.  Returns a Series of labels indexed by
        `variables` in the order given; with `return_log_prob`, (series, natural log of max_m P(m, event) under the normalised
        joint).  Zero-probability or out-of-domain evidence gives None labels and -inf.  Ties go to the lowest label code.  The
        MAP variables that interact through the summed ones share a table on the device: a request whose table would reach 2^31
        cells raises (inherent to marginal MAP).  `likelihood`: likelihood findings as in `query`, multiplied into the joint before it
        is summed and maximised; a MAP variable may carry one."""
        event = dict(event or {})
        be = self._map_backend(variables, event)
        if likelihood:
            self._event_backend(likelihood)  # (an unknown name: the reference's KeyError)
        f = be.flat
        mv = [f.id[name] for name in variables]
        ev = [f.id[name] for name in event]
        ecodes = [f.code_of(v, lab) for v, lab in zip(ev, event.values())]
        flags, log_z = self._map_log_z(be)
        more = {"likelihoods": be.likelihood_block([be.encode_likelihood(likelihood, event)])} if likelihood else {}
        codes, log_p = be.engine.map(np.array(mv, np.int32).reshape(1, len(mv)), np.array(ev, np.int32).reshape(1, len(ev)),
                                     np.array(ecodes, np.int32).reshape(1, len(ev)), flags=flags, **more)
        labels = [label_table(f, v)[codes[0, k]] for k, v in enumerate(mv)]
        series = pd.Series(labels, index=pd.Index(list(variables)), dtype=object)
        lp = float(log_p[0]) - log_z if np.isfinite(log_p[0]) else -np.inf
        return (series, lp) if return_log_prob else series

    def map_frame(self, *variables, events: pd.DataFrame, return_log_prob=False, sub_batch=32768):
        """`map_query(*variables)` for every row of `events`, in the convention of `mpe_frame`: the columns are evidence variables,
        NaN / None = not observed in that row.  Rows are grouped by their pattern of observed columns, one engine call per group
        (in sub-batches of `sub_batch` rows).  Returns a DataFrame with the index of `events` and one column per MAP variable, in
        the order given (None where the row's evidence has probability zero); with `return_log_prob`, (frame, log probabilities
        as a numpy array).  A MAP variable that a row observes raises ValueError."""
        observed_cols = [c for c in events.columns if c not in variables or events[c].notna().any()]
        be = self._map_backend(variables, observed_cols)
        f = be.flat
        cols = list(observed_cols)
        ev_ids, codes, observed = encode_frame(be, cols, events)
        mv = np.array([f.id[name] for name in variables], np.int32)
        n = len(events)
        out = np.full((n, len(mv)), -1, np.int32)
        log_p = np.full(n, -np.inf, np.float64)
        if n:
            flags, log_z = self._map_log_z(be)
            for part, on in iter_parts(pattern_groups(observed), observed, sub_batch):
                out[part], log_p[part] = be.engine.map(np.broadcast_to(mv, (len(part), len(mv))), *part_args(ev_ids, codes, part, on), flags=flags)
            log_p = np.where(np.isfinite(log_p), log_p - log_z, -np.inf)
        data = {name: label_table(f, int(v))[out[:, k]] for k, (name, v) in enumerate(zip(variables, mv))}
        frame = pd.DataFrame(data, index=events.index, columns=list(variables), dtype=object)
        return (frame, log_p) if return_log_prob else frame

    # ---- evidence likelihood P(e) (an extension: sum-product elimination without normalisation, MIBN_Q_UNNORMALISED) --------
    @staticmethod
    def _cpts_are_distributions(be):
        """True when every CPT row (parent configuration) is present and sums to 1 within 1e-12: the product of the CPTs is then
        normalised (Z = 1) and a barren node sums out to 1, so P(e) may prune to the ancestors of the evidence.  Cached per
        backend (a backend is rebuilt when the CPTs change)."""
        ok = getattr(be, "_cpts_normalised", None)
        if ok is None:
            f = be.flat
            ok = True
            for v in range(len(f.card)):
                a, b = int(f.value_off[v]), int(f.value_off[v + 1])
                rows = np.asarray(f.values[a:b], np.float64).reshape(-1, int(f.card[v]))
                if not (np.all(f.present[a:b] == 1.0) and np.all(np.abs(rows.sum(axis=1) - 1.0) <= 1e-12)):
                    ok = False
                    break
            be._cpts_normalised = ok
        return ok

    def _evidence_rows(self, be, ev_ids, codes, observed, sub_batch=32768):
        """P(row) of every row of `codes` [n, len(ev_ids)] under the normalised joint, where observed[r, j] says whether row r
        observes column j.  Rows are grouped by their pattern of observed columns, one engine call (no query variable,
        Q_UNNORMALISED) per group and sub-batch.  A code of -1 gives 0.  With CPTs that are not all distributions every CPT takes
        part (Q_NOPRUNE) and the result is divided by Z, the mass of the empty event: one more request per call."""
        n = len(codes)
        out = np.zeros(n, np.float64)
        if n == 0:
            return out
        eng = be.engine
        flags = _capi.Q_UNNORMALISED
        z = 1.0
        if not self._cpts_are_distributions(be):
            flags |= _capi.Q_NOPRUNE
            none = np.zeros((1, 0), np.int32)
            z = float(eng.query_fixed(none, none, none, flags=flags)[0, 0])
        for part, on in iter_parts(pattern_groups(observed), observed, sub_batch):
            out[part] = eng.query_fixed(np.zeros((len(part), 0), np.int32), *part_args(ev_ids, codes, part, on), flags=flags)[:, 0]
        if flags & _capi.Q_NOPRUNE:
            out = out / z if z > 0 else np.zeros(n, np.float64)
        return out

    def _bethe_rows(self, be, ev_ids, codes, observed, sub_batch, n_iterations, tol, damping):
        """(log_z, iterations, residual) of every row of `codes`: the Bethe approximation of log P(row) from loopy belief propagation,
        one request per row in row order, in engine calls of `sub_batch` rows.  Every CPT takes part; with CPTs that are not all
        distributions the log_z of the empty event is subtracted: one more request, as `_evidence_rows` does with Z."""
        n = len(codes)
        log_z, its, res = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.float64)
        step = max(1, int(sub_batch))
        for s in range(0, n, step):
            rows = slice(s, s + step)
            log_z[rows], _, _, its[rows], res[rows] = be.engine.bp_evidence_batch(*csr_rows(ev_ids, codes[rows], observed[rows]),
                                                                                  int(n_iterations), tol, damping)
        if n and not self._cpts_are_distributions(be):
            z = float(be.engine.bp_evidence_batch(np.zeros(2, np.int64), [], [], int(n_iterations), tol, damping)[0][0])
            log_z = log_z - z if np.isfinite(z) else np.full(n, -np.inf)
        return log_z, its, res

    def evidence_proba(self, X, log=False, sub_batch=32768, algorithm="exact", n_iterations=100, tol=1e-9, damping=0.0, return_info=False):
        """Probability of an observed event, P(e) = the normalised joint summed over every unobserved variable: the reference's
        `predict_proba` "also for a partial event" (bayes_net.py:934-962), without its dense table of the observed columns.

        A dict gives a float.  A DataFrame gives a float64 Series with X's index: each row is an event, NaN / None = not observed
        in that row (the convention of `query_frame` and `mpe_frame`).  Rows are grouped by their pattern of observed columns, one
        engine call per group (in sub-batches of `sub_batch` rows).  A label outside its domain, or an event of probability zero,
        gives 0 (log: -inf).  Unknown column names raise KeyError before any engine work.  With `log`, natural logarithms; a
        P(e) below the smallest double reads as 0 and its log as -inf.

        `algorithm="lbp"`: an APPROXIMATION for networks on which the exact call raises (a 20 x 20 grid) - the Bethe approximation
        of log P(e) from at most `n_iterations` flooding sweeps of loopy belief propagation (`tol`, `damping` as in `marginals`), one
        request per row, every CPT taking part.  Exact on polytrees; on a network with loops it has NO error bound, and its error has
        either sign: it is not a lower bound of log P(e).  With `log` it returns the logarithm itself, never the logarithm of an
        underflowed number: a fully observed row of a 1 000-variable chain has a finite log.  Without `log`, its exponential.
        `return_info=True`: (result, info) - for a dict {"iterations", "residual", "converged"}, for a DataFrame a frame of these
        three columns with X's index (exact: zeros, converged)."""
        self._mpe_arguments(algorithm, n_iterations, tol, damping, 0)
        lbp = algorithm == "lbp"
        if isinstance(X, dict):
            cols = list(X)
            be = self._event_backend(cols, every_cpt=lbp)
            f = be.flat
            ev_ids = np.array([f.id[c] for c in cols], np.int32)
            observed = np.array([X[c] is not None for c in cols], bool).reshape(1, len(cols))
            codes = np.array([f.code_of(int(v), X[c]) if X[c] is not None else -1 for c, v in zip(cols, ev_ids)],
                             np.int32).reshape(1, len(cols))
            info = {"iterations": 0, "residual": 0.0, "converged": True}
            if lbp:
                log_z, its, res = self._bethe_rows(be, ev_ids, codes, observed, sub_batch, n_iterations, tol, damping)
                info = {"iterations": int(its[0]), "residual": float(res[0]), "converged": bool(res[0] <= tol)}
                p = float(log_z[0]) if log else float(np.exp(log_z[0]))
            else:
                p = float(self._evidence_rows(be, ev_ids, codes, observed, sub_batch)[0])
                if log:
                    p = float(np.log(p)) if p > 0 else -np.inf
            return (p, info) if return_info else p
        cols = list(X.columns)
        be = self._event_backend(cols, every_cpt=lbp)
        ev_ids, codes, observed = encode_frame(be, cols, X)
        its, res = np.zeros(len(X), np.int32), np.zeros(len(X), np.float64)
        if lbp:
            p, its, res = self._bethe_rows(be, ev_ids, codes, observed, sub_batch, n_iterations, tol, damping)
            if not log:
                p = np.exp(p)
        else:
            p = self._evidence_rows(be, ev_ids, codes, observed, sub_batch)
            if log:
                with np.errstate(divide="ignore"):
                    p = np.log(p)
        out = pd.Series(p, index=X.index, dtype=np.float64)
        if return_info:
            return out, pd.DataFrame({"iterations": its, "residual": res, "converged": res <= tol}, index=X.index)
        return out

    def log_likelihood(self, X, sub_batch=32768, algorithm="exact", n_iterations=100, tol=1e-9, damping=0.0) -> float:
        """Log-likelihood of a data set: the sum over its rows of log P(row) (`evidence_proba`; NaN / None = not observed in
        that row).  A row of probability zero makes it -inf.  `algorithm="lbp"`: the sum of the rows' Bethe approximations, as in
        `evidence_proba` - finite where the rows' probabilities underflow, without an error bound on a network with loops."""
        more = dict(algorithm=algorithm, n_iterations=n_iterations, tol=tol, damping=damping)
        if isinstance(X, dict):
            return self.evidence_proba(X, log=True, sub_batch=sub_batch, **more)
        return float(self.evidence_proba(X, log=True, sub_batch=sub_batch, **more).sum())

    # ---- the joint of every family (an extension: the factor beliefs of loopy belief propagation, mibn_bp_evidence_batch) ----
    def family_marginals(self, event: dict = None, likelihood: dict = None, algorithm="lbp", n_iterations=100, tol=1e-9, damping=0.0,
                         return_info=False):
        """The posterior joint of every family - a node with its parents - given `event`: {node: Series over [*parents, node]} in
        the index layout of `bn.P[node]` (every cell present, zeros included; a member the event observes holds its one-hot).

        `algorithm="lbp"` (default): the factor beliefs of loopy belief propagation, one device call for all families - exact on
        polytrees, on a network with loops an approximation WITHOUT an error bound (`n_iterations`, `tol`, `damping`,
        `return_info` as in `marginals`).  It answers where `query(*family)` raises (a 20 x 20 grid).
        `algorithm="exact"`: one `query(*family)` per node, for comparison; it raises what `query` raises where that is refused -
        a family member in the event among them.  `likelihood`: likelihood findings as in `query`."""
        self._marginals_algorithm(algorithm)
        if algorithm == "lbp":
            self._mpe_arguments(algorithm, n_iterations, tol, damping, 0)
        event = dict(event or {})
        be = self._event_backend(list(event) + list(likelihood or {}), every_cpt=True)
        f = be.flat
        info = {"iterations": 0, "residual": 0.0, "converged": True}
        if algorithm == "lbp":
            findings = be.encode_likelihood(likelihood, event)
            _, ev, codes = be.encode((), event, findings)
            more = {"likelihoods": be.likelihood_block([findings])} if findings else {}
            _, _, fbel, it, res = be.engine.bp_evidence(np.array(ev, np.int32).reshape(1, len(ev)), np.array(codes, np.int32).reshape(1, len(ev)),
                                                        int(n_iterations), tol, damping, fbeliefs=True, **more)
            info = {"iterations": int(it[0]), "residual": float(res[0]), "converged": bool(res[0] <= tol)}
        out = {}
        off = be.engine.family_off
        for v, node in enumerate(f.names):
            members = [f.names[u] for u in f.scope[v]]
            if len(members) > 1:
                index = pd.MultiIndex.from_product([f.domains[u] for u in f.scope[v]], names=members)
            else:
                index = pd.Index(f.domains[v], name=node)
            if algorithm == "lbp":
                values = fbel[0, off[v]:off[v + 1]].copy()
            else:
                ans = self.query(*members, event=event, **({"likelihood": likelihood} if likelihood else {}))
                ans = ans.reorder_levels(members) if len(members) > 1 else ans
                values = ans.reindex(index, fill_value=0.0).to_numpy()
            out[node] = pd.Series(values, index=index, name=self.P[node].name if node in self.P else None)
        return (out, info) if return_info else out

    # ---- the joint and likelihoods (bayes_net.py:398-465, 934-973) -----------------
    # cells of the observed columns' dense table from which predict_proba answers row by row through P(e): the planner builds no
    # table of 2^31 cells or more, so the dense path cannot run there
    PREDICT_DENSE_CELL_CAP = 2 ** 31

    def _all_names(self):
        names = []
        for P in self.P.values():
            for n in (P.index.names if P.index.names[0] is not None else [P.name]):
                if n not in names:
                    names.append(n)
        return sorted(names)

    def full_joint_dist(self, event: dict = None, keep_zeros=False) -> pd.Series:
        """The normalised product of all CPTs (bayes_net.py:460-465; like the reference, `event` is accepted and
        ignored).  On the device it is the posterior of all variables given no evidence."""
        names = self._all_names()
        fjd = self.backend.joint_series(names, keep_zeros=keep_zeros)
        fjd.name = f"P({', '.join(names)})"
        return fjd

    def predict_proba(self, X):
        """Likelihood of one sample (dict -> float) or of the rows of a DataFrame (bayes_net.py:934-962).  The
        reference marginalises its full joint onto the observed columns; here the unobserved variables are
        eliminated on the device, which is the same table.  As in the reference, a single observed column returns
        that column's marginal (not indexed by the rows), and a row of probability zero raises KeyError.

        Where the observed columns' dense table would have `PREDICT_DENSE_CELL_CAP` cells or more - beyond what the planner can
        build (a table of 2^31 cells) - the rows are answered one by one through P(e) (`evidence_proba`) instead; the Series has
        the same shape (same index, same name, KeyError for a row of probability zero)."""
        if isinstance(X, dict):
            return self.predict_proba(pd.DataFrame([X])).iloc[0]
        names = self._all_names()
        observed = [n for n in names if n in set(X.columns)]
        if len(observed) > 1:
            fast = self._predict_proba_rows(X, observed, f"P({', '.join(names)})")
            if fast is not None:
                return fast
        fjd = self.backend.joint_series(observed)
        fjd.name = f"P({', '.join(names)})"
        if len(observed) > 1:
            return fjd[pd.MultiIndex.from_frame(X[observed])]
        return fjd

    def _predict_proba_rows(self, X, observed, name):
        """`fjd[pd.MultiIndex.from_frame(X[observed])]` without the pandas look-up: the rows' labels are encoded column by column
        (`Index.get_indexer` on the sorted label domains), the dense joint is gathered at the raveled codes, and the result carries
        the index pandas' look-up returns - `fjd.index.take(positions)`: the joint's own levels with the rows' codes.  A row that
        is not in the joint (a label outside a domain, probability zero) raises KeyError like the look-up does.  Returns None where
        the columns cannot be encoded in bulk (unhashable / mixed labels): the caller takes the pandas path."""
        be = self.backend
        f = be.flat
        try:
            ids = [f.id[n] for n in observed]
            codes = []
            for n, v in zip(observed, ids):
                c = f.dom_index[v].get_indexer(X[n])
                codes.append(c)
        except (KeyError, TypeError, ValueError, pd.errors.InvalidIndexError):
            return None
        shape = [int(f.card[v]) for v in ids]
        bad = np.zeros(len(X), bool)
        for c in codes:
            bad |= c < 0
        if float(np.prod([float(c) for c in shape])) >= self.PREDICT_DENSE_CELL_CAP:
            # (wide rows: P(row) per row, every column observed; a row the dense look-up would miss stays bad)
            self._event_backend(observed)
            ev_ids = np.array(ids, np.int32)
            cm = np.stack(codes, axis=1).astype(np.int32) if len(X) else np.zeros((0, len(ids)), np.int32)
            vals = self._evidence_rows(be, ev_ids, np.where(bad[:, None], -1, cm).astype(np.int32), np.ones(cm.shape, bool))
            bad |= ~(vals > 0)
            if bad.any():
                rows = X[observed][bad].head(5).itertuples(index=False, name=None)
                raise KeyError(f"{[tuple(r) for r in rows]} not in index")
            idx = pd.MultiIndex(levels=[f.dom_index[v] for v in ids], codes=codes, names=list(observed), verify_integrity=False)
            return pd.Series(vals, index=idx, name=name)
        dense = be.marginal(observed)
        flat = np.ravel_multi_index([np.where(bad, 0, c) for c in codes], shape) if len(X) else np.zeros(0, np.int64)
        vals = dense[flat]
        bad |= ~(vals > 0)
        if bad.any():
            rows = X[observed][bad].head(5).itertuples(index=False, name=None)
            raise KeyError(f"{[tuple(r) for r in rows]} not in index")
        idx = pd.MultiIndex(levels=[f.dom_index[v] for v in ids], codes=codes, names=list(observed), verify_integrity=False)
        return pd.Series(vals, index=idx, name=name)

    def predict_log_proba(self, X):
        """bayes_net.py:964-973."""
        return np.log(self.predict_proba(X))

    # ---- parameter learning (bayes_net.py:467-516) ----------------------------------
    def partial_fit(self, X: pd.DataFrame, weights=None):
        """`weights` (an extension): non-negative integer row multiplicities, or the name of the column of X that holds them -
        see `learning.row_weights`."""
        from . import learning
        return learning.partial_fit(self, X, weights=weights)

    def fit(self, X: pd.DataFrame, weights=None):
        from . import learning
        return learning.fit(self, X, weights=weights)

    def fit_em(self, X: pd.DataFrame, n_iter=20, tol=1e-6, prior_count=0.0, init="auto", sub_batch=32768, algorithm="exact",
               bp_iterations=100, bp_tol=1e-9, damping=0.0):
        """CPTs from rows with missing values by expectation-maximisation, expected counts on the device (an extension:
        the reference's `fit` drops incomplete rows) - see `learning.fit_em`.  `algorithm="lbp"`: the E-step from the family
        beliefs of loopy belief propagation, for networks beyond the reach of the exact one."""
        from . import learning
        return learning.fit_em(self, X, n_iter=n_iter, tol=tol, prior_count=prior_count, init=init, sub_batch=sub_batch, algorithm=algorithm,
                               bp_iterations=bp_iterations, bp_tol=bp_tol, damping=damping)

    def score(self, X: pd.DataFrame, score="bic", ess=1.0, weights=None) -> float:
        """The structure's score on the complete rows of X: the sum of its families' "loglik", "bic", "aic", "bdeu" or "k2"
        scores, counted and reduced on the device (an extension, see `learning.family_scores`).  With "loglik" it is the
        log-likelihood of X under the CPTs `fit(X)` would learn.  `weights`: integer row multiplicities (`learning.row_weights`)."""
        from . import learning
        return learning.net_score(self, X, score=score, ess=ess, weights=weights)


def accelerate(bn, device=None, backend_factory=None):
    """Attach the MI355X backend to an existing *reference* `sorobn.BayesNet` instance.

    Replaces the two bound methods `BayesNet.query` dispatches to - `_variable_elimination`
    (bayes_net.py:848) and `_gibbs_sampling` (851-853) - and leaves `query`'s own post-processing
    (869-875) and `impute` (877-908) untouched, so naming / sorting stay byte-identical; also replaces
    `full_joint_dist` (398-465), on which the reference's `predict_proba` / `predict_log_proba` build.

    `backend_factory(bn) -> Backend` is a test seam (the GPU-less build container injects the CPU plan simulator of
    tests/simengine.py); the default builds the HIP backend and raises without a gfx950 device.
    """
    state = {"backend": None}
    make = backend_factory or (lambda b: Backend(b, device=device))

    def backend():
        b = state["backend"]
        if b is None or b.stale(bn):
            b = state["backend"] = make(bn)
        return b

    def _variable_elimination(self, *query, event):
        return backend().variable_elimination(*query, event=event)

    def _gibbs_sampling(self, *query, event, n_iterations):
        return backend().gibbs_sampling(*query, event=event, n_iterations=n_iterations,
                                        seed=getattr(self, "seed", None) or 0)

    def full_joint_dist(self, event: dict = None, keep_zeros=False):  # bayes_net.py:398-465
        names = sorted({n for P in self.P.values() for n in P.index.names})
        fjd = backend().joint_series(names, keep_zeros=keep_zeros)
        fjd.name = f"P({', '.join(names)})"
        return fjd

    bn._variable_elimination = types.MethodType(_variable_elimination, bn)
    bn._gibbs_sampling = types.MethodType(_gibbs_sampling, bn)
    bn.full_joint_dist = types.MethodType(full_joint_dist, bn)  # predict_proba / predict_log_proba build on it (952)
    bn._mibn_backend = backend
    return bn
