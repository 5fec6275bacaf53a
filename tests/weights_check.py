"""Twin of the row-weight extension (csrc/count_weighted_kernel.hip.h, `learning.row_weights`, `structure.bootstrap`): numpy and
the other twins only, no engine.

  * weighted contingency tables by `np.add.at` on int64;
  * the bootstrap weight sets from `sample_check.philox_uniform`, by the rule include/mibn.h pins;
  * `WeightedTwinDataset` / `WeightedTwinEngine`: TEST DOUBLES for the counting engine with weight sets - a table under set s is
    the twin's table of the rows written out w_s[i] times (`structure_check.family_score`, `ci_check.ci_stat` by import);
  * `bootstrap_loop`: the plain loop - the brute-force `structure_check.hill_climb` once per replicate on the expanded rows."""
import numpy as np

import ci_check as cc
import sample_check
import structure_check as sc

MAX_WEIGHT_SUM = 2 ** 32 - 1


def weighted_table(codes, card, cols, w=None):
    """Dense int64 C-order table over `cols` (last fastest) with row i counted w[i] times (None: once)."""
    codes = np.asarray(codes)
    flat = np.zeros(len(codes), np.int64)
    cells = 1
    for c in cols:
        flat = flat * int(card[c]) + codes[:, c].astype(np.int64)
        cells *= int(card[c])
    out = np.zeros(cells, np.int64)
    np.add.at(out, flat, np.ones(len(codes), np.int64) if w is None else np.asarray(w).astype(np.int64))
    return out.reshape([int(card[c]) for c in cols])


def expand(codes, w):
    """The rows written out w[i] times each, in order."""
    return np.repeat(np.asarray(codes), np.asarray(w).astype(np.int64), axis=0)


def bootstrap_sets(n_rows, n_sets, seed):
    """uint32 [n_sets, n_rows]: for set s and draw j, u = philox_uniform(j, s, key of mibn_sample) and row
    min(floor(u * n_rows), n_rows - 1) gains one."""
    lo, hi = sample_check._seed_words(seed)
    k0, k1 = lo, hi ^ 0x85EBCA6B
    out = np.zeros((n_sets, n_rows), np.uint32)
    j = np.arange(n_rows, dtype=np.uint64)
    for s in range(n_sets):
        if n_rows:
            u = sample_check.philox_uniform(j, s, k0, k1)
            idx = np.minimum(np.floor(u * np.float64(n_rows)).astype(np.int64), n_rows - 1)
            np.add.at(out[s], idx, np.uint32(1))
    return out


class WeightedTwinDataset:
    """TEST DOUBLE for _capi.Dataset with weight sets (never on the product path).  `log`: one entry per device call,
    ("score" | "ci", [(scope, set), ...])."""

    def __init__(self, codes, card, log):
        self.codes, self.card, self.log = np.asarray(codes), [int(c) for c in card], log
        self.n_rows = len(self.codes)
        self.sets = np.zeros((0, self.n_rows), np.uint32)
        self._rows = {}

    def set_weights(self, w):
        w = np.zeros((0, self.n_rows), np.uint32) if w is None else np.atleast_2d(np.asarray(w))
        assert w.shape[1] == self.n_rows and all(int(s.sum(dtype=np.int64)) <= MAX_WEIGHT_SUM for s in w)
        self.sets, self._rows = w.astype(np.uint32), {}

    def bootstrap(self, n_sets, seed=0, return_weights=False):
        self.sets, self._rows = bootstrap_sets(self.n_rows, int(n_sets), seed), {}
        return self.sets.copy() if return_weights else None

    def rows(self, s):
        s = int(s)
        assert -1 <= s < len(self.sets)
        if s not in self._rows:
            self._rows[s] = self.codes if s < 0 else expand(self.codes, self.sets[s])
        return self._rows[s]

    def score_families(self, families, kind="bic", ess=1.0, wset=None):
        sets = [-1] * len(families) if wset is None else [int(s) for s in wset]
        self.log.append(("score", [(tuple(f), s) for f, s in zip(families, sets)]))
        return np.array([sc.family_score(self.rows(s), self.card, f[-1], list(f[:-1]), kind, ess)[0] for f, s in zip(families, sets)], np.float64)

    def ci_tests(self, tests, kind="g2", wset=None):
        sets = [-1] * len(tests) if wset is None else [int(s) for s in wset]
        self.log.append(("ci", [(tuple(t), s) for t, s in zip(tests, sets)]))
        got = [cc.ci_stat(self.rows(s), self.card, t[-2], t[-1], list(t[:-2]), kind) for t, s in zip(tests, sets)]
        return np.array([g[0] for g in got], np.float64), np.array([g[2] for g in got], np.int64)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


class WeightedTwinEngine:
    """TEST DOUBLE for the counting engine: `dataset` -> WeightedTwinDataset, `count_tables` by `weighted_table`; `calls` is the
    log of every data set it made."""

    def __init__(self):
        self.calls = []

    def dataset(self, codes, card):
        return WeightedTwinDataset(codes, card, self.calls)

    def count_tables(self, codes, card, tables, weights=None):
        return [weighted_table(codes, card, t, weights) for t in tables]


def bootstrap_loop(codes, card, n_boot, seed, kind="bic", ess=1.0, **search):
    """The plain loop: for every replicate the brute-force hill climb on the rows written out by its weight set ->
    [(edges as position pairs, trace [(op, u, v, gain)], total)]."""
    sets = bootstrap_sets(len(codes), n_boot, seed)
    out = []
    for w in sets:
        parents, trace, total, _ = sc.hill_climb(sc.scorer(expand(codes, w), card, kind, ess), len(card), **search)
        out.append((sc.edges_of(parents), trace, total))
    return out
