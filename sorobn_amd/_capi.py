"""ctypes binding of the C-ABI in include/mibn.h (libmibn.so, built in-tree by __graft_entry__.build()).

There is deliberately no fallback: if the library is missing or no gfx950 device is visible the
calls raise, they never route to a CPU implementation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIBN_LIB") or os.path.join(_HERE, "libmibn.so")  # MIBN_LIB: kernel-variant experiments

# every symbol include/mibn.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "mibn_device_count", "mibn_version", "mibn_create", "mibn_destroy", "mibn_last_error",
    "mibn_set_network", "mibn_set_order_hints", "mibn_query_batch", "mibn_last_stats",
    "mibn_plan_stats", "mibn_create_planner", "mibn_set_option", "mibn_gibbs",
    "mibn_last_kernel_stats", "mibn_submit_batch", "mibn_wait", "mibn_drain", "mibn_total_stats",
    "mibn_total_kernel_stats", "mibn_sample", "mibn_sampling_query", "mibn_count_tables",
    "mibn_query_batch_ex", "mibn_plan_order", "mibn_estimate_costs", "mibn_device_synchronize", "mibn_gibbs_shard",
    "mibn_comm_unique_id", "mibn_comm_init", "mibn_comm_destroy", "mibn_comm_allgather_f64",
    "mibn_comm_reduce_i64", "mibn_comm_allreduce_max_f64", "mibn_comm_barrier", "mibn_gibbs_conditional", "mibn_sample_probe",
    "mibn_comm_probe", "mibn_device_info", "mibn_comm_count", "mibn_mpe_batch", "mibn_expect_batch",
    "mibn_dataset_create", "mibn_dataset_destroy", "mibn_score_families", "mibn_posterior_sample_batch", "mibn_map_batch",
    "mibn_ci_tests", "mibn_set_likelihoods", "mibn_bp_batch", "mibn_bp_mpe_batch", "mibn_bp_evidence_batch",
    "mibn_dataset_set_weights", "mibn_dataset_bootstrap", "mibn_score_families_w", "mibn_ci_tests_w", "mibn_count_tables_w",
    "mibn_best_dag", "mibn_arc_posteriors",
]
MAX_WEIGHT_SUM = 2 ** 32 - 1  # W_s of a weight set (include/mibn.h)
BEST_DAG_MAX_VARS = 24  # MIBN_BEST_DAG_MAX_VARS
ARC_POSTERIOR_MAX_VARS = 24  # MIBN_ARC_POSTERIOR_MAX_VARS
NO_PARENTS = 0xFFFFFFFF  # parents_out of mibn_best_dag where no DAG exists

OK, E_ARG, E_NODEVICE, E_HIP, E_NOMEM, E_STATE, E_LIMIT, E_COMM = 0, -1, -2, -3, -4, -5, -6, -7
Q_NOPRUNE = 1
Q_UNNORMALISED = 2  # P(q, e) instead of P(q | e); zero query variables allowed: one cell, P(e) (see mibn.h)
DRAW_PRUNE = 1  # mibn_posterior_sample_batch: every CPT is a complete distribution, prune to the ancestors of the evidence
MAP_PRUNE = 1  # mibn_map_batch: every CPT is a complete distribution, prune to the ancestors of the MAP variables and the evidence
COMM_ID_BYTES = 128
SCORE_KINDS = {"loglik": 0, "bic": 1, "aic": 2, "bdeu": 3, "k2": 4}  # MIBN_SCORE_*
CI_KINDS = {"g2": 0, "x2": 1}  # MIBN_CI_*


class MibnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mibn error {code}: {msg}")
        self.code = code
        self.msg = msg


class Stats(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "alg_bytes", "alg_flops", "n_steps", "kernel_ms", "plan_ms", "h2d_ms", "d2h_ms",
        "total_ms", "n_launches", "arena_bytes", "max_step_cells", "n_workgroups")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_double), ("ms", C.c_double),
                ("alg_bytes", C.c_double), ("items", C.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        vp = C.c_void_p
        L.mibn_device_count.argtypes = [C.POINTER(C.c_int)]
        L.mibn_version.restype = C.c_char_p
        L.mibn_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.mibn_create_planner.argtypes = [C.POINTER(vp)]
        L.mibn_destroy.argtypes = [vp]
        L.mibn_destroy.restype = None
        L.mibn_last_error.argtypes = [vp]
        L.mibn_last_error.restype = C.c_char_p
        L.mibn_set_network.argtypes = [vp, C.c_int32, i32p, i64p, i32p, i64p, f64p]
        L.mibn_set_order_hints.argtypes = [vp, C.c_int32, i32p]
        L.mibn_query_batch.argtypes = [vp, C.c_int64, i64p, i32p, i64p, i32p, i32p, i64p, f64p]
        L.mibn_query_batch_ex.argtypes = [vp, C.c_uint32, C.c_int64, i64p, i32p, i64p, i32p, i32p, i64p, f64p]
        L.mibn_mpe_batch.argtypes = [vp, C.c_int64, i64p, i32p, i32p, i32p, f64p]
        L.mibn_map_batch.argtypes = [vp, C.c_uint32, C.c_int64, i64p, i32p, i64p, i32p, i32p, i32p, f64p]
        L.mibn_set_likelihoods.argtypes = [vp, C.c_int64, i64p, i32p, i64p, f64p]
        L.mibn_bp_batch.argtypes = [vp, C.c_int64, i64p, i32p, i32p, C.c_int32, C.c_double, C.c_double, f64p, i32p, f64p]
        L.mibn_bp_mpe_batch.argtypes = [vp, C.c_int64, i64p, i32p, i32p, C.c_int32, C.c_double, C.c_double, C.c_int32, i32p, f64p, i32p, f64p, i32p]
        L.mibn_bp_evidence_batch.argtypes = [vp, C.c_int64, i64p, i32p, i32p, C.c_int32, C.c_double, C.c_double, f64p, f64p, f64p, f64p, C.c_int64, f64p,
                                             i32p, f64p]
        L.mibn_posterior_sample_batch.argtypes = [vp, C.c_int64, i64p, i32p, i32p, i64p, C.c_uint64, C.c_uint32, i32p, f64p]
        L.mibn_expect_batch.argtypes = [vp, C.c_uint32, C.c_int64, i64p, i32p, i64p, i32p, i32p, i64p, i64p, f64p, C.c_int64, f64p, f64p]
        L.mibn_plan_order.argtypes = [vp, C.c_int32, i32p, C.c_int32, i32p, i32p, i32p]
        L.mibn_estimate_costs.argtypes = [vp, C.c_int64, i64p, i32p, i64p, i32p, f64p]
        L.mibn_device_synchronize.argtypes = [vp]
        L.mibn_gibbs_shard.argtypes = [vp, C.c_int32, i32p, C.c_int32, i32p, i32p, i32p, C.c_int64, C.c_int64,
                                       C.c_int64, C.c_uint64, i64p]
        L.mibn_gibbs_conditional.argtypes = [vp, C.c_int32, i32p, i32p, i32p, C.c_int32, C.c_int64, C.POINTER(C.c_uint8), f64p]
        L.mibn_comm_probe.argtypes = [vp]
        L.mibn_device_info.argtypes = [vp, C.c_char_p, C.c_int32]
        L.mibn_comm_unique_id.argtypes = [vp, C.c_char_p]
        L.mibn_comm_init.argtypes = [vp, C.c_int32, C.c_int32, C.c_char_p]
        L.mibn_comm_destroy.argtypes = [vp]
        L.mibn_comm_count.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.mibn_comm_allgather_f64.argtypes = [vp, f64p, C.c_int64, f64p]
        L.mibn_comm_reduce_i64.argtypes = [vp, i64p, C.c_int64, C.c_int32]
        L.mibn_comm_allreduce_max_f64.argtypes = [vp, f64p, C.c_int64]
        L.mibn_comm_barrier.argtypes = [vp]
        L.mibn_submit_batch.argtypes = [vp, C.c_int64, i64p, i32p, i64p, i32p, i32p, i64p, f64p, C.POINTER(C.c_int32)]
        L.mibn_wait.argtypes = [vp, C.c_int32]
        L.mibn_drain.argtypes = [vp]
        L.mibn_total_stats.argtypes = [vp, C.POINTER(Stats)]
        L.mibn_total_kernel_stats.argtypes = [vp, C.c_int32, C.POINTER(KernelStat), C.POINTER(C.c_int32)]
        L.mibn_sample.argtypes = [vp, C.c_int64, C.c_int32, i32p, i32p, C.c_uint64, C.POINTER(C.c_uint8)]
        L.mibn_sample_probe.argtypes = [vp, C.c_int64, C.POINTER(C.c_uint8), C.c_int32, f64p, f64p]
        L.mibn_sampling_query.argtypes = [vp, C.c_int32, C.c_int32, i32p, C.c_int32, i32p, i32p, C.c_int64, C.c_uint64, f64p, i64p]
        L.mibn_count_tables.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_uint8), C.c_int32, i32p, C.c_int32, i64p, i32p, i64p, i64p]
        L.mibn_dataset_create.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_uint8), C.c_int32, i32p, i32p]
        L.mibn_dataset_destroy.argtypes = [vp, C.c_int32]
        L.mibn_score_families.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, i64p, i32p, f64p]
        L.mibn_ci_tests.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, i64p, i32p, f64p, i64p]
        u32p = C.POINTER(C.c_uint32)
        L.mibn_dataset_set_weights.argtypes = [vp, C.c_int32, C.c_int32, u32p]
        L.mibn_dataset_bootstrap.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint64, u32p]
        L.mibn_score_families_w.argtypes = [vp, C.c_int32, C.c_int32, C.c_double, C.c_int32, i64p, i32p, i32p, f64p]
        L.mibn_ci_tests_w.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, i64p, i32p, i32p, f64p, i64p]
        L.mibn_count_tables_w.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_uint8), C.c_int32, i32p, C.c_int32, i64p, i32p, i64p, u32p, i64p]
        L.mibn_best_dag.argtypes = [vp, C.c_int32, C.c_int64, i32p, u32p, f64p, u32p, i32p, f64p]
        L.mibn_arc_posteriors.argtypes = [vp, C.c_int32, C.c_int64, i32p, u32p, f64p, f64p, f64p, f64p]
        L.mibn_last_stats.argtypes = [vp, C.POINTER(Stats)]
        L.mibn_last_kernel_stats.argtypes = [vp, C.c_int32, C.POINTER(KernelStat), C.POINTER(C.c_int32)]
        L.mibn_plan_stats.argtypes = [vp, C.c_int32, i32p, C.c_int32, i32p, C.POINTER(Stats)]
        L.mibn_set_option.argtypes = [vp, C.c_char_p, C.c_double]
        L.mibn_gibbs.argtypes = [vp, C.c_int32, i32p, C.c_int32, i32p, i32p, i32p, C.c_int64,
                                 C.c_int64, C.c_uint64, i64p]
        _lib = L
    return _lib


def device_count():
    n = C.c_int(0)
    lib().mibn_device_count(C.byref(n))
    return n.value


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _candidate_args(children, parent_masks, scores):
    """The candidate list of mibn_best_dag / mibn_arc_posteriors -> (n_fam, (fam_child, fam_parents, fam_score) as pointers); an
    empty list is padded to one entry, so that no pointer is null."""
    child = _i32(children).reshape(-1)
    masks = np.ascontiguousarray(parent_masks, dtype=np.uint32).reshape(-1)
    sc = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    if not len(child) == len(masks) == len(sc):
        raise ValueError("children, parent_masks and scores need one entry per candidate")
    n_fam = len(child)
    if n_fam == 0:
        child, masks, sc = np.zeros(1, np.int32), np.zeros(1, np.uint32), np.zeros(1, np.float64)
    return n_fam, (_p(child, C.c_int32), _p(masks, C.c_uint32), _p(sc, C.c_double))  # (a pointer keeps its array alive)


class Dataset:
    """A code matrix resident on the device (mibn_dataset_create), made by `Engine.dataset`.  Closed by `close()`, by leaving its
    `with` block, or when it is garbage collected; it keeps its engine alive until then."""

    def __init__(self, engine, ds_id, n_rows, card):
        self.engine = engine
        self.id = ds_id
        self.n_rows = n_rows
        self.card = card
        self.n_sets = 0

    def set_weights(self, w):
        """w: non-negative integers [n_sets, n_rows] (or one set [n_rows]), every set summing to at most 2^32 - 1 -> the weight
        sets of the data set (mibn_dataset_set_weights); None or zero sets drops them."""
        w = np.zeros((0, self.n_rows), np.uint32) if w is None else np.ascontiguousarray(np.atleast_2d(np.asarray(w)), dtype=np.uint32)
        if w.ndim != 2 or w.shape[1] != self.n_rows:
            raise ValueError("weights must be [n_sets, n_rows]")
        eng = self.engine
        eng._check(eng._L.mibn_dataset_set_weights(eng._h, self.id, len(w), _p(w if w.size else np.zeros(1, np.uint32), C.c_uint32)))
        self.n_sets = len(w)

    def bootstrap(self, n_sets, seed=0, return_weights=False):
        """Replaces the weight sets by `n_sets` multinomial resamples drawn on the device (mibn_dataset_bootstrap: set s is a function of
        (seed, s, n_rows) alone); with return_weights -> uint32 [n_sets, n_rows]."""
        w = np.zeros((int(n_sets), self.n_rows), np.uint32) if return_weights else None
        eng = self.engine
        eng._check(eng._L.mibn_dataset_bootstrap(eng._h, self.id, int(n_sets), int(seed) & (2 ** 64 - 1),
                                                 _p(w, C.c_uint32) if w is not None and w.size else None))
        self.n_sets = int(n_sets)
        return w

    def score_families(self, families, kind="bic", ess=1.0, wset=None):
        """families: sequences of column indices, parents first, CHILD LAST -> float64 array of their scores (`kind` one of
        SCORE_KINDS, `ess` the equivalent sample size of "bdeu"); one call, whatever the number of families.  After `close()`
        the library refuses the id (MibnError, E_ARG).  wset: one weight-set index per family (-1 = every row once) ->
        mibn_score_families_w; None is the unweighted call."""
        if kind not in SCORE_KINDS:
            raise ValueError(f"score must be one of {sorted(SCORE_KINDS)}, not {kind!r}")
        families = [tuple(f) for f in families]
        scope_off = np.concatenate([[0], np.cumsum([len(f) for f in families])]).astype(np.int64)
        scope_cols = _i32([c for f in families for c in f]) if scope_off[-1] else np.zeros(1, np.int32)
        scores = np.zeros(max(1, len(families)), np.float64)
        eng = self.engine
        if wset is not None:
            wset = _i32(wset).reshape(-1)
            if len(wset) != len(families):
                raise ValueError("wset needs one entry per family")
            eng._check(eng._L.mibn_score_families_w(eng._h, self.id, SCORE_KINDS[kind], float(ess), len(families), _p(scope_off, C.c_int64),
                                                    _p(scope_cols, C.c_int32), _p(wset if len(wset) else np.zeros(1, np.int32), C.c_int32),
                                                    _p(scores, C.c_double)))
            return scores[:len(families)]
        eng._check(eng._L.mibn_score_families(eng._h, self.id, SCORE_KINDS[kind], float(ess), len(families), _p(scope_off, C.c_int64),
                                              _p(scope_cols, C.c_int32), _p(scores, C.c_double)))
        return scores[:len(families)]

    def ci_tests(self, tests, kind="g2", wset=None):
        """tests: sequences of column indices (*Z, x, y), the conditioning columns first -> (stat float64[n], adj_dof int64[n]):
        the G2 or X2 statistic (`kind` one of CI_KINDS) of x and y given Z and the degrees of freedom adjusted for empty rows,
        columns and strata; one call, whatever the number of tests.  wset: one weight-set index per test (-1 = every row once) ->
        mibn_ci_tests_w; None is the unweighted call."""
        if kind not in CI_KINDS:
            raise ValueError(f"test must be one of {sorted(CI_KINDS)}, not {kind!r}")
        tests = [tuple(t) for t in tests]
        scope_off = np.concatenate([[0], np.cumsum([len(t) for t in tests])]).astype(np.int64)
        scope_cols = _i32([c for t in tests for c in t]) if scope_off[-1] else np.zeros(1, np.int32)
        stat = np.zeros(max(1, len(tests)), np.float64)
        dof = np.zeros(max(1, len(tests)), np.int64)
        eng = self.engine
        if wset is not None:
            wset = _i32(wset).reshape(-1)
            if len(wset) != len(tests):
                raise ValueError("wset needs one entry per test")
            eng._check(eng._L.mibn_ci_tests_w(eng._h, self.id, CI_KINDS[kind], len(tests), _p(scope_off, C.c_int64), _p(scope_cols, C.c_int32),
                                              _p(wset if len(wset) else np.zeros(1, np.int32), C.c_int32), _p(stat, C.c_double), _p(dof, C.c_int64)))
            return stat[:len(tests)], dof[:len(tests)]
        eng._check(eng._L.mibn_ci_tests(eng._h, self.id, CI_KINDS[kind], len(tests), _p(scope_off, C.c_int64), _p(scope_cols, C.c_int32),
                                        _p(stat, C.c_double), _p(dof, C.c_int64)))
        return stat[:len(tests)], dof[:len(tests)]

    def close(self):
        eng = self.engine
        if self.id >= 0 and eng is not None and getattr(eng, "_h", None) is not None and eng._h.value:
            ds_id, self.id = self.id, -1
            eng._check(eng._L.mibn_dataset_destroy(eng._h, ds_id))
        self.id = -1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One mibn context (= one GPU) holding one flattened network."""

    def __init__(self, device=0, planner_only=False):
        self._h = C.c_void_p()
        self._L = lib()
        if planner_only:
            rc = self._L.mibn_create_planner(C.byref(self._h))
        else:
            rc = self._L.mibn_create(int(device), C.byref(self._h))
        if rc != OK:
            why = {E_NODEVICE: "no gfx950 HIP device visible (there is no CPU fallback)",
                   E_ARG: "bad device index", E_HIP: "HIP runtime error"}.get(rc, "?")
            raise MibnError(rc, f"mibn_create failed: {why}")
        self.planner_only = planner_only
        self.device = device
        # experiment hook: MIBN_OPTS="name=value,..." sets engine options on every engine of the process (a parity run of the GPU
        # suite under a non-default option, e.g. MIBN_OPTS=mfma_kernel=1 python -m pytest tests -m gpu)
        for kv in os.environ.get("MIBN_OPTS", "").split(","):
            if "=" in kv:
                k, v = kv.split("=", 1)
                self.set_option(k.strip(), float(v))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.mibn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            raise MibnError(rc, self._L.mibn_last_error(self._h).decode())

    def set_network(self, card, scope_off, scope_vars, value_off, values):
        card, scope_vars = _i32(card), _i32(scope_vars)
        scope_off, value_off = _i64(scope_off), _i64(value_off)
        values = np.ascontiguousarray(values, dtype=np.float64)
        self._check(self._L.mibn_set_network(
            self._h, len(card), _p(card, C.c_int32), _p(scope_off, C.c_int64),
            _p(scope_vars, C.c_int32), _p(value_off, C.c_int64), _p(values, C.c_double)))
        self.card = card
        self.family_off = np.concatenate([[0], np.cumsum(np.diff(value_off))]).astype(np.int64)  # factor v's cells in a family-belief row
        self._card_list = card.tolist()
        self._one = {}

    def set_order_hints(self, hints):
        h = _i32(np.asarray(hints).reshape(-1, len(self.card)))
        self._check(self._L.mibn_set_order_hints(self._h, h.shape[0], _p(h, C.c_int32)))

    def set_option(self, name, value):
        self._check(self._L.mibn_set_option(self._h, name.encode(), float(value)))

    def set_likelihoods(self, likelihoods):
        """Stages the likelihood findings of the NEXT batch call (mibn_set_likelihoods): likelihoods = (l_off, l_vars, v_off, values),
        request b's findings are l_vars[l_off[b]:l_off[b + 1]], finding k's weights values[v_off[k]:v_off[k + 1]] - one per state of
        l_vars[k].  The query, mpe and map calls do this themselves for their `likelihoods=` argument."""
        l_off, l_vars, v_off, values = likelihoods
        l_off, v_off, l_vars = _i64(l_off), _i64(v_off), _i32(l_vars)
        values = np.ascontiguousarray(values, dtype=np.float64)
        if len(l_off) < 1 or len(v_off) != len(l_vars) + 1:
            raise ValueError("likelihoods: l_off needs one entry per request plus one, v_off one per finding plus one")
        self._check(self._L.mibn_set_likelihoods(
            self._h, len(l_off) - 1, _p(l_off, C.c_int64), _p(l_vars if len(l_vars) else np.zeros(1, np.int32), C.c_int32),
            _p(v_off, C.c_int64), _p(values if len(values) else np.zeros(1, np.float64), C.c_double)))

    def query_batch(self, q_off, q_vars, e_off, e_vars, e_codes, out_off=None, flags=0, likelihoods=None):
        """CSR request batch -> flat float64 posteriors (+ out_off).  flags: Q_NOPRUNE, Q_UNNORMALISED (per call, see mibn.h).
        likelihoods: the findings of the requests as (l_off, l_vars, v_off, values), see set_likelihoods."""
        q_off, e_off = _i64(q_off), _i64(e_off)
        q_vars, e_vars, e_codes = _i32(q_vars), _i32(e_vars), _i32(e_codes)
        B = len(q_off) - 1
        if out_off is None:
            cells = np.ones(B, np.int64)
            if B:
                nq = np.diff(q_off)
                if nq.min() == nq.max() and nq[0] > 0:
                    cells = np.prod(self.card[q_vars].reshape(B, -1).astype(np.int64), axis=1)
                else:
                    cells = np.array([int(np.prod(self.card[q_vars[a:b]].astype(np.int64)))
                                      for a, b in zip(q_off[:-1], q_off[1:])], np.int64)
            out_off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
        out_off = _i64(out_off)
        out = np.zeros(int(out_off[-1]), np.float64)
        e_vars_ = e_vars if len(e_vars) else np.zeros(1, np.int32)
        e_codes_ = e_codes if len(e_codes) else np.zeros(1, np.int32)
        q_vars_ = q_vars if len(q_vars) else np.zeros(1, np.int32)
        out_ = out if len(out) else np.zeros(1, np.float64)
        if likelihoods is not None:
            self.set_likelihoods(likelihoods)
        self._check(self._L.mibn_query_batch_ex(
            self._h, int(flags), B, _p(q_off, C.c_int64), _p(q_vars_, C.c_int32), _p(e_off, C.c_int64),
            _p(e_vars_, C.c_int32), _p(e_codes_, C.c_int32), _p(out_off, C.c_int64),
            _p(out_, C.c_double)))
        return out, out_off

    def query_one(self, q, ev, codes, flags=0, likelihoods=None):
        """One request (lists of variable ids / codes) -> dense posterior [cells].  The latency path of a single `query()`:
        preallocated ctypes arrays per request shape, one C call (query_fixed builds a dozen numpy arrays on the way)."""
        nq, ne = len(q), len(ev)
        card = self._card_list
        cells = 1
        try:
            for v in q:
                cells *= card[v]
        except (IndexError, TypeError):
            cells = 1  # (an unknown id: the library builds the error message)
        one = self._one
        key = (nq, ne)
        buf = one.get(key)
        if buf is None:
            buf = one[key] = ((C.c_int64 * 2)(0, nq), (C.c_int64 * 2)(0, ne), (C.c_int64 * 2)(0, 0),
                              (C.c_int32 * max(1, nq))(), (C.c_int32 * max(1, ne))(), (C.c_int32 * max(1, ne))())
        q_off, e_off, out_off, qa, ea, ca = buf
        out_off[1] = cells
        qa[:nq] = q
        if ne:
            ea[:ne] = ev
            ca[:ne] = codes
        out = np.zeros(max(1, cells), np.float64)
        if likelihoods is not None:
            self.set_likelihoods(likelihoods)
        rc = self._L.mibn_query_batch_ex(self._h, int(flags), 1, q_off, qa, e_off, ea, ca, out_off,
                                         out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != OK:
            self._check(rc)
        return out[:cells]

    def query_fixed(self, qvars, evars, ecodes, flags=0, likelihoods=None):
        """Fixed-shape batch: qvars[B, nq], evars[B, ne], ecodes[B, ne] -> posteriors[B, cells]
        (all requests must have the same query-table size).  nq = 0 (flags with Q_UNNORMALISED): one cell per request, P(e)."""
        if len(qvars) == 0:
            return np.zeros((0, 0), np.float64)
        qvars = _i32(qvars).reshape(len(qvars), -1)
        B, nq = qvars.shape
        evars = _i32(evars).reshape(B, -1)
        ecodes = _i32(ecodes).reshape(B, -1)
        ne = evars.shape[1]
        q_off = np.arange(B + 1, dtype=np.int64) * nq
        e_off = np.arange(B + 1, dtype=np.int64) * ne
        out, out_off = self.query_batch(q_off, qvars.reshape(-1), e_off, evars.reshape(-1),
                                        ecodes.reshape(-1), flags=flags, likelihoods=likelihoods)
        return out.reshape(B, -1) if B else out.reshape(0, 0)

    def mpe_batch(self, e_off, e_vars, e_codes, likelihoods=None):
        """CSR evidence -> (codes[B, n_vars] int32, log_p[B] float64): the most probable explanation of every request
        (mibn_mpe_batch).  likelihoods: as in query_batch."""
        n_vars = len(self.card)
        e_off = _i64(e_off)
        B = len(e_off) - 1
        e_vars, e_codes = _i32(e_vars), _i32(e_codes)
        codes = np.empty((B, n_vars), np.int32)
        log_p = np.empty(B, np.float64)
        if B == 0:
            return codes, log_p
        if likelihoods is not None:
            self.set_likelihoods(likelihoods)
        self._check(self._L.mibn_mpe_batch(self._h, B, _p(e_off, C.c_int64), _p(e_vars, C.c_int32), _p(e_codes, C.c_int32),
                                           _p(codes, C.c_int32), _p(log_p, C.c_double)))
        return codes, log_p

    def bp_batch(self, e_off, e_vars, e_codes, max_iterations=100, tol=1e-9, damping=0.0, likelihoods=None):
        """CSR evidence -> (beliefs[B, sum(card)] float64, iterations[B] int32, residual[B] float64): loopy belief propagation
        (mibn_bp_batch) - every single-variable posterior of every request, variable v's at columns sum(card[:v]) .. + card[v];
        a request has converged when its residual is <= tol.  likelihoods: as in query_batch."""
        e_off = _i64(e_off)
        B = len(e_off) - 1
        e_vars, e_codes = _i32(e_vars), _i32(e_codes)
        width = int(np.sum(self.card, dtype=np.int64))
        beliefs = np.zeros((B, width), np.float64)
        iterations = np.zeros(B, np.int32)
        residual = np.zeros(B, np.float64)
        if likelihoods is not None:
            self.set_likelihoods(likelihoods)
        pad = np.zeros(1, np.int32)
        self._check(self._L.mibn_bp_batch(
            self._h, B, _p(e_off, C.c_int64), _p(e_vars if len(e_vars) else pad, C.c_int32), _p(e_codes if len(e_codes) else pad, C.c_int32),
            int(max_iterations), float(tol), float(damping), _p(beliefs if beliefs.size else np.zeros(1), C.c_double),
            _p(iterations if B else pad, C.c_int32), _p(residual if B else np.zeros(1), C.c_double)))
        return beliefs, iterations, residual

    def bp(self, evars, ecodes, max_iterations=100, tol=1e-9, damping=0.0, likelihoods=None):
        """Fixed-shape batch: evars[B, ne], ecodes[B, ne] -> (beliefs[B, sum(card)], iterations[B], residual[B]), like mpe."""
        evars = _i32(evars)
        B = len(evars)
        evars = evars.reshape(B, -1)
        ecodes = _i32(ecodes).reshape(B, -1)
        e_off = np.arange(B + 1, dtype=np.int64) * evars.shape[1]
        return self.bp_batch(e_off, evars.reshape(-1), ecodes.reshape(-1), max_iterations, tol, damping, likelihoods=likelihoods)

    def bp_mpe_batch(self, e_off, e_vars, e_codes, max_iterations=100, tol=1e-9, damping=0.5, polish_sweeps=10, likelihoods=None):
        """CSR evidence -> (codes[B, n_vars] int32, log_p[B] float64, iterations[B] int32, residual[B] float64, info[B, 3] int32):
        approximate most probable explanation by max-product belief propagation with an ICM polish (mibn_bp_mpe_batch).  log_p is the
        log-probability of the returned codes; info holds best_iteration, sweeps run, moves made.  likelihoods: as in query_batch."""
        e_off = _i64(e_off)
        B = len(e_off) - 1
        e_vars, e_codes = _i32(e_vars), _i32(e_codes)
        n_vars = len(self.card)
        codes = np.zeros((B, n_vars), np.int32)
        log_p = np.zeros(B, np.float64)
        iterations = np.zeros(B, np.int32)
        residual = np.zeros(B, np.float64)
        info = np.zeros((B, 3), np.int32)
        if likelihoods is not None:
            self.set_likelihoods(likelihoods)
        pad, padf = np.zeros(1, np.int32), np.zeros(1, np.float64)
        self._check(self._L.mibn_bp_mpe_batch(
            self._h, B, _p(e_off, C.c_int64), _p(e_vars if len(e_vars) else pad, C.c_int32), _p(e_codes if len(e_codes) else pad, C.c_int32),
            int(max_iterations), float(tol), float(damping), int(polish_sweeps), _p(codes if codes.size else pad, C.c_int32),
            _p(log_p if B else padf, C.c_double), _p(iterations if B else pad, C.c_int32), _p(residual if B else padf, C.c_double),
            _p(info if B else np.zeros(3, np.int32), C.c_int32)))
        return codes, log_p, iterations, residual, info

    def bp_mpe(self, evars, ecodes, max_iterations=100, tol=1e-9, damping=0.5, polish_sweeps=10, likelihoods=None):
        """Fixed-shape batch: evars[B, ne], ecodes[B, ne] -> what bp_mpe_batch returns, like mpe."""
        evars = _i32(evars)
        B = len(evars)
        evars = evars.reshape(B, -1)
        ecodes = _i32(ecodes).reshape(B, -1)
        e_off = np.arange(B + 1, dtype=np.int64) * evars.shape[1]
        return self.bp_mpe_batch(e_off, evars.reshape(-1), ecodes.reshape(-1), max_iterations, tol, damping, polish_sweeps, likelihoods=likelihoods)

    def bp_evidence_batch(self, e_off, e_vars, e_codes, max_iterations=100, tol=1e-9, damping=0.0, likelihoods=None, weight=None, acc=None,
                          beliefs=False, fbeliefs=False):
        """CSR evidence -> (log_z[B] float64, beliefs[B, sum(card)] or None, fbeliefs[B, fcells] or None, iterations[B] int32,
        residual[B] float64): the Bethe approximation of log P(e) and the belief of every family from loopy belief propagation
        (mibn_bp_evidence_batch).  Family v's cells are at columns family_off[v] .. family_off[v + 1], in the C-order of (parents.., v).
        acc: a contiguous float64 array of fcells expected counts, updated IN PLACE - every request's family beliefs are added, times
        weight[b] (None: 1.0), in request order.  beliefs / fbeliefs: whether to return them.  likelihoods: as in query_batch."""
        e_off = _i64(e_off)
        B = len(e_off) - 1
        e_vars, e_codes = _i32(e_vars), _i32(e_codes)
        fcells = int(self.family_off[-1])
        if acc is not None and not (isinstance(acc, np.ndarray) and acc.dtype == np.float64 and acc.flags.c_contiguous and acc.flags.writeable):
            raise ValueError("acc must be a writeable C-contiguous float64 array (it is updated in place)")
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.float64)
            if len(w) != B:
                raise ValueError("weight needs one entry per request")
        log_z = np.zeros(B, np.float64)
        bel = np.zeros((B, int(np.sum(self.card, dtype=np.int64))), np.float64) if beliefs else None
        fbel = np.zeros((B, fcells), np.float64) if fbeliefs else None
        iterations = np.zeros(B, np.int32)
        residual = np.zeros(B, np.float64)
        if likelihoods is not None:
            self.set_likelihoods(likelihoods)
        pad, padf = np.zeros(1, np.int32), np.zeros(1, np.float64)

        def opt(a):
            return None if a is None else _p(a.reshape(-1) if a.size else padf, C.c_double)
        self._check(self._L.mibn_bp_evidence_batch(
            self._h, B, _p(e_off, C.c_int64), _p(e_vars if len(e_vars) else pad, C.c_int32), _p(e_codes if len(e_codes) else pad, C.c_int32),
            int(max_iterations), float(tol), float(damping), opt(w), _p(log_z if B else padf, C.c_double), opt(bel), opt(fbel),
            int(acc.size) if acc is not None else 0, opt(acc), _p(iterations if B else pad, C.c_int32), _p(residual if B else padf, C.c_double)))
        return log_z, bel, fbel, iterations, residual

    def bp_evidence(self, evars, ecodes, max_iterations=100, tol=1e-9, damping=0.0, **more):
        """Fixed-shape batch: evars[B, ne], ecodes[B, ne] -> what bp_evidence_batch returns, like bp."""
        evars = _i32(evars)
        B = len(evars)
        evars = evars.reshape(B, -1)
        ecodes = _i32(ecodes).reshape(B, -1)
        e_off = np.arange(B + 1, dtype=np.int64) * evars.shape[1]
        return self.bp_evidence_batch(e_off, evars.reshape(-1), ecodes.reshape(-1), max_iterations, tol, damping, **more)

    def posterior_sample_batch(self, e_off, e_vars, e_codes, s_off, seed=0, flags=0):
        """CSR evidence + sample offsets s_off[B + 1] -> (codes[s_off[B] - s_off[0], n_vars] int32, p_e[B] float64): exact samples of
        P(x | e_b), row s_off[b] - s_off[0] + i the i-th sample of request b (mibn_posterior_sample_batch).  s_off[0] is the global
        row index of the first sample (the Philox counter): 0 unless the call draws a later part of a stream.  flags: DRAW_PRUNE."""
        n_vars = len(self.card)
        e_off, s_off = _i64(e_off), _i64(s_off)
        B = len(e_off) - 1
        e_vars, e_codes = _i32(e_vars), _i32(e_codes)
        rows = int(s_off[-1] - s_off[0]) if B else 0
        codes = np.empty((max(0, rows), n_vars), np.int32)
        p_e = np.empty(B, np.float64)
        if B == 0:
            return codes, p_e
        e_vars_ = e_vars if len(e_vars) else np.zeros(1, np.int32)
        e_codes_ = e_codes if len(e_codes) else np.zeros(1, np.int32)
        codes_ = codes if codes.size else np.zeros(1, np.int32)
        self._check(self._L.mibn_posterior_sample_batch(self._h, B, _p(e_off, C.c_int64), _p(e_vars_, C.c_int32), _p(e_codes_, C.c_int32),
                                                        _p(s_off, C.c_int64), int(seed) & (2**64 - 1), int(flags), _p(codes_, C.c_int32),
                                                        _p(p_e, C.c_double)))
        return codes, p_e

    def posterior_sample(self, evars, ecodes, n, seed=0, flags=0):
        """Fixed-shape batch: evars[B, ne], ecodes[B, ne], n samples each -> (codes[B * n, n_vars], p_e[B]), like mpe."""
        evars = _i32(evars)
        B = len(evars)
        evars = evars.reshape(B, -1)
        ecodes = _i32(ecodes).reshape(B, -1)
        e_off = np.arange(B + 1, dtype=np.int64) * evars.shape[1]
        s_off = np.arange(B + 1, dtype=np.int64) * int(n)
        return self.posterior_sample_batch(e_off, evars.reshape(-1), ecodes.reshape(-1), s_off, seed=seed, flags=flags)

    def expect_batch(self, q_off, q_vars, e_off, e_vars, e_codes, acc_base, acc_stride, acc, weight=None, flags=0):
        """CSR request batch -> expected counts (mibn_expect_batch): every request's posterior P(q | e) is added into `acc` (a
        contiguous float64 array, updated IN PLACE) at acc_base[b] + sum_k idx_k * acc_stride[q_off[b] + k]; returns p_out [B],
        P(e_b) of every request.  A request may have no query variable (it only fills p_out).  flags: Q_NOPRUNE."""
        q_off, e_off = _i64(q_off), _i64(e_off)
        q_vars, e_vars, e_codes = _i32(q_vars), _i32(e_vars), _i32(e_codes)
        acc_base, acc_stride = _i64(acc_base), _i64(acc_stride)
        B = len(q_off) - 1
        if not (isinstance(acc, np.ndarray) and acc.dtype == np.float64 and acc.flags.c_contiguous and acc.flags.writeable):
            raise ValueError("acc must be a writeable C-contiguous float64 array (it is updated in place)")
        if len(acc_base) != B or len(acc_stride) != len(q_vars):
            raise ValueError("acc_base needs one entry per request, acc_stride one per query variable")
        p_out = np.zeros(max(1, B), np.float64)
        w = None
        if weight is not None:
            w = np.ascontiguousarray(weight, dtype=np.float64)
            if len(w) != B:
                raise ValueError("weight needs one entry per request")
        pad32, pad64 = np.zeros(1, np.int32), np.zeros(1, np.int64)
        acc_ = acc.reshape(-1) if acc.size else np.zeros(1, np.float64)
        self._check(self._L.mibn_expect_batch(
            self._h, int(flags), B, _p(q_off, C.c_int64), _p(q_vars if len(q_vars) else pad32, C.c_int32), _p(e_off, C.c_int64),
            _p(e_vars if len(e_vars) else pad32, C.c_int32), _p(e_codes if len(e_codes) else pad32, C.c_int32),
            _p(acc_base if B else pad64, C.c_int64), _p(acc_stride if len(acc_stride) else pad64, C.c_int64),
            _p(w, C.c_double) if w is not None and B else None, int(acc.size), _p(acc_, C.c_double), _p(p_out, C.c_double)))
        return p_out[:B]

    def mpe(self, evars, ecodes, likelihoods=None):
        """Fixed-shape batch: evars[B, ne], ecodes[B, ne] -> (codes[B, n_vars], log_p[B]), like query_fixed."""
        evars = _i32(evars)
        B = len(evars)
        evars = evars.reshape(B, -1)
        ecodes = _i32(ecodes).reshape(B, -1)
        e_off = np.arange(B + 1, dtype=np.int64) * evars.shape[1]
        return self.mpe_batch(e_off, evars.reshape(-1), ecodes.reshape(-1), likelihoods=likelihoods)

    def map_batch(self, m_off, m_vars, e_off, e_vars, e_codes, flags=0, likelihoods=None):
        """CSR MAP variables + CSR evidence -> (codes[m_off[B] - m_off[0]] int32, log_p[B] float64): marginal MAP of every request
        (mibn_map_batch) - codes[m_off[b] - m_off[0] + k] is the code of m_vars[m_off[b] + k] in argmax_m sum_h P(m, h, e_b), log_p[b] the
        log of that maximum.  flags: MAP_PRUNE.  likelihoods: as in query_batch."""
        m_off, e_off = _i64(m_off), _i64(e_off)
        B = len(e_off) - 1
        if len(m_off) != B + 1:
            raise ValueError("m_off and e_off need one entry per request, plus one")
        m_vars, e_vars, e_codes = _i32(m_vars), _i32(e_vars), _i32(e_codes)
        codes = np.empty(max(0, int(m_off[-1] - m_off[0])) if B else 0, np.int32)
        log_p = np.empty(B, np.float64)
        if B == 0:
            return codes, log_p
        pad32 = np.zeros(1, np.int32)
        if likelihoods is not None:
            self.set_likelihoods(likelihoods)
        self._check(self._L.mibn_map_batch(self._h, int(flags), B, _p(m_off, C.c_int64), _p(m_vars if len(m_vars) else pad32, C.c_int32),
                                           _p(e_off, C.c_int64), _p(e_vars if len(e_vars) else pad32, C.c_int32),
                                           _p(e_codes if len(e_codes) else pad32, C.c_int32), _p(codes if codes.size else pad32, C.c_int32),
                                           _p(log_p, C.c_double)))
        return codes, log_p

    def map(self, mvars, evars, ecodes, flags=0, likelihoods=None):
        """Fixed-shape batch: mvars[B, nm], evars[B, ne], ecodes[B, ne] -> (codes[B, nm], log_p[B]), like mpe."""
        mvars, evars, ecodes = _i32(mvars), _i32(evars), _i32(ecodes)
        B = len(mvars)
        nm, ne = (mvars.size // B, evars.size // B) if B else (0, 0)  # (either may be 0: no reshape(B, -1) of an empty array)
        m_off = np.arange(B + 1, dtype=np.int64) * nm
        e_off = np.arange(B + 1, dtype=np.int64) * ne
        codes, log_p = self.map_batch(m_off, mvars.reshape(-1), e_off, evars.reshape(-1), ecodes.reshape(-1), flags=flags, likelihoods=likelihoods)
        return codes.reshape(B, nm), log_p

    def submit_fixed(self, qvars, evars, ecodes):
        """Asynchronous query_fixed: returns a handle for wait().  At most two calls in flight."""
        qvars = _i32(qvars).reshape(len(qvars), -1)
        B, nq = qvars.shape
        evars = _i32(evars).reshape(B, -1)
        ecodes = _i32(ecodes).reshape(B, -1)
        ne = evars.shape[1]
        q_off = np.arange(B + 1, dtype=np.int64) * nq
        e_off = np.arange(B + 1, dtype=np.int64) * ne
        cells = np.prod(self.card[qvars].astype(np.int64), axis=1) if B else np.zeros(0, np.int64)
        out_off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
        out = np.zeros(max(1, int(out_off[-1])), np.float64)
        ticket = C.c_int32(-1)
        keep = (q_off, qvars, e_off, evars, ecodes, out_off, out)  # the library reads them during the call only, `out` until wait
        self._check(self._L.mibn_submit_batch(
            self._h, B, _p(q_off, C.c_int64), _p(qvars.reshape(-1), C.c_int32), _p(e_off, C.c_int64),
            _p(evars.reshape(-1) if ne else np.zeros(1, np.int32), C.c_int32),
            _p(ecodes.reshape(-1) if ne else np.zeros(1, np.int32), C.c_int32), _p(out_off, C.c_int64),
            _p(out, C.c_double), C.byref(ticket)))
        return {"ticket": ticket.value, "out": out, "B": B, "n": int(out_off[-1]), "keep": keep}

    def wait(self, handle):
        self._check(self._L.mibn_wait(self._h, handle["ticket"]))
        return handle["out"][:handle["n"]].reshape(handle["B"], -1) if handle["B"] else handle["out"][:0].reshape(0, 0)

    def wait_flat(self, handle):
        """wait() for a call whose query tables differ in size from request to request (a 2-state and a 3-state query
        variable in one fixed-arity batch): the posteriors back to back, request i at the offsets the caller derives from the cards."""
        self._check(self._L.mibn_wait(self._h, handle["ticket"]))
        return handle["out"][:handle["n"]]

    def drain(self):
        self._check(self._L.mibn_drain(self._h))

    def stats(self):
        s = Stats()
        self._check(self._L.mibn_last_stats(self._h, C.byref(s)))
        return s.as_dict()

    def total_stats(self):
        """Counters accumulated since the engine was created (take differences over a region of calls)."""
        s = Stats()
        self._check(self._L.mibn_total_stats(self._h, C.byref(s)))
        return s.as_dict()

    def total_kernel_stats(self):
        arr = (KernelStat * 64)()
        n = C.c_int32(0)
        self._check(self._L.mibn_total_kernel_stats(self._h, 64, arr, C.byref(n)))
        return {arr[i].name.decode(): {"launches": arr[i].launches, "ms": arr[i].ms, "alg_bytes": arr[i].alg_bytes,
                                       "items": arr[i].items} for i in range(n.value)}

    def kernel_stats(self):
        """Per-kernel breakdown of the last query_batch: list of dicts (name, launches, ms, alg_bytes, items)."""
        arr = (KernelStat * 64)()
        n = C.c_int32(0)
        self._check(self._L.mibn_last_kernel_stats(self._h, 64, arr, C.byref(n)))
        return [{"name": arr[i].name.decode(), "launches": arr[i].launches, "ms": arr[i].ms,
                 "alg_bytes": arr[i].alg_bytes, "items": arr[i].items} for i in range(n.value)]

    def plan_stats(self, qvars, evars):
        q, e = _i32(qvars), _i32(evars)
        e_ = e if len(e) else np.zeros(1, np.int32)
        s = Stats()
        self._check(self._L.mibn_plan_stats(self._h, len(q), _p(q, C.c_int32), len(e),
                                            _p(e_, C.c_int32), C.byref(s)))
        return s.as_dict()

    def plan_order(self, qvars, evars):
        """The elimination order the planner executes for this request (hidden variables, first eliminated first)."""
        q, e = _i32(qvars), _i32(evars)
        e_ = e if len(e) else np.zeros(1, np.int32)
        order = np.zeros(len(self.card), np.int32)
        n = C.c_int32(0)
        self._check(self._L.mibn_plan_order(self._h, len(q), _p(q, C.c_int32), len(e), _p(e_, C.c_int32),
                                            _p(order, C.c_int32), C.byref(n)))
        return order[:n.value].copy()

    def gibbs(self, qvars, evars, ecodes, n_chains, n_iterations, seed=0, cycle=None, chain_first=0):
        """Histogram of chains [chain_first, chain_first + n_chains) of stream `seed` (mibn_gibbs_shard)."""
        q, e, c = _i32(qvars), _i32(evars), _i32(ecodes)
        e_ = e if len(e) else np.zeros(1, np.int32)
        c_ = c if len(c) else np.zeros(1, np.int32)
        cells = int(np.prod(self.card[q].astype(np.int64)))
        counts = np.zeros(cells, np.int64)
        cyc = None
        if cycle is not None:
            cyc_arr = _i32(cycle)
            cyc = _p(cyc_arr, C.c_int32)
        self._check(self._L.mibn_gibbs_shard(self._h, len(q), _p(q, C.c_int32), len(e),
                                             _p(e_, C.c_int32), _p(c_, C.c_int32), cyc, int(chain_first), int(n_chains),
                                             int(n_iterations), int(seed) & (2**64 - 1),
                                             _p(counts, C.c_int64)))
        return counts

    def gibbs_conditional(self, var, states, evars=(), ecodes=(), cycle=None):
        """P(var = x | the rest of each row of `states` [n_rows, n_vars]) as the Gibbs kernel computes it (mibn_gibbs_conditional)."""
        e, c = _i32(evars), _i32(ecodes)
        e_ = e if len(e) else np.zeros(1, np.int32)
        c_ = c if len(c) else np.zeros(1, np.int32)
        st = np.ascontiguousarray(states, np.uint8).reshape(-1, len(self.card))
        out = np.zeros((len(st), int(self.card[var])), np.float64)
        cyc = None
        if cycle is not None:
            cyc_arr = _i32(cycle)
            cyc = _p(cyc_arr, C.c_int32)
        self._check(self._L.mibn_gibbs_conditional(self._h, len(e), _p(e_, C.c_int32), _p(c_, C.c_int32), cyc, int(var), len(st),
                                                   st.ctypes.data_as(C.POINTER(C.c_uint8)), _p(out, C.c_double)))
        return out

    # ---- shard balancing / multi-GPU ------------------------------------------------------
    def estimate_costs(self, qvars, evars):
        """Planner cost estimate (section-8(d) bytes of the cheaper sweep order) per request of a fixed-shape batch."""
        qvars = _i32(qvars).reshape(len(qvars), -1)
        B, nq = qvars.shape
        evars = _i32(evars).reshape(B, -1)
        ne = evars.shape[1]
        q_off = np.arange(B + 1, dtype=np.int64) * nq
        e_off = np.arange(B + 1, dtype=np.int64) * ne
        cost = np.zeros(max(1, B), np.float64)
        ev = evars.reshape(-1) if evars.size else np.zeros(1, np.int32)
        self._check(self._L.mibn_estimate_costs(self._h, B, _p(q_off, C.c_int64), _p(qvars.reshape(-1), C.c_int32),
                                                _p(e_off, C.c_int64), _p(ev, C.c_int32), _p(cost, C.c_double)))
        return cost[:B]

    def synchronize(self):
        self._check(self._L.mibn_device_synchronize(self._h))

    def comm_probe(self):
        """librccl.so loads and has the entry points mibn_comm_* needs (no id, no socket, no thread)."""
        self._check(self._L.mibn_comm_probe(self._h))

    def device_info(self):
        buf = C.create_string_buffer(1024)
        self._check(self._L.mibn_device_info(self._h, buf, 1024))
        return buf.value.decode(errors="replace")

    def comm_unique_id(self):
        buf = C.create_string_buffer(COMM_ID_BYTES)
        self._check(self._L.mibn_comm_unique_id(self._h, buf))
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        assert len(unique_id) == COMM_ID_BYTES
        self._check(self._L.mibn_comm_init(self._h, int(rank), int(world), unique_id))

    def comm_count(self):
        """(ncclCommCount, ncclCommUserRank) of the live communicator - what RCCL itself reports."""
        n, r = C.c_int32(0), C.c_int32(-1)
        self._check(self._L.mibn_comm_count(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def comm_destroy(self):
        self._check(self._L.mibn_comm_destroy(self._h))

    def comm_allgather(self, send, world):
        send = np.ascontiguousarray(send, dtype=np.float64).reshape(-1)
        recv = np.empty(len(send) * int(world), np.float64)
        self._check(self._L.mibn_comm_allgather_f64(self._h, _p(send, C.c_double), len(send), _p(recv, C.c_double)))
        return recv.reshape(int(world), -1)

    def comm_reduce_i64(self, buf, root=0):
        out = np.ascontiguousarray(buf, dtype=np.int64).copy()
        self._check(self._L.mibn_comm_reduce_i64(self._h, _p(out.reshape(-1), C.c_int64), out.size, int(root)))
        return out

    def comm_allreduce_max(self, values):
        out = np.ascontiguousarray(values, dtype=np.float64).copy().reshape(-1)
        self._check(self._L.mibn_comm_allreduce_max_f64(self._h, _p(out, C.c_double), len(out)))
        return out

    def comm_barrier(self):
        self._check(self._L.mibn_comm_barrier(self._h))

    def sample(self, n_samples, init_vars=(), init_codes=(), seed=0):
        """Forward samples: uint8 codes [n_samples, n_vars]."""
        iv, ic = _i32(init_vars), _i32(init_codes)
        out = np.zeros((int(n_samples), len(self.card)), np.uint8)
        iv_ = iv if len(iv) else np.zeros(1, np.int32)
        ic_ = ic if len(ic) else np.zeros(1, np.int32)
        self._check(self._L.mibn_sample(self._h, int(n_samples), len(iv), _p(iv_, C.c_int32), _p(ic_, C.c_int32),
                                        int(seed) & (2**64 - 1), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def sample_probe(self, states):
        """The sampling kernel's walk over GIVEN joint states [n_rows, n_vars] (mibn_sample_probe) -> (likelihood [n_rows],
        running sums of every variable's conditional row [n_rows, n_vars, max card])."""
        st = np.ascontiguousarray(states, np.uint8).reshape(-1, len(self.card))
        stride = int(self.card.max())
        lik = np.zeros(len(st), np.float64)
        cdf = np.zeros((len(st), len(self.card), stride), np.float64)
        self._check(self._L.mibn_sample_probe(self._h, len(st), st.ctypes.data_as(C.POINTER(C.c_uint8)), stride,
                                              _p(lik, C.c_double), _p(cdf, C.c_double)))
        return lik, cdf

    def sampling_query(self, mode, qvars, evars, ecodes, n_samples, seed=0):
        """mode 1 = rejection, 2 = likelihood weighting -> (weight_sum, counts) per joint query state."""
        q, e, c = _i32(qvars), _i32(evars), _i32(ecodes)
        e_ = e if len(e) else np.zeros(1, np.int32)
        c_ = c if len(c) else np.zeros(1, np.int32)
        cells = int(np.prod(self.card[q].astype(np.int64)))
        wsum = np.zeros(cells, np.float64)
        counts = np.zeros(cells, np.int64)
        self._check(self._L.mibn_sampling_query(self._h, int(mode), len(q), _p(q, C.c_int32), len(e), _p(e_, C.c_int32),
                                                _p(c_, C.c_int32), int(n_samples), int(seed) & (2**64 - 1),
                                                _p(wsum, C.c_double), _p(counts, C.c_int64)))
        return wsum, counts

    def dataset(self, codes, card):
        """codes: uint8 [n_rows, n_cols] (row- or column-major, sent as it is) with codes[:, c] < card[c] -> a `Dataset` kept on
        the device until it is closed: the rows are uploaded once, `Dataset.score_families` then moves only family lists and
        scores."""
        codes = np.asarray(codes, dtype=np.uint8)
        if codes.ndim != 2:
            raise ValueError("codes must be a [n_rows, n_cols] matrix")
        if not (codes.flags.f_contiguous or codes.flags.c_contiguous):
            codes = np.ascontiguousarray(codes)
        row_major = 0 if codes.flags.f_contiguous else 1
        n_rows, n_cols = codes.shape
        card = _i32(card)
        if len(card) != n_cols:
            raise ValueError("card needs one entry per column")
        ds_id = C.c_int32(-1)
        self._check(self._L.mibn_dataset_create(self._h, n_rows, n_cols, codes.ctypes.data_as(C.POINTER(C.c_uint8)), row_major,
                                                _p(card if len(card) else np.zeros(1, np.int32), C.c_int32), C.byref(ds_id)))
        return Dataset(self, ds_id.value, n_rows, card)

    def best_dag(self, n_vars, children, parent_masks, scores):
        """The best-scoring DAG from a list of local scores (mibn_best_dag): candidate f lets child children[f] take exactly the parent
        set parent_masks[f] (bit u = column u) at scores[f] -> (parents uint32[n_vars], order int32[n_vars] roots first, total).  No
        DAG from these candidates: total -inf, every parents entry NO_PARENTS."""
        n_fam, fam = _candidate_args(children, parent_masks, scores)
        n = max(0, int(n_vars))
        parents, order, total = np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.int32), C.c_double(0.0)
        self._check(self._L.mibn_best_dag(self._h, int(n_vars), n_fam, *fam, _p(parents, C.c_uint32), _p(order, C.c_int32), C.byref(total)))
        return parents[:n], order[:n], float(total.value)

    def arc_posteriors(self, n_vars, children, parent_masks, scores):
        """Exact posteriors over all DAGs from a list of local log scores (mibn_arc_posteriors; the candidates as in `best_dag`) ->
        (log_post float64[n_fam]: the log posterior that a candidate's child has exactly its parent set, arc float64[n_vars,
        n_vars]: arc[u, v] = P(u -> v), log_evidence).  Under an order-modular prior, not a uniform one (include/mibn.h).  No DAG
        from these candidates: log_evidence -inf, every log_post -inf, every arc 0."""
        n_fam, fam = _candidate_args(children, parent_masks, scores)
        n = max(0, int(n_vars))
        log_post, arc, evidence = np.zeros(max(1, n_fam), np.float64), np.zeros(max(1, n * n), np.float64), C.c_double(0.0)
        self._check(self._L.mibn_arc_posteriors(self._h, int(n_vars), n_fam, *fam, _p(log_post, C.c_double), _p(arc, C.c_double), C.byref(evidence)))
        return log_post[:n_fam], arc[:n * n].reshape(n, n), float(evidence.value)

    def count_tables(self, codes, card, tables, weights=None):
        """codes: uint8 [n_rows, n_cols] (row- or column-major, sent as it is); tables: list of column-index tuples
        -> list of dense int64 contingency tables shaped by the cards of their columns.  weights: non-negative integers
        [n_rows] summing to at most 2^32 - 1, row i counts weights[i] times (mibn_count_tables_w); None: every row once."""
        codes = np.asarray(codes, dtype=np.uint8)
        if codes.ndim != 2:
            raise ValueError("codes must be a [n_rows, n_cols] matrix")
        if not (codes.flags.f_contiguous or codes.flags.c_contiguous):
            codes = np.ascontiguousarray(codes)
        row_major = 0 if codes.flags.f_contiguous else 1
        n_rows, n_cols = codes.shape
        card = _i32(card)
        scope_off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
        scope_cols = _i32([c for t in tables for c in t]) if len(tables) else np.zeros(0, np.int32)
        cells = [int(np.prod(card[list(t)].astype(np.int64))) for t in tables]
        counts_off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
        counts = np.zeros(max(1, int(counts_off[-1])), np.int64)
        sc = scope_cols if len(scope_cols) else np.zeros(1, np.int32)
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.uint32).reshape(-1)
            if len(w) != n_rows:
                raise ValueError("weights needs one entry per row")
            self._check(self._L.mibn_count_tables_w(
                self._h, n_rows, n_cols, codes.ctypes.data_as(C.POINTER(C.c_uint8)), row_major, _p(card if len(card) else np.zeros(1, np.int32), C.c_int32),
                len(tables), _p(scope_off, C.c_int64), _p(sc, C.c_int32), _p(counts_off, C.c_int64), _p(w if len(w) else np.zeros(1, np.uint32), C.c_uint32),
                _p(counts, C.c_int64)))
            return [counts[a:b].reshape([int(card[c]) for c in t]) for t, a, b in zip(tables, counts_off[:-1], counts_off[1:])]
        self._check(self._L.mibn_count_tables(
            self._h, n_rows, n_cols, codes.ctypes.data_as(C.POINTER(C.c_uint8)), row_major, _p(card if len(card) else np.zeros(1, np.int32), C.c_int32),
            len(tables), _p(scope_off, C.c_int64), _p(sc, C.c_int32), _p(counts_off, C.c_int64), _p(counts, C.c_int64)))
        return [counts[a:b].reshape([int(card[c]) for c in t]) for t, a, b in zip(tables, counts_off[:-1], counts_off[1:])]
