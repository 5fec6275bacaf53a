"""The host layer under query_frame, mpe_frame, sample_frame and evidence_proba (sorobn_amd/events.py) without a device: the
pattern groups against brute force, the exact sequence of engine calls the three frame methods make (a recording engine in place
of the simulator's), and the decoder of code matrices."""
import numpy as np
import pandas as pd
import pytest

import golden_util as gu
import netspec
import simengine
import sorobn_amd
import event_frames as we
from sorobn_amd import _capi, events


# ---- pattern groups ---------------------------------------------------------------------------------------------------------------

def _observed_cases():
    """(observed, tag): 0, 1, 5, 62, 63 and 70 columns, 0 - 200 rows, few distinct patterns (rows drawn from 3 patterns) and many
    (independent cells)."""
    rng = np.random.default_rng(63)
    for n_cols in (0, 1, 5, 62, 63, 70):
        for n in (0, 1, 7, 200):
            many = rng.random((n, n_cols)) < 0.5
            basis = rng.random((3, n_cols)) < 0.5
            few = basis[rng.integers(0, 3, n)]
            yield many, f"{n_cols} columns, {n} rows, many"
            yield few, f"{n_cols} columns, {n} rows, few"


def _lists(groups):
    return [np.asarray(g).tolist() for g in groups]


def test_pattern_groups_against_brute_force():
    n_wide = n_narrow = 0
    for observed, tag in _observed_cases():
        n, n_cols = observed.shape
        groups = _lists(events.pattern_groups(observed))
        assert sorted(r for g in groups for r in g) == list(range(n)), tag  # a partition of the rows
        assert all(g for g in groups) or n_cols == 0, tag
        if n_cols == 0:
            assert groups == [list(range(n))], tag
        elif n_cols < 63:
            pat = observed @ (1 << np.arange(n_cols, dtype=np.int64))
            assert groups == [np.flatnonzero(pat == p).tolist() for p in np.unique(pat)], tag
            n_narrow += 1
        else:
            mask = [sum(1 << j for j in range(n_cols) if observed[r, j]) for r in range(n)]  # (Python integers: no 64-bit limit)
            of_group = [mask[g[0]] for g in groups]
            assert all(mask[r] == m for g, m in zip(groups, of_group) for r in g), tag
            assert all(a < b for a, b in zip(of_group, of_group[1:])), tag  # ascending mask, every pattern once
            assert all(g == sorted(g) for g in groups), tag
            n_wide += 1
        by_row = _lists(events.pattern_groups(observed, wide_by_row=True))
        assert by_row == ([[r] for r in range(n)] if n_cols >= 63 else groups), tag
    assert n_narrow >= 24 and n_wide >= 16


def test_iter_parts_cuts_groups_and_names_the_observed_columns():
    observed = np.array([[1, 0, 1], [0, 0, 0], [1, 0, 1], [1, 0, 1], [0, 0, 0]], bool)
    groups = events.pattern_groups(observed)
    got = [(p.tolist(), on.tolist()) for p, on in events.iter_parts(groups, observed, 2)]
    assert got == [([1, 4], []), ([0, 2], [0, 2]), ([3], [0, 2])]
    whole = [(p.tolist(), on.tolist()) for p, on in events.iter_parts(groups, observed, None)]
    assert whole == [([1, 4], []), ([0, 2, 3], [0, 2])]
    assert list(events.iter_parts(events.pattern_groups(np.zeros((0, 0), bool)), np.zeros((0, 0), bool), 4)) == []


# ---- the engine calls of the three frame methods ----------------------------------------------------------------------------------

class Recorder:
    """In place of an engine's `mpe`, `posterior_sample_batch` and `query_fixed`: keeps every call's arguments as lists and
    returns zeros of the shape the engine returns."""

    def __init__(self, backend):
        self.calls = []
        self.n_vars = len(backend.flat.card)
        self.card = backend.flat.card
        eng = backend.engine
        eng.mpe, eng.posterior_sample_batch, eng.query_fixed = self.mpe, self.posterior_sample_batch, self.query_fixed

    @staticmethod
    def _l(a):
        return np.asarray(a).tolist()

    def mpe(self, evars, ecodes):
        self.calls.append(("mpe", self._l(evars), self._l(ecodes)))
        return np.zeros((len(evars), self.n_vars), np.int32), np.zeros(len(evars))

    def posterior_sample_batch(self, e_off, e_vars, e_codes, s_off, seed=0, flags=0):
        self.calls.append(("draw", self._l(e_vars), self._l(e_codes), self._l(e_off), self._l(s_off), seed, flags))
        return np.zeros((int(s_off[-1] - s_off[0]), self.n_vars), np.int32), np.ones(len(e_off) - 1)

    def query_fixed(self, qvars, evars, ecodes, flags=0):
        self.calls.append(("query", self._l(qvars), self._l(evars), self._l(ecodes), flags))
        cells = int(np.prod(self.card[np.asarray(qvars)[0]])) if np.asarray(qvars).size else 1
        return np.zeros((len(qvars), cells))


@pytest.fixture()
def asia():
    spec = next(e["spec"] for e in gu.load("examples.json") if e["spec"]["name"] == "asia")
    bn = netspec.build(spec, sorobn_amd.BayesNet)
    bn._backend = simengine.sim_backend(bn)
    return bn, Recorder(bn._backend)


# 8 rows, three patterns over (Smoker = bit 0, Dispnea = bit 1, Positive X-ray = bit 2): mask 3 in rows 0, 2, 3, 5, 7, mask 4 in rows
# 1, 6 and mask 5 in row 4; "maybe" is outside the domain (code -1), the domains are [False, True]
NARROW = pd.DataFrame({"Smoker": [True, None, False, True, False, "maybe", None, True],
                       "Dispnea": [False, None, True, True, np.nan, False, None, True],
                       "Positive X-ray": [None, True, None, None, True, None, False, None]}, dtype=object,
                      index=list("abcdefgh"))


def test_narrow_frame_call_sequence(asia):
    bn, rec = asia
    f = bn.backend.flat
    S, D, X = f.id["Smoker"], f.id["Dispnea"], f.id["Positive X-ray"]
    assert bn._cpts_are_distributions(bn.backend)

    bn.mpe_frame(NARROW, sub_batch=3)
    assert rec.calls == [("mpe", [[S, D]] * 3, [[1, 0], [0, 1], [1, 1]]),   # rows 0, 2, 3
                         ("mpe", [[S, D]] * 2, [[-1, 0], [1, 1]]),          # rows 5, 7
                         ("mpe", [[X]] * 2, [[1], [0]]),                    # rows 1, 6
                         ("mpe", [[S, X]], [[0, 1]])]                       # row 4

    rec.calls.clear()
    bn.sample_frame(NARROW, n=2, seed=7, sub_batch=3)
    P = _capi.DRAW_PRUNE
    assert rec.calls == [("draw", [S, D] * 3, [1, 0, 0, 1, 1, 1], [0, 2, 4, 6], [0, 2, 4, 6], 7, P),
                         ("draw", [S, D] * 2, [-1, 0, 1, 1], [0, 2, 4], [6, 8, 10], 7, P),
                         ("draw", [X] * 2, [1, 0], [0, 1, 2], [10, 12, 14], 7, P),  # (s_off goes on across the groups)
                         ("draw", [S, X], [0, 1], [0, 2], [14, 16], 7, P)]

    rec.calls.clear()
    B = f.id["Bronchitis"]
    bn.query_frame("Bronchitis", events=NARROW)
    assert rec.calls == [("query", [[B]] * 5, [[S, D]] * 5, [[1, 0], [0, 1], [1, 1], [-1, 0], [1, 1]], 0),  # one call per group
                         ("query", [[B]] * 2, [[X]] * 2, [[1], [0]], 0),
                         ("query", [[B]], [[S, X]], [[0, 1]], 0)]


@pytest.fixture()
def chain70():
    bn = netspec.build(we.wide_spec(), sorobn_amd.BayesNet)
    bn._backend = simengine.sim_backend(bn)
    return bn, Recorder(bn._backend)


def _wide_frame_of_two_patterns():
    """8 rows over the 70 columns: rows 1, 4 and 6 miss column 69 (a bit no int64 mask has), the others miss column 0 - so the
    pattern of rows 1, 4, 6 has the lower mask."""
    data = np.ones((8, we.N_VARS), np.int64).astype(object)
    late = [1, 4, 6]
    early = [r for r in range(8) if r not in late]
    data[late, 69] = None
    data[early, 0] = None
    return pd.DataFrame(data, columns=we.COLS, dtype=object), late, early


def test_wide_frame_mpe_makes_one_call_per_pattern(chain70):
    bn, rec = chain70
    f = bn.backend.flat
    frame, late, early = _wide_frame_of_two_patterns()
    ids = [f.id[c] for c in we.COLS]
    bn.mpe_frame(frame)
    assert rec.calls == [("mpe", [ids[:69]] * 3, [[1] * 69] * 3), ("mpe", [ids[1:]] * 5, [[1] * 69] * 5)]
    rec.calls.clear()
    bn.query_frame("035", events=frame.drop(columns=["035"]))
    assert [(c[0], len(c[1])) for c in rec.calls] == [("query", 3), ("query", 5)]
    rec.calls.clear()
    bn.evidence_proba(frame)
    assert [(c[0], len(c[1])) for c in rec.calls] == [("query", 3), ("query", 5)]


def test_wide_frame_samples_row_by_row(chain70):
    """A seed of sample_frame means the frame it gave when 63 or more columns went to the engine one row per call."""
    bn, rec = chain70
    f = bn.backend.flat
    frame, late, early = _wide_frame_of_two_patterns()
    ids = [f.id[c] for c in we.COLS]
    assert bn._cpts_are_distributions(bn.backend)
    bn.sample_frame(frame, n=3, seed=5)
    want = [("draw", ids[:69] if r in late else ids[1:], [1] * 69, [0, 69], [3 * r, 3 * r + 3], 5, _capi.DRAW_PRUNE) for r in range(8)]
    assert rec.calls == want


# ---- the decoder ------------------------------------------------------------------------------------------------------------------

def test_decode_labels(asia):
    bn, _ = asia
    f = bn.backend.flat
    names = bn._all_names()
    S, D = f.id["Smoker"], f.id["Dispnea"]
    given = pd.DataFrame({"Smoker": [True, "maybe", None]}, dtype=object)
    out = np.zeros((6, len(f.card)), np.int32)  # 3 events, n = 2: rows 2 r and 2 r + 1 belong to event r
    out[:, D] = [0, 1, -1, -1, 1, 0]
    out[:, S] = [1, 1, -1, -1, 0, 1]
    data = events.decode_labels(f, names, out, given, 2)
    assert list(data) == names and all(col.dtype == object and len(col) == 6 for col in data.values())
    assert data["Dispnea"].tolist() == [False, True, None, None, True, False]        # code -1 -> None
    assert data["Smoker"].tolist() == [True, True, "maybe", "maybe", False, True]    # given labels kept, verbatim; else decoded
    assert data["Bronchitis"].tolist() == [False] * 6
    one = events.decode_labels(f, names, out[2:3], {"Smoker": "maybe", "Dispnea": None})
    assert one["Smoker"].tolist() == ["maybe"] and one["Dispnea"].tolist() == [None] and one["Bronchitis"].tolist() == [False]
    many = events.decode_labels(f, names, out, {"Smoker": (1, 2)}, 6)
    assert many["Smoker"].tolist() == [(1, 2)] * 6 and many["Dispnea"].tolist() == data["Dispnea"].tolist()


def test_encode_frame(asia):
    bn, _ = asia
    be = bn.backend
    ev_ids, codes, observed = events.encode_frame(be, list(NARROW.columns), NARROW)
    assert ev_ids.dtype == np.int32 and codes.dtype == np.int32 and observed.dtype == bool
    assert ev_ids.tolist() == [be.flat.id[c] for c in NARROW.columns]
    assert observed.tolist() == NARROW.notna().to_numpy().tolist()
    assert codes[observed].tolist() == [1, 0, 1, 0, 1, 1, 1, 0, 1, -1, 0, 0, 1, 1]
    with pytest.raises(KeyError):
        events.encode_frame(be, ["Nope"], pd.DataFrame({"Nope": [1]}))
