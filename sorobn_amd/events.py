"""Frames of partial events, host side: what `query_frame`, `mpe_frame`, `sample_frame` and `evidence_proba` share.

Row r of an events frame is an event: its columns are evidence variables, NaN / None = not observed in that row.  The columns are
encoded once (`encode_frame`), rows with the same pattern of observed columns go to the engine together (`pattern_groups`,
`iter_parts`, `part_args`), and a matrix of codes comes back as label columns (`decode_labels`)."""
import numpy as np
import pandas as pd

# the widest frame whose pattern of observed columns packs into an int64 bit mask
MASK_COLUMNS = 62


def encode_frame(be, cols, frame):
    """Backend, evidence column names, DataFrame -> (ev_ids int32 [n_cols], codes int32 [n, n_cols], observed bool [n, n_cols]).
    A label outside its domain has code -1, an empty domain gives -1 throughout; an unknown name raises KeyError(name)."""
    f = be.flat
    ev_ids = np.array([be.var_id(c) for c in cols], np.int32)
    codes = np.empty((len(frame), len(cols)), np.int32)
    observed = np.empty((len(frame), len(cols)), bool)
    for j, c in enumerate(cols):
        col = frame[c]
        observed[:, j] = col.notna().to_numpy()
        codes[:, j] = pd.Index(f.domains[ev_ids[j]]).get_indexer(col) if len(f.domains[ev_ids[j]]) else -1
    return ev_ids, codes, observed


def pattern_groups(observed, wide_by_row=False):
    """observed [n, n_cols] bool -> list of row-index arrays, one per pattern of observed columns: groups in ascending order of
    the packed bit mask (column j is bit j), rows ascending within a group.  No columns: one group of all rows.  Beyond
    MASK_COLUMNS the mask order is the lexicographic order of the reversed columns; with `wide_by_row` such a frame gives one
    group per row, in row order, instead."""
    n, n_cols = observed.shape
    if n_cols == 0:
        return [np.arange(n)]
    if n_cols > MASK_COLUMNS and wide_by_row:
        return [np.array([r]) for r in range(n)]
    if n_cols <= MASK_COLUMNS:
        pat = observed @ (1 << np.arange(n_cols, dtype=np.int64))
    else:
        pat = np.asarray(np.unique(observed[:, ::-1], axis=0, return_inverse=True)[1]).reshape(-1)
    return [np.flatnonzero(pat == p) for p in np.unique(pat)]


def iter_parts(groups, observed, sub_batch):
    """(part, on) for every engine call: `part` the rows of one group, at most `sub_batch` of them (None: the whole group), `on`
    the columns those rows observe."""
    for rows in groups:
        if not len(rows):
            continue
        on = np.flatnonzero(observed[rows[0]])
        step = len(rows) if sub_batch is None else sub_batch
        for s in range(0, len(rows), step):
            yield rows[s:s + step], on


def part_args(ev_ids, codes, part, on):
    """The fixed-shape evidence of one part: (evars, ecodes), both [len(part), len(on)]."""
    return np.broadcast_to(ev_ids[on], (len(part), len(on))), codes[np.ix_(part, on)]


def csr_rows(ev_ids, codes, observed):
    """One request per row, in row order, as CSR evidence: (e_off int64 [n + 1], e_vars, e_codes) - the observed columns of every
    row, in column order.  For the calls whose requests need not share a shape (belief propagation)."""
    e_off = np.zeros(len(codes) + 1, np.int64)
    np.cumsum(observed.sum(axis=1), out=e_off[1:])
    return e_off, np.broadcast_to(ev_ids, observed.shape)[observed].astype(np.int32), codes[observed].astype(np.int32)


def label_table(f, v):
    """Labels of variable v by code, with None at index -1 (code -1 = no answer)."""
    dom = np.empty(int(f.card[v]) + 1, dtype=object)
    dom[:-1] = list(f.domains[v])
    dom[-1] = None
    return dom


def decode_labels(f, names, out, given, n=1):
    """Codes out [rows, n_vars] int32 -> {name: object column of labels} in the order of `names`; code -1 gives None.  `given`
    is the evidence the rows were computed from - an events frame with rows / n rows, row r of it behind rows r * n .. r * n + n - 1
    of `out`, or one event dict behind every row - and observed evidence keeps its given label, also where that lies outside the
    domain."""
    data = {}
    for name in names:
        v = f.id[name]
        col = label_table(f, v)[out[:, v]]
        if name in given:
            if isinstance(given, dict):
                labels = np.empty(len(col), dtype=object)
                labels[:] = [given[name]] * len(col)
                obs = np.ones(len(col), bool)
            else:
                labels = np.repeat(given[name].to_numpy(dtype=object), n)
                obs = np.repeat(given[name].notna().to_numpy(), n)
            col[obs] = labels[obs]
        data[name] = col
    return data
