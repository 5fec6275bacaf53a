"""The event frames shared by the tests of mpe_frame, sample_frame and evidence_proba.  The wide one has more evidence columns
than a 64-bit pattern mask has bits (the frame methods group rows by their pattern of observed columns).

A binary chain of 70 variables (netspec.grid_spec with one row: every table has at most 4 cells) in which P(010 = 1 | 009 = 0) is
set to 0, and a frame of 12 rows over all 70 columns with 3 patterns of missing cells, interleaved so that pattern order is not
row order.  Row OUT_OF_DOMAIN_ROW has a label outside its domain, row ZERO_ROW has probability zero; every other row has positive
probability.

`asia_frame` is the narrow companion: 5 evidence columns of the Asia example, 8 rows, 6 patterns, one label outside its domain."""
import functools

import numpy as np
import pandas as pd

import mpe_check as mc
import netspec
import sorobn_amd

N_VARS = 70
COLS = [f"{c:03d}" for c in range(N_VARS)]
# columns missing in pattern 0, 1, 2 (they differ above and below bit 62 of the packed mask) and the pattern of every row
MISSING = [[], [5, 33, 64, 65, 66, 67, 68, 69], [0, *range(20, 31)]]
ROW_PATTERN = [2, 0, 1, 0, 2, 1, 1, 0, 2, 0, 1, 2]
OUT_OF_DOMAIN_ROW, ZERO_ROW = 4, 7


def wide_spec():
    spec = netspec.grid_spec(1, N_VARS, 2, seed=70, name="chain70")
    rows = spec["cpts"]["010"]["rows"]  # [009, 010, p] in C-order: rows 0 and 1 are 009 = 0
    assert rows[0][:2] == [0, 0] and rows[1][:2] == [0, 1]
    rows[0][-1], rows[1][-1] = 1.0, 0.0
    return spec


@functools.lru_cache(maxsize=None)
def wide_net():
    """(BayesNet on device 0, its FlatNetwork), built once per process."""
    bn = netspec.build(wide_spec(), sorobn_amd.BayesNet).use_device(0)
    return bn, mc.flat_of(bn)


def wide_frame():
    rng = np.random.default_rng(12)
    data = rng.integers(0, 2, size=(len(ROW_PATTERN), N_VARS)).astype(object)
    data[:, 10] = np.where(data[:, 9] == 0, 0, data[:, 10])  # (no row but ZERO_ROW meets the zero of the CPT of 010)
    data[ZERO_ROW, 9], data[ZERO_ROW, 10] = 0, 1
    data[OUT_OF_DOMAIN_ROW, 50] = 7
    for r, p in enumerate(ROW_PATTERN):
        data[r, MISSING[p]] = None
    data[2, 5] = np.nan  # (NaN and None both mean "not observed")
    assert ROW_PATTERN[ZERO_ROW] == 0 and 50 not in MISSING[ROW_PATTERN[OUT_OF_DOMAIN_ROW]]
    return pd.DataFrame(data, columns=COLS, index=pd.RangeIndex(100, 100 + len(data)), dtype=object)


def asia_frame():
    return pd.DataFrame({"Smoker": [True, None, False, True, None, "maybe", True, False],
                         "Visit to Asia": [None, True, False, None, None, True, True, None],
                         "Dispnea": [True, True, None, False, None, True, None, False],
                         "Positive X-ray": [None, None, True, True, None, False, True, None],
                         "TB or cancer": [None, False, None, None, None, None, None, None]}, dtype=object, index=list("abcdefgh"))


def row_event(row):
    """A frame row -> the event dict of its observed cells."""
    return {c: v for c, v in row.items() if not pd.isna(v)}
