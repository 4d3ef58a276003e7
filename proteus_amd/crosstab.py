"""The per-tile cross-tabulation of include/dswx_hip.h ("crosstab") stated in numpy.

A and B are two arrays of one shape; B is uint8, A of any histogram kind.  A `Spec` holds A's binning (a_kind, a_lo,
a_shift: proteus_amd/histogram.py), col_bits (0 .. 8: C = 1 << col_bits columns, R = 256 >> col_bits rows) and two tables of
256 bytes.  For the pair (x, y) = (A[i], B[i]):

    bin = histogram.bin_of(x)                    (-1: not counted)
    row = row_of_bin[bin], col = col_of_byte[y]
    counted in cells[row * C + col] iff bin >= 0, row < R and col < C

One record is uint64 [256].  This module calls neither dswx_crosstab_host nor the device: the tests pin the three to each
other (and to np.histogram2d).  The helpers below build the tables (`classes`, `fold`, `WTR_CLASSES`) and read a square
table (`agreement`).
"""
import numpy as np

from . import histogram as _h

CELLS = 256
MAX_PAIRS = 6                                     # DSWX_CROSSTAB_MAX_PAIRS: pairs of one dswx_batch_crosstab call
NOT_COUNTED = 255                                 # a table entry past every row count below 256 and every column count below 256
IDENTITY = np.arange(256, dtype=np.uint8)
ZEROS = np.zeros(256, dtype=np.uint8)
WTR_VALUES = (0, 1, 2, 252, 253, 254, 255)        # not water, open water, partial surface water, snow, cloud, ocean, fill


def _table(t, what):
    t = np.asarray(t)
    if t.shape != (256,) or t.dtype.kind not in 'iub' or np.any(t < 0) or np.any(t > 255):
        raise ValueError(f'{what} is 256 values of 0 .. 255')
    return np.ascontiguousarray(t.astype(np.uint8))


class Spec:
    """dswx_crosstab_spec_t: how A is binned, how many columns there are, and the two tables."""

    def __init__(self, a_kind=_h.HIST_U8, a_lo=0, a_shift=0, col_bits=4, row_of_bin=IDENTITY, col_of_byte=IDENTITY):
        self.a_kind, self.a_lo, self.a_shift = _h.check(_h.DTYPES.get(a_kind, np.uint8), a_kind, a_lo, a_shift)
        self.col_bits = int(col_bits)
        if not 0 <= self.col_bits <= 8:
            raise ValueError(f'col_bits {col_bits} outside 0 .. 8')
        self.row_of_bin, self.col_of_byte = _table(row_of_bin, 'row_of_bin'), _table(col_of_byte, 'col_of_byte')

    n_cols = property(lambda self: 1 << self.col_bits)
    n_rows = property(lambda self: 256 >> self.col_bits)

    def table(self, record):
        """A record (or [..., 256] records) as [..., n_rows, n_cols]."""
        record = np.asarray(record)
        return record.reshape(record.shape[:-1] + (self.n_rows, self.n_cols))

    def __repr__(self):
        return f'Spec(a_kind={self.a_kind}, a_lo={self.a_lo}, a_shift={self.a_shift}, col_bits={self.col_bits})'


def cell_of(a, b, spec):
    """int64 array of the shape of `a`: the cell of every pair, -1 where it is not counted."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError(f'{a.shape} against {b.shape}')
    if b.dtype != np.uint8 and b.dtype != np.bool_:
        raise ValueError(f'plane b is uint8, not {b.dtype}')
    bin_ = _h.bin_of(a, spec.a_kind, spec.a_lo, spec.a_shift)
    row = spec.row_of_bin.astype(np.int64)[np.maximum(bin_, 0)]
    col = spec.col_of_byte.astype(np.int64)[b.astype(np.uint8)]
    counted = (bin_ >= 0) & (row < spec.n_rows) & (col < spec.n_cols)
    return np.where(counted, row * spec.n_cols + col, -1)


def crosstab(a, b, spec):
    """uint64 [256]: the record of one tile."""
    c = cell_of(a, b, spec).reshape(-1)
    return np.bincount(c[c >= 0], minlength=CELLS).astype(np.uint64)


def crosstab_tiles(a, b, spec):
    """uint64 [n_tiles, 256]: the record of every tile pair (a[t], b[t])."""
    if len(a) != len(b):
        raise ValueError(f'{len(a)} tiles against {len(b)}')
    out = np.zeros((len(a), CELLS), dtype=np.uint64)
    for t in range(len(a)):
        out[t] = crosstab(a[t], b[t], spec)
    return out


def classes(values, other=None):
    """A table (uint8 [256]) that sends the listed byte values to 0 .. k - 1 in their order and every other value to
    `other` (a class index), or to NOT_COUNTED when None."""
    values = [int(v) for v in values]
    if len(set(values)) != len(values) or any(not 0 <= v <= 255 for v in values):
        raise ValueError('classes: distinct byte values')
    if len(values) > (255 if other is None else 256):
        raise ValueError('classes: too many values')
    if other is not None and not 0 <= int(other) <= 255:
        raise ValueError('classes: other is a class index 0 .. 255')
    t = np.full(256, NOT_COUNTED if other is None else int(other), dtype=np.uint8)
    t[values] = np.arange(len(values), dtype=np.uint8)
    return t


def fold(n_rows):
    """A row table (uint8 [256]) that folds the 256 linear bins of a band into n_rows rows of 256 / n_rows bins each
    (n_rows a power of two)."""
    n_rows = int(n_rows)
    if n_rows < 1 or n_rows > 256 or n_rows & (n_rows - 1):
        raise ValueError(f'fold: {n_rows} rows is not a power of two up to 256')
    return (np.arange(256) // (256 // n_rows)).astype(np.uint8)


def _wtr_classes():
    """WTR_VALUES against WTR_VALUES: 8 columns (col_bits 3), rows and columns 0 .. 6 in the order of WTR_VALUES, every other
    value in class 7."""
    t = classes(WTR_VALUES, other=len(WTR_VALUES))
    return Spec(_h.HIST_U8, col_bits=3, row_of_bin=t, col_of_byte=t)


WTR_CLASSES = _wtr_classes()


def agreement(table):
    """A square table [k, k] of counts (rows one classification, columns the other) -> dict: 'n' (pairs), 'overall' (the
    diagonal's share), 'row' and 'col' (float64 [k]: the diagonal over the row / column sum, NaN for an empty one) and
    'kappa' (Cohen's: (po - pe) / (1 - pe); NaN when pe is 1 or the table is empty).  Host arithmetic on 256 numbers."""
    t = np.asarray(table).astype(np.float64)
    if t.ndim != 2 or t.shape[0] != t.shape[1]:
        raise ValueError(f'agreement: a square table, not {t.shape}')
    n = t.sum()
    diag, rows, cols = np.diag(t), t.sum(axis=1), t.sum(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        po = diag.sum() / n if n else np.nan
        pe = float((rows * cols).sum() / (n * n)) if n else np.nan
        kappa = (po - pe) / (1.0 - pe) if n and pe != 1.0 else np.nan
        return {'n': int(np.asarray(table).sum()), 'overall': float(po), 'row': diag / rows, 'col': diag / cols,
                'kappa': float(kappa)}
