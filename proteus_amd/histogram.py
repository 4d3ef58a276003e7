"""The per-tile histogram of include/dswx_hip.h ("histogram") stated in numpy.

One record is uint64 [256].  The bin of an element follows the kind of its plane:

    HIST_U8             bin = the byte
    HIST_U16, HIST_I16  d = int(v) - lo; counted in bin d >> shift when 0 <= d < (256 << shift), otherwise NOT counted
    HIST_DIAG           uint16 in the saved DIAG form (the decimal digits are the five test bits): every digit 0 or 1 and
                        v <= 11111 -> d0 + 2 d1 + 4 d2 + 8 d3 + 16 d4; 65535 (nodata) -> 32; anything else -> 33

`bin_of` returns -1 for an element that is not counted.  This module calls neither dswx_histogram_host nor the device: the
tests pin the three to each other (and to np.bincount).
"""
import numpy as np

BINS = 256
HIST_U8, HIST_U16, HIST_I16, HIST_DIAG = range(4)
KINDS = {np.dtype(np.uint8): HIST_U8, np.dtype(np.uint16): HIST_U16, np.dtype(np.int16): HIST_I16}
DTYPES = {HIST_U8: np.dtype(np.uint8), HIST_U16: np.dtype(np.uint16), HIST_I16: np.dtype(np.int16),
          HIST_DIAG: np.dtype(np.uint16)}
DIAG_NODATA_BIN, DIAG_OTHER_BIN = 32, 33


def kind_of(dtype):
    """The DSWX_HIST_* value a dtype is binned with when none is named (uint16 is linear: name HIST_DIAG for a DIAG plane)."""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        dt = np.dtype(np.uint8)
    if dt.newbyteorder('=') not in KINDS:
        raise ValueError(f'no histogram for {dt} planes (uint8, uint16, int16)')
    return KINDS[dt.newbyteorder('=')]


def check(dtype, kind, lo, shift):
    """(kind, lo, shift) as the entries take them: the kind from the dtype when None, and matching it otherwise."""
    kind = kind_of(dtype) if kind is None else int(kind)
    if kind not in DTYPES:
        raise ValueError(f'kind {kind} is not a HIST_* value')
    dt = np.dtype(dtype)
    if (np.dtype(np.uint8) if dt == np.bool_ else dt.newbyteorder('=')) != DTYPES[kind]:
        raise ValueError(f'kind {kind} bins {DTYPES[kind]} planes, not {dt}')
    lo, shift = int(lo), int(shift)
    if not 0 <= shift <= 8:
        raise ValueError(f'shift {shift} outside 0 .. 8')
    if not -2 ** 31 <= lo < 2 ** 31:
        raise ValueError(f'lo {lo} is not an int32')
    return kind, lo, shift


def bin_of(a, kind=None, lo=0, shift=0):
    """int64 array of the shape of `a`: the bin of every element, -1 where it is not counted."""
    a = np.asarray(a)
    kind, lo, shift = check(a.dtype, kind, lo, shift)
    v = a.astype(np.int64)
    if kind == HIST_U8:
        return v
    if kind == HIST_DIAG:
        digits = [(v // 10 ** k) % 10 for k in range(5)]
        binary = np.all([d <= 1 for d in digits], axis=0) & (v <= 11111)
        pattern = sum(d << k for k, d in enumerate(digits))
        return np.where(v == 65535, DIAG_NODATA_BIN, np.where(binary, pattern, DIAG_OTHER_BIN))
    d = v - lo
    return np.where((d >= 0) & (d < (256 << shift)), d >> shift, -1)


def histogram(a, kind=None, lo=0, shift=0):
    """uint64 [256]: the record of one tile."""
    b = bin_of(a, kind, lo, shift).reshape(-1)
    return np.bincount(b[b >= 0], minlength=BINS).astype(np.uint64)


def histogram_tiles(a, kind=None, lo=0, shift=0):
    """uint64 [n_tiles, 256]: the record of every tile a[t] of an array [n_tiles, ...]."""
    out = np.zeros((len(a), BINS), dtype=np.uint64)
    for t in range(len(a)):
        out[t] = histogram(a[t], kind, lo, shift)
    return out
