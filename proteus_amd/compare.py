"""The per-tile comparison of include/dswx_hip.h ("compare") stated in numpy.

Two arrays of one element kind (uint8, uint16, int16, float32, float64).  A pair (x, y) is CLOSE when numpy's
isclose(a, b, rtol, atol, equal_nan) says so; spelled out here operation by operation, so that the statement does not move
with numpy's promotion rules:

    integers   |x - y| <= atol + rtol |y| in float64
    float64    the same
    float32    atol, rtol rounded to float32; one float32 subtraction, one float32 multiply, one float32 add
    floats     d <= tol needs a finite y; x == y is close (equal infinities, -0 / +0); NaN / NaN is close iff equal_nan

The record: n_diff (pairs that are not close), first (the smallest flat index of one, -1 if none), max_abs_diff (the maximum
of |float64(x) - float64(y)| over the not-close pairs without a NaN; 0.0 if there is none).  This module calls neither
dswx_compare_host nor the device: the tests pin the three to each other (and to np.isclose).
"""
import numpy as np

RECORD = np.dtype([('n_diff', '<i8'), ('first', '<i8'), ('max_abs_diff', '<f8'), ('reserved', '<u8')])
KINDS = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.int16): 2, np.dtype(np.float32): 3,
         np.dtype(np.float64): 4}


def kind_of(dtype):
    """The DSWX_CMP_* value of a dtype."""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        dt = np.dtype(np.uint8)
    if dt.newbyteorder('=') not in KINDS:
        raise ValueError(f'no comparison for {dt} planes (uint8, uint16, int16, float32, float64)')
    return KINDS[dt.newbyteorder('=')]


def check_tolerances(atol, rtol):
    atol, rtol = float(atol), float(rtol)
    if not (np.isfinite(atol) and np.isfinite(rtol) and atol >= 0 and rtol >= 0):
        raise ValueError(f'atol and rtol must be finite and not negative (atol {atol}, rtol {rtol})')
    return atol, rtol


def not_close(a, b, atol=0.0, rtol=0.0, equal_nan=True):
    """bool array: the pairs that are NOT close.  a, b: arrays of one kind and one shape."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        raise ValueError(f'{a.dtype} {a.shape} against {b.dtype} {b.shape}')
    kind_of(a.dtype)
    atol, rtol = check_tolerances(atol, rtol)
    ft = np.float32 if a.dtype == np.float32 else np.float64
    x, y = a.astype(ft, copy=False), b.astype(ft, copy=False)
    with np.errstate(all='ignore'):
        d = np.abs(np.subtract(x, y, dtype=ft))
        tol = np.add(ft(atol), np.multiply(ft(rtol), np.abs(y), dtype=ft), dtype=ft)
        close = ((d <= tol) & np.isfinite(y)) | (x == y)
        if equal_nan:
            close |= np.isnan(x) & np.isnan(y)
    return ~close


def compare(a, b, atol=0.0, rtol=0.0, equal_nan=True):
    """The record (numpy scalar of dtype RECORD) of one tile: a and b taken in C order."""
    a, b = np.asarray(a), np.asarray(b)
    bad = not_close(a, b, atol, rtol, equal_nan).reshape(-1)
    rec = np.zeros((), dtype=RECORD)
    idx = np.flatnonzero(bad)
    rec['n_diff'] = idx.size
    rec['first'] = idx[0] if idx.size else -1
    if idx.size:
        x = a.reshape(-1)[idx].astype(np.float64)
        y = b.reshape(-1)[idx].astype(np.float64)
        ok = ~(np.isnan(x) | np.isnan(y))
        if ok.any():
            with np.errstate(all='ignore'):
                rec['max_abs_diff'] = np.abs(x[ok] - y[ok]).max()
    return rec[()]


def compare_tiles(a, b, atol=0.0, rtol=0.0, equal_nan=True):
    """RECORD [n_tiles]: the record of every tile pair (a[t], b[t]) of two arrays [n_tiles, ...]."""
    if len(a) != len(b):
        raise ValueError(f'{len(a)} tiles against {len(b)}')
    out = np.zeros(len(a), dtype=RECORD)
    for t in range(len(a)):
        out[t] = compare(a[t], b[t], atol, rtol, equal_nan)
    return out
