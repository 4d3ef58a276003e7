"""The per-tile comparison of include/dswx_hip.h ("compare") without a GPU: the rule as a scalar loop written here, pinned
to np.isclose of the installed numpy, to the numpy statement (proteus_amd/compare.py) and to the library's scalar statement
(dswx_compare_host) on inputs aimed at the boundary of the rule; the properties the header promises; every error path of the
three entries that needs no device; the header's macro; the C example."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.compare import RECORD, compare, compare_tiles, kind_of, not_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (np.uint8, np.uint16, np.int16, np.float32, np.float64)
# (atol, rtol): equality, np.allclose's defaults with the product's atol, each alone, integer-sized ones, a float32 product
# that overflows, tolerances below the float32 denormals
TOLERANCES = ((0.0, 0.0), (1e-6, 1e-5), (1e-6, 0.0), (0.0, 1e-5), (3.0, 0.0), (2.5, 0.01), (1.0, 0.5), (1e-46, 0.0),
              (1e-40, 1e-3), (1e30, 1e30))


# ---- the rule, written out again: one pair at a time ---------------------------------------------------------------
def scalar_close(x, y, dtype, atol, rtol, equal_nan):
    if np.dtype(dtype) == np.float32:
        f = np.float32
        x, y, at, rt = f(x), f(y), f(atol), f(rtol)                     # the tolerances rounded to float32 first
        if x == y:
            return True
        if np.isnan(x) or np.isnan(y):
            return bool(equal_nan and np.isnan(x) and np.isnan(y))
        d = abs(f(x - y))                                               # one float32 subtraction
        tol = f(at + f(rt * abs(y)))                                    # a float32 multiply, then a float32 add
        return bool(d <= tol and np.isfinite(y))
    x, y = float(x), float(y)                                           # integers convert exactly
    if x == y:
        return True
    if math.isnan(x) or math.isnan(y):
        return bool(equal_nan and math.isnan(x) and math.isnan(y))
    if math.isinf(x) and math.isinf(y):
        return False                                                    # inf - (-inf): d = inf, y not finite
    return abs(x - y) <= atol + rtol * abs(y) and math.isfinite(y)


def scalar_compare(a, b, atol, rtol, equal_nan):
    """(n_diff, first, max_abs_diff) and the not-close flags, by the loop."""
    n, first, mx, flags = 0, -1, 0.0, []
    with np.errstate(all='ignore'):
        for i, (x, y) in enumerate(zip(a.tolist() if a.dtype != np.float32 else list(a),
                                       b.tolist() if b.dtype != np.float32 else list(b))):
            bad = not scalar_close(x, y, a.dtype, atol, rtol, equal_nan)
            flags.append(bad)
            if bad:
                n += 1
                first = i if first < 0 else first
                fx, fy = float(x), float(y)
                if not (math.isnan(fx) or math.isnan(fy)):
                    mx = max(mx, abs(fx - fy))
    return (n, first, mx), np.array(flags, dtype=bool)


def as_tuple(rec):
    assert int(rec['reserved']) == 0
    return int(rec['n_diff']), int(rec['first']), float(rec['max_abs_diff'])


# ---- inputs aimed at the boundary ------------------------------------------------------------------------------------
def boundary_pairs(dtype, atol, rtol, rng):
    """(a, b) of `dtype`: differences exactly at atol + rtol |y| and one step (an integer, or an ulp of the type) either
    side of it; the special values of the type; a few random pairs."""
    dt = np.dtype(dtype)
    xs, ys = [], []
    if dt.kind in 'iu':
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        base = sorted({lo, lo + 1, -1 if lo < 0 else 0, 0, 1, 7, 10, 100, 200, hi // 2, hi - 1, hi}
                      | {int(v) for v in rng.integers(lo, hi + 1, size=12)})
        for y in base:
            t = math.floor(atol + rtol * abs(y))
            for sign in (-1, 1):
                for step in (-1, 0, 1):
                    x = y + sign * (min(t, 1 << 20) + step)
                    if lo <= x <= hi:
                        xs.append(x)
                        ys.append(y)
        for x, y in ((lo, hi), (hi, lo), (lo, lo), (hi, hi), (0, hi), (hi, 0)):         # the extremes against each other
            xs.append(x)
            ys.append(y)
        a, b = np.array(xs, dtype=dt), np.array(ys, dtype=dt)
    else:
        f = dt.type
        tiny, big, den = np.finfo(dt).tiny, np.finfo(dt).max, np.nextafter(f(0), f(1))
        base = [f(v) for v in (0.0, -0.0, 1.0, -1.0, 1e-6, 1e-5, 0.1, 3.0, 1000.0, 12345.678, -7e5, 1e20, tiny, -tiny, den, 2 * den,
                               tiny * 3, big, -big)] + [f(v) for v in rng.normal(size=8) * 100]
        with np.errstate(all='ignore'):
            for y in base:
                tol = f(f(atol) + f(f(rtol) * abs(y)))
                for sign in (-1, 1):
                    x0 = f(y + f(sign) * tol)
                    for x in (np.nextafter(x0, f(-np.inf)), x0, np.nextafter(x0, f(np.inf))):
                        xs.append(x)
                        ys.append(y)
                    xs.append(y)                                                      # and the other way round: the rule is
                    ys.append(x0)                                                     # not symmetric (rtol scales |y|)
        nan, inf = f(np.nan), f(np.inf)
        special = [nan, inf, -inf, f(0.0), f(-0.0), f(1.0), den, -den, tiny, big, -big]
        for x in special:
            for y in special:
                xs.append(x)
                ys.append(y)
        a, b = np.array(xs, dtype=dt), np.array(ys, dtype=dt)
    return a, b


@pytest.mark.parametrize('dtype', KINDS, ids=lambda d: np.dtype(d).name)
def test_the_rule_is_numpys_isclose_and_all_statements_agree(dtype):
    rng = np.random.default_rng(8101)
    n_pairs = 0
    for atol, rtol in TOLERANCES:
        a, b = boundary_pairs(dtype, atol, rtol, rng)
        for equal_nan in (True, False):
            want, flags = scalar_compare(a, b, atol, rtol, equal_nan)
            with np.errstate(all='ignore'):
                ref = ~np.isclose(a, b, rtol=rtol, atol=atol, equal_nan=equal_nan)
            assert np.array_equal(flags, ref), (atol, rtol, equal_nan, np.flatnonzero(flags != ref)[:5])
            assert np.array_equal(not_close(a, b, atol, rtol, equal_nan), ref)
            assert as_tuple(compare(a, b, atol, rtol, equal_nan)) == want, (atol, rtol, equal_nan)
            assert as_tuple(_capi.compare_host(a, b, atol, rtol, equal_nan)) == want, (atol, rtol, equal_nan)
            n_pairs += a.size
        if (atol, rtol) != (0.0, 0.0) and np.dtype(dtype).kind == 'f':
            assert flags.any() and not flags.all()                       # both sides of the boundary are in the set
    assert n_pairs > 2000


def test_rtol_atol_zero_is_value_equality():
    rng = np.random.default_rng(8102)
    for dtype in KINDS:
        dt = np.dtype(dtype)
        if dt.kind == 'f':
            a = rng.normal(size=500).astype(dt)
            a[::50] = np.nan
            a[1::50] = np.inf
            a[2::50] = 0.0
        else:
            a = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max + 1, size=500).astype(dt)
        b = a.copy()
        pick = rng.choice(500, size=40, replace=False)
        b[pick] = b[pick][::-1]
        if dt.kind == 'f':
            b[2::50] = -0.0                                               # -0 against +0 is equal
        for equal_nan in (True, False):
            with np.errstate(all='ignore'):
                eq = (a == b) | (np.isnan(a.astype(np.float64)) & np.isnan(b.astype(np.float64)) & equal_nan)
            rec = _capi.compare_host(a, b, 0, 0, equal_nan)
            assert int(rec['n_diff']) == int((~eq).sum())
            assert as_tuple(rec) == as_tuple(compare(a, b, 0, 0, equal_nan))


def _random(dtype, n, rng):
    dt = np.dtype(dtype)
    raw = rng.integers(0, 256, size=n * dt.itemsize, dtype=np.uint8)          # every bit pattern: NaNs, infinities, denormals
    return raw.view(dt)


@pytest.mark.parametrize('dtype', KINDS, ids=lambda d: np.dtype(d).name)
def test_properties_equal_buffers_single_change_and_padding(dtype):
    rng = np.random.default_rng(8103)
    dt = np.dtype(dtype)
    for n in (0, 1, 2, 15, 16, 17, 1000):
        a = _random(dt, n, rng)
        for atol, rtol in ((0, 0), (1e-6, 1e-5)):
            for fn in (compare, _capi.compare_host):
                assert as_tuple(fn(a, a.copy(), atol, rtol, True)) == (0, -1, 0.0), (n, fn)
    # a single changed element is always found, at its index
    a = _random(dt, 257, rng)
    if dt.kind == 'f':
        a[np.isnan(a)] = 1.5
    for i in list(range(0, 257, 16)) + [255, 256]:
        b = a.copy()
        b[i] = 3 if a[i] != 3 else 4
        for fn in (compare, _capi.compare_host):
            rec = fn(a, b, 0, 0, True)
            assert (int(rec['n_diff']), int(rec['first'])) == (1, i), (i, fn)
            with np.errstate(all='ignore'):
                assert float(rec['max_abs_diff']) == abs(float(a[i]) - float(b[i]))
    # padding is never read: the elements past n_elems are poison that differs
    lib = _capi.load_library()
    n, pad = 100, 28
    a = _random(dt, n + pad, rng)
    b = a.copy()
    b[n:] = a[n:][::-1] if dt.kind != 'f' else np.nan
    a[n:] = 77
    b[40] = 9 if a[40] != 9 else 8
    if dt.kind == 'f':
        a[40] = 1.0
    rec = np.zeros(1, dtype=RECORD)
    assert lib.dswx_compare_host(a.ctypes.data, b.ctypes.data, kind_of(dt), n, 0.0, 0.0, 0, rec.ctypes.data) == 0
    want = compare(a[:n], b[:n], 0, 0, False)
    assert as_tuple(rec[0]) == as_tuple(want) and int(rec[0]['first']) <= 40
    # compare_tiles: the tiles of a stack, each its own record
    t = np.stack([a[:n], b[:n], a[:n]])
    u = np.stack([a[:n], a[:n], b[:n]])
    got = compare_tiles(t, u, 0, 0, True)
    assert got.dtype == RECORD and as_tuple(got[0]) == (0, -1, 0.0)
    assert as_tuple(got[1]) == as_tuple(compare(b[:n], a[:n])) and as_tuple(got[2]) == as_tuple(compare(a[:n], b[:n]))


def test_max_abs_diff_ignores_nan_pairs_and_reports_infinities():
    a = np.array([1.0, np.nan, 5.0, np.nan, np.inf, 2.0], dtype=np.float32)
    b = np.array([1.0, 3.0, 5.5, np.nan, 1.0, np.nan], dtype=np.float32)
    for fn in (compare, _capi.compare_host):
        assert as_tuple(fn(a[:4], b[:4], 0, 0, True)) == (2, 1, 0.5)          # NaN / 3 counts, its difference does not
        assert as_tuple(fn(a[:4], b[:4], 0, 0, False)) == (3, 1, 0.5)         # NaN / NaN counts too
        assert as_tuple(fn(a, b, 0, 0, True)) == (4, 1, math.inf)
        assert as_tuple(fn(a[1:2], b[1:2], 0, 0, True)) == (1, 0, 0.0)        # only a NaN pair: nothing to take a maximum of
    i = np.array([0, 65535, 7], dtype=np.uint16)
    j = np.array([65535, 0, 7], dtype=np.uint16)
    assert as_tuple(_capi.compare_host(i, j, 65534.0, 0, True)) == (2, 0, 65535.0)   # no wrap-around of the difference
    assert as_tuple(_capi.compare_host(i, j, 65535.0, 0, True)) == (0, -1, 0.0)
    k = np.array([-32768, 32767], dtype=np.int16)
    assert as_tuple(_capi.compare_host(k, k[::-1].copy(), 0, 1.0, True)) == (2, 0, 65535.0)     # tol = |y| < 65535
    assert as_tuple(_capi.compare_host(k, k[::-1].copy(), 0, 2.0, True)) == (1, 0, 65535.0)     # 2 * 32767 < 65535 <= 2 * 32768


def test_record_layout_and_header():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_COMPARE 1' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert RECORD.itemsize == ctypes.sizeof(_capi.CompareRecord) == 32
    for name in RECORD.names:
        assert RECORD.fields[name][1] == getattr(_capi.CompareRecord, name).offset
    assert [kind_of(d) for d in KINDS] == [_capi.CMP_U8, _capi.CMP_U16, _capi.CMP_I16, _capi.CMP_F32, _capi.CMP_F64] == list(range(5))
    for name, v in zip(('DSWX_CMP_U8', 'DSWX_CMP_U16', 'DSWX_CMP_I16', 'DSWX_CMP_F32', 'DSWX_CMP_F64'), range(5)):
        assert f'{name} = {v}' in text
    with pytest.raises(ValueError):
        kind_of(np.int32)
    if shutil.which('gcc'):                                              # the record as a C compiler lays it out
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, 'rec.c')
            with open(src, 'w') as f:
                f.write('#include <stdio.h>\n#include <stddef.h>\n#include "dswx_hip.h"\n#ifndef DSWX_HAS_COMPARE\n#error no compare\n#endif\n'
                        'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(dswx_compare_t), offsetof(dswx_compare_t, n_diff),'
                        ' offsetof(dswx_compare_t, first), offsetof(dswx_compare_t, max_abs_diff), offsetof(dswx_compare_t, reserved));'
                        ' return 0; }\n')
            subprocess.run(['gcc', '-std=c11', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), src, '-o', os.path.join(d, 'rec')],
                           check=True)
            out = subprocess.run([os.path.join(d, 'rec')], capture_output=True, text=True, check=True).stdout.split()
            assert out == ['32', '0', '8', '16', '24']


def test_error_paths_that_need_no_device():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    pa, pb, out = vp(0x10000), vp(0x30000), vp(0x20000)      # never dereferenced: every call fails before the device is touched

    def dev(ctx=None, a=pa, b=pb, kind=_capi.CMP_I16, n_tiles=3, n=100, sa=0, sb=0, atol=0.0, rtol=0.0, out=out):
        return lib.dswx_compare_device(ctx, a, b, kind, n_tiles, n, sa, sb, atol, rtol, 1, out, None)
    assert dev() == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()                      # null context, arguments fine
    for kind in (-1, 5, 6, 100):
        assert dev(kind=kind) == _capi.ERR_ARG and b'kind' in lib.dswx_last_error()
    for kw in ({'n_tiles': -1}, {'n': -1}, {'sa': -5}, {'sb': -5}):
        assert dev(**kw) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error(), kw
    assert dev(n=100, sa=99) == _capi.ERR_ARG and b'stride' in lib.dswx_last_error()
    assert dev(n=100, sb=99) == _capi.ERR_ARG and b'stride' in lib.dswx_last_error()
    assert dev(n=100, sa=100, sb=101) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()  # strides of their own
    for kw in ({'a': None}, {'b': None}, {'out': None}):
        assert dev(**kw) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error(), kw
    assert dev(n_tiles=1 << 40) == _capi.ERR_ARG and dev(n=1 << 50) == _capi.ERR_ARG       # sizes whose products would overflow
    for bad in (-1.0, -1e-300, math.nan, math.inf):
        assert dev(atol=bad) == _capi.ERR_ARG and b'atol' in lib.dswx_last_error(), bad
        assert dev(rtol=bad) == _capi.ERR_ARG and b'rtol' in lib.dswx_last_error(), bad
    for kind, eb in ((_capi.CMP_U16, 2), (_capi.CMP_I16, 2), (_capi.CMP_F32, 4), (_capi.CMP_F64, 8)):
        for off in range(1, eb):
            assert dev(a=vp(0x10000 + off), kind=kind) == _capi.ERR_ALIGN, (kind, off)
            assert dev(b=vp(0x30000 + off), kind=kind) == _capi.ERR_ALIGN, (kind, off)
        assert dev(a=vp(0x10000 + eb), b=vp(0x30000 + 3 * eb), kind=kind) == _capi.ERR_ARG    # aligned: on to the context check
        assert b'ctx' in lib.dswx_last_error()
    assert dev(a=vp(0x10001), b=vp(0x30007), kind=_capi.CMP_U8) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()
    for off in (1, 2, 4):
        assert dev(out=vp(0x20000 + off)) == _capi.ERR_ALIGN and b'out' in lib.dswx_last_error()
    assert dev(a=pa, b=pa) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()            # a == b is legal
    # dswx_batch_compare: without a device there is no batch to hand it
    rec = np.zeros(4, dtype=RECORD)
    assert lib.dswx_batch_compare(None, None, 1, 0, 1, 0.0, 0.0, 1, rec.ctypes.data, None) == _capi.ERR_ARG
    assert b'batch is NULL' in lib.dswx_last_error()
    # dswx_compare_host
    a = np.arange(8, dtype=np.int16)

    def host(a_ptr=a.ctypes.data, b_ptr=a.ctypes.data, kind=_capi.CMP_I16, n=8, atol=0.0, rtol=0.0, out_ptr=rec.ctypes.data):
        return lib.dswx_compare_host(a_ptr, b_ptr, kind, n, atol, rtol, 1, out_ptr)
    assert host() == 0 and as_tuple(rec[0]) == (0, -1, 0.0)
    for kind in (-1, 5):
        assert host(kind=kind) == _capi.ERR_ARG and b'kind' in lib.dswx_last_error()
    assert host(n=-1) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error()
    for kw in ({'a_ptr': None}, {'b_ptr': None}, {'out_ptr': None}):
        assert host(**kw) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error(), kw
    rec[0]['n_diff'] = 99
    assert host(a_ptr=None, b_ptr=None, n=0) == 0 and as_tuple(rec[0]) == (0, -1, 0.0)      # empty buffers need no pointer
    for bad in (-1.0, math.nan, math.inf):
        assert host(atol=bad) == _capi.ERR_ARG and host(rtol=bad) == _capi.ERR_ARG and b'rtol' in lib.dswx_last_error()
    with pytest.raises(ValueError):
        compare(a, a.astype(np.uint16))
    with pytest.raises(ValueError):
        compare(a, a, atol=-1)
    with pytest.raises(ValueError):
        _capi.compare_host(a, a[:4])


def test_compare_example_compiles_against_the_header(tmp_path):
    """examples/batch_compare.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device
    the program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_compare')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_compare.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
