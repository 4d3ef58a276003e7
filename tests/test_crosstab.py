"""The per-tile cross-tabulation of include/dswx_hip.h ("crosstab") without a GPU: the rule as a scalar loop written here,
pinned to the numpy statement (proteus_amd/crosstab.py), to the library's scalar statement (dswx_crosstab_host) and, where it
applies, to np.histogram2d; the three reductions of the definition against the existing histogram; the header's macro and
struct layouts against a C compiler; every error path of the three entries that needs no device; the helpers on hand-made
tables; the C example."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import dswx_oracle as o
from proteus_amd import _capi
from proteus_amd import crosstab as ct
from proteus_amd.crosstab import CELLS, IDENTITY, NOT_COUNTED, WTR_CLASSES, ZEROS, Spec, agreement, classes, crosstab, fold
from proteus_amd.histogram import DTYPES, HIST_DIAG, HIST_I16, HIST_U16, HIST_U8, histogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = o.get_binary_representation(np.arange(32, dtype=np.uint16))
# (kind, lo, shift) per A kind: ranges that leave part of the domain outside the 256 bins
BINNINGS = {'u8': (HIST_U8, 0, 0), 'u16': (HIST_U16, 1000, 5), 'i16': (HIST_I16, -4096, 6), 'diag': (HIST_DIAG, 0, 0)}


def a_data(rng, name, n):
    kind, lo, shift = BINNINGS[name]
    dt = DTYPES[kind]
    if kind == HIST_U8:
        return rng.integers(0, 256, size=n).astype(dt)
    if kind == HIST_DIAG:
        return np.where(rng.random(n) < 0.8, PATTERNS[rng.integers(0, 32, size=n)],
                        np.where(rng.random(n) < 0.5, 65535, rng.integers(0, 65536, size=n))).astype(dt)
    info = np.iinfo(dt)
    near = np.clip(rng.integers(lo - 64, lo + (256 << shift) + 64, size=n), info.min, info.max)
    return np.where(rng.random(n) < 0.7, near, rng.integers(info.min, info.max + 1, size=n)).astype(dt)


# ---- the rule, written out again: one pair at a time -------------------------------------------------------------------
def scalar_bin(v, kind, lo, shift):
    """The histogram bin of one element (a Python int), None if it is not counted."""
    if kind == HIST_U8:
        return v
    if kind == HIST_DIAG:
        if v == 65535:
            return 32
        text = str(v)
        if v <= 11111 and set(text) <= {'0', '1'}:
            return sum(int(c) << k for k, c in enumerate(reversed(text)))
        return 33
    d = v - lo
    return d >> shift if 0 <= d < (256 << shift) else None


def scalar_crosstab(a, b, spec):
    cells = [0] * CELLS
    n_cols, n_rows = 1 << spec.col_bits, 256 >> spec.col_bits
    rows, cols = spec.row_of_bin.tolist(), spec.col_of_byte.tolist()
    for x, y in zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()):
        bin_ = scalar_bin(x, spec.a_kind, spec.a_lo, spec.a_shift)
        if bin_ is None:
            continue
        row, col = rows[bin_], cols[y]
        if row < n_rows and col < n_cols:
            cells[row * n_cols + col] += 1
    return np.array(cells, dtype=np.uint64)


def all_agree(a, b, spec):
    want = scalar_crosstab(a, b, spec)
    for name, got in (('numpy statement', crosstab(a, b, spec)), ('dswx_crosstab_host', _capi.crosstab_host(a, b, spec))):
        assert got.dtype == np.uint64 and got.shape == (CELLS,), name
        assert np.array_equal(got, want), (name, spec, np.flatnonzero(got != want)[:8])
    return want


def random_tables(rng, col_bits, excluded):
    """Tables over the whole row / column range; `excluded`: a fifth of the entries on each side out of range."""
    n_rows, n_cols = 256 >> col_bits, 1 << col_bits
    rows, cols = rng.integers(0, n_rows, size=256), rng.integers(0, n_cols, size=256)
    if excluded:
        if n_rows < 256:
            rows = np.where(rng.random(256) < 0.2, rng.integers(n_rows, 256, size=256), rows)
        if n_cols < 256:
            cols = np.where(rng.random(256) < 0.2, rng.integers(n_cols, 256, size=256), cols)
    return rows.astype(np.uint8), cols.astype(np.uint8)


@pytest.mark.parametrize('name', list(BINNINGS))
@pytest.mark.parametrize('col_bits', [0, 2, 4, 8])
def test_loop_numpy_and_host_entry_agree(name, col_bits):
    rng = np.random.default_rng(9100 + col_bits)
    kind, lo, shift = BINNINGS[name]
    n = 3001
    a, b = a_data(rng, name, n), rng.integers(0, 256, size=n).astype(np.uint8)
    for excluded in (False, True):
        rows, cols = random_tables(rng, col_bits, excluded)
        spec = Spec(kind, lo, shift, col_bits, rows, cols)
        got = all_agree(a, b, spec)
        if not excluded and name in ('u8', 'diag'):
            assert got.sum() == n                                                            # every pair is counted
        if excluded and 0 < col_bits < 8:
            assert 0 < got.sum() < n
    # everything excluded, on either side (where the side has an excluded value at all)
    if col_bits > 0:
        assert all_agree(a, b, Spec(kind, lo, shift, col_bits, np.full(256, 255, dtype=np.uint8), ZEROS)).sum() == 0
    if col_bits < 8:
        assert all_agree(a, b, Spec(kind, lo, shift, col_bits, ZEROS, np.full(256, 255, dtype=np.uint8))).sum() == 0
    # the empty array
    assert all_agree(a[:0], b[:0], Spec(kind, lo, shift, col_bits)).sum() == 0
    # 2-D arrays are taken in C order
    rows, cols = random_tables(rng, col_bits, True)
    spec = Spec(kind, lo, shift, col_bits, rows, cols)
    assert np.array_equal(all_agree(a[:3000].reshape(60, 50), b[:3000].reshape(60, 50), spec), crosstab(a[:3000], b[:3000], spec))
    assert np.array_equal(ct.crosstab_tiles(a[:3000].reshape(3, 1000), b[:3000].reshape(3, 1000), spec),
                          np.stack([crosstab(a[k * 1000:(k + 1) * 1000], b[k * 1000:(k + 1) * 1000], spec) for k in range(3)]))


@pytest.mark.parametrize('name', list(BINNINGS))
def test_identity_tables_are_histogram2d(name):
    """col_bits 4, identity tables, bins and bytes below 16: the record is np.histogram2d of (bin, byte)."""
    rng = np.random.default_rng(9200)
    kind = BINNINGS[name][0]
    n = 5000
    values = rng.integers(0, 16, size=n)
    a, lo, shift = {'u8': (values.astype(np.uint8), 0, 0), 'u16': ((values * 8 + 500 + rng.integers(0, 8, size=n)).astype(np.uint16), 500, 3),
                    'i16': ((values * 4 - 77 + rng.integers(0, 4, size=n)).astype(np.int16), -77, 2),
                    'diag': (PATTERNS[values], 0, 0)}[name]
    b = rng.integers(0, 16, size=n).astype(np.uint8)
    spec = Spec(kind, lo, shift, 4)
    got = all_agree(a, b, spec)
    h2d, _, _ = np.histogram2d(values, b, bins=(16, 16), range=((0, 16), (0, 16)))
    assert np.array_equal(spec.table(got), h2d.astype(np.uint64))
    assert got.sum() == n


@pytest.mark.parametrize('name', list(BINNINGS))
def test_the_three_reductions_against_the_histogram(name):
    rng = np.random.default_rng(9300)
    kind, lo, shift = BINNINGS[name]
    lib = _capi.load_library()
    n = 4001
    a, b = a_data(rng, name, n), rng.integers(0, 256, size=n).astype(np.uint8)
    # 1. col_bits 0, zero columns, identity rows: the histogram of A
    got = all_agree(a, b, Spec(kind, lo, shift, 0, IDENTITY, ZEROS))
    assert np.array_equal(got, histogram(a, kind, lo, shift))
    assert np.array_equal(got, _capi.histogram_host(a, kind, lo, shift))
    # 2. col_bits 8, zero rows, identity columns: the U8 histogram of B over the pairs whose A element is counted
    got = all_agree(a, b, Spec(kind, lo, shift, 8, ZEROS, IDENTITY))
    counted = ct._h.bin_of(a, kind, lo, shift) >= 0
    assert np.array_equal(got, histogram(b[counted]))
    rec = np.zeros(CELLS, dtype=np.uint64)
    bc = np.ascontiguousarray(b[counted])
    assert lib.dswx_histogram_host(bc.ctypes.data, HIST_U8, 0, 0, bc.size, rec.ctypes.data) == 0
    assert np.array_equal(got, rec)
    if name in ('u16', 'i16'):
        assert 0 < counted.sum() < n
    # 3. nothing excluded: row sums = histogram of row_of_bin[bin(A)], column sums = histogram of col_of_byte[B]
    rows, cols = random_tables(rng, 3, False)
    spec = Spec(kind, lo, shift, 3, rows, cols)
    table = spec.table(all_agree(a, b, spec))
    bins = ct._h.bin_of(a, kind, lo, shift)
    assert np.array_equal(table.sum(axis=1), histogram(rows[bins[counted]])[:32])
    assert np.array_equal(table.sum(axis=0), histogram(cols[b[counted]])[:8])


def test_host_entry_takes_buffers_at_odd_addresses():
    lib = _capi.load_library()
    rng = np.random.default_rng(9400)
    n = 501
    raw_a, raw_b = np.zeros(2 * n + 16, dtype=np.uint8), np.zeros(n + 16, dtype=np.uint8)
    sa = 1 if raw_a.ctypes.data % 2 == 0 else 0
    sb = 1 if raw_b.ctypes.data % 2 == 0 else 0
    for name, (kind, lo, shift) in BINNINGS.items():
        a, b = a_data(rng, name, n), rng.integers(0, 256, size=n).astype(np.uint8)
        rows, cols = random_tables(rng, 5, True)
        spec = Spec(kind, lo, shift, 5, rows, cols)
        raw_a[sa:sa + a.nbytes] = a.view(np.uint8)
        raw_b[sb:sb + n] = b
        out = np.full(CELLS, 99, dtype=np.uint64)                                            # overwritten, not added to
        assert (raw_a.ctypes.data + sa) % 2 == 1 and (raw_b.ctypes.data + sb) % 2 == 1
        assert lib.dswx_crosstab_host(raw_a.ctypes.data + sa, raw_b.ctypes.data + sb, ctypes.byref(_capi.CrosstabSpec.of(spec)), n,
                                      out.ctypes.data) == 0
        assert np.array_equal(out, crosstab(a, b, spec)), name


C_LAYOUT = r'''
#include <stddef.h>
#include <stdio.h>
#include "dswx_hip.h"
int main(void) {
    printf("%d %d %d\n", DSWX_HAS_CROSSTAB, DSWX_CROSSTAB_CELLS, DSWX_CROSSTAB_MAX_PAIRS);
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(dswx_crosstab_spec_t), offsetof(dswx_crosstab_spec_t, a_kind),
           offsetof(dswx_crosstab_spec_t, a_lo), offsetof(dswx_crosstab_spec_t, a_shift), offsetof(dswx_crosstab_spec_t, col_bits),
           offsetof(dswx_crosstab_spec_t, row_of_bin), offsetof(dswx_crosstab_spec_t, col_of_byte));
    printf("%zu %zu %zu %zu\n", sizeof(dswx_crosstab_pair_t), offsetof(dswx_crosstab_pair_t, plane_a),
           offsetof(dswx_crosstab_pair_t, plane_b), offsetof(dswx_crosstab_pair_t, spec));
    return 0;
}
'''


def test_header_says_has_crosstab_abi_7_and_the_struct_layouts(tmp_path):
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_CROSSTAB 1' in text and '#define DSWX_CROSSTAB_CELLS 256' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert _capi.HAS_CROSSTAB == 1 and _capi.CROSSTAB_CELLS == CELLS == 256 and _capi.CROSSTAB_MAX_PAIRS == ct.MAX_PAIRS == 6
    assert text.index('---- histogram:') < text.index('---- crosstab:') < text.index('---- device plumbing')
    for name in ('dswx_crosstab_device', 'dswx_batch_crosstab', 'dswx_crosstab_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    S, P = _capi.CrosstabSpec, _capi.CrosstabPair
    assert ctypes.sizeof(S) == 528 and ctypes.sizeof(P) == 536
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / 'layout.c'
    src.write_text(C_LAYOUT)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split('\n')
    assert lines[0].split() == ['1', '256', '6']
    assert [int(v) for v in lines[1].split()] == [ctypes.sizeof(S), S.a_kind.offset, S.a_lo.offset, S.a_shift.offset, S.col_bits.offset,
                                                  S.row_of_bin.offset, S.col_of_byte.offset] == [528, 0, 4, 8, 12, 16, 272]
    assert [int(v) for v in lines[2].split()] == [ctypes.sizeof(P), P.plane_a.offset, P.plane_b.offset, P.spec.offset] == [536, 0, 4, 8]


def test_error_paths_that_need_no_device():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    pa, pb, out = vp(0x10000), vp(0x30000), vp(0x20000)          # never dereferenced: every call fails before the device is touched

    def spec_of(kind=HIST_I16, lo=0, shift=0, col_bits=4):
        s = _capi.CrosstabSpec.of(Spec())
        s.a_kind, s.a_lo, s.a_shift, s.col_bits = kind, lo, shift, col_bits
        return s

    def dev(ctx=None, a=pa, b=pb, spec='default', n_tiles=3, n=100, a_stride=0, b_stride=0, out=out, **kw):
        s = spec_of(**kw) if spec == 'default' else spec
        return lib.dswx_crosstab_device(ctx, a, b, ctypes.byref(s) if s is not None else None, n_tiles, n, a_stride, b_stride, out, None)
    assert dev() == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()                      # null context, arguments fine
    assert dev(spec=None) == _capi.ERR_ARG and b'spec' in lib.dswx_last_error()
    for kind in (-1, 4, 5, 100):
        assert dev(kind=kind) == _capi.ERR_ARG and b'kind' in lib.dswx_last_error()
    for kind in (HIST_U8, HIST_U16, HIST_I16, HIST_DIAG):
        for shift in (-1, 9, 100):
            assert dev(kind=kind, shift=shift) == _capi.ERR_ARG and b'shift' in lib.dswx_last_error(), (kind, shift)
        for col_bits in (-1, 9, 100):
            assert dev(kind=kind, col_bits=col_bits) == _capi.ERR_ARG and b'col_bits' in lib.dswx_last_error(), (kind, col_bits)
        for shift, col_bits in ((0, 0), (8, 8)):
            assert dev(kind=kind, shift=shift, col_bits=col_bits) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()
    for kw in ({'n_tiles': -1}, {'n': -1}, {'a_stride': -5}, {'b_stride': -5}):
        assert dev(**kw) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error(), kw
    for kw in ({'a_stride': 99}, {'b_stride': 99}):
        assert dev(**kw) == _capi.ERR_ARG and b'stride' in lib.dswx_last_error(), kw
    assert dev(a_stride=101, b_stride=100) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()
    for kw in ({'a': None}, {'b': None}, {'out': None}):
        assert dev(**kw) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error(), kw
    assert dev(a=None, b=None, out=None, n_tiles=0) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()
    assert dev(n_tiles=1 << 40) == _capi.ERR_ARG and dev(n=1 << 50) == _capi.ERR_ARG       # the limits of dswx_compare_device
    assert b'too large' in lib.dswx_last_error()
    for kind in (HIST_U16, HIST_I16, HIST_DIAG):
        assert dev(a=vp(0x10001), kind=kind) == _capi.ERR_ALIGN and b'aligned' in lib.dswx_last_error(), kind
        assert dev(a=vp(0x10002), kind=kind) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error(), kind
    assert dev(a=vp(0x10001), kind=HIST_U8) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()         # bytes: any address
    assert dev(b=vp(0x30001)) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()                       # plane b: any address
    assert dev(a=pa, b=pa, kind=HIST_U8) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()             # a == b is legal
    for off in (1, 2, 4):
        assert dev(out=vp(0x20000 + off)) == _capi.ERR_ALIGN and b'out' in lib.dswx_last_error()
    # dswx_batch_crosstab: without a device there is no batch to hand it
    rec = np.zeros(CELLS, dtype=np.uint64)
    pair = _capi.CrosstabPair(14, 14, spec_of(kind=HIST_U8))
    assert lib.dswx_batch_crosstab(None, None, ctypes.byref(pair), 1, 0, 1, rec.ctypes.data, None) == _capi.ERR_ARG
    assert b'batch is NULL' in lib.dswx_last_error()
    # dswx_crosstab_host
    a, b = np.arange(8, dtype=np.int16), np.arange(8, dtype=np.uint8)

    def host(pa=a.ctypes.data, pb=b.ctypes.data, spec='default', n=8, out_ptr=rec.ctypes.data, **kw):
        s = spec_of(**kw) if spec == 'default' else spec
        return lib.dswx_crosstab_host(pa, pb, ctypes.byref(s) if s is not None else None, n, out_ptr)
    assert host() == 0 and rec.sum() == 8 and all(rec[17 * k] == 1 for k in range(8))
    assert host(spec=None) == _capi.ERR_ARG and b'spec' in lib.dswx_last_error()
    for kind in (-1, 4):
        assert host(kind=kind) == _capi.ERR_ARG and b'kind' in lib.dswx_last_error()
    for shift in (-1, 9):
        assert host(shift=shift) == _capi.ERR_ARG and b'shift' in lib.dswx_last_error()
    for col_bits in (-1, 9):
        assert host(col_bits=col_bits) == _capi.ERR_ARG and b'col_bits' in lib.dswx_last_error()
    assert host(n=-1) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error()
    for kw in ({'pa': None}, {'pb': None}, {'out_ptr': None}):
        assert host(**kw) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error(), kw
    assert host(out_ptr=rec.ctypes.data + 4) == _capi.ERR_ALIGN and b'out' in lib.dswx_last_error()
    assert rec.sum() == 8                                                                    # a refused call writes nothing
    assert host(pa=None, pb=None, n=0) == 0 and rec.sum() == 0                               # empty buffers need no pointers
    # the Python side refuses what the library would
    for kw in ({'a_shift': 9}, {'col_bits': 9}, {'col_bits': -1}, {'a_kind': 7}, {'row_of_bin': np.zeros(255, dtype=np.uint8)},
               {'col_of_byte': np.full(256, 256)}, {'col_of_byte': np.zeros(256)}):
        with pytest.raises(ValueError):
            Spec(**kw)
    with pytest.raises(ValueError):
        crosstab(a, b, Spec(HIST_U8))                                                        # a kind of another dtype
    with pytest.raises(ValueError):
        crosstab(a, b.astype(np.uint16), Spec(HIST_I16))                                     # plane b is uint8
    with pytest.raises(ValueError):
        crosstab(a, b[:7], Spec(HIST_I16))
    with pytest.raises(ValueError):
        _capi.crosstab_host(a, b.astype(np.int8), Spec(HIST_I16))
    with pytest.raises(ValueError):
        _capi.crosstab_host(a.astype(np.float32), b, Spec(HIST_I16))


def test_classes_wtr_classes_and_fold():
    t = classes([0, 1, 2, 252])
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert (t[0], t[1], t[2], t[252]) == (0, 1, 2, 3) and np.all(np.delete(t, [0, 1, 2, 252]) == NOT_COUNTED)
    t = classes([7, 3], other=2)
    assert (t[7], t[3]) == (0, 1) and np.all(np.delete(t, [7, 3]) == 2)
    for bad in ([1, 1], [256], [-1]):
        with pytest.raises(ValueError):
            classes(bad)
    with pytest.raises(ValueError):
        classes([1], other=256)
    # the listed values are counted, everything else is not
    a = np.array([0, 1, 2, 252, 9, 9, 1, 0], dtype=np.uint8)
    b = np.array([0, 1, 1, 252, 0, 9, 7, 0], dtype=np.uint8)
    spec = Spec(col_bits=2, row_of_bin=classes([0, 1, 2, 252]), col_of_byte=classes([0, 1, 252]))
    table = spec.table(all_agree(a, b, spec))
    assert table.shape == (64, 4) and table.sum() == 5
    assert (table[0, 0], table[1, 1], table[2, 1], table[3, 2]) == (2, 1, 1, 1)
    # WTR_CLASSES: 8 x 8 over 0, 1, 2, snow, cloud, ocean-masked, fill, and class 7 for anything else
    assert WTR_CLASSES.a_kind == HIST_U8 and WTR_CLASSES.col_bits == 3 and (WTR_CLASSES.n_rows, WTR_CLASSES.n_cols) == (32, 8)
    assert ct.WTR_VALUES == (0, 1, 2, 252, 253, 254, 255)
    for k, v in enumerate(ct.WTR_VALUES):
        assert WTR_CLASSES.row_of_bin[v] == k and WTR_CLASSES.col_of_byte[v] == k
    assert np.all(np.delete(WTR_CLASSES.row_of_bin, ct.WTR_VALUES) == 7)
    wtr2 = np.array([0, 1, 2, 1, 0, 255, 254, 77], dtype=np.uint8)
    wtr = np.array([0, 1, 253, 252, 0, 255, 254, 1], dtype=np.uint8)
    table = WTR_CLASSES.table(all_agree(wtr2, wtr, WTR_CLASSES))[:8]
    want = np.zeros((8, 8), dtype=np.uint64)
    for r, c in ((0, 0), (1, 1), (2, 4), (1, 3), (0, 0), (6, 6), (5, 5), (7, 1)):
        want[r, c] += 1
    assert np.array_equal(table, want)
    # fold: 256 linear bins into n rows
    assert np.array_equal(fold(256), IDENTITY) and np.all(fold(1) == 0)
    f = fold(16)
    assert f.dtype == np.uint8 and np.array_equal(f, np.arange(256) // 16)
    for bad in (0, 3, 512):
        with pytest.raises(ValueError):
            fold(bad)
    band = np.array([0, 63, 64, 1023, 1024, 16383, 16384, -1], dtype=np.int16)
    spec = Spec(HIST_I16, 0, 6, 4, fold(16), classes([1, 2]))
    table = spec.table(all_agree(band, np.array([1, 1, 2, 1, 2, 2, 1, 1], dtype=np.uint8), spec))
    assert table.shape == (16, 16) and table.sum() == 6
    assert (table[0, 0], table[0, 1], table[1, 1], table[15, 1]) == (3, 1, 1, 1)


def test_agreement_on_hand_made_tables():
    r = agreement([[5, 1], [2, 4]])
    assert r['n'] == 12 and r['overall'] == 0.75 and abs(r['kappa'] - 0.5) < 1e-15
    assert np.allclose(r['row'], [5 / 6, 4 / 6], rtol=0, atol=1e-15) and np.allclose(r['col'], [5 / 7, 4 / 5], rtol=0, atol=1e-15)
    r = agreement(np.diag([3, 0, 9]))                                                        # perfect, with an empty class
    assert r['overall'] == 1.0 and r['kappa'] == 1.0 and np.isnan(r['row'][1]) and np.isnan(r['col'][1]) and r['row'][0] == 1.0
    r = agreement([[0, 4], [6, 0]])                                                          # never agree
    assert r['overall'] == 0.0 and r['kappa'] < 0 and abs(r['kappa'] - (0 - 0.48) / (1 - 0.48)) < 1e-15
    r = agreement([[1, 1], [1, 1]])                                                          # chance
    assert r['overall'] == 0.5 and r['kappa'] == 0.0
    r = agreement([[7, 0], [0, 0]])                                                          # one class only: pe = 1
    assert r['overall'] == 1.0 and np.isnan(r['kappa'])
    r = agreement(np.zeros((3, 3)))
    assert r['n'] == 0 and np.isnan(r['overall']) and np.isnan(r['kappa'])
    big = np.array([[2 ** 40, 3], [5, 2 ** 41]], dtype=np.uint64)
    assert agreement(big)['n'] == 2 ** 40 + 2 ** 41 + 8
    for bad in (np.zeros((2, 3)), np.zeros(4)):
        with pytest.raises(ValueError):
            agreement(bad)
    # from a record: the 8 x 8 WTR table
    rec = np.zeros(CELLS, dtype=np.uint64)
    rec[0 * 8 + 0], rec[1 * 8 + 1], rec[1 * 8 + 4] = 10, 5, 5
    r = agreement(WTR_CLASSES.table(rec)[:8])
    assert r['overall'] == 0.75 and r['row'][1] == 0.5 and r['col'][1] == 1.0 and r['col'][4] == 0.0 and np.isnan(r['row'][4])


def test_product_crosstab_on_the_host_prints_the_table(tmp_path, capsys):
    """compare_dswx_hls_products(..., crosstab=True) without a device: the numpy statement; everything printed without the flag
    and the return value stay as they are."""
    from proteus_amd import geotiff
    from proteus_amd.dswx_hls import compare_dswx_hls_products
    rng = np.random.default_rng(9500)
    H, W = 40, 31
    base = rng.choice(np.array([0, 1, 2, 252, 255], dtype=np.uint8), size=(2, H, W))
    other = base.copy()
    moved = [(1, 3, 4), (1, 17, 20), (1, 39, 30)]
    for band, y, x in moved:
        base[band, y, x], other[band, y, x] = 1, 253
    for name, arr in (('a', base), ('b', other)):
        geotiff.write_geotiff(str(tmp_path / f'{name}.tif'), arr, metadata={'PRODUCT': 'DSWx-HLS'}, nodata=255,
                              descriptions=['WTR', 'WTR-2'],
                              geo_tags=geotiff.geo_tags_from_geotransform((500000.0, 30.0, 0.0, 4000000.0, 0.0, -30.0), 32611))
    capsys.readouterr()
    plain = compare_dswx_hls_products(str(tmp_path / 'a.tif'), str(tmp_path / 'b.tif'))
    plain_text = capsys.readouterr().out
    with_table = compare_dswx_hls_products(str(tmp_path / 'a.tif'), str(tmp_path / 'b.tif'), crosstab=True)
    text = capsys.readouterr().out
    assert plain is False and with_table is False
    extra = [line for line in text.splitlines() if line not in plain_text.splitlines()]
    assert [line for line in text.splitlines() if line not in extra] == plain_text.splitlines()
    check_printed_tables(extra, base, other, ['WTR', 'WTR-2'])
    assert f'agreement {(H * W - 3) / (H * W):.6f} ({H * W - 3} of {H * W} pixels)' in text


def check_printed_tables(lines, file_1, file_2, descriptions):
    """The lines compare_dswx_hls_products adds with crosstab=True, parsed back: per band the header, the column values and
    one row per value of file 1, every cell against a count made here."""
    assert lines[0].startswith('Cross-tabulating')
    at = 1
    for b, desc in enumerate(descriptions):
        v1, v2 = np.unique(file_1[b]), np.unique(file_2[b])
        same = int(np.count_nonzero(file_1[b] == file_2[b]))
        assert lines[at].strip() == f'Band {b + 1} - {desc}: agreement {same / file_1[b].size:.6f} ({same} of {file_1[b].size} pixels)'
        assert [int(v) for v in lines[at + 1].split()] == v2.tolist()
        for i, a in enumerate(v1):
            cells = [int(v) for v in lines[at + 2 + i].split()]
            assert cells[0] == a
            assert cells[1:] == [int(np.count_nonzero((file_1[b] == a) & (file_2[b] == c))) for c in v2], (desc, a)
        at += 2 + len(v1)
    assert at == len(lines)


def test_crosstab_example_compiles_against_the_header(tmp_path):
    """examples/batch_crosstab.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device
    the program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_crosstab')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_crosstab.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
