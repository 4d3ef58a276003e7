"""The per-tile histogram of include/dswx_hip.h ("histogram") without a GPU: the bin rule as a scalar loop written here,
pinned to the numpy statement (proteus_amd/histogram.py), to np.bincount of this file's own binning and to the library's
scalar statement (dswx_histogram_host) on inputs aimed at the edges of the rule; every error path of the three entries that
needs no device; the header's macro; the C example."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import dswx_oracle as o
from proteus_amd import _capi
from proteus_amd.histogram import (BINS, HIST_DIAG, HIST_I16, HIST_U16, HIST_U8, bin_of, histogram, histogram_tiles,
                                   kind_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOS = (-32768, -9999, 0, 1, 65535 - 255)


# ---- the rule, written out again: one element at a time ---------------------------------------------------------------
def scalar_bin(v, kind, lo, shift):
    """The bin of one element (a Python int), None if it is not counted."""
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


def scalar_histogram(a, kind, lo=0, shift=0):
    bins = [0] * BINS
    for v in a.reshape(-1).tolist():
        b = scalar_bin(v, kind, lo, shift)
        if b is not None:
            bins[b] += 1
    return np.array(bins, dtype=np.uint64)


def own_bincount(a, kind, lo=0, shift=0):
    """np.bincount of this file's own binning (vectorised apart from the DIAG table, which the scalar rule fills)."""
    v = a.reshape(-1).astype(np.int64)
    if kind == HIST_U8:
        b = v
    elif kind == HIST_DIAG:
        table = np.array([scalar_bin(x, HIST_DIAG, 0, 0) for x in range(65536)], dtype=np.int64)
        b = table[v]
    else:
        d = v - lo
        b = (d >> shift)[(d >= 0) & (d < 256 * 2 ** shift)]
    return np.bincount(b, minlength=BINS).astype(np.uint64)


def all_agree(a, kind, lo=0, shift=0):
    want = scalar_histogram(a, kind, lo, shift)
    assert want.dtype == np.uint64 and want.shape == (BINS,)
    for name, got in (('numpy statement', histogram(a, kind, lo, shift)), ('bincount', own_bincount(a, kind, lo, shift)),
                      ('dswx_histogram_host', _capi.histogram_host(a, kind, lo, shift))):
        assert got.dtype == np.uint64 and got.shape == (BINS,), name
        assert np.array_equal(got, want), (name, kind, lo, shift, np.flatnonzero(got != want)[:8])
    return want


def test_u8_every_value_the_empty_array_and_a_constant():
    rng = np.random.default_rng(11)
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(all_agree(every, HIST_U8), np.ones(BINS, dtype=np.uint64))
    assert all_agree(np.zeros(0, dtype=np.uint8), HIST_U8).sum() == 0
    for value in (0, 0x80, 255):
        h = all_agree(np.full(1000, value, dtype=np.uint8), HIST_U8)
        assert h[value] == 1000 and h.sum() == 1000
    a = rng.integers(0, 256, size=(37, 53), dtype=np.uint8)
    assert all_agree(a, HIST_U8).sum() == a.size
    assert np.array_equal(_capi.histogram_host(a), histogram(a))                           # the kind follows the dtype
    assert np.array_equal(all_agree(a, HIST_U8, lo=77, shift=8), histogram(a))               # lo and shift are ignored
    assert np.array_equal(histogram_tiles(a), np.stack([histogram(r) for r in a]))


@pytest.mark.parametrize('dtype,kind', [(np.int16, HIST_I16), (np.uint16, HIST_U16)])
def test_linear_bins_at_every_shift_and_edge(dtype, kind):
    rng = np.random.default_rng(12)
    info = np.iinfo(dtype)
    assert kind_of(dtype) == kind
    for shift in range(9):
        span = 256 << shift
        for lo in LOS:
            edges = [lo - 1, lo, lo + span - 1, lo + span, lo + span // 2, lo + (1 << shift) - 1, lo + (1 << shift),
                     info.min, info.max, info.min + 1, info.max - 1, 0, -1, 1]
            edges = [v for v in edges if info.min <= v <= info.max]
            a = np.concatenate([np.array(edges, dtype=dtype), np.array(edges, dtype=dtype)[:3],
                                rng.integers(info.min, info.max + 1, size=300).astype(dtype),
                                np.clip(rng.integers(lo - 20, lo + span + 20, size=300), info.min, info.max).astype(dtype)])
            h = all_agree(a, kind, lo, shift)
            v = a.astype(np.int64)
            assert h.sum() == np.count_nonzero((v >= lo) & (v < lo + span))                  # out of range: not counted
            for e in edges:                                                                  # each edge alone
                one = all_agree(np.array([e], dtype=dtype), kind, lo, shift)
                inside = lo <= e < lo + span
                assert one.sum() == (1 if inside else 0)
                if inside:
                    assert one[(e - lo) >> shift] == 1
    # the whole domain once: at shift 8 every element of either type is counted from the type's minimum
    every = np.arange(info.min, info.max + 1).astype(dtype)
    h = all_agree(every, kind, info.min, 8)
    assert np.array_equal(h, np.full(BINS, 256, dtype=np.uint64))
    # lo at the ends of int32: nothing of a 16-bit plane is in range, and nothing overflows
    for lo in (-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 65536):
        assert all_agree(every[::97], kind, lo, 8).sum() == 0


def test_diag_patterns_nodata_and_everything_else():
    patterns = o.get_binary_representation(np.arange(32, dtype=np.uint16))                   # the 32 saved forms
    assert patterns.dtype == np.uint16 and patterns[31] == 11111 and patterns[2] == 10
    h = all_agree(patterns, HIST_DIAG)
    assert np.array_equal(h[:32], np.ones(32, dtype=np.uint64)) and h[32:].sum() == 0
    assert np.array_equal(bin_of(patterns, HIST_DIAG), np.arange(32))
    assert bin_of(o.get_binary_representation(np.array([32 + 5], dtype=np.uint16)), HIST_DIAG)[0] == 32   # the fill bit: 65535
    other = np.array([2, 12, 11112, 20000, 11121, 65534], dtype=np.uint16)
    h = all_agree(other, HIST_DIAG)
    assert h[33] == other.size and h.sum() == other.size
    h = all_agree(np.array([65535, 65535, 0, 11111], dtype=np.uint16), HIST_DIAG)
    assert h[32] == 2 and h[0] == 1 and h[31] == 1 and h.sum() == 4
    every = np.arange(65536, dtype=np.uint16)                                                # the whole domain
    h = all_agree(every, HIST_DIAG)
    assert np.array_equal(h[:33], np.ones(33, dtype=np.uint64)) and h[33] == 65536 - 33 and h[34:].sum() == 0
    assert np.array_equal(all_agree(every[::7], HIST_DIAG, lo=5, shift=3), histogram(every[::7], HIST_DIAG))   # ignored


def test_host_entry_takes_a_buffer_at_an_odd_address():
    lib = _capi.load_library()
    rng = np.random.default_rng(13)
    raw = np.zeros(2 * 501 + 16, dtype=np.uint8)
    start = 1 if raw.ctypes.data % 2 == 0 else 0                                             # an odd address
    for dtype, kind, lo, shift in ((np.int16, HIST_I16, -9999, 7), (np.uint16, HIST_U16, 1, 8), (np.uint16, HIST_DIAG, 0, 0),
                                   (np.uint8, HIST_U8, 0, 0)):
        a = rng.integers(0, 256, size=501 * np.dtype(dtype).itemsize, dtype=np.uint8)
        if kind == HIST_DIAG:
            a = o.get_binary_representation(rng.integers(0, 64, size=501).astype(np.uint16)).view(np.uint8)
        raw[start:start + a.size] = a
        out = np.full(BINS, 99, dtype=np.uint64)                                             # overwritten, not added to
        assert (raw.ctypes.data + start) % 2 == 1
        assert lib.dswx_histogram_host(raw.ctypes.data + start, kind, lo, shift, 501, out.ctypes.data) == 0
        assert np.array_equal(out, histogram(a.view(dtype), kind, lo, shift)), kind


def test_header_says_has_histogram_and_abi_7():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_HISTOGRAM 1' in text and '#define DSWX_HIST_BINS 256' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert _capi.HAS_HISTOGRAM == 1 and _capi.HIST_BINS == BINS == 256
    assert (_capi.HIST_U8, _capi.HIST_U16, _capi.HIST_I16, _capi.HIST_DIAG) == (HIST_U8, HIST_U16, HIST_I16, HIST_DIAG) == (0, 1, 2, 3)
    for name, v in (('DSWX_HIST_U8', 0), ('DSWX_HIST_U16', 1), ('DSWX_HIST_I16', 2), ('DSWX_HIST_DIAG', 3), ('DSWX_HIST_KINDS', 4)):
        assert f'{name} = {v}' in text
    assert text.index('---- compare:') < text.index('---- histogram:') < text.index('---- device plumbing')
    for name in ('dswx_histogram_device', 'dswx_batch_histogram', 'dswx_histogram_host'):
        assert name in _capi.EXPORTED_SYMBOLS
    with pytest.raises(ValueError):
        kind_of(np.float32)


def test_error_paths_that_need_no_device():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    plane, out = vp(0x10000), vp(0x20000)            # never dereferenced: every call fails before the device is touched

    def dev(ctx=None, plane=plane, kind=HIST_I16, lo=0, shift=0, n_tiles=3, n=100, stride=0, out=out):
        return lib.dswx_histogram_device(ctx, plane, kind, lo, shift, n_tiles, n, stride, out, None)
    assert dev() == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()                      # null context, arguments fine
    for kind in (-1, 4, 5, 100):
        assert dev(kind=kind) == _capi.ERR_ARG and b'kind' in lib.dswx_last_error()
    for kind in (HIST_U8, HIST_U16, HIST_I16, HIST_DIAG):
        for shift in (-1, 9, 100):
            assert dev(kind=kind, shift=shift) == _capi.ERR_ARG and b'shift' in lib.dswx_last_error(), (kind, shift)
        for shift in (0, 8):
            assert dev(kind=kind, shift=shift) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error(), (kind, shift)
    for kw in ({'n_tiles': -1}, {'n': -1}, {'stride': -5}):
        assert dev(**kw) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error(), kw
    assert dev(n=100, stride=99) == _capi.ERR_ARG and b'stride' in lib.dswx_last_error()
    assert dev(n=100, stride=101) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()
    for kw in ({'plane': None}, {'out': None}):
        assert dev(**kw) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error(), kw
    assert dev(n_tiles=1 << 40) == _capi.ERR_ARG and dev(n=1 << 50) == _capi.ERR_ARG       # sizes whose products would overflow
    assert b'too large' in lib.dswx_last_error()
    for kind in (HIST_U16, HIST_I16, HIST_DIAG):
        assert dev(plane=vp(0x10001), kind=kind) == _capi.ERR_ALIGN and b'aligned' in lib.dswx_last_error(), kind
        assert dev(plane=vp(0x10002), kind=kind) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error(), kind
    assert dev(plane=vp(0x10001), kind=HIST_U8) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()      # bytes: any address
    for off in (1, 2, 4):
        assert dev(out=vp(0x20000 + off)) == _capi.ERR_ALIGN and b'out' in lib.dswx_last_error()
    for lo in (-2 ** 31, 2 ** 31 - 1):
        assert dev(lo=lo) == _capi.ERR_ARG and b'ctx' in lib.dswx_last_error()                 # any int32 is a lo
    # dswx_batch_histogram: without a device there is no batch to hand it
    rec = np.zeros(BINS, dtype=np.uint64)
    assert lib.dswx_batch_histogram(None, 1, 0, 1, 0, 6, rec.ctypes.data, None) == _capi.ERR_ARG
    assert b'batch is NULL' in lib.dswx_last_error()
    # dswx_histogram_host
    a = np.arange(8, dtype=np.int16)

    def host(ptr=a.ctypes.data, kind=HIST_I16, lo=0, shift=0, n=8, out_ptr=rec.ctypes.data):
        return lib.dswx_histogram_host(ptr, kind, lo, shift, n, out_ptr)
    assert host() == 0 and np.array_equal(rec[:9], [1] * 8 + [0]) and rec.sum() == 8
    for kind in (-1, 4):
        assert host(kind=kind) == _capi.ERR_ARG and b'kind' in lib.dswx_last_error()
    for shift in (-1, 9):
        assert host(shift=shift) == _capi.ERR_ARG and b'shift' in lib.dswx_last_error()
    assert host(n=-1) == _capi.ERR_ARG and b'negative' in lib.dswx_last_error()
    for kw in ({'ptr': None}, {'out_ptr': None}):
        assert host(**kw) == _capi.ERR_ARG and b'NULL' in lib.dswx_last_error(), kw
    assert host(out_ptr=rec.ctypes.data + 4) == _capi.ERR_ALIGN and b'out' in lib.dswx_last_error()
    assert rec.sum() == 8                                                                    # a refused call writes nothing
    assert host(ptr=None, n=0) == 0 and rec.sum() == 0                                       # an empty buffer needs no pointer
    # the Python side refuses what the library would
    with pytest.raises(ValueError):
        histogram(a, HIST_I16, shift=9)
    with pytest.raises(ValueError):
        histogram(a, HIST_U8)                                                                # a kind of another dtype
    with pytest.raises(ValueError):
        histogram(a, 7)
    with pytest.raises(ValueError):
        _capi.histogram_host(a.astype(np.float32))
    with pytest.raises(ValueError):
        _capi.histogram_host(a, HIST_DIAG)


def test_histogram_example_compiles_against_the_header(tmp_path):
    """examples/batch_histogram.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device
    the program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_histogram')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_histogram.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
