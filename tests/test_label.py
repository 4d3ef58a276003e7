"""The connected bodies of include/dswx_hip.h ("label") without a GPU: three statements pinned to each other -- the library's
scalar union-find (dswx_label_host), the numpy statement (proteus_amd/label.py: min-propagation to a fixed point) and
scipy.ndimage.label, exactly, for both connectivities -- on every pattern of tests/_label_cases.py; sizes against np.bincount,
the summary against summary_of; rows that do not wrap, tiles that do not connect, a table with one member byte, strides with
poisoned padding, odd addresses, min_size either side of the largest body; every refusal, with the outputs untouched; the
header; the struct mirrors; the WTR spec; the host entry under ASan + UBSan in a stand-alone program; the C example."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.label import SUMMARY_WORDS, Spec, label_tiles, summary_of, wtr_label_spec
from proteus_amd.stack import wtr_spec
from tests import _label_cases as C

try:
    from scipy import ndimage
except ImportError:                                # (only the comparison with scipy is skipped then)
    ndimage = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT8 = 0xEE
PAD = 200                                          # a MEMBER byte of C.plane_of: padding that was read would join bodies
KEYS = ('label', 'size', 'sieved', 'summary')
EB = {'label': 4, 'size': 4, 'sieved': 1, 'summary': 8}


def scipy_labels(member, connectivity):
    """scipy.ndimage.label of one raster, its labels 1 .. K mapped to 1 + the first index of each."""
    lab, k = ndimage.label(member, structure=np.ones((3, 3)) if connectivity == 8 else None)
    flat = lab.reshape(-1)
    first = np.zeros(k + 1, dtype=np.int64)
    idx = np.flatnonzero(flat)
    # (the first pixel of a label in raster order: reversed, so that the smallest index is written last)
    first[flat[idx[::-1]]] = idx[::-1] + 1
    return first[lab].astype(np.uint32)


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4])


def three_statements(tiles, spec, what):
    """Host entry == numpy statement == scipy (labels), size == bincount of the labels, summary == summary_of."""
    host, stated = _capi.label_host(tiles, spec), label_tiles(tiles, spec)
    same(host, stated, what)
    member = spec.member_of_byte[tiles] != 0
    for t in range(len(tiles)):
        lab = host['label'][t]
        if ndimage is not None:
            assert np.array_equal(lab, scipy_labels(member[t], spec.connectivity)), (what, t, 'scipy')
        counts = np.bincount(lab.reshape(-1))
        assert np.array_equal(host['size'][t], np.where(lab > 0, counts[lab], 0)), (what, t, 'bincount')
        assert np.array_equal(lab > 0, member[t])
        small = member[t] & (host['size'][t] < spec.min_size)
        assert np.array_equal(host['sieved'][t], np.where(small, spec.replace, tiles[t])), (what, t, 'sieved')
    assert np.array_equal(host['summary'], summary_of(host['label'], host['size'], spec)), (what, 'summary')
    return host


SHAPES = ((1, 1), (1, 37), (41, 1), (2, 2), (7, 16), (33, 50), (40, 129))


@pytest.mark.parametrize('H,W', SHAPES)
def test_host_entry_numpy_statement_and_scipy_agree_on_every_pattern(H, W):
    """H == 1, W == 1 and shapes either side of 16 and of the kernels' rectangle: empty, all members, one pixel, checkerboard,
    diagonals of both slopes, spiral, serpentine, two bodies touching at a corner, the row-wrap pattern, noise at 0.1, 0.5,
    0.593 and 0.9 -- the patterns are the tiles of ONE plane, so neighbouring tiles must not connect either."""
    rng = np.random.default_rng(9000 + H * 131 + W)
    pats = C.patterns(H, W, rng)
    tiles, table = C.plane_of(np.stack(list(pats.values())), rng)
    for conn in (4, 8):
        host = three_statements(tiles, Spec(conn, 3, table, replace=77), (H, W, conn))
        names = list(pats)
        bodies = dict(zip(names, host['summary'][:, 0].tolist()))
        assert bodies['empty'] == 0 and bodies['full'] == 1 and bodies['one_pixel'] == 1 and bodies['spiral'] == 1 and bodies['serpentine'] == 1
        assert bodies['checkerboard'] == (1 if conn == 8 and min(H, W) >= 2 else (H * W + 1) // 2)      # (a line has no diagonals)
        if H >= 2 and W >= 2:
            assert bodies['corner_touch'] == (1 if conn == 8 else 2)
        if W >= 3:
            assert bodies['row_wrap'] == np.count_nonzero(pats['row_wrap'])          # every pixel its own body: rows do not wrap
        t = names.index('full')
        keep = int(H * W >= 3)                                        # (min_size is 3)
        assert host['summary'][t, :6].tolist() == [1, H * W, H * W, 1, keep, keep * H * W] and np.all(host['label'][t] == 1)


def test_rows_do_not_wrap_and_tiles_do_not_connect():
    """The last column of row y and the first column of row y + 1 are consecutive indices and two bodies; the last row of tile
    t and the first row of tile t + 1 are consecutive in memory and two bodies -- also with a stride equal to the raster."""
    table = np.zeros(256, dtype=np.uint8)
    table[1] = 1
    tile = np.zeros((1, 3, 5), dtype=np.uint8)
    tile[0, 0, 4] = tile[0, 1, 0] = 1
    for conn in (4, 8):
        host = three_statements(tile, Spec(conn, 1, table), ('wrap', conn))
        assert host['summary'][0, 0] == 2 and host['label'][0, 0, 4] == 5 and host['label'][0, 1, 0] == 6
    tiles = np.zeros((3, 4, 6), dtype=np.uint8)
    tiles[0, 3, :] = tiles[1, 0, :] = tiles[1, 3, 2] = tiles[2, 0, 2] = tiles[2, 0, 3] = 1
    for conn in (4, 8):
        host = three_statements(tiles, Spec(conn, 1, table), ('tiles', conn))
        assert host['summary'][:, 0].tolist() == [1, 2, 1] and host['summary'][:, 2].tolist() == [6, 6, 2]
        assert host['label'][1, 0, 0] == 1 and host['label'][0, 3, 0] == 19           # every tile counts from its own pixel 0


def test_a_table_where_only_byte_255_is_a_member():
    rng = np.random.default_rng(9010)
    tiles, table = C.plane_of(np.stack([C.noise(19, 35, d, rng) for d in C.DENSITIES]), rng, only_255=True)
    assert table.sum() == 1 and table[255] == 1
    for conn in (4, 8):
        host = three_statements(tiles, Spec(conn, 2, table, replace=0), ('only 255', conn))
        assert np.array_equal(host['label'] != 0, tiles == 255)
    # any non-zero table entry is a member; the value does not matter
    a = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    t1, t2 = (np.arange(256) % 3 == 0).astype(np.uint8), ((np.arange(256) % 3 == 0) * np.arange(1, 257) % 256).astype(np.uint8)
    t2[(np.arange(256) % 3 == 0) & (t2 == 0)] = 9
    same(_capi.label_host(a, Spec(8, 1, t1)), _capi.label_host(a, Spec(8, 1, t2)), 'table values')


def run_host(tiles, spec, stride=None, plane_off=0, out_off=0, want=KEYS):
    """dswx_label_host on a buffer [T][stride] whose first H * W bytes per tile are the rasters, placed `plane_off` bytes into
    an aligned allocation, every other byte PAD; the outputs `out_off` bytes into theirs, every output byte a sentinel
    beforehand.  Returns (rc, {output: plane}); nothing outside the wanted planes may have changed."""
    lib = _capi.load_library()
    T, H, W = tiles.shape
    n = H * W
    stride = n if stride is None else stride
    raw = np.full(max(T * stride, 1) + 64, PAD, dtype=np.uint8)
    base = (-raw.ctypes.data) % 16 + plane_off
    for t in range(T):
        raw[base + t * stride:base + t * stride + n] = tiles[t].reshape(-1)
    bufs, out = {}, _capi.LabelOut()
    for k in KEYS:
        count = T * (SUMMARY_WORDS if k == 'summary' else n)
        b = np.full(count * EB[k] + 64, SENT8, dtype=np.uint8)
        start = (-b.ctypes.data) % 16 + out_off
        bufs[k] = (b, start, count)
        if k in want:
            setattr(out, k, b.ctypes.data + start)
    rc = lib.dswx_label_host(raw.ctypes.data + base, ctypes.byref(_capi.LabelSpec.of(spec)), T, H, W, 0 if stride == n else stride,
                             ctypes.byref(out))
    res = {}
    for k in want:
        b, start, count = bufs[k]
        a = b[start:start + count * EB[k]].copy().view(_capi.LABEL_DTYPES[k])
        res[k] = a.reshape((T, SUMMARY_WORDS) if k == 'summary' else (T, H, W))
    for k, (b, start, count) in bufs.items():
        used = count * EB[k] if k in want else 0
        assert np.all(b[:start] == SENT8) and np.all(b[start + used:] == SENT8), k
    return rc, res


def test_strides_with_poisoned_padding_odd_addresses_and_every_subset_of_the_outputs():
    """The padding up to the stride and around the plane is full of a MEMBER byte and is not read; the plane and every output
    at odd addresses; label alone, label + size, label + size + one of the others, all four."""
    rng = np.random.default_rng(9020)
    cases = 0
    for (T, H, W) in ((0, 5, 7), (1, 1, 1), (3, 17, 33), (2, 32, 16), (4, 9, 130)):
        tiles, table = C.plane_of(rng.random((T, H, W)) < 0.55, rng)
        for conn in (4, 8):
            spec = Spec(conn, 1 + cases % 4, table, replace=(0, 255)[cases % 2])
            want = label_tiles(tiles, spec)
            for stride in (H * W, H * W + 3):
                for keys in (('label',), ('label', 'size'), ('label', 'size', 'sieved'), ('label', 'size', 'summary'), KEYS):
                    rc, got = run_host(tiles, spec, stride, plane_off=(0, 1, 7)[cases % 3], out_off=(0, 1, 2, 3)[cases % 4], want=keys)
                    assert rc == 0, _capi.load_library().dswx_last_error()
                    same(got, {k: want[k] for k in keys}, (T, H, W, conn, stride, keys))
                    cases += 1
    padded = np.full((4, 9 * 130 + 3), PAD, dtype=np.uint8)
    padded[:, :9 * 130] = tiles.reshape(4, -1)
    same(_capi.label_host(padded, spec, raster=(9, 130)), want, 'the Python wrapper on a padded plane')
    same(_capi.label_host(tiles, spec, want=('summary',)), {k: want[k] for k in ('label', 'size', 'summary')}, 'summary brings label and size')


def test_min_size_either_side_of_the_largest_body():
    """min_size 1 copies; 2 removes the specks; the largest size keeps exactly the largest bodies; one above removes every
    member."""
    rng = np.random.default_rng(9030)
    tiles, table = C.plane_of(rng.random((2, 31, 47)) < 0.45, rng)
    member = table[tiles] != 0
    for conn in (4, 8):
        base = _capi.label_host(tiles, Spec(conn, 1, table, replace=9))
        assert np.array_equal(base['sieved'], tiles) and np.array_equal(base['summary'][:, 4:6], base['summary'][:, 0:2])
        largest = int(base['summary'][:, 2].max())
        assert largest > 2
        for min_size in (2, largest, largest + 1):
            host = three_statements(tiles, Spec(conn, min_size, table, replace=9), (conn, min_size))
            kept = member & (host['size'] >= min_size)
            assert np.array_equal(host['sieved'] == 9, member & ~kept)
            assert host['summary'][:, 5].tolist() == kept.sum(axis=(1, 2)).tolist()
            if min_size == 2:
                assert np.array_equal(host['summary'][:, 0] - host['summary'][:, 4], host['summary'][:, 8])      # bin 0 = size 1
            if min_size == largest + 1:
                assert not kept.any() and host['summary'][:, 4].tolist() == [0, 0]
        # the largest body and the smallest label on a tie: two bodies of three pixels, the later one first in memory order
        tie = np.zeros((1, 4, 7), dtype=np.uint8)
        tie[0, 0, 4:7] = tie[0, 2, 0:3] = tie[0, 3, 6] = 1
        host = three_statements(tie, Spec(conn, 3, table), ('tie', conn))
        assert host['summary'][0, :6].tolist() == [3, 7, 3, 5, 2, 6] and host['summary'][0, 8:11].tolist() == [1, 2, 0]


def test_refusals_with_the_outputs_untouched():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    table = np.zeros(256, dtype=np.uint8)
    table[1] = 1
    good = Spec(8, 2, table, replace=0)
    H, W = 4, 6
    tiles = np.ones((3, H, W), dtype=np.uint8)
    n = 3 * H * W
    planes = {k: np.full((3 * SUMMARY_WORDS if k == 'summary' else n) * EB[k] + 16, SENT8, dtype=np.uint8) for k in KEYS}
    at = {k: planes[k].ctypes.data + (-planes[k].ctypes.data) % 8 for k in KEYS}

    def outs(**kw):
        o = _capi.LabelOut.of(**at)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def spec_c(**kw):
        s = _capi.LabelSpec.of(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def host(plane=tiles.ctypes.data, spec=None, n_tiles=3, height=H, width=W, stride=0, out=None, null_spec=False, null_out=False):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out
        return lib.dswx_label_host(plane, None if null_spec else ctypes.byref(spec), n_tiles, height, width, stride,
                                   None if null_out else ctypes.byref(out))

    def dev(plane=0x10000, spec=None, n_tiles=3, height=H, width=W, stride=0, out=None, null_spec=False, null_out=False, ctx=None):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out                   # host addresses, never dereferenced: every call fails first
        return lib.dswx_label_device(ctx, vp(plane) if plane else None, None if null_spec else ctypes.byref(spec), n_tiles, height,
                                     width, stride, None if null_out else ctypes.byref(out), None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        refused(call(null_spec=True), _capi.ERR_ARG, b'spec is NULL')
        refused(call(null_out=True), _capi.ERR_ARG, b'out is NULL')
        for c in (0, 1, 6, 16, -8):
            refused(call(spec=spec_c(connectivity=c)), _capi.ERR_ARG, b'connectivity')
        for v in (-1, 256, 1 << 20):
            refused(call(spec=spec_c(replace=v)), _capi.ERR_ARG, b'replace')
        refused(call(spec=spec_c(min_size=0)), _capi.ERR_ARG, b'min_size')
        for kw in ({'n_tiles': -1}, {'height': -1}, {'width': -1}, {'stride': -5}):
            refused(call(**kw), _capi.ERR_ARG, b'negative')
        refused(call(stride=H * W - 1), _capi.ERR_ARG, b'stride')
        refused(call(height=(1 << 31) + 1, width=1, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(height=1 << 16, width=(1 << 15) + 1, n_tiles=1), _capi.ERR_ARG, b'2^31')
        refused(call(height=1 << 40, width=1 << 40, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(plane=0), _capi.ERR_ARG, b'plane is NULL')
        refused(call(out=outs(label=None)), _capi.ERR_ARG, b'label is NULL')
        refused(call(out=outs(label=None, size=None, sieved=None, summary=None)), _capi.ERR_ARG, b'label is NULL')
        refused(call(out=outs(size=None)), _capi.ERR_ARG, b'size is NULL')
        refused(call(out=outs(size=None, summary=None)), _capi.ERR_ARG, b'sieved')
        refused(call(out=outs(size=None, sieved=None)), _capi.ERR_ARG, b'summary')
    # the device entry: alignment; then, with everything in order, the context -- checked last
    for off in (1, 2, 3):
        refused(dev(out=outs(label=at['label'] + off)), _capi.ERR_ALIGN, b'label')
        refused(dev(out=outs(size=at['size'] + off)), _capi.ERR_ALIGN, b'size')
    for off in (1, 2, 4, 7):
        refused(dev(out=outs(summary=at['summary'] + off)), _capi.ERR_ALIGN, b'summary')
    refused(dev(out=outs(sieved=at['sieved'] + 1)), _capi.ERR_ARG, b'ctx')                # sieved and the plane take any address
    refused(dev(plane=0x10001), _capi.ERR_ARG, b'ctx')
    refused(dev(), _capi.ERR_ARG, b'ctx')
    refused(dev(height=1 << 16, width=1 << 15, n_tiles=1), _capi.ERR_ARG, b'ctx')          # 2^31 pixels are legal
    refused(dev(plane=0, n_tiles=0), _capi.ERR_ARG, b'ctx')                              # nothing to read: no plane needed
    refused(dev(out=outs(size=None, sieved=None, summary=None)), _capi.ERR_ARG, b'ctx')   # label alone
    refused(dev(out=outs(sieved=None, summary=None)), _capi.ERR_ARG, b'ctx')
    refused(lib.dswx_batch_label(None, 14, ctypes.byref(spec_c()), 0, 1, ctypes.byref(outs()), None), _capi.ERR_ARG, b'batch is NULL')
    # a refused call wrote nothing
    for k in KEYS:
        assert np.all(planes[k] == SENT8), k
    # n_tiles == 0 or an empty raster is legal and writes nothing
    assert host(plane=None, n_tiles=0) == 0 and host(plane=None, height=0) == 0 and host(plane=None, width=0) == 0
    for k in KEYS:
        assert np.all(planes[k] == SENT8), k
    # and the same arguments, accepted: every pixel is a member, one body per tile
    assert host() == 0
    off = {k: at[k] - planes[k].ctypes.data for k in KEYS}
    assert np.all(planes['label'][off['label']:][:4 * n].view(np.uint32) == 1) and np.all(planes['size'][off['size']:][:4 * n].view(np.uint32) == H * W)
    assert np.all(planes['sieved'][off['sieved']:][:n] == 1)
    assert planes['summary'][off['summary']:][:8 * 3 * SUMMARY_WORDS].view(np.uint64).reshape(3, -1)[:, :6].tolist() == [[1, 24, 24, 1, 1, 24]] * 3
    # host buffers take any address
    assert host(out=outs(label=at['label'] + 1, size=at['size'] + 3, summary=at['summary'] + 5)) == 0
    # the Python side refuses what the library would
    for bad in (lambda: Spec(6, 1, table), lambda: Spec(8, 0, table), lambda: Spec(8, 1, table, replace=256), lambda: Spec(8, 1, table[:255]),
                lambda: label_tiles(np.zeros((2, 2, 2), dtype=np.int16), good), lambda: label_tiles(np.zeros((2, 2), dtype=np.uint8), good),
                lambda: _capi.label_host(np.zeros((2, 2, 2), dtype=np.uint16), good),
                lambda: _capi.label_host(tiles, good, want=('area',)), lambda: _capi.label_host(tiles, good, want=())):
        with pytest.raises(ValueError):
            bad()


def test_header_says_has_label_and_abi_7():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_LABEL 1' in text and '#define DSWX_LABEL_SUMMARY_WORDS 40' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert (_capi.HAS_LABEL, _capi.LABEL_SUMMARY_WORDS, SUMMARY_WORDS) == (1, 40, 40)
    assert text.index('---- grid:') < text.index('---- label:') < text.index('---- device plumbing')
    for name in ('dswx_label_device', 'dswx_batch_label', 'dswx_label_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    section = text[text.index('---- label:'):text.index('---- device plumbing')]
    assert 'deterministic and independent of the launch geometry' in section and 'order in which atomics' in section
    assert 'MUST NOT OVERLAP' in section and 'NOT CHECKED' in section
    assert 'renumbering' in section and 'GDAL' in section and 'No workgroup ever waits for another' in section
    rule = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_label_rule.h')).read()
    assert f'DSWX_LABEL_RECT_H = {_capi.LABEL_RECT_H};' in rule and f'DSWX_LABEL_RECT_W = {_capi.LABEL_RECT_W};' in rule


def test_struct_mirrors_match_offsetof_as_gcc_sees_the_header(tmp_path):
    assert ctypes.sizeof(_capi.LabelSpec) == 268
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    mirrors = {'dswx_label_spec_t': _capi.LabelSpec, 'dswx_label_out_t': _capi.LabelOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for st, cls in mirrors.items():
        for n, _ in cls._fields_:
            lines.append(f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));')
        lines.append(f'  printf("{st}.sizeof %zu\\n", sizeof({st}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'off.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'off'
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in mirrors.items():
        assert int(got[f'{st}.sizeof']) == ctypes.sizeof(cls), st
        for n, _ in cls._fields_:
            assert int(got[f'{st}.{n}']) == getattr(cls, n).offset, (st, n)
    o = _capi.LabelOut.of(label=16, size=None, summary=64)
    assert (o.label, o.size, o.sieved, o.summary) == (16, None, None, 64)
    s = _capi.LabelSpec.of(Spec(4, 17, np.arange(256) % 7, replace=3))
    assert (s.connectivity, s.replace, s.min_size) == (4, 3, 17) and list(s.member_of_byte) == [b % 7 for b in range(256)]


def test_wtr_label_spec_takes_category_0_of_the_stack_table():
    for collapsed in (True, False):
        for partial in (True, False):
            g, s = wtr_label_spec(5, collapsed=collapsed, partial_is_water=partial), wtr_spec(collapsed=collapsed, partial_is_water=partial)
            assert (g.connectivity, g.min_size, g.replace) == (8, 5, 0) and np.array_equal(g.member_of_byte != 0, s.cat_of_byte == 0)
    assert np.flatnonzero(wtr_label_spec(1).member_of_byte).tolist() == [1, 2]
    assert np.flatnonzero(wtr_label_spec(1, partial_is_water=False).member_of_byte).tolist() == [1]
    assert np.flatnonzero(wtr_label_spec(1, collapsed=False).member_of_byte).tolist() == [1, 2, 3, 4]
    # a lake of four pixels, a speck, cloud between them: the speck becomes "not water", everything else is copied
    tile = np.array([[[1, 1, 253, 2], [2, 1, 0, 0], [255, 0, 0, 252]]], dtype=np.uint8)
    got = label_tiles(tile, wtr_label_spec(2, connectivity=4))
    assert got['sieved'][0].tolist() == [[1, 1, 253, 0], [2, 1, 0, 0], [255, 0, 0, 252]]
    assert got['summary'][0, :6].tolist() == [2, 5, 4, 1, 1, 4] and got['label'][0, 0, 3] == 4


def test_host_entry_and_rule_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/label_host_san.cpp with proteus_amd/csrc/dswx_label.hip compiled into it, host code under ASan + UBSan:
    odd addresses, guard bytes around every output, heap blocks of exactly the bytes the entry may touch.  A child process;
    nothing is loaded into this interpreter."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'label_host_san')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'proteus_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'native', 'label_host_san.cpp'), os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_label.hip'), '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0 and 'libclang_rt.asan' in res.stderr:     # (only the runtime: an error in the sources must fail)
        pytest.skip(f'sanitizer runtime missing: {res.stderr[-300:]}')
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr and 'LeakSanitizer' not in res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out['failures'] == 0 and out['cases'] >= 100


def test_label_example_compiles_against_the_header(tmp_path):
    """examples/batch_label.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device the
    program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_label')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_label.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
