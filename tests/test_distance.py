"""The distance transform of include/dswx_hip.h ("distance") without a GPU: four statements pinned to each other -- the
library's scalar transform (dswx_distance_host), the numpy statement (proteus_amd/distance.py), a brute-force statement of the
definition written here (every pixel against every target, the tie rule of `nearest` included) and
scipy.ndimage.distance_transform_edt, exactly -- on every pattern of tests/_distance_cases.py at radii 0, 1, 2 and 5; the
summary against counts made another way; strides with poisoned padding, odd addresses; every refusal, with the outputs
untouched; the header; the struct mirrors; the WTR spec; the host entry under ASan + UBSan in a stand-alone program; the C
example."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.distance import NONE, SUMMARY_WORDS, Spec, distance_tiles, summary_of, wtr_distance_spec
from proteus_amd.label import wtr_label_spec
from tests import _distance_cases as C

try:
    from scipy import ndimage
except ImportError:                                # (only the comparison with scipy is skipped then)
    ndimage = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT8 = 0xEE
PAD = 200                                          # a TARGET byte of C.plane_of: padding that was read would be near
KEYS = ('dist2', 'nearest', 'within', 'summary')
EB = {'dist2': 4, 'nearest': 4, 'within': 1, 'summary': 8}
RADII = (0, 1, 2, 5)


def keys_of(radius):
    return KEYS if radius else ('dist2', 'nearest', 'summary')


def brute(target, radius):
    """The definition, pixel by pixel: the smallest (d2, xq, yq) over the targets q that reach p."""
    H, W = target.shape
    ys, xs = (a.astype(np.int64) for a in np.nonzero(target))
    dist2 = np.full((H, W), NONE, dtype=np.uint32)
    nearest = np.full((H, W), NONE, dtype=np.uint32)
    if not len(ys):
        return dist2, nearest
    for y in range(H):
        for x in range(W):
            d2 = (ys - y) ** 2 + (xs - x) ** 2
            k = np.argmin((d2 << 40) | (xs << 20) | ys)                 # the smallest (d2, xq, yq) over ALL targets ...
            if radius == 0 or d2[k] <= radius * radius:                  # ... reaches p or none does: it has the smallest d2
                dist2[y, x], nearest[y, x] = d2[k], ys[k] * W + xs[k]
    return dist2, nearest


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4])


def four_statements(tiles, spec, what, brute_force=True):
    """Host entry == numpy statement == brute force; dist2 == scipy squared (R == 0, a plane with a target); nearest names a
    target at exactly dist2; within and the summary from dist2."""
    keys = keys_of(spec.max_radius)
    host, stated = _capi.distance_host(tiles, spec, want=keys), distance_tiles(tiles, spec)
    same(host, stated, what)
    target = spec.target_of_byte[tiles] != 0
    n, H, W = tiles.shape
    for t in range(n):
        d2, near = host['dist2'][t], host['nearest'][t]
        if brute_force:
            bd, bn = brute(target[t], spec.max_radius)
            assert np.array_equal(d2, bd) and np.array_equal(near, bn), (what, t, 'brute force')
        if ndimage is not None and spec.max_radius == 0 and target[t].any():
            assert np.array_equal(d2, np.rint(ndimage.distance_transform_edt(~target[t]) ** 2).astype(np.uint32)), (what, t, 'scipy')
        reached = d2 != NONE
        assert np.array_equal(near != NONE, reached) and np.array_equal(d2 == 0, target[t])
        yy, xx = np.indices((H, W))
        qy, qx = near[reached].astype(np.int64) // W, near[reached].astype(np.int64) % W
        assert np.all(target[t][qy, qx]) and np.array_equal((yy[reached] - qy) ** 2 + (xx[reached] - qx) ** 2, d2[reached]), (what, t, 'nearest')
        if spec.max_radius:
            assert np.all(d2[reached] <= spec.max_radius ** 2)
            assert np.array_equal(host['within'][t], np.where(reached & ~target[t], spec.mark, tiles[t])), (what, t, 'within')
        else:
            assert reached.all() == bool(target[t].any()) and (reached.any() == reached.all())
    assert np.array_equal(host['summary'], summary_of(host['dist2'])), (what, 'summary')
    return host


@pytest.mark.parametrize('W', (1, 15, 16, 17, 40))
def test_host_entry_numpy_statement_brute_force_and_scipy_agree_on_every_pattern(W):
    """This width x H in {1, 2, 7, 16, 17, 33} x R in {0, 1, 2, 5}: no target, all targets, one target in each corner and in
    the centre, one full row, one full column, a diagonal, two targets equidistant from many pixels, a checkerboard, noise at
    0.5, 0.05 and 0.002 -- the patterns are the tiles of ONE plane, so neighbouring tiles must not see each other."""
    for H in (1, 2, 7, 16, 17, 33):
        rng = np.random.default_rng(9000 + H * 131 + W)
        pats = C.patterns(H, W, rng)
        tiles, table = C.plane_of(np.stack(list(pats.values())), rng)
        for radius in RADII:
            four_statements(tiles, Spec(table, radius, mark=(7, 99)[radius % 2]), (H, W, radius))


def test_the_tie_rule_smallest_column_then_smallest_row():
    table = np.zeros(256, dtype=np.uint8)
    table[1] = 1
    t = np.zeros((1, 5, 5), dtype=np.uint8)
    t[0, 0, 2] = t[0, 2, 0] = t[0, 2, 4] = t[0, 4, 2] = 1          # four targets at distance 2 from the centre
    host = four_statements(t, Spec(table), 'cross')
    assert host['dist2'][0, 2, 2] == 4 and host['nearest'][0, 2, 2] == 2 * 5 + 0          # the smallest column
    t = np.zeros((1, 5, 3), dtype=np.uint8)
    t[0, 0, 1] = t[0, 4, 1] = 1                                      # one column, above and below
    host = four_statements(t, Spec(table), 'column')
    assert host['nearest'][0, 2].tolist() == [1, 1, 1]                                    # the smallest row
    t = np.zeros((1, 3, 4), dtype=np.uint8)
    t[0, 0, 0] = t[0, 2, 1] = 1                                      # two targets, no tie: (0, 2) is 4 from the first and 5 from the second
    host = four_statements(t, Spec(table), 'two')
    assert host['nearest'][0].tolist() == [[0, 0, 0, 9], [0, 9, 9, 9], [9, 9, 9, 9]]
    # a radius that cuts the diagonal neighbour off: d2 == 2 > 1 * 1
    host = four_statements(t, Spec(table, 1, mark=5), 'radius 1')
    assert host['dist2'][0].tolist() == [[0, 1, NONE, NONE], [1, 1, NONE, NONE], [1, 0, 1, NONE]]
    assert host['within'][0].tolist() == [[1, 5, 0, 0], [5, 5, 0, 0], [5, 1, 5, 0]]
    assert host['summary'][0, :6].tolist() == [2, 5, 5, 1, 1, 5] and host['summary'][0, 8:10].tolist() == [5, 0]


def test_summary_against_counts_made_another_way():
    rng = np.random.default_rng(9050)
    tiles, table = C.plane_of(np.stack([C.noise(37, 53, d, rng) for d in C.DENSITIES] + [C.empty(37, 53), C.full(37, 53)]), rng)
    for radius in (0, 4):
        host = _capi.distance_host(tiles, Spec(table, radius), want=('dist2', 'summary'))
        for t in range(len(tiles)):
            d = host['dist2'][t].reshape(-1).astype(np.int64)
            s = host['summary'][t]
            reached = d != NONE
            assert s[0] == np.count_nonzero(table[tiles[t]]) and s[0] + s[1] + s[2] == d.size and s[2] == np.count_nonzero(~reached)
            assert s[6] == s[7] == 0
            if reached.any():
                assert s[3] == d[reached].max() and s[4] == np.argmax(np.where(reached, d, -1)) and s[5] == d[reached].sum()
            else:
                assert s[3] == s[4] == s[5] == 0
            ring = d[reached & (d > 0)]
            bins = np.bincount(np.floor(np.log2(ring)).astype(int), minlength=32) if ring.size else np.zeros(32, dtype=int)
            assert s[8:].tolist() == bins.tolist() and s[8:].sum() == s[1]


def test_padded_strides_odd_addresses_and_a_table_with_one_target_byte():
    rng = np.random.default_rng(9060)
    H, W, T = 9, 21, 3
    plane, table = C.plane_of(np.stack([C.noise(H, W, d, rng) for d in C.DENSITIES]), rng, only_255=True)
    spec = Spec(table, 3, mark=4)
    want = distance_tiles(plane, spec)
    stride = H * W + 11
    padded = np.full((T, stride), 255, dtype=np.uint8)               # the padding is full of the target byte
    padded[:, :H * W] = plane.reshape(T, -1)
    same(_capi.distance_host(padded, spec, want=KEYS, raster=(H, W)), want, 'padded')
    # every buffer at an odd address, through the C entry itself
    lib = _capi.load_library()
    src = np.full(T * stride + 3, 255, dtype=np.uint8)
    src[3:] = padded.reshape(-1)
    bufs = {k: np.full((T * (SUMMARY_WORDS if k == 'summary' else H * W)) * EB[k] + 9, SENT8, dtype=np.uint8) for k in KEYS}
    off = {'dist2': 1, 'nearest': 3, 'within': 5, 'summary': 7}
    out = _capi.DistanceOut.of(**{k: bufs[k].ctypes.data + off[k] for k in KEYS})
    assert lib.dswx_distance_host(src.ctypes.data + 3, ctypes.byref(_capi.DistanceSpec.of(spec)), T, H, W, stride, ctypes.byref(out)) == 0
    for k in KEYS:
        nb = want[k].size * EB[k]
        assert np.array_equal(bufs[k][off[k]:off[k] + nb].copy().view(want[k].dtype), want[k].reshape(-1)), k
        assert np.all(bufs[k][:off[k]] == SENT8) and np.all(bufs[k][off[k] + nb:] == SENT8), k


def test_refusals_with_the_outputs_untouched():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    table = np.zeros(256, dtype=np.uint8)
    table[1] = 1
    good = Spec(table, 2, mark=9)
    H, W = 4, 6
    tiles = np.ones((3, H, W), dtype=np.uint8)
    n = 3 * H * W
    planes = {k: np.full((3 * SUMMARY_WORDS if k == 'summary' else n) * EB[k] + 16, SENT8, dtype=np.uint8) for k in KEYS}
    at = {k: planes[k].ctypes.data + (-planes[k].ctypes.data) % 8 for k in KEYS}

    def outs(**kw):
        o = _capi.DistanceOut.of(**at)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def spec_c(**kw):
        s = _capi.DistanceSpec.of(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def host(plane=tiles.ctypes.data, spec=None, n_tiles=3, height=H, width=W, stride=0, out=None, null_spec=False, null_out=False):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out
        return lib.dswx_distance_host(plane, None if null_spec else ctypes.byref(spec), n_tiles, height, width, stride,
                                      None if null_out else ctypes.byref(out))

    def dev(plane=0x10000, spec=None, n_tiles=3, height=H, width=W, stride=0, out=None, null_spec=False, null_out=False, ctx=None):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out                   # host addresses, never dereferenced: every call fails first
        return lib.dswx_distance_device(ctx, vp(plane) if plane else None, None if null_spec else ctypes.byref(spec), n_tiles, height,
                                        width, stride, None if null_out else ctypes.byref(out), None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        refused(call(null_spec=True), _capi.ERR_ARG, b'spec is NULL')
        refused(call(null_out=True), _capi.ERR_ARG, b'out is NULL')
        for v in (-1, 256, 1 << 20):
            refused(call(spec=spec_c(mark=v)), _capi.ERR_ARG, b'mark')
        for kw in ({'n_tiles': -1}, {'height': -1}, {'width': -1}, {'stride': -5}):
            refused(call(**kw), _capi.ERR_ARG, b'negative')
        refused(call(stride=H * W - 1), _capi.ERR_ARG, b'stride')
        refused(call(height=46341, width=1, n_tiles=1), _capi.ERR_ARG, b'46340')
        refused(call(height=1, width=46341, n_tiles=1), _capi.ERR_ARG, b'46340')
        refused(call(height=1 << 40, width=1 << 40, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(height=1, width=_capi.DISTANCE_MAX_WIDTH + 1, n_tiles=1), _capi.ERR_ARG, b'DSWX_DISTANCE_MAX_WIDTH')
        refused(call(height=46340, width=8192, n_tiles=1 << 33), _capi.ERR_ARG, b'too large')
        refused(call(plane=0), _capi.ERR_ARG, b'plane is NULL')
        refused(call(out=outs(dist2=None)), _capi.ERR_ARG, b'dist2 is NULL')
        refused(call(out=outs(dist2=None, nearest=None, within=None, summary=None)), _capi.ERR_ARG, b'dist2 is NULL')
        refused(call(spec=spec_c(max_radius=0)), _capi.ERR_ARG, b'within')
    # the device entry: alignment; then, with everything in order, the context -- checked last
    for off in (1, 2, 3):
        refused(dev(out=outs(dist2=at['dist2'] + off)), _capi.ERR_ALIGN, b'dist2')
        refused(dev(out=outs(nearest=at['nearest'] + off)), _capi.ERR_ALIGN, b'nearest')
    for off in (1, 2, 4, 7):
        refused(dev(out=outs(summary=at['summary'] + off)), _capi.ERR_ALIGN, b'summary')
    refused(dev(out=outs(within=at['within'] + 1)), _capi.ERR_ARG, b'ctx')                # within and the plane take any address
    refused(dev(plane=0x10001), _capi.ERR_ARG, b'ctx')
    refused(dev(), _capi.ERR_ARG, b'ctx')
    refused(dev(height=46340, width=_capi.DISTANCE_MAX_WIDTH, n_tiles=1), _capi.ERR_ARG, b'ctx')     # the largest raster is legal
    refused(dev(plane=0, n_tiles=0), _capi.ERR_ARG, b'ctx')                              # nothing to read: no plane needed
    refused(dev(out=outs(nearest=None, within=None, summary=None)), _capi.ERR_ARG, b'ctx')  # dist2 alone
    refused(dev(spec=spec_c(max_radius=0), out=outs(within=None)), _capi.ERR_ARG, b'ctx')
    refused(lib.dswx_batch_distance(None, 14, ctypes.byref(spec_c()), 0, 1, ctypes.byref(outs()), None), _capi.ERR_ARG, b'batch is NULL')
    # a refused call wrote nothing
    for k in KEYS:
        assert np.all(planes[k] == SENT8), k
    # n_tiles == 0 or an empty raster is legal and writes nothing
    assert host(plane=None, n_tiles=0) == 0 and host(plane=None, height=0) == 0 and host(plane=None, width=0) == 0
    for k in KEYS:
        assert np.all(planes[k] == SENT8), k
    # and the same arguments, accepted: every pixel is a target
    assert host() == 0
    off = {k: at[k] - planes[k].ctypes.data for k in KEYS}
    assert np.all(planes['dist2'][off['dist2']:][:4 * n].view(np.uint32) == 0)
    assert planes['nearest'][off['nearest']:][:4 * n].view(np.uint32).tolist() == list(range(H * W)) * 3
    assert np.all(planes['within'][off['within']:][:n] == 1)
    assert planes['summary'][off['summary']:][:8 * 3 * SUMMARY_WORDS].view(np.uint64).reshape(3, -1)[:, :6].tolist() == [[24, 0, 0, 0, 0, 0]] * 3
    # host buffers take any address
    assert host(out=outs(dist2=at['dist2'] + 1, nearest=at['nearest'] + 3, summary=at['summary'] + 5)) == 0
    # the Python side refuses what the library would
    for bad in (lambda: Spec(table, -1), lambda: Spec(table, 1 << 32), lambda: Spec(table, 1, mark=256), lambda: Spec(table, 1, mark=-1),
                lambda: Spec(table[:255]), lambda: distance_tiles(np.zeros((2, 2, 2), dtype=np.int16), good),
                lambda: distance_tiles(np.zeros((2, 2), dtype=np.uint8), good),
                lambda: _capi.distance_host(np.zeros((2, 2, 2), dtype=np.uint16), good),
                lambda: _capi.distance_host(tiles, good, want=('area',)), lambda: _capi.distance_host(tiles, good, want=()),
                lambda: _capi.distance_host(tiles, Spec(table), want=('within',)),
                lambda: _capi.distance_host(np.zeros((1, 1, _capi.DISTANCE_MAX_WIDTH + 1), dtype=np.uint8), good),
                lambda: _capi.distance_host(np.zeros((1, 46341), dtype=np.uint8), good, raster=(46341, 1))):
        with pytest.raises(ValueError):
            bad()


def test_header_says_has_distance_and_abi_7():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_DISTANCE 1' in text and '#define DSWX_DISTANCE_SUMMARY_WORDS 40' in text
    assert '#define DSWX_DISTANCE_NONE 0xFFFFFFFFu' in text and f'#define DSWX_DISTANCE_MAX_WIDTH {_capi.DISTANCE_MAX_WIDTH}' in text
    assert f'#define DSWX_DISTANCE_MAX_SIDE {_capi.DISTANCE_MAX_SIDE}' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert (_capi.HAS_DISTANCE, _capi.DISTANCE_SUMMARY_WORDS, SUMMARY_WORDS, _capi.DISTANCE_NONE, NONE) == (1, 40, 40, 0xFFFFFFFF, 0xFFFFFFFF)
    assert _capi.DISTANCE_MAX_WIDTH >= 8192 and (_capi.DISTANCE_MAX_SIDE - 1) ** 2 * 2 < NONE and _capi.DISTANCE_MAX_SIDE ** 2 < 1 << 31
    assert text.index('---- body table:') < text.index('---- distance:') < text.index('---- device plumbing')
    for name in ('dswx_distance_device', 'dswx_batch_distance', 'dswx_distance_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    section = text[text.index('---- distance:'):text.index('---- device plumbing')]
    assert 'deterministic and independent of the launch geometry' in section and 'order in which atomics' in section
    assert 'MUST NOT OVERLAP' in section and 'NOT CHECKED' in section and 'No workgroup ever waits for another' in section
    assert 'lexicographic in (d2, xq, yq)' in section and 'distance_transform_edt' in section and '160 KiB' in section
    rule = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_distance_rule.h')).read()
    for name, v in (('BAND_H', _capi.DISTANCE_BAND_H), ('COLS', _capi.DISTANCE_COLS), ('BLOCK_W', _capi.DISTANCE_BLOCK_W), ('NEAR', _capi.DISTANCE_NEAR)):
        assert f'DSWX_DISTANCE_{name} = {v};' in rule, name


def test_struct_mirrors_match_offsetof_as_gcc_sees_the_header(tmp_path):
    assert ctypes.sizeof(_capi.DistanceSpec) == 264
    assert _capi.ANALYTIC_STRUCTS['dswx_distance_spec_t'] is _capi.DistanceSpec and _capi.ANALYTIC_STRUCTS['dswx_distance_out_t'] is _capi.DistanceOut
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    mirrors = {'dswx_distance_spec_t': _capi.DistanceSpec, 'dswx_distance_out_t': _capi.DistanceOut}
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
    o = _capi.DistanceOut.of(dist2=16, nearest=None, summary=64)
    assert (o.dist2, o.nearest, o.within, o.summary) == (16, None, None, 64)
    s = _capi.DistanceSpec.of(Spec(np.arange(256) % 7, 17, mark=3))
    assert (s.max_radius, s.mark) == (17, 3) and list(s.target_of_byte) == [b % 7 for b in range(256)]


def test_wtr_distance_spec_takes_the_members_of_the_label_spec():
    for collapsed in (True, False):
        for partial in (True, False):
            d, g = wtr_distance_spec(3, collapsed=collapsed, partial_is_water=partial), wtr_label_spec(1, collapsed=collapsed, partial_is_water=partial)
            assert (d.max_radius, d.mark) == (3, 200) and np.array_equal(d.target_of_byte != 0, g.member_of_byte != 0)
    assert np.flatnonzero(wtr_distance_spec().target_of_byte).tolist() == [1, 2] and wtr_distance_spec().max_radius == 0
    assert np.flatnonzero(wtr_distance_spec(partial_is_water=False).target_of_byte).tolist() == [1]
    assert np.flatnonzero(wtr_distance_spec(collapsed=False).target_of_byte).tolist() == [1, 2, 3, 4]
    # a lake, cloud and land: the ring of one pixel round the water, cloud included, is marked; the water itself is copied
    tile = np.array([[[1, 1, 253, 0], [2, 0, 0, 0], [255, 0, 0, 252]]], dtype=np.uint8)
    got = distance_tiles(tile, wtr_distance_spec(1, mark=9))
    assert got['within'][0].tolist() == [[1, 1, 9, 0], [2, 9, 0, 0], [9, 0, 0, 252]]
    assert got['dist2'][0, 2].tolist() == [1, NONE, NONE, NONE] and got['summary'][0, :6].tolist() == [3, 3, 6, 1, 2, 3]


def test_host_entry_and_rule_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/distance_host_san.cpp with proteus_amd/csrc/dswx_distance.hip compiled into it, host code under ASan +
    UBSan: odd addresses, guard bytes around every output, heap blocks of exactly the bytes the entry may touch.  A child
    process; nothing is loaded into this interpreter."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'distance_host_san')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'proteus_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'native', 'distance_host_san.cpp'), os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_distance.hip'), '-o', exe]
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


def test_distance_example_compiles_against_the_header(tmp_path):
    """examples/batch_distance.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device the
    program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_distance')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_distance.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
