"""The reach entries on the host (include/dswx_hip.h "reach"): dswx_reach_host and proteus_amd.reach.reach_tiles pinned to each
other byte for byte (acc, mask, head), to a per-pixel loop over the predicate in Python ints, to a floating-point distance
from point to segment, and -- burn then reach -- to matplotlib.path inside OR distance <= R.  No GPU."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd import burn as BN
from proteus_amd.reach import HEAD_WORDS, MAX_RADIUS, Spec, reach_tiles
from tests import _reach_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('acc', 'mask', 'head')
SENT8 = 0xA5
CASES = K.named_cases()


@pytest.fixture(scope='module')
def results():
    """The host entry's outputs of every case, computed once."""
    return {c['name']: K.host(c, K.spec_of(c, burn=200, background=3)) for c in CASES}


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_three_statements_agree(c, results):
    """dswx_reach_host, reach_tiles and the per-pixel loop in Python ints: acc, mask and every head word of every tile."""
    got, want = results[c['name']], K.numpy_statement(c, K.spec_of(c, burn=200, background=3))
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (c['name'], k)
    assert np.array_equal(got['mask'], np.where(got['acc'] != 0, 200, 3).astype(np.uint8))
    for t in range(len(c['first']) - 1):
        acc, head = K.brute(K.tile_records(c, t), c['R'], c['H'], c['W'])
        assert np.array_equal(got['acc'][t], acc), (c['name'], t, np.argwhere(got['acc'][t] != acc)[:4])
        assert got['head'][t].tolist() == head + [0], (c['name'], t)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_float_distance_agrees_away_from_the_radius(c, results):
    """A second statement with no integer in it: the float distance from centre to segment decides every pixel whose distance
    is further than 0.05 pixel from R like the entry does, and abstains on at most 1 % of the case's pixels."""
    got = results[c['name']]
    n = len(c['first']) - 1
    abstained = 0
    for t in range(n):
        d = K.float_distance(K.tile_records(c, t), c['H'], c['W'])
        sure = np.abs(d - c['R']) > K.BAND
        abstained += int((~sure).sum())
        assert np.array_equal((got['acc'][t] != 0)[sure], (d <= c['R'])[sure]), (c['name'], t)
    print(c['name'], 'abstained on', abstained, 'of', n * c['H'] * c['W'])
    assert abstained <= K.SHARE * n * c['H'] * c['W'], (c['name'], abstained)


def test_what_the_named_cases_are_there_for(results):
    at = {c['name']: c for c in CASES}
    # the circle of 5 pixels around the centre of (40, 40) passes exactly through the centres at (3, 4), (4, 3), (5, 0), (0, 5)
    acc = results['point_circle']['acc'][0]
    for dc, dr in ((3, 4), (4, 3), (5, 0), (0, 5), (-3, -4), (-5, 0), (0, -5), (-4, 3)):
        assert acc[40 + dr, 40 + dc] == 1, (dc, dr)
    assert acc[40 + 4, 40 + 4] == 0 and acc[40, 40 + 6] == 0 and acc.sum() == 81
    # the corners of the tile: a quarter of the disc each, six rows; on five of them the disc also holds the centre beside the
    # raster (on the sixth, five pixels up or down, it holds the centre of its own column alone)
    head = results['point_circle']['head'][1]
    assert head[2] == 2 and head[4] == 5 and head[5] == 5 and head[3] == 12
    # both directions of every segment give the same pixels: acc is even everywhere
    for name in ('directions', 'outside', 'coast'):
        assert (results[name]['acc'] % 2 == 0).all(), name
    out = results['outside']
    assert (out['head'][:8, 6] > 0).all() and (out['head'][8:, 6] == 0).all() and (out['head'][8:, 2] == 0).all()
    assert out['acc'][0][:, 0].any() and not out['acc'][0][:, 2:].any()             # across the left side only
    assert out['acc'][4][0, 0] and out['acc'][4].sum() == out['acc'][4][:2, :2].sum()   # across the top left corner only
    # R = 0: the centres ON the edges, nothing else
    zero = results['radius_zero']
    assert zero['head'][:, 6].tolist() == [21, 31, 1, 56] and zero['acc'][2][40, 40] == 1 and zero['acc'][0][3, 4] == 2
    # the extremes: a tile wholly reached, tiles partly reached across a line that 64-bit arithmetic cannot place
    ext = results['extreme']['head'][:, 6].tolist()
    assert ext[2] == ext[4] == ext[5] == 96 * 96 and all(0 < ext[t] < 96 * 96 for t in (0, 1, 3))
    assert results['extreme']['head'][3].tolist()[:3] == [3, 0, 1]                  # (M, M) and (-M, M) are legal and reach nothing
    lon = results['long']
    assert lon['head'][0, 3] >= 2 * 300 and lon['head'][1, 3] == 2 * 300 and at['long']['H'] > 4 * 64
    pile = results['pile']
    assert pile['acc'][0][3, 3] == 3000 and pile['acc'][1][3, 3] == 3000 and pile['head'][:, 6].tolist() == [1, 1]
    bad = results['malformed']['head']
    assert bad[0].tolist()[:3] == [12, 8, 4] and bad[1].tolist() == [0] * 8 and bad[2].tolist()[:2] == [1, 1]
    assert results['decreasing']['head'][:, 0].tolist() == [8, 0, 4, 0, 4, 0, 0, 0]
    for c in CASES:
        r = results[c['name']]
        assert (r['head'][:, 7] == 0).all() and (r['head'][:, 2] <= r['head'][:, 0]).all() and (r['head'][:, 4] <= r['head'][:, 3]).all()
        if c['name'].startswith('width_'):                   # the edge across the whole width is cut at both sides on its rows
            assert r['head'][0, 4] == r['head'][0, 5] == r['head'][0, 3] > 0 and r['head'][3].tolist() == [0] * 8


def test_src_in_place_ors_the_reach_onto_a_burnt_mask_and_tile_strides():
    rng = np.random.default_rng(21)
    H, W, R = 24, 31, 2 * 256 + 77
    ring = np.array([(5.3, 4.1), (25.2, 6.6), (20.9, 19.4), (7.7, 15.2)])
    verts, first = BN.tiles([BN.records([BN.quantise(ring)], [1]), BN.records([BN.quantise(ring + 2.5)], [1])])
    burnt = _capi.burn_host(verts, first, H, W, BN.Spec(burn=1, background=0))
    alone = _capi.reach_host(verts, first, H, W, Spec(R))
    m = burnt['mask'].copy()
    res = _capi.reach_host(verts, first, H, W, Spec(R), src=m, mask=m)
    assert res['mask'] is m and np.array_equal(m, ((burnt['acc'] != 0) | (alone['acc'] != 0)).astype(np.uint8))
    assert (m > burnt['mask']).any() and (m > alone['mask']).any() and np.array_equal(res['acc'], alone['acc'])
    # src apart, with strides above height * width that differ: the bytes between the rasters stay as they are
    ms, ss = H * W + 7, H * W + 3
    wide_src = rng.integers(0, 256, size=(2, ss), dtype=np.uint8)
    wide = np.full((2, ms), SENT8, dtype=np.uint8)
    spec = Spec(R, 9, 1, ms, ss)
    res = _capi.reach_host(verts, first, H, W, spec, src=wide_src, mask=wide)
    want = reach_tiles(verts, first, H, W, spec, src=wide_src)
    assert np.array_equal(wide[:, :H * W].reshape(2, H, W), want['mask']) and (wide[:, H * W:] == SENT8).all()
    assert np.array_equal(want['mask'], np.where(alone['acc'] != 0, 9, wide_src[:, :H * W].reshape(2, H, W)))
    for keys in (('acc',), ('head',), ('mask',), ('mask', 'head')):
        res = _capi.reach_host(verts, first, H, W, Spec(R, 9, 1), want=keys)
        assert set(res) == set(keys) | {'acc'}
        for k in res:
            assert np.array_equal(res[k], np.where(alone['acc'] != 0, 9, 1) if k == 'mask' else alone[k]), (keys, k)


def test_burn_then_reach_is_the_buffered_polygon():
    """Polygons with odd coordinates on 96 x 96, R = 3.3 and 33.3 pixels: burn + reach in place equals matplotlib.path inside OR
    float distance to the ring <= R, wherever that distance is further than 0.05 pixel from R; at most 1 % abstained."""
    mpath = pytest.importorskip('matplotlib.path')
    rng = np.random.default_rng(6)
    H = W = 96
    ys, xs = np.mgrid[0:H, 0:W]
    centres = np.stack([256.0 * xs.ravel() + 128, 256.0 * ys.ravel() + 128], axis=1)
    for trial in range(8):
        k = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(8, 30, k)
        p = np.rint(256 * np.stack([48 + rad * np.cos(ang), 48 + rad * np.sin(ang)], axis=1)).astype(np.int64) | 1
        R = (845, 8525)[trial % 2]
        verts, first = BN.tiles([BN.records([p], [1])])
        m = _capi.burn_host(verts, first, H, W, BN.Spec())['mask']
        _capi.reach_host(verts, first, H, W, Spec(R), src=m, mask=m)
        inside = mpath.Path(np.concatenate([p, p[:1]]).astype(np.float64), closed=True).contains_points(centres).reshape(H, W)
        d = K.float_distance(verts, H, W)
        sure = np.abs(d - R) > K.BAND
        assert np.array_equal(m[0].astype(bool)[sure], (inside | (d <= R))[sure]), trial
        assert (~sure).sum() <= K.SHARE * H * W and inside.any() and (m[0].astype(bool) & ~inside).any()


def test_refusals_spec_header_and_struct_mirror(tmp_path):
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    c = CASES[1]
    n, H, W = len(c['first']) - 1, c['H'], c['W']
    verts = np.ascontiguousarray(c['verts'])
    acc = np.full(n * H * W + 4, 0xA5A5A5A5, dtype=np.uint32)
    out = _capi.BurnOut.of(acc=acc.ctypes.data)

    def spec_c(**kw):
        s = _capi.ReachSpec.of(Spec(300, 9, 1))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def host(spec, null_spec=False):
        return lib.dswx_reach_host(vp(verts.ctypes.data), vp(c['first'].ctypes.data), None if null_spec else ctypes.byref(spec), n, H, W, None, ctypes.byref(out))

    def dev(spec):
        return lib.dswx_reach_device(None, vp(0x10000), vp(0x20000), ctypes.byref(spec), n, H, W, None, ctypes.byref(out), None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        refused(call(spec_c(radius=MAX_RADIUS + 1)), _capi.ERR_ARG, b'radius 1048577 above DSWX_REACH_MAX_RADIUS 1048576 (1/256 pixel)')
        refused(call(spec_c(radius=0xFFFFFFFF)), _capi.ERR_ARG, b'radius')
        refused(call(spec_c(reserved=1)), _capi.ERR_ARG, b'reserved 1 must be 0')
        refused(call(spec_c(burn=256)), _capi.ERR_ARG, b'burn')                       # and the burn's own: one of each kind
        refused(call(spec_c(mask_tile_stride=H * W - 1)), _capi.ERR_ARG, b'mask_tile_stride')
    refused(host(None, null_spec=True), _capi.ERR_ARG, b'spec is NULL')
    refused(dev(spec_c()), _capi.ERR_ARG, b'ctx')                                     # everything in order: the context, checked last
    refused(dev(spec_c(radius=MAX_RADIUS)), _capi.ERR_ARG, b'ctx')
    refused(lib.dswx_batch_reach(None, 9, vp(0x10000), vp(0x20000), ctypes.byref(spec_c()), vp(acc.ctypes.data), None, 0, 1, None),
            _capi.ERR_ARG, b'batch is NULL')
    assert (acc == 0xA5A5A5A5).all()                                                  # a refused call wrote nothing
    assert host(spec_c(radius=MAX_RADIUS)) == 0 and (acc[:n * H * W] == 2).all() and (acc[n * H * W:] == 0xA5A5A5A5).all()
    for bad in (lambda: Spec(-1), lambda: Spec(MAX_RADIUS + 1), lambda: Spec(5, burn=256)):
        with pytest.raises(ValueError):
            bad()
    # the header and the mirrors
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_REACH 1' in text and '#define DSWX_REACH_HEAD_WORDS 8' in text and '#define DSWX_REACH_MAX_RADIUS (1 << 20)' in text
    assert (_capi.HAS_REACH, _capi.REACH_HEAD_WORDS, HEAD_WORDS, _capi.REACH_MAX_RADIUS, MAX_RADIUS) == (1, 8, 8, 1 << 20, 1 << 20)
    assert text.index('---- burn:') < text.index('---- reach:') < text.index('---- mosaic:') and lib.dswx_abi_version() == 7
    for name in ('dswx_reach_device', 'dswx_batch_reach', 'dswx_reach_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    rule = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_reach_rule.h')).read()
    assert f'#define DSWX_REACH_THREAD_ROWS {_capi.REACH_THREAD_ROWS}\n' in rule and f'#define DSWX_REACH_SCAN_STEP {_capi.REACH_SCAN_STEP}\n' in rule
    assert ctypes.sizeof(_capi.ReachSpec) == 32 and _capi.ANALYTIC_STRUCTS['dswx_reach_spec_t'] is _capi.ReachSpec
    if shutil.which('gcc') is None:
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for f, _ in _capi.ReachSpec._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(dswx_reach_spec_t, {f}));')
    lines += ['  printf("sizeof %zu\\n", sizeof(dswx_reach_spec_t));', '  printf("out %zu\\n", sizeof(dswx_reach_out_t));', '  return 0;', '}']
    (tmp_path / 'off.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'off.c'), '-o',
                    str(tmp_path / 'off')], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / 'off')], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got['sizeof']) == 32 and int(got['out']) == ctypes.sizeof(_capi.BurnOut)
    assert all(int(got[f]) == getattr(_capi.ReachSpec, f).offset for f, _ in _capi.ReachSpec._fields_)


def test_host_entry_and_rule_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/reach_host_san.cpp with proteus_amd/csrc/dswx_reach.hip (and dswx_burn.hip, whose checks it shares) compiled
    into it, host code under ASan + UBSan: odd addresses, heap blocks of exactly the bytes the entry may touch, coordinates up
    to and past +-2^30 with the largest radius (a signed overflow in the predicate would be a finding), every pixel against a
    256-bit statement of the predicate.  A child process; nothing is loaded into this interpreter."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'reach_host_san')
    csrc = os.path.join(ROOT, 'proteus_amd', 'csrc')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', csrc, os.path.join(ROOT, 'tests', 'native', 'reach_host_san.cpp'),
           os.path.join(csrc, 'dswx_reach.hip'), os.path.join(csrc, 'dswx_burn.hip'), '-o', exe]
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


def test_reach_example_compiles_against_the_header_and_leaves_quietly_without_a_device(tmp_path):
    """examples/batch_reach.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device the
    program says so and exits 0."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_reach')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_reach.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'no device' in r.stdout, (r.returncode, r.stdout, r.stderr)
