"""The LAND layer (create_landcover_mask :994-1115) over the whole byte domain, every entry and every tile geometry.

dswx_layers.hip has two kernels for it: dswx_landcover_v3 (four pixels per thread, 256-entry LDS code table, 256-bit
forest table in LDS), chosen when width % 4 == 0, the WorldCover, CGLS and LAND pointers are 4-byte aligned and the
LAND tile stride is a multiple of 4; dswx_landcover_v1 (one pixel per thread) otherwise.  Three entries reach them:
dswx_landcover_mask_host, _device (packed tiles) and _batch (an explicit LAND tile stride).  Every case here is
compared bit for bit with the numpy oracle (oracle/dswx_oracle.py), on inputs drawn by oracle/land_inputs.py: every
WorldCover and CGLS byte, the counted codes +-1, forest lists with 0, 255, duplicates and classes outside 0..255, any
int32 thresholds, and year offsets whose developed classes wrap modulo 256.  The layer entries do not set
last_kernel_info, so the kernel of each geometry case is named by `dispatch`, a restatement of the host's condition."""
import ctypes

import numpy as np
import pytest

from oracle import c_oracle
from oracle import dswx_oracle as o
from oracle import land_inputs as L
from proteus_amd import _capi
from proteus_amd.synth import SEED

SENTINEL = 0x77
SHAPES = [(1, 1), (1, 4), (1, 5), (3, 7), (33, 41), (64, 64), (65, 63), (100, 37), (257, 260)]
WC_MODES = ['classes', 'full', 'near', 'dense', 10, 50, 80, 95, 0, 255]
FOREST_KEYS = ['default', 'edge', 'all', 'none', 'empty']
THR_KEYS = list(L.THRESHOLD_SETS)
# 156 and -1 wrap the high / low class; -100 gives low = 156; the int32 ends wrap 100 + offset past 2^31
YEAR_OFFSETS = [0, 21, 99, 155, 156, 255, -1, -100, 2 ** 31 - 1, -2 ** 31]
N_SWEEP = 90


def sweep_cases():
    """Seeded draws over the five axes, each axis walked in its own shuffled order so that every value of every axis
    occurs (90 cases, not the 31,500 of the cross product)."""
    rng = np.random.default_rng(SEED + 7)
    axes = [SHAPES, WC_MODES, FOREST_KEYS, THR_KEYS, YEAR_OFFSETS]
    orders = [np.concatenate([rng.permutation(len(a)) for _ in range(-(-N_SWEEP // len(a)))]) for a in axes]
    return [tuple(a[order[i]] for a, order in zip(axes, orders)) for i in range(N_SWEEP)]


SWEEP = sweep_cases()


def sweep_inputs(i):
    (h, w), mode = SWEEP[i][:2]
    rng = np.random.default_rng(5000 + i)
    return L.worldcover(rng, h, w, mode), L.copernicus(rng, h, w)


def oracle(wc, cg, forest, thr, year_offset):
    return o.landcover_mask_from_warped(wc, cg, forest, year=2000 + year_offset, thresholds=thr)


def rule_of(wc, cg, forest, thr):
    """Which step of the hierarchy decides each pixel: 0 fill, 1 tree, 2 low, 3 high, 4 water (the later one wins)."""
    water, urban, tree = L.counts(wc)
    is_forest = np.isin(cg, [c for c in (forest or []) if 0 <= c <= 255])
    rule = np.zeros(cg.shape, np.int64)
    for k, hit in enumerate((np.where(is_forest, tree, 0) >= thr[0], urban >= thr[1], urban >= thr[2],
                             water >= thr[3]), 1):
        rule[hit] = k
    return rule


def dispatch(width, offsets, stride):
    """The host's choice between the kernels (land_launch): 'v3' or 'v1'."""
    return 'v3' if width % 4 == 0 and all(off % 4 == 0 for off in offsets) and stride % 4 == 0 else 'v1'


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


# ---- the byte domain through the host entry ---------------------------------------------------------------------
def test_sweep_is_not_vacuous():
    """Across the sweep every count (water, urban, tree) takes every value 0..9, every step of the hierarchy decides
    some pixel, and both kernels run (host entry: aligned device buffers, packed tiles)."""
    seen = [set(), set(), set()]
    rules, kernels = set(), set()
    for i, ((h, w), mode, fk, tk, off) in enumerate(SWEEP):
        wc, cg = sweep_inputs(i)
        for k, c in enumerate(L.counts(wc)):
            seen[k] |= set(np.unique(c).tolist())
        rules |= set(np.unique(rule_of(wc, cg, L.FOREST_SETS[fk], L.THRESHOLD_SETS[tk])).tolist())
        kernels.add(dispatch(w, (0, 0, 0), h * w))
    assert seen == [set(range(10))] * 3
    assert rules == {0, 1, 2, 3, 4}
    assert kernels == {'v1', 'v3'}
    assert {c[4] for c in SWEEP} == set(YEAR_OFFSETS) and {c[0] for c in SWEEP} == set(SHAPES)


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(N_SWEEP), ids=[f'{h}x{w}-{m}-{f}-{t.replace(" ", "_")}-{y}'
                                                   for (h, w), m, f, t, y in SWEEP])
def test_host_entry_domain_sweep(ctx, i):
    _, _, fk, tk, off = SWEEP[i]
    wc, cg = sweep_inputs(i)
    forest, thr = L.FOREST_SETS[fk], L.THRESHOLD_SETS[tk]
    got = ctx.landcover_mask(wc, cg, forest, thr, off)
    assert got.dtype == np.uint8 and np.array_equal(got, oracle(wc, cg, forest, thr, off))


# ---- geometry: tiles, pointer offsets, strides, sentinels ---------------------------------------------------------
# (n tiles, H, W, byte offsets of the WorldCover / CGLS / LAND pointers, LAND stride - H W, kernel the dispatch selects)
GEOMETRY = [
    (1, 33, 64, (0, 0, 0), 0, 'v3'),     # aligned, packed
    (2, 17, 40, (0, 0, 0), 4, 'v3'),     # aligned, stride H W + 4
    (3, 9, 36, (0, 0, 0), 1, 'v1'),      # W % 4 == 0, but the stride is odd
    (4, 21, 48, (1, 0, 0), 0, 'v1'),     # WorldCover pointer off by one byte
    (5, 8, 52, (0, 2, 0), 4, 'v1'),      # CGLS pointer off by two bytes
    (2, 30, 60, (0, 0, 3), 5, 'v1'),     # LAND pointer off by three bytes, odd stride
    (3, 11, 44, (3, 1, 2), 0, 'v1'),     # every pointer misaligned
    (1, 1, 4, (0, 0, 0), 0, 'v3'),       # one row of one quad
    (4, 1, 8, (0, 0, 0), 4, 'v3'),       # one-row tiles, stride H W + 4
    (1, 40, 45, (0, 0, 0), 0, 'v1'),     # W % 4 == 1
    (2, 19, 66, (0, 0, 0), 4, 'v1'),     # W % 4 == 2, aligned stride
    (3, 13, 39, (2, 3, 1), 1, 'v1'),     # W % 4 == 3, misaligned
    (5, 3, 5, (1, 1, 1), 5, 'v1'),       # tiny tiles
    (4, 1, 1, (0, 0, 0), 4, 'v1'),       # one pixel per tile
    (5, 25, 96, (0, 0, 0), 1, 'v1'),     # W % 4 == 0, odd stride, five tiles
    (5, 25, 96, (0, 0, 0), 4, 'v3'),     # the same five tiles, stride H W + 4
    (3, 37, 100, (0, 0, 0), 0, 'v3'),    # more than one 256-quad block per tile ...
    (3, 37, 100, (2, 0, 1), 0, 'v1'),    # ... and the same misaligned
]


def _upload_at(buf, arr, offset):
    if arr.size:
        buf.upload(arr.ravel(), offset)


def _device_entry(ctx, wc_ptr, cg_ptr, n, h, w, forest, thr, off, out_ptr):
    """dswx_landcover_mask_device (packed LAND tiles; Context.landcover_mask_device goes through _batch)."""
    fc = np.ascontiguousarray(list(forest or []), dtype=np.int32)
    t = np.ascontiguousarray(thr, dtype=np.int32)
    _capi._check(ctx.lib.dswx_landcover_mask_device(
        ctx.handle, ctypes.c_void_p(wc_ptr), ctypes.c_void_p(cg_ptr), int(n), int(h), int(w),
        ctypes.c_void_p(fc.ctypes.data) if fc.size else None, int(fc.size), ctypes.c_void_p(t.ctypes.data), int(off),
        ctypes.c_void_p(out_ptr), None))


@pytest.mark.gpu
@pytest.mark.parametrize('g', range(len(GEOMETRY)),
                         ids=[f'n{n}-{h}x{w}-off{"".join(map(str, offs))}-s{ds}-{k}' for n, h, w, offs, ds, k in GEOMETRY])
def test_batch_entry_at_any_address_and_stride(ctx, g):
    """The batch entry at the case's pointer offsets and stride, into a LAND buffer pre-filled with 0x77: every tile
    equals the oracle, every byte before, between and after the rasters is still 0x77.  The same inputs through the
    device entry, aligned and packed (v3 whenever W % 4 == 0), give the same rasters."""
    n, h, w, (o_wc, o_cg, o_land), ds, kernel = GEOMETRY[g]
    hw, stride = h * w, h * w + ds
    assert dispatch(w, (o_wc, o_cg, o_land), stride) == kernel
    rng = np.random.default_rng(7000 + g)
    modes = ['dense', 'classes', 'full', 'near', 'dense']
    wc = np.stack([L.worldcover(rng, h, w, modes[t]) for t in range(n)])
    cg = np.stack([L.copernicus(rng, h, w) for t in range(n)])
    forest, thr = L.FOREST_SETS[FOREST_KEYS[g % 3]], L.THRESHOLD_SETS[THR_KEYS[g % 2]]
    off = YEAR_OFFSETS[g % len(YEAR_OFFSETS)]
    exp = np.stack([oracle(wc[t], cg[t], forest, thr, off) for t in range(n)])
    slack = 64
    d_wc, d_cg = ctx.malloc(wc.nbytes + slack), ctx.malloc(cg.nbytes + slack)
    d_out = ctx.malloc(o_land + n * stride + slack)
    d_wc0, d_cg0, d_packed = ctx.malloc(wc.nbytes + slack), ctx.malloc(cg.nbytes + slack), ctx.malloc(n * hw + slack)
    try:
        _upload_at(d_wc, wc, o_wc)
        _upload_at(d_cg, cg, o_cg)
        ctx.lib.dswx_memset_d(ctx.handle, ctypes.c_void_p(d_out.ptr), SENTINEL, d_out.nbytes)
        ctx.landcover_mask_device(d_wc.ptr + o_wc, d_cg.ptr + o_cg, n, h, w, forest, d_out.ptr + o_land,
                                  thresholds=thr, year_offset=off, out_tile_stride=stride)
        ctx.synchronize()
        got = d_out.download(np.uint8, d_out.nbytes)
        assert (got[:o_land] == SENTINEL).all()
        for t in range(n):
            base = o_land + t * stride
            assert np.array_equal(got[base:base + hw].reshape(h, w), exp[t]), t
            assert (got[base + hw:base + stride] == SENTINEL).all(), t
        assert (got[o_land + n * stride:] == SENTINEL).all()
        # the twin: aligned pointers, packed tiles, the device entry (v3 when W % 4 == 0)
        _upload_at(d_wc0, wc, 0)
        _upload_at(d_cg0, cg, 0)
        ctx.lib.dswx_memset_d(ctx.handle, ctypes.c_void_p(d_packed.ptr), SENTINEL, d_packed.nbytes)
        _device_entry(ctx, d_wc0.ptr, d_cg0.ptr, n, h, w, forest, thr, off, d_packed.ptr)
        ctx.synchronize()
        twin = d_packed.download(np.uint8, d_packed.nbytes)
        assert (twin[n * hw:] == SENTINEL).all()
        twin = twin[:n * hw].reshape(n, h, w)
        assert np.array_equal(twin, exp)
        for t in range(n):
            base = o_land + t * stride
            assert np.array_equal(got[base:base + hw].reshape(h, w), twin[t]), t
    finally:
        for b in (d_wc, d_cg, d_out, d_wc0, d_cg0, d_packed):
            b.free()


def test_geometry_cases_reach_both_kernels():
    """The geometry table covers n = 1..5, W % 4 = 0..3, every pointer offset 0..3, strides H W + {0, 1, 4, 5}, and
    both kernels -- v3 also at a stride other than H W."""
    assert {c[0] for c in GEOMETRY} == {1, 2, 3, 4, 5}
    assert {c[2] % 4 for c in GEOMETRY} == {0, 1, 2, 3}
    for k in range(3):
        assert {c[3][k] for c in GEOMETRY} == {0, 1, 2, 3}
    assert {c[4] for c in GEOMETRY} == {0, 1, 4, 5}
    assert {c[5] for c in GEOMETRY} == {'v1', 'v3'}
    assert any(c[5] == 'v3' and c[4] != 0 for c in GEOMETRY)


# ---- full-size tiles into a DeviceBatch, then the classifier ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('n, h, w, align, kernel', [
    (3, 3660, 3660, 256, 'v3'),     # padded stride (a multiple of 256 pixels), W % 4 == 0
    (3, 1001, 1203, 1, 'v1'),       # contiguous tiles, W % 4 == 3: v1 at the batch stride
    (2, 999, 1002, 256, 'v1'),      # padded stride, W % 4 == 2
])
def test_land_into_the_batch_then_classify(ctx, n, h, w, align, kernel):
    """dswx_landcover_mask_batch writes LAND straight into the LAND plane of a resident DeviceBatch (the bench's chain
    and the product's device path); the classifier then reads it.  LAND and every output layer of every tile against
    the oracles, and the padding between the LAND rasters untouched."""
    b = _capi.DeviceBatch(ctx, n, h, w, masks=True, tile_align=align)
    d_wc = ctx.malloc(n * 9 * h * w)
    d_cg = ctx.malloc(n * h * w)
    try:
        assert dispatch(w, (0, 0, b.pin.land % 4), b.tile_stride) == kernel
        b.synth(SEED, tile0=880)
        forest, thr, off = L.EDGE_FOREST, L.THRESHOLD_SETS['standard'], 21
        exp_land = []
        for t in range(n):
            rng = np.random.default_rng(8800 + t)
            wc, cg = L.worldcover(rng, h, w, 'blocks'), L.copernicus(rng, h, w)
            d_wc.upload(wc.ravel(), t * 9 * h * w)
            d_cg.upload(cg.ravel(), t * h * w)
            exp_land.append(oracle(wc, cg, forest, thr, off))
            del wc, cg
        plane_bytes = n * b.tile_stride
        ctx.lib.dswx_memset_d(ctx.handle, ctypes.c_void_p(b.pin.land), SENTINEL, plane_bytes)
        ctx.landcover_mask_device(d_wc.ptr, d_cg.ptr, n, h, w, forest, b.pin.land, thresholds=thr, year_offset=off,
                                  out_tile_stride=b.tile_stride)
        ctx.synchronize()
        plane = np.empty(plane_bytes, np.uint8)
        _capi._check(ctx.lib.dswx_memcpy_d2h(ctx.handle, ctypes.c_void_p(plane.ctypes.data),
                                             ctypes.c_void_p(b.pin.land), plane_bytes))
        for t in range(n):
            base = t * b.tile_stride
            assert np.array_equal(plane[base:base + h * w].reshape(h, w), exp_land[t]), t
            assert (plane[base + h * w:base + b.tile_stride] == SENTINEL).all(), t
        rules = set()
        p = _capi.default_params()
        b.classify(p)
        ctx.synchronize()
        for t in range(n):
            host = {k: b.read_tile(k, t) for k in _capi.BAND_NAMES + ('fmask', 'shad', 'ocean')}
            assert np.array_equal(b.read_tile('land', t), exp_land[t]), t
            exp = c_oracle.classify(p, [host[k] for k in _capi.BAND_NAMES], host['fmask'], land=exp_land[t],
                                    shad=host['shad'], ocean=host['ocean'])
            for key in b.out_layers:
                assert np.array_equal(b.read_tile(key, t), exp[key]), (t, key)
            assert b.read_counters()[t].tolist() == exp['counters'].tolist(), t
            rules |= set(np.unique(exp_land[t]).tolist())
        assert {200, 201, 21, 121, 255} <= rules
    finally:
        b.free()
        d_wc.free()
        d_cg.free()


# ---- argument checks ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_arguments_refused_and_empty_rasters(ctx):
    from proteus_amd import pipeline
    h, w, n = 6, 8, 2
    rng = np.random.default_rng(99)
    wc = np.stack([L.worldcover(rng, h, w, 'dense') for _ in range(n)])
    cg = np.stack([L.copernicus(rng, h, w) for _ in range(n)])
    d_wc, d_cg, d_out = ctx.malloc(wc.nbytes), ctx.malloc(cg.nbytes), ctx.malloc(n * h * w + 64)
    try:
        d_wc.upload(wc.ravel())
        d_cg.upload(cg.ravel())
        ctx.lib.dswx_memset_d(ctx.handle, ctypes.c_void_p(d_out.ptr), SENTINEL, d_out.nbytes)
        for kw in (dict(n_tiles=n, out_tile_stride=h * w - 1), dict(n_tiles=-1), dict(n_tiles=65536)):
            kw = dict(dict(n_tiles=n, out_tile_stride=0), **kw)
            with pytest.raises(_capi.DswxError):
                ctx.landcover_mask_device(d_wc.ptr, d_cg.ptr, kw['n_tiles'], h, w, L.DEFAULT_FOREST, d_out.ptr,
                                          out_tile_stride=kw['out_tile_stride'])
        # zero-size rasters are no work: nothing is written
        for nn, hh, ww in ((0, h, w), (n, 0, w), (n, h, 0)):
            ctx.landcover_mask_device(d_wc.ptr, d_cg.ptr, nn, hh, ww, L.DEFAULT_FOREST, d_out.ptr, out_tile_stride=0)
            _device_entry(ctx, d_wc.ptr, d_cg.ptr, nn, hh, ww, L.DEFAULT_FOREST, (6, 3, 7, 3), 0, d_out.ptr)
        ctx.synchronize()
        assert (d_out.download(np.uint8, d_out.nbytes) == SENTINEL).all()
        for empty in ((0, 5), (5, 0)):
            got = ctx.landcover_mask(np.zeros((3 * empty[0], 3 * empty[1]), np.uint8), np.zeros(empty, np.uint8),
                                     L.DEFAULT_FOREST)
            assert got.shape == empty
    finally:
        d_wc.free()
        d_cg.free()
        d_out.free()
    # a WorldCover raster that is not 3 H x 3 W
    for bad in ((3 * h, 3 * w + 1), (3 * h - 1, 3 * w), (h, w)):
        with pytest.raises(ValueError):
            ctx.landcover_mask(np.zeros(bad, np.uint8), cg[0], L.DEFAULT_FOREST)
    eng = pipeline.TileEngine(ctx)
    try:
        for bad in ((3 * h, 3 * w + 1), (h, w)):
            with pytest.raises(ValueError):
                eng.landcover_mask(eng.upload(np.zeros(bad, np.uint8)), eng.upload(cg[0]), L.DEFAULT_FOREST,
                                   (6, 3, 7, 3), 0)
        got = eng.landcover_mask(eng.upload(wc[0]), eng.upload(cg[0]), L.EDGE_FOREST, (6, 3, 7, 3), -1).numpy()
        assert np.array_equal(got, oracle(wc[0], cg[0], L.EDGE_FOREST, (6, 3, 7, 3), -1))
    finally:
        eng.close()
