"""The quotient thresholds (wigt, pswt_1_mndwi, pswt_2_mndwi, pswt_1_ndvi) and awgt over the domain dswx_make_dev_params
accepts, on every form the division-free predicate has on the device.

fl64(n / d) > t is never computed on the device: quot_gt / quot_lt (dswx_device.h: the direct kernel dswx_classify_v8 and the
generic dswx_classify_v1) compare r = fma(-t, d, n) with h * d, lut_group (dswx_tables.h: the table-driven kernel, its MASKS
and 'cover' stage-1 instantiations) takes the sign of a second fma, and both get t's half gaps from dswx_make_dev_params.
The pixels are those of oracle/quotient_inputs.py -- for every d the reachable n either side of t * d, quotients equal to
the threshold, n / 0 and 0 / 0 -- which tests/test_quotient_domain.py shows on the CPU to separate every threshold from its
neighbours.  Every comparison is equality with the scalar C oracle (true division): the eight integer layers and the three
counters, all written over a sentinel."""
import ctypes
import functools
import math

import numpy as np
import pytest

from oracle import c_oracle
from oracle import quotient_inputs as qi
from proteus_amd import _capi
from tests.test_gpu_band_domain import ALL_LAYERS, ctxs        # noqa: F401  (ctxs is a fixture)
from tests.test_gpu_raster_domain import Dev, SENTINELS

pytestmark = pytest.mark.gpu

ERR_ARG = -1                                   # DSWX_ERR_ARG (include/dswx_hip.h)
SENT = SENTINELS[0]                            # 0xA5: no layer value, no DIAG half and no plausible counter byte
FORMS = ('lut plain', 'lut masks', 'cover', 'direct', 'generic')
WIDTH = 56                                     # the builder's rows are multiples of 56 pixels: [N / 56, 56] rasters, tiles of 7
KERNEL_OF = {'lut plain': 'dswx_classify_lut', 'lut masks': 'dswx_classify_lut', 'cover': 'dswx_classify_lut',
             'direct': 'dswx_classify_v8', 'generic': 'dswx_classify_v1'}


def params(thr, collapse=True, mode='mask', clip=False):
    return _capi.make_params(thr, band_fills=[None] * 6, fmask_fill=None, clip_negative_reflectance=clip,
                             collapse_wtr_classes=collapse, mask_adjacent_to_cloud_mode=mode)


def mask_planes(n):
    """LAND through all bytes, SHAD and OCEAN 0 / 1 (the counters then differ from the pixel count)."""
    i = np.arange(n, dtype=np.int64)
    return dict(land=((i * 13 + (i >> 8) * 7) & 255).astype(np.uint8), shad=(i % 3 != 0).astype(np.uint8),
                ocean=(i % 9 != 0).astype(np.uint8))


def dtype_of(layer):
    return np.uint16 if layer == 'diag' else np.uint8


def host_run(ctx, p, bands, fm, masks=None, layers=ALL_LAYERS):
    """dswx_classify_host on one [H, W] raster with every output and the counters pre-filled with the sentinel.
    Returns (status, {layer: array, 'counters': [3]})."""
    h, w = bands[0].shape
    keep = [np.ascontiguousarray(b, np.int16) for b in bands] + [np.ascontiguousarray(fm, np.uint8)]
    pin, pout = _capi.PlanesIn(), _capi.PlanesOut()
    for i in range(6):
        pin.band[i] = keep[i].ctypes.data
    pin.fmask = keep[6].ctypes.data
    for m, v in (masks or {}).items():
        keep.append(np.ascontiguousarray(v, np.uint8).reshape(h, w))
        setattr(pin, m, keep[-1].ctypes.data)
    res = {k: np.full((h, w), SENT * 0x0101 if k == 'diag' else SENT, dtype_of(k)) for k in layers}
    for k in layers:
        setattr(pout, k, res[k].ctypes.data)
    cnt = np.full(3, SENT, np.int64)
    rc = ctx.lib.dswx_classify_host(ctx.handle, ctypes.byref(p), 1, h, w, ctypes.byref(pin), ctypes.byref(pout),
                                    _capi._host_ptr(cnt))
    res['counters'] = cnt
    return rc, res


def untouched(res):
    return all((v.view(np.uint8) == SENT).all() for k, v in res.items() if k != 'counters') and \
        (res['counters'] == SENT).all()


class DeviceCase:
    """The planes of `bands` / `fm` / `masks` ([T * stride] pixels each) on the device at `off` bytes past a 256-byte
    boundary, and sentinel-filled outputs and counters for `n_launches` launches."""

    def __init__(self, dev, bands, fm, masks, n_tiles, off=0, n_launches=1):
        self.dev, self.n_tiles, self.size = dev, n_tiles, bands[0].size
        self.pin = _capi.PlanesIn()
        for i in range(6):
            self.pin.band[i] = dev.put(np.ascontiguousarray(bands[i], np.int16).ravel(), off).ptr
        self.pin.fmask = dev.put(np.ascontiguousarray(fm, np.uint8).ravel(), off).ptr
        for m, v in (masks or {}).items():
            setattr(self.pin, m, dev.put(np.ascontiguousarray(v, np.uint8).ravel(), off).ptr)
        self.launches = []
        for _ in range(n_launches):
            outs = {k: dev.span(self.size * (2 if k == 'diag' else 1), off) for k in ALL_LAYERS}
            cnt = dev.span(n_tiles * 24)
            pout = _capi.PlanesOut()
            for k, s in outs.items():
                s.fill(SENT)
                setattr(pout, k, s.ptr)
            cnt.fill(SENT)
            self.launches.append((pout, outs, cnt))

    def read(self, launch=0):
        """{layer: flat array, 'counters': [T, 3]} (the guards around every output were seen untouched)."""
        _, outs, cnt = self.launches[launch]
        got = {k: s.get().view(dtype_of(k)) for k, s in outs.items()}
        got['counters'] = cnt.get().view(np.int64).reshape(self.n_tiles, 3)
        return got

    def is_untouched(self, launch=0):
        _, outs, cnt = self.launches[launch]
        return all(s.untouched() for s in outs.values()) and cnt.untouched()


def check(got, exp, what, layers=ALL_LAYERS):
    for k in layers:
        g, e = np.asarray(got[k]).ravel(), exp[k].ravel()
        if not np.array_equal(g, e):
            bad = np.flatnonzero(g != e)
            raise AssertionError((what, k, bad.size, bad[:4].tolist(), g[bad[:4]].tolist(), e[bad[:4]].tolist()))
    assert np.asarray(got['counters']).reshape(-1, 3).sum(axis=0).tolist() == exp['counters'].tolist(), (what, 'counters')


def run_form(ctxs, form, thr, bands, collapse=True, clip=False):
    """One row of pixels [1, N] through one kernel form against the C oracle."""
    n = bands[0].size
    shape = (n // WIDTH, WIDTH)
    bands = [b.reshape(shape) for b in bands]
    fm = np.zeros(shape, np.uint8)
    masks = {m: v.reshape(shape) for m, v in mask_planes(n).items()} if form == 'lut masks' else {}
    p = params(thr, collapse, clip=clip)
    # Fmask is 0 everywhere: no snow to dilate and nothing adjacent to cloud, so 'cover' gives the layers of 'ignore'
    exp = c_oracle.classify(params(thr, collapse, 'ignore', clip) if form == 'cover' else p, bands, fm, **masks)
    if form == 'generic':
        ctx = ctxs['lut']
        with Dev(ctx) as d:
            case = DeviceCase(d, bands, fm, masks, n // 7)
            ctx.classify_device(p, n // 7, 7, case.pin, case.launches[0][0], counters_ptr=case.launches[0][2].ptr)
            ctx.synchronize()
            got = case.read()
        info = ctx.last_kernel_info()
        assert 'dswx_classify_v1' in info and 'lut' not in info and 'v8' not in info, info
        assert (got['counters'] == [7, 0, 7]).all()
    else:
        ctx = ctxs['direct' if form == 'direct' else 'lut']
        rc, got = host_run(ctx, params(thr, collapse, 'cover', clip) if form == 'cover' else p, bands, fm, masks)
        assert rc == 0, rc
        info = ctx.last_kernel_info()
        assert KERNEL_OF[form] in info and ('dswx_cover_dilate' in info) == (form == 'cover'), info
        if form != 'direct':                    # the MASKS instantiation when, and only when, mask planes are given
            assert ('dswx_classify_lut<true' if masks else 'dswx_classify_lut<false') in info, info
    check(got, exp, form)
    return exp


# ---- 1. the quotient thresholds on every form ---------------------------------------------------------------------------
SETS = qi.quotient_sets()
BOTH_COLLAPSE = ('defaults', 'zeros', 'zero ndvi')


@functools.lru_cache(maxsize=2)
def set_tile(k, clip=False):
    _, m3, v, sections = (CLIP_SETS if clip else SETS)[k]
    bands, secs = qi.tile(sections, v, clip=clip)
    for b in bands:
        b.setflags(write=False)
    return bands, secs, qi.thresholds_of(m3, v)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('k', range(len(SETS)), ids=[s[0] for s in SETS])
def test_quotient_thresholds_on_every_form(ctxs, k, form):
    bands, secs, thr = set_tile(k)
    for collapse in (True, False) if SETS[k][0] in BOTH_COLLAPSE else (True,):
        exp = run_form(ctxs, form, thr, bands, collapse)
        if form == 'lut plain' and collapse:
            # the set does separate: in every section of a threshold inside the quotients' range its DIAG digit takes both values
            digits = exp['diag'].ravel()
            for (kind, t, lo, hi), slot in zip(secs, (0, 3, 4, 3)):
                if abs(t) < 32767:
                    d = (digits[lo:hi] // 10 ** (3 if kind == 'ndvi' else slot)) % 10
                    assert d.any() and not d.all(), (kind, t)


# ---- 2. the default clip ------------------------------------------------------------------------------------------------
CLIP_SETS = qi.clip_sets()


@pytest.mark.parametrize('form', ['lut plain', 'direct'])
@pytest.mark.parametrize('k', range(len(CLIP_SETS)), ids=[s[0] for s in CLIP_SETS])
def test_thresholds_in_0_1_with_the_default_clip(ctxs, k, form):
    bands, secs, thr = set_tile(k, True)
    run_form(ctxs, form, thr, bands, clip=True)


# ---- 3. awgt ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('awgt', qi.AWGT, ids=[qi._fmt(t) for t in qi.AWGT])
def test_awesh_thresholds_on_every_form(ctxs, awgt, form):
    thr = qi.thresholds_of(qi.DEFAULTS[:3], qi.DEFAULTS[3], awgt=awgt)
    exp = run_form(ctxs, form, thr, qi.awesh_tile(awgt))
    if abs(4.0 * awgt) < qi.AWESH4_MAX:
        d = (exp['diag'].ravel() // 100) % 10
        assert d.any() and not d.all()


# ---- 4. thresholds change between launches ------------------------------------------------------------------------------
QUOTIENT_FIELDS = ('wigt', 'pswt_1_mndwi', 'pswt_2_mndwi', 'pswt_1_ndvi')


@pytest.mark.parametrize('kernel', ['lut', 'direct'])
@pytest.mark.parametrize('field', QUOTIENT_FIELDS)
def test_every_launch_sees_its_own_threshold(ctxs, field, kernel):
    """t = fl64(n0 / d0), its upper neighbour, its lower neighbour and t again in `field`, everything else equal, four
    launches back to back on one context and one stream: the launches differ exactly on the pixels whose quotient is t."""
    n0, d0 = qi.RANDOM_PAIRS[3]
    t = n0 / d0
    ndvi = field == 'pswt_1_ndvi'
    bands, secs = qi.tile(() if ndvi else (t,), t if ndvi else None)
    base = qi.thresholds_of(qi.DEFAULTS[:3], qi.DEFAULTS[3])
    series = [dict(base, **{field: x}) for x in (t, math.nextafter(t, math.inf), math.nextafter(t, -math.inf), t)]
    fm = np.zeros(bands[0].shape, np.uint8)
    exps = [c_oracle.classify(params(thr), bands, fm) for thr in series]
    differ = [int(np.count_nonzero(exps[0]['diag'] != e['diag'])) for e in exps]
    assert differ[0] == 0 and differ[3] == 0 and differ[1 if ndvi else 2] >= 8 and differ[2 if ndvi else 1] == 0, differ
    ctx = ctxs[kernel]
    with Dev(ctx) as d:
        case = DeviceCase(d, bands, fm, None, 1, n_launches=4)
        for thr, (pout, _, cnt) in zip(series, case.launches):
            ctx.classify_device(params(thr), 1, bands[0].size, case.pin, pout, counters_ptr=cnt.ptr)
        ctx.synchronize()
        assert ('dswx_classify_lut' if kernel == 'lut' else 'dswx_classify_v8') in ctx.last_kernel_info()
        for i, exp in enumerate(exps):
            check(case.read(i), exp, (field, kernel, i))


# ---- 5. the device entries ----------------------------------------------------------------------------------------------
MIXED = ((0.25, -0.0, qi.RANDOM_PAIRS[5][0] / qi.RANDOM_PAIRS[5][1]), math.nextafter(-0.5, 0.0))
PER_TILE = 56 * 1001                           # pixels per tile: 248 (mod 256), whole 8-pixel groups


@functools.lru_cache(maxsize=1)
def mixed_tiles():
    """The mixed set cut into [T, 1001, 56] tiles (the last tile is filled up from the start of the row)."""
    thr = qi.thresholds_of(*MIXED)
    bands, _ = qi.tile(MIXED[0], MIXED[1])
    T = -(-bands[0].size // PER_TILE)
    bands = [np.resize(b.ravel(), T * PER_TILE).reshape(T, 1001, 56) for b in bands]
    fm = np.zeros(bands[0].shape, np.uint8)
    p = params(thr)
    exp = [c_oracle.classify(p, [b[t] for b in bands], fm[t]) for t in range(T)]
    return p, bands, fm, exp


def check_tiles(got, exp, what):
    T = len(exp)
    for k in ALL_LAYERS:
        g = np.asarray(got[k]).reshape(T, -1)
        for t in range(T):
            assert np.array_equal(g[t], exp[t][k].ravel()), (what, k, t)
    assert np.asarray(got['counters']).reshape(T, 3).tolist() == [e['counters'].tolist() for e in exp], what


def test_classify_device_at_a_16_byte_aligned_address(ctxs):
    p, bands, fm, exp = mixed_tiles()
    ctx = ctxs['lut']
    T = len(exp)
    with Dev(ctx) as d:
        case = DeviceCase(d, bands, fm, None, T, off=16)
        assert case.pin.band[1] % 256 == 16 and case.pin.fmask % 256 == 16
        ctx.classify_device(p, T, PER_TILE, case.pin, case.launches[0][0], counters_ptr=case.launches[0][2].ptr)
        ctx.synchronize()
        assert 'dswx_classify_lut' in ctx.last_kernel_info()
        check_tiles(case.read(), exp, 'classify_device')


def test_classify_batch_on_a_contiguous_stride(ctxs):
    p, bands, fm, exp = mixed_tiles()
    ctx = ctxs['lut']
    T = len(exp)
    assert PER_TILE % 256 != 0 and T > 1
    with Dev(ctx) as d:
        case = DeviceCase(d, bands, fm, None, T)
        geom = _capi.BatchGeom(n_tiles=T, height=1001, width=56, tile_stride=PER_TILE)
        ctx.classify_batch(p, geom, case.pin, case.launches[0][0], counters_ptr=case.launches[0][2].ptr)
        ctx.synchronize()
        assert 'dswx_classify_lut' in ctx.last_kernel_info()
        check_tiles(case.read(), exp, 'classify_batch')


def test_batch_classify_on_resident_tiles(ctxs):
    p, bands, fm, exp = mixed_tiles()
    ctx = ctxs['lut']
    T = len(exp)
    b = _capi.DeviceBatch(ctx, T, 1001, 56, extra_layers=('wtr1_aerosol',))
    try:
        for t in range(T):
            for i, name in enumerate(_capi.BAND_NAMES):
                b.write_tile(name, t, bands[i][t])
            b.write_tile('fmask', t, fm[t])
        b.write_counters_sentinel(-7)
        b.classify(p)
        ctx.synchronize()
        assert 'dswx_classify_lut' in ctx.last_kernel_info()
        got = {k: np.stack([b.read_tile(k, t) for t in range(T)]) for k in ALL_LAYERS}
        got['counters'] = b.read_counters()
        check_tiles(got, exp, 'batch_classify')
    finally:
        b.free()


# ---- 6. refusals and the ends of the accepted range ---------------------------------------------------------------------
REFUSED = (math.nan, math.inf, -math.inf, math.nextafter(1e100, math.inf), math.nextafter(1e-290, 0.0), 5e-324, -5e-324)
ACCEPTED = (1e100, -1e100, 1e-290, -1e-290)
assert len(_capi.THRESHOLD_NAMES) == 12


@pytest.mark.parametrize('value', REFUSED, ids=[repr(v) for v in REFUSED])
def test_thresholds_outside_the_range_are_refused(ctxs, value):
    """In each of the twelve threshold fields in turn: DSWX_ERR_ARG from dswx_classify_host and dswx_classify_device,
    and nothing written."""
    bands = [b.reshape(-1, WIDTH) for b in qi.awesh_tile(0.0)]
    fm = np.zeros(bands[0].shape, np.uint8)
    ctx = ctxs['lut']
    with Dev(ctx) as d:
        case = DeviceCase(d, bands, fm, None, 1)
        pout, _, cnt = case.launches[0]
        for field in _capi.THRESHOLD_NAMES:
            p = params(dict(qi.thresholds_of(qi.DEFAULTS[:3], qi.DEFAULTS[3]), **{field: value}))
            assert getattr(p, field) == value or value != value
            rc, res = host_run(ctx, p, bands, fm)
            assert rc == ERR_ARG and untouched(res), (field, rc)
            rc = ctx.lib.dswx_classify_device(ctx.handle, ctypes.byref(p), 1, bands[0].size, ctypes.byref(case.pin),
                                              ctypes.byref(pout), ctypes.c_void_p(cnt.ptr), None)
            assert rc == ERR_ARG, (field, rc)
        ctx.synchronize()
        assert case.is_untouched()


@pytest.mark.parametrize('value', ACCEPTED, ids=[repr(v) for v in ACCEPTED])
def test_the_ends_of_the_range_are_accepted(ctxs, value):
    bands = [b.reshape(-1, WIDTH) for b in qi.awesh_tile(0.0)]
    fm = np.zeros(bands[0].shape, np.uint8)
    for field in _capi.THRESHOLD_NAMES:
        p = params(dict(qi.thresholds_of(qi.DEFAULTS[:3], qi.DEFAULTS[3]), **{field: value}))
        for kernel in ('lut', 'direct'):
            rc, got = host_run(ctxs[kernel], p, bands, fm)
            assert rc == 0, (field, kernel, rc)
            check(got, c_oracle.classify(p, bands, fm), (field, kernel))
