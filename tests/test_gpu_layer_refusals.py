"""The refusals of the layer entries, one fault at a time, each entry reached directly through ctypes.

The seven terrain shadow entries (dswx_shadow_layer_host / _device: angles; _host_q / _device_q, _host_q32 / _device_q32:
thresholds on the arccos / arctan arguments; _batch: the same with a tile stride), the three landcover entries
(dswx_landcover_mask_host / _device / _batch) and dswx_interpret_layer_host validate their arguments in the host half of
dswx_layers.hip.  Every case here breaks ONE argument of an otherwise good call (shadow: a 12 x 12 float32 DEM with
margin 2; landcover: 8 x 8) and asserts DSWX_ERR_ARG and the text dswx_last_error() then holds -- the texts as the
library's source states them, written out below.  After the table of an entry the output buffer still holds its
sentinel, n_tiles = 0 is accepted and writes nothing, and one good call on the same context returns OK and equals the
numpy oracle (oracle/dswx_oracle.py) exactly: a refusal leaves nothing behind in the context."""
import ctypes

import numpy as np
import pytest

from oracle import dswx_oracle as o
from oracle import shadow_inputs as si
from proteus_amd import _capi

SENT = 0x77
NAN = float('nan')
NULL_ARG, SUN_NULL = 'NULL argument', 'sun_vector is NULL'
TOO_SMALL, BAD_MARGIN = 'at least 2 elements are required', 'bad margin'
THRESHOLD_NAN, ANGLE_NAN = 'shadow threshold is NaN', 'shadow angle threshold is NaN'
N_TILES, SHADOW_STRIDE = 'n_tiles out of range', 'shadow_tile_stride smaller'
BAD_SIZE, LAND_STRIDE, NEGATIVE = 'bad size', 'land_tile_stride smaller than the raster', 'negative size'

H, W, MARGIN = 12, 12, 2
OH, OW = H - 2 * MARGIN, W - 2 * MARGIN
SHADOW_ENTRIES = ('host', 'host_q', 'host_q32', 'device', 'device_q', 'device_q32', 'batch')
LH, LW = 8, 8
LAND_ENTRIES = ('host', 'device', 'batch')
FOREST = (111, 113, 115)
LAND_THRESHOLDS = (6, 3, 7, 3)


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def refused(ctx, rc, text, what):
    """The status and the message of a refused call."""
    msg = ctx.lib.dswx_last_error().decode('utf-8', 'replace')
    assert rc == _capi.ERR_ARG, (what, rc, msg)
    assert text in msg, (what, msg)


def ptr(x):
    return None if x is None else ctypes.c_void_p(x)


# ---- terrain shadow -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shadow_case():
    """(case, {legacy: the oracle's layer cropped by MARGIN}) on a rough 12 x 12 surface."""
    c = si.Case('refusals', np.ascontiguousarray(si.rough(H, W), dtype=np.float32), *si.SUN0, *si.THR0, 30.0, 30.0)
    return c, {legacy: si.expected(c, legacy, MARGIN) for legacy in (False, True)}


def shadow_call(lib, entry, f):
    """One shadow entry on the fields `f` (a, b: the two angles for 'host' / 'device', else slope_arg_max, inc_q_min)."""
    fn = getattr(lib, 'dswx_shadow_layer_' + entry)
    head = (f['ctx'], ptr(f['dem']))
    mid = (f['h'], f['w'], f['margin'], f['sun'], f['sa'], f['ca'])
    if entry.startswith('host'):
        return fn(*head, *mid, f['a'], f['b'], f['sx'], f['sy'], ptr(f['out']))
    if entry == 'batch':
        return fn(*head, f['n'], *mid, f['a'], f['b'], 0, f['sx'], f['sy'], ptr(f['out']), f['stride'], None)
    return fn(*head, f['n'], *mid, f['a'], f['b'], f['sx'], f['sy'], ptr(f['out']), None)


def shadow_faults(entry):
    """(one broken field, the message) for every fault of an entry."""
    faults = [(dict(ctx=None), NULL_ARG), (dict(dem=None), NULL_ARG), (dict(out=None), NULL_ARG), (dict(sun=None), SUN_NULL),
              (dict(h=1), TOO_SMALL), (dict(w=1), TOO_SMALL), (dict(margin=-1), BAD_MARGIN), (dict(margin=H // 2), BAD_MARGIN)]
    nan_text = ANGLE_NAN if entry in ('host', 'device') else THRESHOLD_NAN
    faults += [(dict(a=NAN), nan_text), (dict(b=NAN), nan_text)]
    if not entry.startswith('host'):
        faults += [(dict(n=-1), N_TILES), (dict(n=65536), N_TILES)]
    if entry == 'batch':
        faults += [(dict(stride=OH * OW - 1), SHADOW_STRIDE)]
    return faults


@pytest.mark.gpu
@pytest.mark.parametrize('entry', SHADOW_ENTRIES)
def test_shadow_refusals(ctx, shadow_case, entry):
    case, expected = shadow_case
    host, legacy = entry.startswith('host'), entry.endswith('q32')
    sun, sa, ca = si.sun_scalars(case.az, case.el)
    vec = (ctypes.c_double * 3)(*[float(v) for v in sun])
    a, b = ((case.min_slope, case.max_inc) if entry in ('host', 'device')
            else _capi.shadow_thresholds(case.min_slope, case.max_inc, legacy))
    n = 1 if host else 2
    dems = np.ascontiguousarray(np.broadcast_to(case.dem, (n, H, W)))
    out = np.full(n * OH * OW + 64, SENT, np.uint8)
    d_dem = d_out = None
    try:
        if host:
            src, dst = dems.ctypes.data, out.ctypes.data
        else:
            d_dem, d_out = ctx.malloc(dems.nbytes), ctx.malloc(out.nbytes)
            d_dem.upload(dems.ravel())
            d_out.upload(out)
            src, dst = d_dem.ptr, d_out.ptr
        good = dict(ctx=ctx.handle, dem=src, n=n, h=H, w=W, margin=MARGIN, sun=ctypes.byref(vec), sa=float(sa), ca=float(ca),
                    a=a, b=b, sx=case.sx, sy=case.sy, out=dst, stride=0)
        faults = shadow_faults(entry)
        assert len(faults) == 10 + (0 if host else 2) + (entry == 'batch')
        for broken, text in faults:
            refused(ctx, shadow_call(ctx.lib, entry, dict(good, **broken)), text, (entry, broken))
        if not host:            # no tiles: no work, whatever else a good call says
            assert shadow_call(ctx.lib, entry, dict(good, n=0)) == _capi.OK, (entry, ctx.lib.dswx_last_error())
            ctx.synchronize()
            out = d_out.download(np.uint8, out.size)
        assert (out == SENT).all(), (entry, 'a refused or empty call wrote to the output')
        rc = shadow_call(ctx.lib, entry, good)
        assert rc == _capi.OK, (entry, ctx.lib.dswx_last_error())
        if not host:
            ctx.synchronize()
            out = d_out.download(np.uint8, out.size)
        assert (out[n * OH * OW:] == SENT).all(), entry
        got = out[:n * OH * OW].reshape(n, OH, OW)
        for t in range(n):
            assert np.array_equal(got[t], expected[legacy]), (entry, t, np.argwhere(got[t] != expected[legacy])[:8].tolist())
        assert 0 < int(expected[legacy].sum()) < OH * OW          # both classes occur
    finally:
        for buf in (d_dem, d_out):
            if buf is not None:
                buf.free()


# ---- landcover mask -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def land_case():
    """(worldcover [3 LH][3 LW], copernicus [LH][LW], the oracle's LAND layer)."""
    rng = np.random.default_rng(5)
    wc = rng.choice(np.array([10, 10, 30, 50, 50, 80, 90, 95], np.uint8), (3 * LH, 3 * LW))
    cg = rng.choice(np.array([111, 113, 20, 126, 200], np.uint8), (LH, LW))
    return wc, cg, o.landcover_mask_from_warped(wc, cg, FOREST, thresholds=LAND_THRESHOLDS)


def land_call(lib, entry, f):
    head = (f['ctx'], ptr(f['wc']), ptr(f['cg']))
    tail = (f['h'], f['w'], ptr(f['fc']), f['nfc'], ptr(f['thr']), 0, ptr(f['out']))
    if entry == 'host':
        return lib.dswx_landcover_mask_host(*head, *tail)
    if entry == 'batch':
        return lib.dswx_landcover_mask_batch(*head, f['n'], *tail, f['stride'], None)
    return lib.dswx_landcover_mask_device(*head, f['n'], *tail, None)


def land_faults(entry):
    faults = [(dict(ctx=None), NULL_ARG), (dict(wc=None), NULL_ARG), (dict(cg=None), NULL_ARG), (dict(out=None), NULL_ARG),
              (dict(thr=None), NULL_ARG), (dict(h=-1), BAD_SIZE), (dict(fc=None, nfc=1), BAD_SIZE)]
    if entry != 'host':
        faults += [(dict(n=-1), N_TILES), (dict(n=65536), N_TILES)]
    if entry == 'batch':
        faults += [(dict(stride=LH * LW - 1), LAND_STRIDE)]
    return faults


@pytest.mark.gpu
@pytest.mark.parametrize('entry', LAND_ENTRIES)
def test_landcover_refusals(ctx, land_case, entry):
    wc, cg, expected = land_case
    host = entry == 'host'
    n = 1 if host else 2
    wcs, cgs = (np.ascontiguousarray(np.broadcast_to(x, (n,) + x.shape)) for x in (wc, cg))
    fc, thr = np.array(FOREST, np.int32), np.array(LAND_THRESHOLDS, np.int32)
    out = np.full(n * LH * LW + 64, SENT, np.uint8)
    bufs = []
    try:
        if host:
            p_wc, p_cg, dst = wcs.ctypes.data, cgs.ctypes.data, out.ctypes.data
        else:
            bufs = [ctx.malloc(x.nbytes) for x in (wcs, cgs, out)]
            for buf, x in zip(bufs, (wcs, cgs, out)):
                buf.upload(x.ravel())
            p_wc, p_cg, dst = (buf.ptr for buf in bufs)
        good = dict(ctx=ctx.handle, wc=p_wc, cg=p_cg, n=n, h=LH, w=LW, fc=fc.ctypes.data, nfc=fc.size, thr=thr.ctypes.data,
                    out=dst, stride=0)
        faults = land_faults(entry)
        assert len(faults) == 7 + (0 if host else 2) + (entry == 'batch')
        for broken, text in faults:
            refused(ctx, land_call(ctx.lib, entry, dict(good, **broken)), text, (entry, broken))
        if not host:
            assert land_call(ctx.lib, entry, dict(good, n=0)) == _capi.OK, (entry, ctx.lib.dswx_last_error())
            ctx.synchronize()
            out = bufs[2].download(np.uint8, out.size)
        assert (out == SENT).all(), (entry, 'a refused or empty call wrote to the output')
        rc = land_call(ctx.lib, entry, good)
        assert rc == _capi.OK, (entry, ctx.lib.dswx_last_error())
        if not host:
            ctx.synchronize()
            out = bufs[2].download(np.uint8, out.size)
        assert (out[n * LH * LW:] == SENT).all(), entry
        got = out[:n * LH * LW].reshape(n, LH, LW)
        for t in range(n):
            assert np.array_equal(got[t], expected), (entry, t)
        assert len(np.unique(expected)) >= 3
    finally:
        for buf in bufs:
            buf.free()


# ---- interpreted layer --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_interpret_refusals(ctx):
    diag = np.array(sorted(o.DIAG_TO_CLASS) + [-1, 33, 1 << 40], np.int64)
    out = np.full(diag.size + 64, SENT, np.uint8)
    fn = ctx.lib.dswx_interpret_layer_host
    p_in, p_out = ctypes.c_void_p(diag.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    for args, text in (((None, p_in, diag.size, p_out), NULL_ARG), ((ctx.handle, None, diag.size, p_out), NULL_ARG),
                       ((ctx.handle, p_in, diag.size, None), NULL_ARG), ((ctx.handle, p_in, -1, p_out), NEGATIVE)):
        refused(ctx, fn(*args), text, args[2:3])
    assert fn(ctx.handle, None, 0, None) == _capi.OK          # nothing to do: the pointers are not looked at
    assert (out == SENT).all()
    assert fn(ctx.handle, p_in, diag.size, p_out) == _capi.OK, ctx.lib.dswx_last_error()
    assert (out[diag.size:] == SENT).all()
    assert np.array_equal(out[:diag.size], o.generate_interpreted_layer(diag))
