"""The terrain shadow layer (_compute_opera_shadow_layer :4215-4283) over its whole input domain, on every C-ABI entry,
and generate_interpreted_layer over its int64 domain.

dswx_layers.hip has two shadow kernels: dswx_shadow_v3 (four pixels per thread; an approximate packed-float32 evaluation
with host-computed error bounds decides a pixel, the exact arithmetic recomputes it inside the bound or when
S = n0^2 + n1^2 + 1 is not below 2^60; unaligned 8-byte loads, the last quad of a row overlapping its neighbour), chosen
when margin >= 2 and the output is at least 4 pixels wide, and dswx_shadow_v2 (one pixel per thread, the exact arithmetic
alone) otherwise or under lab_configure(shadow_kernel=2).  Nine entries reach them: dswx_shadow_layer_host / _device
(angles, thresholds found with libm), _host_q / _device_q (thresholds on the arccos / arctan arguments, float64
products: numpy >= 2), _host_q32 / _device_q32 (all-float32 arithmetic: numpy < 2) and _batch (either, with a tile
stride).  Every comparison is np.array_equal against the numpy oracle on the named domains of oracle/shadow_inputs.py
(tests/test_shadow_domain.py shows on the CPU that those domains do what they are for), in both promotions, with no
mismatch budget -- but for the angle forms against numpy, where a pixel between libm's and numpy's thresholds may differ
and every other difference is a failure."""
import ctypes

import numpy as np
import pytest

from oracle import dswx_oracle as o
from oracle import shadow_inputs as si
from proteus_amd import _capi

SENT = 0x77
H0, W0 = si.H0, si.W0
MARGINS = (2, 3)             # an even and an odd one: the filter kernel's loads at 8-byte and at 4-byte boundaries
PROMOTIONS = [False, True]   # legacy (float32 arithmetic, the _q32 forms) or not
PROMOTION_IDS = ['nep50', 'legacy']
HOST_ENTRIES, DEVICE_ENTRIES = ('host', 'host_q', 'host_q32'), ('device', 'device_q', 'device_q32', 'batch')
# one case per domain for the entry tests: (domain, case name or geometry shape)
ENTRY_CASES = (('magnitudes', 'mixed_scales'), ('spacings', 'spacing_30.1_0.333333'), ('sun', 49), ('on_threshold', 'scale_1e3'),
               ('geometry', (9, 7)))


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.lab_configure(shadow_kernel=0)
    c.close()


def thresholds(case, legacy):
    """(slope_arg_max, inc_q_min) of a case for the _q / _q32 / _batch forms, located with numpy's own arccos / arctan."""
    return _capi.shadow_thresholds(case.min_slope, case.max_inc, legacy)


def libm_thresholds(ctx, min_slope, max_inc):
    a, b = ctypes.c_double(), ctypes.c_double()
    _capi._check(ctx.lib.dswx_shadow_thresholds(float(min_slope), float(max_inc), ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def call(ctx, entry, dem_ptr, n, h, w, margin, case, a, b, out_ptr, stride=0, stream=None, f32=False):
    """One C-ABI entry, called directly; returns its status.  (a, b) = (min_slope_angle, max_sun_local_inc_angle) for the
    angle forms 'host' / 'device', (slope_arg_max, inc_q_min) for the others."""
    sun, sa, ca = si.sun_scalars(case.az, case.el)
    vec = (ctypes.c_double * 3)(*[float(v) for v in sun])
    head, mid = (ctx.handle, ctypes.c_void_p(dem_ptr)), (ctypes.byref(vec), float(sa), float(ca))
    out, st = ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream) if stream else None
    if entry in HOST_ENTRIES:
        return getattr(ctx.lib, 'dswx_shadow_layer_' + entry)(*head, h, w, margin, *mid, a, b, case.sx, case.sy, out)
    if entry == 'batch':
        return ctx.lib.dswx_shadow_layer_batch(*head, n, h, w, margin, *mid, a, b, int(f32), case.sx, case.sy, out, stride, st)
    return getattr(ctx.lib, 'dswx_shadow_layer_' + entry)(*head, n, h, w, margin, *mid, a, b, case.sx, case.sy, out, st)


def entry_args(entry, case, legacy):
    """(entry name, a, b, f32 flag) of an entry for a case in a promotion."""
    a, b = thresholds(case, legacy)
    if entry == 'batch':
        return entry, a, b, legacy
    return entry + ('_q32' if legacy else '_q'), a, b, legacy


def host_call(ctx, entry, case, margin, a, b):
    """A host entry on a case; the layer [oh][ow] -- the bytes past it in the caller's buffer must be untouched."""
    h, w = case.dem.shape
    oh, ow = h - 2 * margin, w - 2 * margin
    out = np.full(oh * ow + 64, SENT, np.uint8)
    dem = np.ascontiguousarray(case.dem)
    rc = call(ctx, entry, dem.ctypes.data, 1, h, w, margin, case, a, b, out.ctypes.data)
    assert rc == 0, (entry, case.name, ctx.lib.dswx_last_error())
    assert (out[oh * ow:] == SENT).all(), (entry, case.name)
    return out[:oh * ow].reshape(oh, ow)


class Rig:
    """Device buffers allocated once and reused: a DEM buffer and an output buffer, with the guard checks around the
    output rasters."""

    def __init__(self, ctx, dem_bytes=1 << 20, out_bytes=1 << 16):
        self.ctx = ctx
        self.d_dem, self.d_out = ctx.malloc(dem_bytes + 64), ctx.malloc(out_bytes + 64)

    def free(self):
        self.d_dem.free()
        self.d_out.free()

    def memset_out(self, nbytes):
        _capi._check(self.ctx.lib.dswx_memset_d(self.ctx.handle, ctypes.c_void_p(self.d_out.ptr), SENT, int(nbytes)))

    def run(self, entry, dems, case, margin, a, b, f32=False, extra=0, dem_off=0, out_off=0):
        """dems [n][H][W] through a device entry: DEM at byte `dem_off`, output at byte `out_off`, tiles oh ow + extra
        bytes apart.  Returns the layers [n][oh][ow] after checking every byte before, between and after them."""
        ctx = self.ctx
        n, h, w = dems.shape
        oh, ow = h - 2 * margin, w - 2 * margin
        stride = oh * ow + extra
        used = out_off + n * stride + 32
        assert dem_off + dems.nbytes <= self.d_dem.nbytes and used <= self.d_out.nbytes
        self.d_dem.upload(dems.ravel(), dem_off)
        self.memset_out(used)
        rc = call(ctx, entry, self.d_dem.ptr + dem_off, n, h, w, margin, case, a, b, self.d_out.ptr + out_off,
                  stride=stride if extra else 0, f32=f32)
        assert rc == 0, (entry, case.name, ctx.lib.dswx_last_error())
        ctx.synchronize()
        return self.tiles(self.d_out.download(np.uint8, used), n, oh, ow, stride, out_off)

    @staticmethod
    def tiles(got, n, oh, ow, stride, out_off):
        assert (got[:out_off] == SENT).all(), 'bytes before the first raster were written'
        rows = got[out_off:out_off + n * stride].reshape(n, stride)
        assert (rows[:, oh * ow:] == SENT).all(), 'bytes between the rasters were written'
        assert (got[out_off + n * stride:] == SENT).all(), 'bytes after the last raster were written'
        return rows[:, :oh * ow].reshape(n, oh, ow)


@pytest.fixture(scope='module')
def rig(ctx):
    r = Rig(ctx)
    yield r
    r.free()


def _mismatch(got, exp):
    return int(np.count_nonzero(got != exp))


# ---- every domain through the filter kernel and through the exact kernel ------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('legacy', PROMOTIONS, ids=PROMOTION_IDS)
@pytest.mark.parametrize('domain', si.DOMAINS)
def test_domain_through_both_kernels(ctx, domain, legacy):
    """Every case at an even and an odd margin through the default dispatch (dswx_shadow_v3) and through the exact kernel
    (lab switch shadow_kernel=2: dswx_shadow_v2), each against the oracle."""
    n_px = n_shadow = 0
    for kernel in (0, 2):
        ctx.lab_configure(shadow_kernel=kernel)
        try:
            for c in si.cases(domain):
                sun, sa, ca = si.sun_scalars(c.az, c.el)
                for margin in MARGINS:
                    got = ctx.shadow_layer(c.dem, sun, sa, ca, c.min_slope, c.max_inc, c.sx, c.sy, margin=margin, float32=legacy)
                    exp = si.expected(c, legacy, margin)
                    assert got.shape == exp.shape
                    assert np.array_equal(got, exp.astype(bool)), (c.name, margin, 'v2' if kernel else 'v3', _mismatch(got, exp))
                    n_px, n_shadow = n_px + exp.size, n_shadow + int((exp == 0).sum())
        finally:
            ctx.lab_configure(shadow_kernel=0)
    print(f'{domain} {"legacy" if legacy else "nep50"}: {n_px} pixels, {n_shadow} shadow')
    assert 0 < n_shadow < n_px


# ---- the dispatch seam and the launch geometry --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('legacy', PROMOTIONS, ids=PROMOTION_IDS)
@pytest.mark.parametrize('margin', si.GEOMETRY_MARGINS)
def test_geometry(rig, margin, legacy):
    """Every output shape oh 1..17 x ow 1..9, 255, 256, 257, 260, 261 at one margin: three tiles through the batch entry,
    the DEM on a 4-byte (not 8-byte) boundary, the output at an odd address, the rasters oh ow + 5 bytes apart in a
    buffer of 0x77.  Margins 2, 3 and 50: the quad kernel from ow = 4 on (one quad at 4, the overlapping last quad at
    5, 6, 7, a second block in x from 257 on), dswx_shadow_v2 below; margins 0 and 1: dswx_shadow_v2, with one-sided
    differences on the borders at margin 0."""
    case = si.cases('geometry')[0]
    a, b = thresholds(case, legacy)
    n_quad = n_v2 = 0
    for oh, ow in si.GEOMETRY_SHAPES:
        if oh + 2 * margin < 2 or ow + 2 * margin < 2:
            continue                                            # refused: test_refusals_launch_nothing
        dems = si.geometry_dems(oh, ow, margin)
        got = rig.run('batch', dems, case, margin, a, b, f32=legacy, extra=5, dem_off=4, out_off=3)
        exp = si.geometry_expected(oh, ow, margin, legacy)
        assert np.array_equal(got, exp), (oh, ow, margin, [_mismatch(got[t], exp[t]) for t in range(len(exp))],
                                          np.argwhere(got != exp)[:8].tolist())
        quad = margin >= 2 and ow >= 4
        n_quad, n_v2 = n_quad + quad, n_v2 + (not quad)
    assert (rig.d_dem.ptr + 4) % 8 == 4 and (rig.d_out.ptr + 3) % 2 == 1
    assert (n_quad, n_v2) == ((17 * 11, 17 * 3) if margin >= 2 else (0, 17 * 14 if margin else 16 * 13))


# ---- every entry on the same cases --------------------------------------------------------------------------------------
def entry_case(domain, pick):
    """(case, dems [n][H][W], margin, expected(legacy) -> [n][oh][ow]) of one ENTRY_CASES row."""
    if domain == 'geometry':
        oh, ow = pick
        return (si.cases('geometry')[0], si.geometry_dems(oh, ow, 3), 3,
                lambda legacy: si.geometry_expected(oh, ow, 3, legacy))
    c = si.cases(domain)[pick] if isinstance(pick, int) else si.case(domain, pick)
    return c, c.dem[None], 3, lambda legacy: si.expected(c, legacy, 3)[None]


@pytest.mark.gpu
@pytest.mark.parametrize('legacy', PROMOTIONS, ids=PROMOTION_IDS)
def test_host_q_entries(ctx, legacy):
    """dswx_shadow_layer_host_q / _host_q32, called directly, on one case per domain (each tile of the geometry case)."""
    for domain, pick in ENTRY_CASES:
        c, dems, margin, exp = entry_case(domain, pick)
        entry, a, b, _ = entry_args('host', c, legacy)
        for t in range(len(dems)):
            got = host_call(ctx, entry, c._replace(dem=dems[t]), margin, a, b)
            assert np.array_equal(got, exp(legacy)[t]), (entry, domain, c.name, t)


@pytest.mark.gpu
@pytest.mark.parametrize('legacy', PROMOTIONS, ids=PROMOTION_IDS)
@pytest.mark.parametrize('entry,extra,kernel', [('device', 0, 0), ('device', 0, 2), ('batch', 0, 0), ('batch', 5, 0),
                                                ('batch', 0, 2), ('batch', 5, 2)],
                         ids=['device-v3', 'device-v2', 'batch-packed-v3', 'batch-stride-v3', 'batch-packed-v2', 'batch-stride-v2'])
def test_device_and_batch_entries(ctx, rig, entry, extra, kernel, legacy):
    """dswx_shadow_layer_device_q / _device_q32 / _batch (float32_arithmetic 0 and 1, with and without a stride) on one
    case per domain, through both kernels; the margin-0 and margin-1 cuts of the same cases too (dswx_shadow_v2 with
    several tiles, a stride and float32 arithmetic)."""
    ctx.lab_configure(shadow_kernel=kernel)
    try:
        for domain, pick in ENTRY_CASES:
            c, dems, margin, exp = entry_case(domain, pick)
            name, a, b, f32 = entry_args(entry, c, legacy)
            got = rig.run(name, dems, c, margin, a, b, f32=f32, extra=extra, dem_off=4 if extra else 0, out_off=1 if extra else 0)
            assert np.array_equal(got, exp(legacy)), (name, domain, c.name, extra, kernel)
        for margin in (0, 1):
            c = si.cases('geometry')[0]
            name, a, b, f32 = entry_args(entry, c, legacy)
            got = rig.run(name, si.geometry_dems(12, 70, margin), c, margin, a, b, f32=f32, extra=extra)
            assert np.array_equal(got, si.geometry_expected(12, 70, margin, legacy)), (name, margin, extra, kernel)
    finally:
        ctx.lab_configure(shadow_kernel=0)


@pytest.mark.gpu
@pytest.mark.parametrize('legacy', PROMOTIONS, ids=PROMOTION_IDS)
@pytest.mark.parametrize('entry', ['device', 'batch'])
def test_device_and_batch_entries_behind_an_upload_on_the_callers_stream(ctx, entry, legacy):
    """On a caller-created stream, no host synchronisation in between: a short hold, the asynchronous upload of the DEM
    (the device buffer holds a flat DEM before), the entry, the asynchronous download.  An entry that ran on another
    stream would read the flat DEM."""
    torch = pytest.importorskip('torch')
    s = torch.cuda.Stream(device=0)
    st = s.cuda_stream
    d_dem, d_out = ctx.malloc(1 << 16), ctx.malloc(1 << 14)
    try:
        for domain, pick in ENTRY_CASES:
            c, dems, margin, exp = entry_case(domain, pick)
            n, h, w = dems.shape
            oh, ow = h - 2 * margin, w - 2 * margin
            extra = 5 if entry == 'batch' else 0
            stride, used = oh * ow + extra, n * (oh * ow + extra) + 32
            name, a, b, f32 = entry_args(entry, c, legacy)
            src = ctx.pinned_empty(dems.shape, np.float32)
            src[...] = dems
            out = ctx.pinned_empty((used,), np.uint8)
            out[:] = 0
            _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ctypes.c_void_p(d_dem.ptr), 0, d_dem.nbytes))
            _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ctypes.c_void_p(d_out.ptr), SENT, used))
            ctx.synchronize()
            with torch.cuda.stream(s):
                torch.cuda._sleep(20_000_000)                      # some milliseconds at any shader clock
            ctx.h2d_async(d_dem.ptr, src, stream=st)
            rc = call(ctx, name, d_dem.ptr, n, h, w, margin, c, a, b, d_out.ptr, stride=stride if extra else 0, stream=st, f32=f32)
            assert rc == 0, (name, c.name, ctx.lib.dswx_last_error())
            ctx.d2h_async(out, d_out.ptr, stream=st)
            ctx.synchronize(st)
            got = Rig.tiles(np.array(out), n, oh, ow, stride, 0)
            assert np.array_equal(got, exp(legacy)), (name, domain, c.name)
    finally:
        torch.cuda.synchronize()
        d_dem.free()
        d_out.free()


# ---- the angle forms ----------------------------------------------------------------------------------------------------
ANGLE_PAIRS = ((-5.0, 40.0), (-91.0, -1.0), (90.0, 180.0), (0.0, 0.0), (1e-30, 55.0), (-33.3, 71.9))


@pytest.mark.gpu
def test_angle_forms_are_the_q_forms_at_the_librarys_thresholds(ctx, rig):
    """dswx_shadow_layer_host / _device against _host_q / _device_q fed the pair that dswx_shadow_thresholds returns for
    the same angles, bit for bit: the degenerate angles (-91 / -1: both tests never true; 90 / 180: always; 0 / 0) and
    the sun domain's own."""
    todo = [(si.case('magnitudes', 'scale_1'), p) for p in ANGLE_PAIRS]
    todo += [(si.case('on_threshold', 'scale_1e3'), p) for p in ANGLE_PAIRS[:4]]
    todo += [(c, (c.min_slope, c.max_inc)) for c in si.cases('sun')[::3]]
    seen = set()
    for c, (mn, mx) in todo:
        slope, incq = libm_thresholds(ctx, mn, mx)
        seen.add((np.isinf(slope), incq in (-1.0, 2.0)))
        for margin in (3, 0):
            host = host_call(ctx, 'host', c, margin, mn, mx)
            assert np.array_equal(host, host_call(ctx, 'host_q', c, margin, slope, incq)), (c.name, mn, mx, margin)
            dev = rig.run('device', c.dem[None], c, margin, mn, mx)
            assert np.array_equal(dev, rig.run('device_q', c.dem[None], c, margin, slope, incq)), (c.name, mn, mx, margin)
            assert np.array_equal(dev[0], host), (c.name, mn, mx, margin)
    assert len(seen) >= 3                      # finite and degenerate thresholds both
    assert libm_thresholds(ctx, -91.0, -1.0) == (-np.inf, 2.0)


@pytest.mark.gpu
def test_angle_forms_against_numpy_on_the_sun_domain(ctx, rig):
    """The angle forms find their thresholds with libm, the oracle applies numpy's arccos / arctan: a pixel may differ
    where the two libraries' boundaries differ, and only there.  Every differing pixel must have its q or its t (as the
    reference's expressions give them under numpy >= 2) between the two libraries' thresholds, ends included.  The
    count per case is printed."""
    total = 0
    for c in si.cases('sun'):
        slope_np, incq_np = thresholds(c, False)
        slope_lm, incq_lm = libm_thresholds(ctx, c.min_slope, c.max_inc)
        q, t, _, _ = (v[3:-3, 3:-3] for v in si.arguments(c, float64=False))
        exp = si.expected(c, False, 3)
        for entry in ('host', 'device'):
            got = host_call(ctx, 'host', c, 3, c.min_slope, c.max_inc) if entry == 'host' else \
                rig.run('device', c.dem[None], c, 3, c.min_slope, c.max_inc)[0]
            differ = got != exp
            with np.errstate(invalid='ignore'):
                between = ((q >= min(incq_np, incq_lm)) & (q <= max(incq_np, incq_lm))) | \
                          ((t >= min(slope_np, slope_lm)) & (t <= max(slope_np, slope_lm)))
            print(f'sun {c.name} {entry}: {int(differ.sum())} pixels differ from numpy (thresholds: slope '
                  f'{slope_lm!r} libm / {slope_np!r} numpy, q {incq_lm!r} libm / {incq_np!r} numpy)')
            assert not (differ & ~between).any(), (c.name, entry, int((differ & ~between).sum()))
            total += int(differ.sum())
    print(f'sun: {total} libm-versus-numpy boundary pixels in all')


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_nothing(ctx, rig):
    """Every refused call leaves the output buffer 0x77 (device entries: checked after a synchronisation); n_tiles = 0 is
    accepted and writes nothing."""
    c = si.case('magnitudes', 'scale_1')
    nan = float('nan')
    slope, incq = thresholds(c, False)
    host_out = np.full(1 << 14, SENT, np.uint8)
    dem = np.ascontiguousarray(c.dem)
    rig.d_dem.upload(dem.ravel())
    rig.memset_out(1 << 14)
    # (height, width, margin) that every entry refuses
    bad_geometry = [(1, 8, 0), (8, 1, 0), (0, 8, 0), (8, 4, 2), (4, 8, 2), (8, 12, 4), (12, 8, 4), (9, 9, 5), (8, 8, -1)]
    refused = 0
    for entry in HOST_ENTRIES + DEVICE_ENTRIES:
        host = entry in HOST_ENTRIES
        a, b = (c.min_slope, c.max_inc) if entry in ('host', 'device') else (slope, incq)
        src, dst = (dem.ctypes.data, host_out.ctypes.data) if host else (rig.d_dem.ptr, rig.d_out.ptr)
        calls = [dict(h=h, w=w, margin=m) for h, w, m in bad_geometry]
        if entry.endswith('q32'):
            a, b = thresholds(c, True)
        else:                                    # a NaN threshold (a C float NaN too, but ctypes passes it the same way)
            calls += [dict(a=nan), dict(b=nan)]
        if not host:
            calls += [dict(n=65536), dict(n=-1)]
        if entry == 'batch':
            calls += [dict(stride=34 * 66 - 1), dict(stride=1), dict(stride=-5)]
        for kw in calls:
            args = dict(dict(n=3 if not host else 1, h=H0, w=W0, margin=3, a=a, b=b, stride=0), **kw)
            rc = call(ctx, entry, src, args['n'], args['h'], args['w'], args['margin'], c, args['a'], args['b'], dst,
                      stride=args['stride'])
            assert rc == _capi.ERR_ARG, (entry, kw, rc)
            refused += 1
        if not host:
            assert call(ctx, entry, src, 0, H0, W0, 3, c, a, b, dst) == 0, entry          # no tiles: no work
    assert refused == 3 * 9 + 2 * 2 + 4 * 9 + 3 * 2 + 4 * 2 + 3
    ctx.synchronize()
    assert (host_out == SENT).all()
    assert (rig.d_out.download(np.uint8, 1 << 14) == SENT).all()
    with pytest.raises(ValueError, match='NaN'):
        _capi.shadow_thresholds(nan, 40.0)
    a, b = ctypes.c_double(), ctypes.c_double()
    assert ctx.lib.dswx_shadow_thresholds(nan, 40.0, ctypes.byref(a), ctypes.byref(b)) == _capi.ERR_ARG
    assert ctx.lib.dswx_shadow_thresholds(-5.0, nan, ctypes.byref(a), ctypes.byref(b)) == _capi.ERR_ARG



# ---- generate_interpreted_layer over int64 -------------------------------------------------------------------------------
def interpret_values():
    v = list(range(-70, 71))
    for k in range(32):
        v += [k + 2 ** 31, k + 2 ** 32, k - 2 ** 32, k + 2 ** 63 - 32]
    v += [-2 ** 63, 2 ** 63 - 1]
    return np.array(v, dtype=np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 100003])
def test_interpret_layer_int64_domain(ctx, n):
    """dswx_interpret_layer_host against the oracle on every value -70 ... 70, values whose low 32 bits look like valid
    keys (k + 2^31, k + 2^32, k - 2^32, k + 2^63 - 32) and the int64 ends, cycled to length n from three starting points;
    the 64 bytes after the n-th output byte stay as they were."""
    base = interpret_values()
    assert base.size == 141 + 128 + 2 and base[-3] == 2 ** 63 - 1
    for start in (0, 141, base.size - 1):
        d = np.ascontiguousarray(np.resize(np.roll(base, -start), n))
        out = np.full(n + 64, SENT, np.uint8)
        _capi._check(ctx.lib.dswx_interpret_layer_host(ctx.handle, ctypes.c_void_p(d.ctypes.data), n,
                                                       ctypes.c_void_p(out.ctypes.data)))
        exp = o.generate_interpreted_layer(d)
        assert np.array_equal(out[:n], exp), (n, start, d[out[:n] != exp][:8].tolist())
        assert (out[n:] == SENT).all(), (n, start)
        if n:
            assert np.array_equal(ctx.interpret_layer(d), exp)
    if n >= 255:            # not vacuous: the five classes and the fill all occur, most of the values map to the fill
        assert set(np.unique(exp).tolist()) == {0, 1, 2, 3, 4, 255}
