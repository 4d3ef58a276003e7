"""The stream contract of the C-ABI (include/dswx_hip.h): every device-pointer entry is "asynchronous on `stream` (NULL = the
context's stream)".  The other GPU tests check WHAT the entries compute, synchronising after every call on one stream, so
an entry that launched on the context's stream instead of the caller's, that blocked the host, or whose context scratch a
call on another stream overwrote would still leave every output bit-exact.

(a) Held-stream conformance: the caller's stream s1 is held by a spin kernel (torch.cuda._sleep); the entry is called on
    s1; it must return while the hold is pending, its outputs (page-locked host memory, or HBM read through the
    independent stream s2) must still hold the sentinel, and after the hold they must match the suite's oracle bit for
    bit, padding and gaps between tiles still the sentinel.
(b) The Float32 PREDICTOR=3 untile shares a scratch of the context: a call on another stream waits for the previous one.
(c) Rounds of calls alternating over two streams of one context, no host synchronisation inside a round."""
import ctypes
import time

import numpy as np
import pytest

from oracle import c_oracle, cog_oracle as co, dswx_oracle as o, land_inputs as L
from proteus_amd import _capi, geotiff
from proteus_amd.synth import SEED as SYNTH_SEED, synth_dem, synth_landcover_inputs, synth_tile

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

H, W = 300, 257
N = H * W
SENT = 0x5A                 # sentinel byte of every output
LAYERS = ('diag', 'wtr1', 'wtr1_aerosol', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud')
COVER_LAYERS = (('diag', 'DIAG'), ('wtr1', 'WTR-1'), ('wtr2', 'WTR-2'), ('wtr', 'WTR'), ('bwtr', 'BWTR'), ('conf', 'CONF'),
                ('cloud', 'CLOUD'))
SUN = (141.0, 55.5)         # azimuth, elevation (degrees)
MIN_SLOPE, MAX_INC = -5.0, 40.0
MIN_HOLD_MS, WORK_FACTOR = 200.0, 20.0


def _sun(az_deg, el_deg):
    az, zen = np.radians(az_deg), np.radians(90 - el_deg)
    return [np.sin(az) * np.sin(zen), np.cos(az) * np.sin(zen), np.cos(zen)], np.sin(az), np.cos(az)


def _dev(arr):
    """A host array as a device tensor (uploaded and complete)."""
    t = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()).to('cuda:0')
    torch.cuda.synchronize()
    return t


def _devbuf(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device='cuda:0')


class Env:
    """The context, the caller's stream s1 (the held one), a second stream s2 whose work does not wait behind s1's, and
    the spin rate of the hold."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.cycles_per_ms = self._calibrate(torch.cuda.Stream(device=0))
        self.s1, self.s2 = self._pick_streams()

    def hold(self, ms, stream=None):
        """Enqueue a hold of `ms` on `stream` (default s1); returns the event recorded behind it."""
        s = stream or self.s1
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(self.cycles_per_ms * ms))
        ev = torch.cuda.Event()
        ev.record(s)
        return ev

    def _calibrate(self, s):
        """Spin cycles per millisecond at the FASTEST clock seen.  The spin counts shader clock cycles, so a hold lasts
        cycles / (the clock while it runs): sized at a slow clock (an idle GPU ramping up, or a short first sample that
        is mostly launch latency) it ends early once the clock rises, and a held call then runs during its 'hold'.
        So: the first sample only wakes the GPU, the next three (~60 ms each) are timed, the highest rate is kept."""
        rate, best = None, 0.0
        for k in range(4):
            cycles = 1 << 22 if rate is None else int(rate * 60.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
            e1.record(s)
            e1.synchronize()
            rate = cycles / max(e0.elapsed_time(e1), 1e-3)
            if k:
                best = max(best, rate)
        return best * 1.5                            # margin: the clock may rise past the fastest sample

    def _visible_during_hold(self, held, stream_arg):
        """Does a small kernel launched on `stream_arg` (a to_byte conversion into page-locked memory) finish, and its
        result show on the host, while `held` is held?"""
        src = _dev(np.arange(64, dtype=np.uint16) + 1)
        out = self.ctx.pinned_empty(64, np.uint8)
        out[:] = 0
        ev = self.hold(100.0, held)
        self.ctx.to_byte_device(src.data_ptr(), np.uint16, 64, out.ctypes.data, stream=stream_arg)
        seen = False
        t0 = time.perf_counter()
        while not ev.query() and time.perf_counter() - t0 < 0.05:
            if (out == np.arange(1, 65)).all():
                seen = True
                break
        seen = seen and not ev.query()
        held.synchronize()
        self.ctx.synchronize(stream_arg)
        return seen

    def _runs_during_hold(self, held, s):
        """Does a small torch kernel on `s` complete while `held` is held?"""
        x = torch.zeros(64, device='cuda:0')
        torch.cuda.synchronize()
        ev = self.hold(100.0, held)
        with torch.cuda.stream(s):
            x.add_(1)
        done = torch.cuda.Event()
        done.record(s)
        t0 = time.perf_counter()
        while not done.query() and time.perf_counter() - t0 < 0.05:
            pass
        ok = done.query() and not ev.query()
        torch.cuda.synchronize()
        return ok

    def _pick_streams(self):
        """s1: a stream whose hold does not hold the context's own stream; s2: one whose work does not wait behind s1.
        Streams share a hardware queue round robin; the checks below need two that do not."""
        cands = [torch.cuda.Stream(device=0) for _ in range(8)]
        s1 = next((s for s in cands if self._visible_during_hold(s, None)), None)
        assert s1 is not None, 'no stream found whose hold leaves the context stream running (or kernel writes to ' \
                               'page-locked memory do not show on the host before a synchronisation)'
        s2 = next((s for s in cands if s is not s1 and self._runs_during_hold(s1, s)), None)
        assert s2 is not None, 'no second stream found that runs while s1 is held'
        return s1, s2


@pytest.fixture(scope='module')
def env():
    c = _capi.Context(0)
    e = Env(c)
    yield e
    torch.cuda.synchronize()
    c.synchronize()
    c.close()


def _pinned(ctx, nbytes, dtype=np.uint8):
    a = ctx.pinned_empty((int(nbytes) // np.dtype(dtype).itemsize,), dtype)
    a.view(np.uint8)[:] = SENT
    return a


def _all_sentinel(arrs):
    return all((a.view(np.uint8) == SENT).all() for a in arrs)


def held_call(env, launch, host_outs, check, device_outs=()):
    """The held-stream protocol for one call: warm-up on s1 (unheld; grow-only scratch, module load, the work's duration),
    then the held call.  host_outs: page-locked arrays the call writes; device_outs: (device pointer, nbytes) it writes,
    read during the hold through s2."""
    ctx, s1 = env.ctx, env.s1

    def reset():
        for a in host_outs:
            a.view(np.uint8)[:] = SENT
        for ptr, nbytes in device_outs:
            ctx.lib.dswx_memset_d(ctx.handle, ctypes.c_void_p(ptr), SENT, int(nbytes))
        torch.cuda.synchronize()

    reset()
    t0 = time.perf_counter()
    launch(s1.cuda_stream)
    s1.synchronize()
    work_ms = (time.perf_counter() - t0) * 1e3
    check()
    reset()
    hold_ms = max(MIN_HOLD_MS, WORK_FACTOR * work_ms)
    ev = env.hold(hold_ms)
    assert not ev.query(), 'the hold ended at once: the hold was sized wrongly'
    t0 = time.perf_counter()
    launch(s1.cuda_stream)
    call_ms = (time.perf_counter() - t0) * 1e3
    assert not ev.query(), (f'the hold ({hold_ms:.0f} ms) ended before the call returned ({call_ms:.1f} ms): the call '
                            f'blocked the host, or the hold was sized wrongly')
    assert _all_sentinel(host_outs), 'an output was written while the caller\'s stream was held: work not on `stream`'
    snaps = []
    for ptr, nbytes in device_outs:
        h = _pinned(ctx, nbytes)
        h.view(np.uint8)[:] = 0
        ctx.d2h_async(h, ptr, nbytes, stream=env.s2.cuda_stream)
        snaps.append(h)
    ctx.synchronize(env.s2.cuda_stream)
    assert all((h == SENT).all() for h in snaps), 'a device output was written while the caller\'s stream was held'
    assert not ev.query(), f'the hold ({hold_ms:.0f} ms) ended during the checks: the hold was sized wrongly'
    s1.synchronize()
    check()


# ---- (a) one case per entry -----------------------------------------------------------------------------------------
def _planes_in(dev, masks):
    pin = _capi.PlanesIn()
    for k in range(6):
        pin.band[k] = dev[f'b{k}'].data_ptr()
    pin.fmask = dev['fmask'].data_ptr()
    if masks:
        pin.land, pin.shad, pin.ocean = (dev[m].data_ptr() for m in ('land', 'shad', 'ocean'))
    return pin


def _upload_tiles(tiles, stride, masks):
    """[synth_tile dicts] -> device planes [n][stride] (gaps 0)."""
    n = len(tiles)
    dev = {}
    for k in range(6):
        a = np.zeros((n, stride), np.int16)
        for t, s in enumerate(tiles):
            a[t, :s['bands'][k].size] = s['bands'][k].ravel()
        dev[f'b{k}'] = _dev(a)
    for m in ('fmask',) + (('land', 'shad', 'ocean') if masks else ()):
        a = np.zeros((n, stride), np.uint8)
        for t, s in enumerate(tiles):
            a[t, :s[m].size] = s[m].ravel()
        dev[m] = _dev(a)
    return dev


def _pinned_outs(ctx, n, stride, layers=LAYERS):
    outs = {name: _pinned(ctx, n * stride * (2 if name == 'diag' else 1), np.uint16 if name == 'diag' else np.uint8)
            for name in layers}
    pout = _capi.PlanesOut()
    for name, a in outs.items():
        setattr(pout, name, a.ctypes.data)
    return outs, pout


def _check_classify(outs, cnt, exps, stride, npx, layers=LAYERS):
    for t, exp in enumerate(exps):
        for name in layers:
            plane = outs[name].reshape(len(exps), stride)
            assert np.array_equal(plane[t, :npx], exp[name].ravel()), (t, name)
            assert (plane[t, npx:].view(np.uint8) == SENT).all(), ('gap written', t, name)
        assert cnt[t].tolist() == exp['counters'].tolist(), t


@pytest.mark.parametrize('variant', ['no masks', 'masks', 'float32 chain'])
def test_classify_device(env, variant):
    ctx = env.ctx
    masks = variant != 'no masks'
    p = _capi.make_params(offset_and_scale=[(1e-4, 0.0)] * 6) if variant == 'float32 chain' else _capi.default_params()
    s = synth_tile(11, H, W, with_masks=masks)
    dev = _upload_tiles([s], N, masks)
    pin = _planes_in(dev, masks)
    outs, pout = _pinned_outs(ctx, 1, N)
    cnt = _pinned(ctx, 24, np.int64).reshape(1, 3)
    kw = {m: s[m] for m in ('land', 'shad', 'ocean')} if masks else {}
    exp = c_oracle.classify(p, s['bands'], s['fmask'], **kw)
    held_call(env, lambda st: ctx.classify_device(p, 1, N, pin, pout, cnt.ctypes.data, stream=st), list(outs.values()) + [cnt],
              lambda: _check_classify(outs, cnt, [exp], N, N))
    assert 'counters folded' in ctx.last_kernel_info()


def test_classify_device_2d_cover(env):
    ctx = env.ctx
    p = _capi.make_params(mask_adjacent_to_cloud_mode='cover')
    tiles = [synth_tile(20 + t, H, W, with_masks=True) for t in range(2)]
    dev = _upload_tiles(tiles, N, True)
    pin = _planes_in(dev, True)
    layers = tuple(k for k, _ in COVER_LAYERS)
    outs, pout = _pinned_outs(ctx, 2, N, layers)
    cnt = _pinned(ctx, 48, np.int64).reshape(2, 3)
    exps = []
    for s in tiles:
        with np.errstate(all='ignore'):
            e = o.classify_tile(s['bands'], s['fmask'], landcover=s['land'], shadow=s['shad'], ocean_mask=s['ocean'],
                                mask_adjacent_to_cloud_mode='cover')
        c = e['counters']
        exps.append(dict({k: e[v + '.collapsed'] if v + '.collapsed' in e else e[v] for k, v in COVER_LAYERS},
                         counters=np.array([c['n_valid'], c['n_cloud_and_valid'], c['n_not_ocean']])))
    held_call(env, lambda st: ctx.classify_device_2d(p, 2, H, W, pin, pout, cnt.ctypes.data, stream=st),
              list(outs.values()) + [cnt], lambda: _check_classify(outs, cnt, exps, N, N, layers))


@pytest.mark.parametrize('stride', [N + 5, N + 1])
def test_classify_batch_odd_stride(env, stride):
    ctx = env.ctx
    p = _capi.default_params()
    tiles = [synth_tile(40 + t, H, W, with_masks=True) for t in range(3)]
    dev = _upload_tiles(tiles, stride, True)
    pin = _planes_in(dev, True)
    outs, pout = _pinned_outs(ctx, 3, stride)
    cnt = _pinned(ctx, 72, np.int64).reshape(3, 3)
    exps = [c_oracle.classify(p, s['bands'], s['fmask'], land=s['land'], shad=s['shad'], ocean=s['ocean']) for s in tiles]
    geom = _capi.BatchGeom(3, H, W, stride)
    held_call(env, lambda st: ctx.classify_batch(p, geom, pin, pout, cnt.ctypes.data, stream=st), list(outs.values()) + [cnt],
              lambda: _check_classify(outs, cnt, exps, stride, N))


def _batch_device_outs(b, names):
    """(device pointer, bytes) of whole planes of a resident batch; 'b0' .. 'b5' are the bands."""
    res = []
    for n in names:
        if n in LAYERS:
            res.append((getattr(b.pout, n), b.n_tiles * b.tile_stride * (2 if n == 'diag' else 1)))
        elif n.startswith('b'):
            res.append((b.pin.band[int(n[1:])], b.n_tiles * b.tile_stride * 2))
        else:
            res.append((getattr(b.pin, n), b.n_tiles * b.tile_stride))
    return res


def test_batch_synth_and_classify(env):
    """dswx_batch_synth / dswx_batch_classify: the planes are the batch's own (HBM)."""
    ctx = env.ctx
    p = _capi.default_params()
    b = _capi.DeviceBatch(ctx, 3, H, W, masks=True)
    try:
        tiles = [synth_tile(60 + t, H, W, with_masks=True) for t in range(3)]
        ins = ['b0', 'b3', 'b5', 'fmask', 'land', 'shad', 'ocean']

        def check_synth():
            for t, s in enumerate(tiles):
                for k in (0, 3, 5):
                    assert np.array_equal(b.read_tile(_capi.BAND_NAMES[k], t), s['bands'][k]), (t, k)
                for m in ('fmask', 'land', 'shad', 'ocean'):
                    assert np.array_equal(b.read_tile(m, t), s[m]), (t, m)
        held_call(env, lambda st: b.synth(SYNTH_SEED, tile0=60, stream=st), [], check_synth, _batch_device_outs(b, ins))
        exps = [c_oracle.classify(p, s['bands'], s['fmask'], land=s['land'], shad=s['shad'], ocean=s['ocean']) for s in tiles]

        def check_classify():
            for t, e in enumerate(exps):
                for name in ('diag',) + tuple(x for x in b.out_layers):
                    assert np.array_equal(b.read_tile(name, t), e[name]), (t, name)
            assert [r.tolist() for r in b.read_counters()] == [e['counters'].tolist() for e in exps]
        outs = _batch_device_outs(b, ['diag'] + b.out_layers) + [(b.counters_ptr, 72)]
        held_call(env, lambda st: b.classify(p, stream=st), [], check_classify, outs)
    finally:
        b.free()



@pytest.mark.parametrize('entry', ['synth_fill', 'synth_batch'])
def test_synth(env, entry):
    ctx = env.ctx
    n, stride = 3, (N if entry == 'synth_fill' else N + 3)
    bands = [_pinned(ctx, n * stride * 2, np.int16) for _ in range(6)]
    planes = {m: _pinned(ctx, n * stride) for m in ('fmask', 'land', 'shad', 'ocean')}
    pin = _capi.PlanesIn()
    for k in range(6):
        pin.band[k] = bands[k].ctypes.data
    for m, a in planes.items():
        setattr(pin, m, a.ctypes.data)

    def launch(st):
        if entry == 'synth_fill':
            ctx.synth_fill(SYNTH_SEED, 80, n, H, W, pin, stream=st)
        else:
            ctx.synth_batch(SYNTH_SEED, 80, _capi.BatchGeom(n, H, W, stride), pin, stream=st)

    def check():
        for t in range(n):
            s = synth_tile(80 + t, H, W, with_masks=True)
            for k in range(6):
                row = bands[k].reshape(n, stride)[t]
                assert np.array_equal(row[:N], s['bands'][k].ravel()) and (row[N:].view(np.uint8) == SENT).all(), (t, k)
            for m, a in planes.items():
                row = a.reshape(n, stride)[t]
                assert np.array_equal(row[:N], s[m].ravel()) and (row[N:] == SENT).all(), (t, m)
    held_call(env, launch, bands + list(planes.values()), check)


def _shadow_expect(dems, margin, legacy):
    with np.errstate(all='ignore'):
        return [o.compute_opera_shadow_layer(d, *SUN, MIN_SLOPE, MAX_INC, legacy_promotion=legacy)
                [margin:d.shape[0] - margin, margin:d.shape[1] - margin].astype(np.uint8) for d in dems]


@pytest.mark.parametrize('entry', ['device', 'q', 'q32', 'batch'])
def test_shadow_layer(env, entry):
    ctx = env.ctx
    n, m = 3, 5
    dems = [synth_dem(90 + t, H, W) for t in range(n)]
    d_dem = _dev(np.stack(dems))
    oh, ow = H - 2 * m, W - 2 * m
    stride = oh * ow + (7 if entry == 'batch' else 0)
    out = _pinned(ctx, n * stride)
    vec, sa, ca = _sun(*SUN)
    legacy = entry == 'q32'

    def launch(st):
        if entry == 'device':
            v = (ctypes.c_double * 3)(*vec)
            _capi._check(ctx.lib.dswx_shadow_layer_device(
                ctx.handle, ctypes.c_void_p(d_dem.data_ptr()), n, H, W, m, ctypes.byref(v), float(sa), float(ca), MIN_SLOPE,
                MAX_INC, 30.0, 30.0, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(st)))
        else:
            ctx.shadow_layer_device(d_dem.data_ptr(), n, H, W, m, vec, sa, ca, MIN_SLOPE, MAX_INC, out.ctypes.data, stream=st,
                                    float32=legacy, out_tile_stride=stride if entry == 'batch' else 0)
    exps = _shadow_expect(dems, m, legacy)

    def check():
        rows = out.reshape(n, stride)
        for t in range(n):
            assert np.array_equal(rows[t, :oh * ow], exps[t].ravel()), t
            assert (rows[t, oh * ow:] == SENT).all(), t
    held_call(env, launch, [out], check)


@pytest.mark.parametrize('entry', ['device', 'batch'])
def test_landcover_mask(env, entry):
    ctx = env.ctx
    n, h, w = 3, 101, 77
    thr = (6, 3, 7, 3)
    inputs = [synth_landcover_inputs(100 + t, h, w) for t in range(n)]
    d_wc, d_cg = _dev(np.stack([x[0] for x in inputs])), _dev(np.stack([x[1] for x in inputs]))
    stride = h * w + (5 if entry == 'batch' else 0)
    out = _pinned(ctx, n * stride)
    fc = np.array(L.DEFAULT_FOREST, np.int32)
    t4 = np.array(thr, np.int32)

    def launch(st):
        if entry == 'device':
            _capi._check(ctx.lib.dswx_landcover_mask_device(
                ctx.handle, ctypes.c_void_p(d_wc.data_ptr()), ctypes.c_void_p(d_cg.data_ptr()), n, h, w,
                ctypes.c_void_p(fc.ctypes.data), int(fc.size), ctypes.c_void_p(t4.ctypes.data), 0,
                ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(st)))
        else:
            ctx.landcover_mask_device(d_wc.data_ptr(), d_cg.data_ptr(), n, h, w, L.DEFAULT_FOREST, out.ctypes.data,
                                      thresholds=thr, stream=st, out_tile_stride=stride)
    exps = [o.landcover_mask_from_warped(wc, cg, L.DEFAULT_FOREST, year=2000, thresholds=thr) for wc, cg in inputs]

    def check():
        rows = out.reshape(n, stride)
        for t in range(n):
            assert np.array_equal(rows[t, :h * w], exps[t].ravel()), t
            assert (rows[t, h * w:] == SENT).all(), t
    held_call(env, launch, [out], check)


def _raster(dtype, shape=(H, W), seed=0):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == 'f':
        a = rng.normal(0.1, 0.05, size=shape).astype(np.float32)
        a[rng.random(shape) < 0.05] = np.nan
        return a
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64).astype(dtype)


@pytest.mark.parametrize('kind', ['u8 overviews', 'u16', 'f32 predictor 3'])
def test_cog_blocks(env, kind):
    ctx = env.ctx
    dtype, factors, predictor = {'u8 overviews': (np.uint8, (2, 4, 8), 2), 'u16': (np.uint16, (), 2),
                                 'f32 predictor 3': (np.float32, (), 3)}[kind]
    arr = _raster(dtype, seed=3)
    tile = 64
    lay = _capi.cog_layout(H, W, arr.dtype.itemsize, factors, tile)
    d_in = _dev(arr)
    out = _pinned(ctx, lay['total_bytes'] + 64)
    want = np.concatenate([d for _, _, d in co.cog_levels(arr, factors, tile, predictor)])
    assert want.size == lay['total_bytes']

    def check():
        assert np.array_equal(out[:want.size], want)
        assert (out[want.size:] == SENT).all()
    held_call(env, lambda st: ctx.cog_blocks_device(d_in.data_ptr(), arr.dtype.itemsize, H, W, out.ctypes.data, factors, tile,
                                                    predictor, stream=st), [out], check)


UNTILE_CASES = [(np.uint8, 1), (np.uint8, 2), (np.uint16, 1), (np.uint16, 2), (np.uint32, 1), (np.uint32, 2),
                (np.float32, 3)]


@pytest.mark.parametrize('dtype,predictor', UNTILE_CASES, ids=[f'{np.dtype(d).name}-p{p}' for d, p in UNTILE_CASES])
def test_untile(env, dtype, predictor):
    ctx = env.ctx
    arr = _raster(dtype, seed=5 + predictor)
    tile = 64
    d_blocks = _dev(co.blocks(arr, tile, predictor))
    es = arr.dtype.itemsize
    out = _pinned(ctx, arr.nbytes + 64)

    def check():
        assert out[:arr.nbytes].view(np.uint8).tobytes() == arr.tobytes()
        assert (out[arr.nbytes:] == SENT).all()
    held_call(env, lambda st: ctx.untile_device(d_blocks.data_ptr(), es, H, W, tile, tile, predictor, out.ctypes.data, stream=st),
              [out], check)


def test_convolve_axis_both_passes(env):
    """The CUBICSPLINE overview: horizontal pass float32 -> float64, vertical pass float64 -> float32, both on s1."""
    ctx = env.ctx
    h, w, f = 61, 50, 4
    a = (np.random.default_rng(8).normal(size=(h, w)) * 1000).astype(np.float32)
    a[3, 4] = np.nan
    oh, ow = -(-h // f), -(-w // f)
    fx, wx = geotiff.convolve_weights(w, ow)
    fy, wy = geotiff.convolve_weights(h, oh)
    d_a = _dev(a)
    d_fx, d_wx = _dev(fx.astype(np.int32)), _dev(np.ascontiguousarray(wx.T))
    d_fy, d_wy = _dev(fy.astype(np.int32)), _dev(np.ascontiguousarray(wy.T))
    tmp = _pinned(ctx, h * ow * 8)
    out = _pinned(ctx, oh * ow * 4 + 32)
    want = co.cubicspline_overview(a, f)

    def launch(st):
        ctx.convolve_axis_device(d_a.data_ptr(), False, h, w, w, 1, ow, wx.shape[1], d_fx.data_ptr(), d_wx.data_ptr(),
                                 tmp.ctypes.data, True, ow, 1, stream=st)
        ctx.convolve_axis_device(tmp.ctypes.data, True, ow, h, 1, ow, oh, wy.shape[1], d_fy.data_ptr(), d_wy.data_ptr(),
                                 out.ctypes.data, False, 1, ow, stream=st)

    def check():
        got = out[:oh * ow * 4].view(np.float32).reshape(oh, ow)
        assert np.array_equal(got, want, equal_nan=True)
        assert (out[oh * ow * 4:] == SENT).all()
    held_call(env, launch, [tmp, out], check)


@pytest.mark.parametrize('use_diag', [True, False])
def test_rgb_planes(env, use_diag):
    ctx = env.ctx
    rng = np.random.default_rng(12)
    bands = [rng.integers(-200, 12000, size=N).astype(np.int16) for _ in range(3)]
    diag = rng.integers(0, 11112, size=N).astype(np.uint16)
    diag[rng.random(N) < 0.1] = 65535
    d = [_dev(b) for b in bands]
    d_diag = _dev(diag)
    scale, offset = [1e-4, 2e-4, 0.5], [0.0, -12.5, 3.0]
    out = _pinned(ctx, 3 * N * 4 + 16)

    def check():
        got = out[:3 * N * 4].view(np.float32).reshape(3, N)
        for c in range(3):
            want = scale[c] * (np.asarray(np.clip(bands[c], 1, None), dtype=np.float32) - offset[c])
            if use_diag:
                want[diag == 65535] = np.nan
            assert np.array_equal(got[c], want, equal_nan=True), c
        assert (out[3 * N * 4:] == SENT).all()
    held_call(env, lambda st: ctx.rgb_planes_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                    d_diag.data_ptr() if use_diag else None, N, scale, offset, True,
                                                    out.ctypes.data, stream=st), [out], check)


@pytest.mark.parametrize('dtype', [np.uint16, np.int16, np.float32])
def test_to_byte(env, dtype):
    ctx = env.ctx
    rng = np.random.default_rng(13)
    if dtype == np.float32:
        a = rng.uniform(-20, 280, size=(60, 77)).astype(np.float32)
        a[::9, ::4] = np.nan
    else:
        a = _raster(dtype, (60, 77), 14)
    d_a = _dev(a)
    out = _pinned(ctx, a.size + 16)
    want = co.gdal_byte(a).ravel()

    def check():
        assert np.array_equal(out[:a.size], want) and (out[a.size:] == SENT).all()
    held_call(env, lambda st: ctx.to_byte_device(d_a.data_ptr(), dtype, a.size, out.ctypes.data, stream=st), [out], check)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.uint32])
def test_gather_2d(env, dtype):
    ctx = env.ctx
    a = _raster(dtype, (H, W), 15)
    oh, ow = 97, 64
    ys, xs = geotiff.resample_nearest_indices(H, W, oh, ow)
    d_a, d_y, d_x = _dev(a), _dev(ys.astype(np.int32)), _dev(xs.astype(np.int32))
    es = a.dtype.itemsize
    out = _pinned(ctx, oh * ow * es + 16)
    want = co.resample_nearest(a, oh, ow)

    def check():
        assert out[:oh * ow * es].view(dtype).reshape(oh, ow).tobytes() == want.tobytes()
        assert (out[oh * ow * es:] == SENT).all()
    held_call(env, lambda st: ctx.gather_2d_device(d_a.data_ptr(), es, H, W, d_y.data_ptr(), oh, d_x.data_ptr(), ow,
                                                   out.ctypes.data, stream=st), [out], check)


def test_copy_2d_pitched(env):
    ctx = env.ctx
    rows, src_pitch, dst_pitch, width = 50, 203, 251, 187
    src = np.random.default_rng(16).integers(0, 256, size=(rows, src_pitch), dtype=np.uint8)
    d_src = _dev(src)
    out = _pinned(ctx, rows * dst_pitch)

    def check():
        got = out.reshape(rows, dst_pitch)
        assert np.array_equal(got[:, :width], src[:, :width])
        assert (got[:, width:] == SENT).all()
    held_call(env, lambda st: ctx.copy_2d_device(out.ctypes.data, dst_pitch, d_src.data_ptr(), src_pitch, width, rows, stream=st),
              [out], check)


def test_memcpy_h2d_then_d2h(env):
    ctx = env.ctx
    nbytes = 1 << 18
    src = _pinned(ctx, nbytes)
    src[:] = np.random.default_rng(17).integers(0, 256, size=nbytes, dtype=np.uint8)
    d_buf = _devbuf(nbytes)
    d_buf.fill_(0)
    out = _pinned(ctx, nbytes)

    def launch(st):
        ctx.h2d_async(d_buf.data_ptr(), src, stream=st)
        ctx.d2h_async(out, d_buf.data_ptr(), stream=st)

    def check():
        assert np.array_equal(out, src)
    held_call(env, launch, [out], check)


def test_event_record_waits_for_the_stream(env):
    ctx = env.ctx
    start, stop = ctx.event(), ctx.event()
    try:
        ev = env.hold(MIN_HOLD_MS)
        ctx.record(start, env.s2.cuda_stream)
        ctx.record(stop, env.s1.cuda_stream)
        ctx.synchronize(env.s2.cuda_stream)
        assert not ev.query(), 'the hold was sized wrongly'
        env.s1.synchronize()
        # `start` was recorded at once on s2, `stop` behind the hold on s1
        assert ctx.elapsed_ms(start, stop) > 0.5 * MIN_HOLD_MS
    finally:
        ctx.destroy_event(start)
        ctx.destroy_event(stop)


def test_stream_synchronize_waits_for_the_hold(env):
    ev = env.hold(MIN_HOLD_MS)
    t0 = time.perf_counter()
    env.ctx.synchronize(env.s1.cuda_stream)
    assert ev.query()
    assert (time.perf_counter() - t0) * 1e3 > 0.5 * MIN_HOLD_MS


# ---- (b) the Float32 untile scratch across streams ------------------------------------------------------------------
def _fp3_inputs(n, shape=(H, W), tile=64):
    rasters = [_raster(np.float32, shape, 200 + k) for k in range(n)]
    return rasters, [_dev(co.blocks(r, tile, 3)) for r in rasters]


@pytest.mark.parametrize('second', ['s2', 'context stream'])
def test_untile_fp3_calls_on_two_streams_are_ordered(env, second):
    """A on the held s1, B right after on another stream: B must wait for A (the scratch holds A's running sums until A's
    gather has read them)."""
    ctx, s1 = env.ctx, env.s1
    (x, y), (d_x, d_y) = _fp3_inputs(2)
    out_a, out_b = _pinned(ctx, x.nbytes), _pinned(ctx, y.nbytes)
    ctx.untile_device(d_x.data_ptr(), 4, H, W, 64, 64, 3, out_a.ctypes.data, stream=s1.cuda_stream)   # warm the scratch
    s1.synchronize()
    out_a.view(np.uint8)[:] = SENT
    b_stream = env.s2.cuda_stream if second == 's2' else None
    hold_ms = 2 * MIN_HOLD_MS
    ev = env.hold(hold_ms)
    ctx.untile_device(d_x.data_ptr(), 4, H, W, 64, 64, 3, out_a.ctypes.data, stream=s1.cuda_stream)
    ea = torch.cuda.Event()
    ea.record(s1)
    ctx.untile_device(d_y.data_ptr(), 4, H, W, 64, 64, 3, out_b.ctypes.data, stream=b_stream)
    eb = None
    if b_stream:
        eb = torch.cuda.Event()
        eb.record(env.s2)
    # B on an independent stream would be done in well under a millisecond: watch for half the hold
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < hold_ms * 0.5e-3:
        assert not (eb.query() if eb else False), 'B completed while A was held: PREDICTOR=3 untiles not ordered'
        assert _all_sentinel([out_b]), 'B wrote its plane while A was held: PREDICTOR=3 untiles not ordered'
        time.sleep(0.002)
    assert not ev.query(), 'the hold was sized wrongly'
    assert _all_sentinel([out_a]), 'A ran during its hold'
    if eb:
        eb.synchronize()
    else:
        ctx.synchronize()
    assert ea.query(), 'B completed before A'
    s1.synchronize()
    assert out_a.tobytes() == x.tobytes()
    assert out_b.tobytes() == y.tobytes()


def test_untile_fp3_scratch_growth_on_alternating_streams():
    """Small, large, small again on alternating streams of a fresh context (unheld: growing the scratch frees the old one)."""
    c = _capi.Context(0)
    s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
    try:
        for k, (shape, st) in enumerate((((40, 33), s1), ((H, W), s2), ((40, 33), s1), ((H, W), None), ((70, 130), s2))):
            (x,), (d_x,) = _fp3_inputs(1, shape, 16)
            out = _pinned(c, x.nbytes)
            c.untile_device(d_x.data_ptr(), 4, shape[0], shape[1], 16, 16, 3, out.ctypes.data,
                            stream=st.cuda_stream if st else None)
            c.synchronize(st.cuda_stream if st else None)
            assert out.tobytes() == x.tobytes(), k
    finally:
        c.close()


# ---- (c) two streams, no host synchronisation inside a round --------------------------------------------------------
def test_two_streams_without_host_synchronisation(env):
    ctx, s1, s2 = env.ctx, env.s1, env.s2
    streams = [s1, s2]
    p = _capi.default_params()
    # classify: one folded tile with masks, and 20 small tiles (the separate counters kernel, partials workspace)
    one = synth_tile(300, H, W, with_masks=True)
    many = [synth_tile(400 + t, 24, 40) for t in range(20)]
    dev_one, dev_many = _upload_tiles([one], N, True), _upload_tiles(many, 24 * 40, False)
    exp_one = c_oracle.classify(p, one['bands'], one['fmask'], land=one['land'], shad=one['shad'], ocean=one['ocean'])
    exp_many = [c_oracle.classify(p, s['bands'], s['fmask']) for s in many]
    # PREDICTOR=3 DEMs, shadow, cog blocks, LAND
    dems, d_dems = _fp3_inputs(3)
    sh_dems = [synth_dem(500 + t, 120, 140) for t in range(2)]
    d_sh = _dev(np.stack(sh_dems))
    sh_stride, sh_px = 110 * 130 + 3, 110 * 130
    sh_exp = _shadow_expect(sh_dems, 5, False)
    vec, sa, ca = _sun(*SUN)
    cog_arr = _raster(np.uint16, (H, W), 9)
    d_cog = _dev(cog_arr)
    cog_want = np.concatenate([d for _, _, d in co.cog_levels(cog_arr, (2, 4), 64, 2)])
    assert cog_want.size == _capi.cog_layout(H, W, 2, (2, 4), 64)['total_bytes']
    land_in = [synth_landcover_inputs(600 + t, 50, 60) for t in range(2)]
    d_wc, d_cg = _dev(np.stack([x[0] for x in land_in])), _dev(np.stack([x[1] for x in land_in]))
    land_exp = [o.landcover_mask_from_warped(wc, cg, L.DEFAULT_FOREST, year=2000, thresholds=(6, 3, 7, 3)) for wc, cg in land_in]
    land_stride = 50 * 60 + 1

    def out_classify(n, stride):
        outs = {k: _devbuf(n * stride * (2 if k == 'diag' else 1)) for k in LAYERS}
        pout = _capi.PlanesOut()
        for k, t in outs.items():
            setattr(pout, k, t.data_ptr())
        return outs, pout, _devbuf(n * 24)

    for rnd in range(20):
        st = [streams[(rnd + k) % 2].cuda_stream for k in range(8)]
        if rnd % 3 == 1:
            env.hold(2.0 + rnd % 4, streams[rnd % 2])
        if rnd % 5 == 2:
            env.hold(1.0, streams[(rnd + 1) % 2])
        o1, pout1, c1 = out_classify(1, N)
        ctx.classify_device(p, 1, N, _planes_in(dev_one, True), pout1, c1.data_ptr(), stream=st[0])
        u = [_devbuf(x.nbytes) for x in dems]
        for k in range(3):
            ctx.untile_device(d_dems[(rnd + k) % 3].data_ptr(), 4, H, W, 64, 64, 3, u[k].data_ptr(), stream=st[1 + k])
        o2, pout2, c2 = out_classify(20, 24 * 40)
        ctx.classify_device(p, 20, 24 * 40, _planes_in(dev_many, False), pout2, c2.data_ptr(), stream=st[4])
        sh = _devbuf(2 * sh_stride)
        ctx.shadow_layer_device(d_sh.data_ptr(), 2, 120, 140, 5, vec, sa, ca, MIN_SLOPE, MAX_INC, sh.data_ptr(), stream=st[5],
                                out_tile_stride=sh_stride)
        cog = _devbuf(cog_want.size)
        ctx.cog_blocks_device(d_cog.data_ptr(), 2, H, W, cog.data_ptr(), (2, 4), 64, 2, stream=st[6])
        land = _devbuf(2 * land_stride)
        ctx.landcover_mask_device(d_wc.data_ptr(), d_cg.data_ptr(), 2, 50, 60, L.DEFAULT_FOREST, land.data_ptr(),
                                  thresholds=(6, 3, 7, 3), stream=st[7], out_tile_stride=land_stride)
        s1.synchronize()
        s2.synchronize()
        torch.cuda.synchronize()

        def host(t, dtype=np.uint8):
            return t.cpu().numpy().view(dtype)
        for k in LAYERS:
            dt = np.uint16 if k == 'diag' else np.uint8
            assert np.array_equal(host(o1[k], dt)[:N], exp_one[k].ravel()), (rnd, k)
            g = host(o2[k], dt)[:20 * 24 * 40].reshape(20, -1)
            for t in range(20):
                assert np.array_equal(g[t], exp_many[t][k].ravel()), (rnd, k, t)
        assert host(c1, np.int64)[:3].tolist() == exp_one['counters'].tolist(), rnd
        assert host(c2, np.int64)[:60].reshape(20, 3).tolist() == [e['counters'].tolist() for e in exp_many], rnd
        for k in range(3):
            assert host(u[k])[:dems[0].nbytes].tobytes() == dems[(rnd + k) % 3].tobytes(), (rnd, k)
        g = host(sh)[:2 * sh_stride].reshape(2, sh_stride)
        for t in range(2):
            assert np.array_equal(g[t, :sh_px], sh_exp[t].ravel()), (rnd, t)
        assert np.array_equal(host(cog)[:cog_want.size], cog_want), rnd
        g = host(land)[:2 * land_stride].reshape(2, land_stride)
        for t in range(2):
            assert np.array_equal(g[t, :50 * 60], land_exp[t].ravel()), (rnd, t)
