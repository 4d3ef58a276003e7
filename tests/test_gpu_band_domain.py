"""The six int16 reflectance planes over their whole range, on every classify kernel and entry.

The per-pixel arithmetic that reads the bands exists four times: packed int16 with saturating sign-bit tests and
thresholds clamped to int16 (table-driven kernel, dswx_tables.h lut_group / make_lut_consts), scalar int with (short)
wrap sums (classify_px: the direct kernel dswx_classify_v8 and the generic dswx_classify_v1), and two float32 chains
(lut_group<F32> and classify_px_f32).  synth_tile draws bands near realistic means, so the rest of the suite hardly
leaves the middle of the int16 range.  Here the bands are full-range (oracle/band_inputs.py): the reference-made
fixtures of those domains on every kernel, exhaustive single-band slices (all 65,536 values of one band against edge
values of the other five), the float32 chain with scales / offsets that make +-inf and NaN indices, every C-ABI entry,
the float64 index planes and the clip-off vector fixtures.  Every integer layer and the three counters (written over a
sentinel) must equal the scalar C oracle bit for bit; 'cover' mode is compared with the numpy oracle."""
import functools

import numpy as np
import pytest

from oracle import band_inputs as bi
from oracle import c_oracle
from oracle import dswx_oracle as o
from proteus_amd import _capi
from proteus_amd.synth import synth_tile, SEED
from tests import _golden as G
from tests.test_c_oracle import NAME, params_of_case, check_case, binary_repr

pytestmark = pytest.mark.gpu

ALL_LAYERS = ('diag', 'wtr1', 'wtr1_aerosol', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud')
MASK_PLANES = ('land', 'shad', 'ocean')
SENTINEL = -7
BAND_CASES = [n for n in G.tile_case_names() if '_band_' in n]
assert len(BAND_CASES) == 7, BAND_CASES


def check(got, exp, layers, what):
    for k in layers:
        assert np.array_equal(np.asarray(got[k]).reshape(exp[k].shape), exp[k]), (what, k)
    assert np.asarray(got['counters']).reshape(-1, 3).sum(axis=0).tolist() == exp['counters'].tolist(), what


def _pinned(c, a):
    q = c.pinned_empty(a.shape, a.dtype)
    q[...] = a
    return q


@pytest.fixture(scope='module')
def ctxs():
    """The automatic choice (table-driven), the direct kernel (fused_variant = 0) and the staged host pipeline."""
    made = {'lut': _capi.Context(0)}
    for name, settings in (('direct', dict(fused_variant=0)), ('staged', dict(host_pipeline=1, host_chunks=3))):
        made[name] = _capi.Context(0)
        made[name].lab_configure(**settings)
    yield made
    for c in made.values():
        c.close()


# ---- 1. the reference-made fixtures on every kernel ---------------------------------------------------------------------
def _as_tiles(a, th, tw):
    """The pixels of a [H, W] plane as [T, th, tw] tiles (the tail that does not fill a tile is dropped)."""
    n = (a.size // (th * tw)) * th * tw
    return np.ascontiguousarray(a.ravel()[:n].reshape(-1, th, tw))


KERNELS = ['lut masks', 'lut plain', 'lut browse', 'direct', 'generic 1x1', 'generic 1x7', 'generic 3x5']


def _fixture_kernel_cases():
    out = []
    for name in BAND_CASES:
        for k in KERNELS:
            if 'cover' in name and k not in ('lut masks', 'direct'):
                continue                    # the dilation is per tile: the fixture is one tile
            out.append((name, k))
    return out


@pytest.mark.parametrize('name, kernel', _fixture_kernel_cases())
def test_fixtures_on_every_kernel(ctxs, name, kernel):
    c = G.tile_case(name)
    f32 = c['offset_and_scale'] is not None
    for collapse in (False, True):
        p = params_of_case(c, collapse)
        masks = {m: c[m] for m in MASK_PLANES if c[m] is not None}
        bands, fmask, layers = c['bands'], c['fmask'], ALL_LAYERS
        if kernel == 'lut plain':
            masks = {}
        if kernel == 'lut browse':
            layers = ALL_LAYERS + ('browse',)
        ctx = ctxs['direct' if kernel == 'direct' else 'lut']
        if kernel.startswith('generic'):
            th, tw = map(int, kernel.split()[1].split('x'))
            bands = [_as_tiles(b, th, tw) for b in bands]
            fmask = _as_tiles(fmask, th, tw)
            masks = {m: _as_tiles(v, th, tw) for m, v in masks.items()}
        got = ctx.classify_host(bands, fmask, p, layers=layers, **masks)
        info = ctx.last_kernel_info()
        if kernel.startswith('lut'):
            assert 'dswx_classify_lut' in info, info
            assert c['mode'] == 'cover' or ('extras' in info) == (kernel == 'lut browse'), info
        elif kernel == 'direct':
            assert 'dswx_classify_v8' in info, info
        elif kernel != 'generic 3x5':
            assert 'dswx_classify_v1' in info, info             # (3 x 5: one 8-pixel group per tile, the rest generic)
        assert (('f32' in info) == f32) or kernel.startswith('generic'), info
        if c['mode'] == 'cover':
            check_case(got, c, collapse, name)
            continue
        if kernel in ('lut masks', 'direct'):
            check_case(got, c, collapse, name)            # the reference's own outputs
        exp = c_oracle.classify(p, bands, fmask, layers=layers, **masks)
        check(got, exp, layers, (name, kernel, collapse))
        if kernel.startswith('generic'):
            assert got['counters'].shape == (bands[0].shape[0], 3)
            want = [c_oracle.classify(p, [b[t] for b in bands], fmask[t], **{m: v[t] for m, v in masks.items()})
                    ['counters'].tolist() for t in range(0, bands[0].shape[0], 97)]
            assert got['counters'][::97].tolist() == want


# ---- 2. exhaustive single-band slices -----------------------------------------------------------------------------------
SLICE_BASES = 16


@functools.lru_cache(maxsize=2)
def slice_tile(thr_key=None):
    """For each band, all 65,536 int16 values x SLICE_BASES base vectors of the other five bands: one tile of
    6 x 16 x 65,536 pixels as [6144, 1024].  Bases: four realistic water / land vectors, then edge values (with the
    thresholds of `thr_key` +-1).  Fmask cycles through all 256 bytes; LAND through all bytes; SHAD and OCEAN 0 / 1."""
    thr = dict(PARAM_SETS[thr_key].get('thresholds') or {}) if thr_key else {}
    thr.setdefault('aerosol_max_nir', PARAM_SETS[thr_key].get('aerosol_max_nir', 1000) if thr_key else 1000)
    rng = np.random.default_rng(5150)
    bases = np.array([(300, 400, 300, 200, 100, 50), (100, 281, 300, 1700, 219, 50),
                      (400, 1000, 600, 1499, 899, 300), (500, 600, 700, 3000, 2500, 1500)], np.int16)
    edges = np.stack([rng.choice(bi.edge_values(b, thr), SLICE_BASES - len(bases)) for b in bi.BAND_NAMES], axis=1)
    bases = np.concatenate([bases, edges.astype(np.int16)])
    v = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    planes = np.empty((6, 6, SLICE_BASES, 65536), np.int16)       # [swept band][plane][base][value]
    for k in range(6):
        for j in range(6):
            planes[k, j] = v[None, :] if j == k else bases[:, j][:, None]
    shape = (6 * SLICE_BASES * 64, 1024)
    bands = [np.ascontiguousarray(planes[:, j].reshape(shape)) for j in range(6)]
    i = np.arange(bands[0].size, dtype=np.int64)
    fm = ((i * 97 + (i >> 16) * 31) & 255).astype(np.uint8).reshape(shape)
    land = ((i * 13 + (i >> 8) * 7) & 255).astype(np.uint8).reshape(shape)
    shad = (((i // 3) * 5 + (i >> 16)) % 4 != 0).astype(np.uint8).reshape(shape)
    ocean = (((i // 5) * 3 + (i >> 12)) % 9 != 0).astype(np.uint8).reshape(shape)
    for b in bands:
        b.setflags(write=False)
    return bands, fm, dict(land=land, shad=shad, ocean=ocean)


_EDGE_A = dict(o.DEFAULT_THRESHOLDS, pswt_1_nir=32767.5, pswt_1_swir1=-32768, pswt_2_blue=32768, pswt_2_nir=32768,
               pswt_2_swir1=-32767.5, pswt_2_swir2=32767, lcmask_nir=32767, awgt=1e5)
_EDGE_B = dict(o.DEFAULT_THRESHOLDS, pswt_1_nir=-32769, pswt_1_swir1=32767.5, pswt_2_blue=-32767.5, pswt_2_nir=-32769,
               pswt_2_swir1=32768, pswt_2_swir2=-32768, lcmask_nir=-32769, awgt=-1e5)
_EDGE_C = dict(o.DEFAULT_THRESHOLDS, pswt_1_nir=32768, pswt_1_swir1=32767, pswt_2_blue=32767.5, pswt_2_nir=32767.5,
               pswt_2_swir1=32768, pswt_2_swir2=32768, lcmask_nir=32766.5, awgt=0.75)
_EDGE_D = dict(o.DEFAULT_THRESHOLDS, pswt_1_nir=40000, pswt_1_swir1=32768.5, pswt_2_blue=1e9, pswt_2_nir=32769,
               pswt_2_swir1=65000, pswt_2_swir2=32768.5, lcmask_nir=1e5, awgt=-0.25)
_FILLS = (-32768.0, 32767.0, 0.0, 1.0)
PARAM_SETS = {
    'defaults': dict(),
    'clip off': dict(clip_negative_reflectance=False),
    **{f'fills {i}': dict(band_fills=[_FILLS[(k + i) % 4] for k in range(6)], fmask_fill=(255.0, 0.0)[i % 2],
                          clip_negative_reflectance=i < 2) for i in range(4)},
    'edges a': dict(thresholds=_EDGE_A, aerosol_max_nir=32767),
    'edges a clip off': dict(thresholds=_EDGE_A, aerosol_max_nir=-32768, clip_negative_reflectance=False),
    'edges b clip off': dict(thresholds=_EDGE_B, aerosol_max_nir=32767, clip_negative_reflectance=False),
    'edges c': dict(thresholds=_EDGE_C, aerosol_max_nir=1000.5),
    # past the int16 range: "x < t" with t > 32768 holds for every int16 x (the packed constants must clamp, not wrap)
    'edges d clip off': dict(thresholds=_EDGE_D, aerosol_max_nir=32768.5, clip_negative_reflectance=False),
}


@functools.lru_cache(maxsize=2)
def _slice_expected(key, collapse):
    bands, fm, masks = slice_tile(key)
    p = _capi.make_params(**PARAM_SETS[key], collapse_wtr_classes=collapse)
    return p, c_oracle.classify(p, bands, fm, **masks)


@pytest.mark.parametrize('key', list(PARAM_SETS))
def test_exhaustive_single_band_slices(ctxs, key):
    """Every parameter set on the table-driven and the direct kernel, both collapse settings."""
    bands, fm, masks = slice_tile(key)
    for collapse in (True, False):
        p, exp = _slice_expected(key, collapse)
        for kernel in ('lut', 'direct'):
            ctx = ctxs[kernel]
            got = ctx.classify_host(bands, fm, p, **masks)
            assert ('dswx_classify_lut' if kernel == 'lut' else 'dswx_classify_v8') in ctx.last_kernel_info()
            check(got, exp, ALL_LAYERS, (key, kernel, collapse))


def test_exhaustive_single_band_slices_generic_kernel(ctxs):
    """The 'edges a clip off' set through 1-wide tiles of 6 pixels: every pixel on dswx_classify_v1.  All 65,536 values
    of each band against the first base vector (all five tests true) and the first edge base: 131,072 tiles (the host
    path takes about 0.2 ms per tile)."""
    key = 'edges a clip off'
    bands, fm, masks = slice_tile(key)
    keep = np.zeros((6, SLICE_BASES, 64, 1024), bool)
    keep[:, [0, 4]] = True
    keep = keep.reshape(bands[0].shape)
    t = lambda a: np.ascontiguousarray(a[keep]).reshape(-1, 6, 1)
    ctx = ctxs['lut']
    p = _capi.make_params(**PARAM_SETS[key])
    sub = [t(b) for b in bands], t(fm), {m: t(v) for m, v in masks.items()}
    exp = c_oracle.classify(p, sub[0], sub[1], **sub[2])
    got = ctx.classify_host(sub[0], sub[1], p, **sub[2])
    assert 'dswx_classify_v1' in ctx.last_kernel_info() and 'lut' not in ctx.last_kernel_info()
    check(got, exp, ALL_LAYERS, key)


# ---- 3. the float32 chain at full range ---------------------------------------------------------------------------------
SCALES = (1e-4, 2.75e-5, 3.0, -1e-4, 0.0)
OFFSETS = (0.0, 7.0, 1000.0, 16384.0, -30.5)


def _f32_set(i):
    """Parameter set i: a scale and an offset per band from SCALES x OFFSETS (green and swir1 share theirs, as do nir and
    red, so that their sums can cancel: set 0 has offsets inside the data for both pairs), thresholds in scaled units of
    the band each compares (scale * (t - offset)), the aerosol nir limit too."""
    gs, nr = (SCALES[i], OFFSETS[(i + 2) % 5]), (SCALES[(i + 1) % 5], OFFSETS[(i + 3) % 5])
    so = [(SCALES[(i + 2) % 5], OFFSETS[(i + 4) % 5]), gs, nr, nr, gs, (SCALES[(i + 3) % 5], OFFSETS[(i + 1) % 5])]
    sc = lambda band, t: so[band][0] * (t - so[band][1])
    thr = dict(o.DEFAULT_THRESHOLDS, pswt_1_nir=sc(3, 1500), pswt_1_swir1=sc(4, 900), pswt_2_blue=sc(0, 1000),
               pswt_2_nir=sc(3, 2500), pswt_2_swir1=sc(4, 3000), pswt_2_swir2=sc(5, 1000), lcmask_nir=sc(3, 1200))
    return so, thr, sc(3, 1000)


F32_CASES = [(dom, i) for dom in ('f32_ties', 'int16') for i in range(5)] + [('denormal', 0), ('denormal', 1),
                                                                               ('overflow', 0), ('overflow', 1)]


def _f32_case(dom, i):
    if dom == 'denormal':
        # a float32-denormal scale (and thresholds) / a denormal awgt: the library must not flush them, as numpy does not
        so = [(1e-42, 0.0), (1e-42, 7.0), (1e-42, 0.0), (1e-42, 1000.0), (1e-42, 0.0), (1e-42, -30.5)] if i == 0 else \
            [(1e-4, 0.0)] * 6
        thr = dict(o.DEFAULT_THRESHOLDS, awgt=(1e-42 if i == 0 else -1e-42), pswt_1_nir=3e-42, pswt_1_swir1=1e-42,
                   pswt_2_blue=2e-42, pswt_2_nir=5e-42, pswt_2_swir1=4e-42, pswt_2_swir2=1e-42, lcmask_nir=1.2e-39)
        aer, bdom = 1e-39, 'int16'
    elif dom == 'overflow':
        # scales near the top of float32: reflectances of +-inf, so that MNDWI, NDVI and AWESH are inf - inf = NaN
        big = 3e38 if i == 0 else -3e38
        so = [(big, 0.0), (big, 0.0), (1e-4, 0.0), (3e38, 7.0), (big, 1000.0), (1e-4, 0.0)]
        thr, aer, bdom = dict(o.DEFAULT_THRESHOLDS), 1000.0, 'int16'
    else:
        so, thr, aer = _f32_set(i)
        bdom = dom
    s = synth_tile(600 + i, 160, 200, with_masks=True)
    s = bi.with_bands(s, bdom, 7000 + 10 * i + len(dom), scale_offset=so)
    return s, so, thr, aer


@pytest.mark.parametrize('kernel', ['lut', 'direct', 'generic'])
@pytest.mark.parametrize('dom, i', F32_CASES)
def test_float32_chain_full_range(ctxs, dom, i, kernel):
    s, so, thr, aer = _f32_case(dom, i)
    bands, fm, masks = s['bands'], s['fmask'], {m: s[m] for m in MASK_PLANES}
    if kernel == 'generic':
        t = lambda a: a.reshape(-1, 1, 5)
        bands, fm, masks = [t(b) for b in bands], t(fm), {m: t(v) for m, v in masks.items()}
    ctx = ctxs['direct' if kernel == 'direct' else 'lut']
    for collapse in (True, False):
        p = _capi.make_params(thr, offset_and_scale=so, aerosol_max_nir=aer, collapse_wtr_classes=collapse)
        exp = c_oracle.classify(p, bands, fm, **masks)
        got = ctx.classify_host(bands, fm, p, **masks)
        info = ctx.last_kernel_info()
        assert {'lut': 'dswx_classify_lut', 'direct': 'dswx_classify_v8', 'generic': 'dswx_classify_v1'}[kernel] in info
        assert kernel == 'generic' or 'f32' in info, info
        check(got, exp, ALL_LAYERS, (dom, i, kernel, collapse))
        if i == 0 and collapse:
            # one set per kernel against the numpy oracle too (float32 arrays, Python-float scalars; its aerosol nir
            # limit is the reference's constant 1000)
            with np.errstate(all='ignore'):
                e = o.classify_tile(s['bands'], s['fmask'], o.Thresholds(**thr), landcover=s['land'], shadow=s['shad'],
                                    ocean_mask=s['ocean'], offset_and_scale=so)
            gn = ctx.classify_host(bands, fm, _capi.make_params(thr, offset_and_scale=so), **masks)
            for layer, key in NAME.items():
                assert np.array_equal(np.asarray(gn[key]).reshape(e[layer].shape), e[layer]), (dom, i, kernel, layer)
            ec = e['counters']
            assert gn['counters'].sum(axis=0).tolist() == [ec['n_valid'], ec['n_cloud_and_valid'], ec['n_not_ocean']]


def test_float32_ties_make_inf_and_nan():
    """The f32_ties domain really gives NaN and +-inf MNDWI / NDVI on the float32 chain."""
    s, so, thr, aer = _f32_case('f32_ties', 0)
    (b, g, r, n, s1, s2), _ = o.condition_inputs(s['bands'], s['fmask'], offset_and_scale=so)
    with np.errstate(all='ignore'):
        mndwi, ndvi = (g - s1) / (g + s1), (n - r) / (n + r)
    for x in (mndwi, ndvi):
        assert x.dtype == np.float32 and np.isnan(x).any() and np.isinf(x).any()


# ---- 4. every entry, full-range bands -----------------------------------------------------------------------------------
ENTRY_DOMAINS = ['int16', 'positive', 'edges', 'mix']


@functools.lru_cache(maxsize=32)
def entry_tile(dom, tile, h, w):
    s = synth_tile(tile, h, w, with_masks=True)
    s = bi.with_bands(s, dom, 9000 + tile, thr=dict(o.DEFAULT_THRESHOLDS, aerosol_max_nir=1000))
    rng = np.random.default_rng(tile)
    s['land'] = rng.integers(0, 256, (h, w)).astype(np.uint8)         # every LAND class, the nir rule included
    return s


def masks_of(s):
    return {m: s[m] for m in MASK_PLANES}


@pytest.mark.parametrize('dom', ENTRY_DOMAINS)
@pytest.mark.parametrize('shape', [(400, 700), (37, 53)])
def test_classify_host_paths(ctxs, shape, dom):
    h, w = shape
    s = entry_tile(dom, 100 + h, h, w)
    p = _capi.default_params()
    exp = c_oracle.classify(p, s['bands'], s['fmask'], **masks_of(s))
    ctx = ctxs['lut']
    check(ctx.classify_host(s['bands'], s['fmask'], p, **masks_of(s)), exp, ALL_LAYERS, 'pageable')
    for name, c, tag in (('zero copy', ctx, 'zero copy across PCIe'), ('staged', ctxs['staged'], 'pipelined over 3 streams')):
        got = c.classify_host([_pinned(c, b) for b in s['bands']], _pinned(c, s['fmask']), p,
                              **{m: _pinned(c, v) for m, v in masks_of(s).items()})
        assert tag in c.last_kernel_info(), c.last_kernel_info()
        check(got, exp, ALL_LAYERS, name)


def _arena_run(ctx, p, tiles, h, w, band_off=0, u8_off=0, two_d=False):
    """The planes of `tiles` (each [h, w]) contiguous in one device arena, int16 planes at `band_off` bytes past a
    256-byte boundary, byte planes at `u8_off`; dswx_classify_device (or _2d) into device outputs; returns the layers
    [T, h, w] and the counters, which start as SENTINEL."""
    n, t = h * w, len(tiles)
    size = t * n
    arena = ctx.malloc(size * 32 + 4096)
    pin, pout = _capi.PlanesIn(), _capi.PlanesOut()
    off = 0

    def place(a, align_off, itemsize):
        nonlocal off
        off = (off + 255) // 256 * 256 + align_off
        arena.upload(np.ascontiguousarray(a).ravel(), off)
        at = off
        off += size * itemsize + 1
        return at
    try:
        for i in range(6):
            pin.band[i] = arena.ptr + place(np.stack([s['bands'][i] for s in tiles]), band_off, 2)
        for name in ('fmask',) + MASK_PLANES:
            setattr(pin, name, arena.ptr + place(np.stack([s[name] for s in tiles]), u8_off, 1))
        where = {}
        for name in ALL_LAYERS:
            off = (off + 255) // 256 * 256 + (0 if name == 'diag' else u8_off)
            where[name] = off
            setattr(pout, name, arena.ptr + off)
            off += size * (2 if name == 'diag' else 1) + 1
        cnt_off = (off + 255) // 256 * 256
        arena.upload(np.full(3 * t, SENTINEL, np.int64), cnt_off)
        if two_d:
            ctx.classify_device_2d(p, t, h, w, pin, pout, counters_ptr=arena.ptr + cnt_off)
        else:
            ctx.classify_device(p, t, n, pin, pout, counters_ptr=arena.ptr + cnt_off)
        ctx.synchronize()
        got = {k: arena.download(np.uint16 if k == 'diag' else np.uint8, size, where[k]).reshape(t, h, w)
               for k in ALL_LAYERS}
        got['counters'] = arena.download(np.int64, 3 * t, cnt_off).reshape(t, 3)
        return got
    finally:
        arena.free()


@pytest.mark.parametrize('dom', ENTRY_DOMAINS)
@pytest.mark.parametrize('entry, band_off, u8_off', [('2d', 0, 0), ('1d', 2, 1), ('1d', 6, 3), ('2d', 2, 5),
                                                     ('1d', 2, 7)])
def test_device_entries_and_unaligned_planes(ctxs, dom, entry, band_off, u8_off):
    """dswx_classify_device_2d on aligned planes, and int16 planes at 2-byte / byte planes at odd offsets (the unaligned
    vector path of the table-driven kernel), three tiles of 41 x 43 (H * W % 8 = 3)."""
    h, w = 41, 43
    tiles = [entry_tile(dom, 300 + t, h, w) for t in range(3)]
    p = _capi.default_params()
    ctx = ctxs['lut']
    got = _arena_run(ctx, p, tiles, h, w, band_off, u8_off, two_d=entry == '2d')
    assert 'dswx_classify_lut' in ctx.last_kernel_info(), ctx.last_kernel_info()
    for t, s in enumerate(tiles):
        exp = c_oracle.classify(p, s['bands'], s['fmask'], **masks_of(s))
        for k in ALL_LAYERS:
            assert np.array_equal(got[k][t], exp[k]), (t, k)
        assert got['counters'][t].tolist() == exp['counters'].tolist(), t


@pytest.mark.parametrize('dom', ENTRY_DOMAINS)
@pytest.mark.parametrize('align, shape', [(256, (400, 700)), (1, (37, 53))])
def test_device_batch_walks(ctxs, align, shape, dom):
    """DeviceBatch.classify over 17 resident tiles walked at 17, 16, 1 and 5 tiles, padded and contiguous ragged."""
    n, (h, w) = 17, shape
    ctx = ctxs['lut']
    b = _capi.DeviceBatch(ctx, n, h, w, masks=True, extra_layers=('wtr1_aerosol',), tile_align=align)
    try:
        b.synth(SEED, tile0=400)                        # (the padding between tiles holds recipe data, as in use)
        p = _capi.default_params()
        exp = []
        for t in range(n):
            st = entry_tile(dom, 400 + t, h, w)
            for name in _capi.BAND_NAMES:
                b.write_tile(name, t, st['bands'][_capi.BAND_NAMES.index(name)])
            for m in ('fmask',) + MASK_PLANES:
                b.write_tile(m, t, st[m])
            exp.append(c_oracle.classify(p, st['bands'], st['fmask'], **masks_of(st)))
        for k in (17, 16, 1, 5):
            b.write_counters_sentinel(SENTINEL)
            b.classify(p, n_tiles=k)
            if align == 1 and k > 1:
                assert 'ragged tiles' in ctx.last_kernel_info()
            ctx.synchronize()
            cnt = b.read_counters()
            for t in range(k):
                assert cnt[t].tolist() == exp[t]['counters'].tolist(), (k, t)
            assert (cnt[k:] == SENTINEL).all(), k
            if k in (17, 5):
                for t in range(k):
                    for key in ALL_LAYERS:
                        assert np.array_equal(b.read_tile(key, t), exp[t][key]), (k, t, key)
    finally:
        b.free()


@pytest.mark.parametrize('dom', ENTRY_DOMAINS)
def test_cover_mode_and_tile_engine(ctxs, dom):
    """'cover' mode against the numpy oracle, and pipeline.TileEngine.classify with resident planes."""
    from proteus_amd import pipeline
    h, w = 400, 700
    s = entry_tile(dom, 500, h, w)
    ctx = ctxs['lut']
    pc = _capi.make_params(mask_adjacent_to_cloud_mode='cover')
    got = ctx.classify_host(s['bands'], s['fmask'], pc, **masks_of(s))
    with np.errstate(all='ignore'):
        e = o.classify_tile(s['bands'], s['fmask'], landcover=s['land'], shadow=s['shad'], ocean_mask=s['ocean'],
                            mask_adjacent_to_cloud_mode='cover')
    for layer, key in NAME.items():
        assert np.array_equal(got[key], e[layer]), ('cover', key)
    c = e['counters']
    assert got['counters'][0].tolist() == [c['n_valid'], c['n_cloud_and_valid'], c['n_not_ocean']]
    p = _capi.default_params()
    exp = c_oracle.classify(p, s['bands'], s['fmask'], **masks_of(s))
    eng = pipeline.TileEngine(ctx)
    try:
        planes = {m: eng.upload(s[m]) for m in MASK_PLANES}
        res = eng.classify([eng.upload(b) for b in s['bands']], eng.upload(s['fmask']), p, layers=ALL_LAYERS, **planes)
        got = {k: res[k].numpy() for k in ALL_LAYERS}
        got['counters'] = res['counters']
        check(got, exp, ALL_LAYERS, 'engine')
    finally:
        eng.close()


# ---- 5. float64 index planes --------------------------------------------------------------------------------------------
def _check_indices(got, bands):
    b, g, r, n, s1, s2 = [np.asarray(x) for x in bands]
    with np.errstate(all='ignore'):
        mndwi, _, _, awesh, ndvi = o.spectral_indices(b, g, r, n, s1, s2)
    for key, want in (('mndwi', mndwi), ('ndvi', ndvi), ('awesh', awesh)):
        x = np.asarray(got[key]).reshape(want.shape)
        assert np.array_equal(np.isnan(x), np.isnan(want)), key
        inf = np.isinf(want)
        assert np.array_equal(x[inf], want[inf]) and not np.isinf(x[~inf]).any(), key
        fin = np.isfinite(want)
        assert np.max(np.abs(x[fin] - want[fin]), initial=0.0) <= 1e-6, key
        assert np.array_equal(x, want, equal_nan=True), key            # in fact bit-equal


@pytest.mark.parametrize('clip', [True, False])
def test_float64_indices_ragged_batch_and_unaligned(ctxs, clip):
    """mndwi / ndvi / awesh (dswx_indices_v1) of int16 bands on a ragged multi-tile host batch (5 tiles of 37 x 53) and
    on planes at odd addresses; the indices are of the clipped bands when the clip is on."""
    ctx = ctxs['lut']
    h, w = 37, 53
    tiles = [entry_tile('int16', 800 + t, h, w) for t in range(5)]
    bands = [np.stack([s['bands'][i] for s in tiles]) for i in range(6)]
    fm = np.stack([s['fmask'] for s in tiles])
    p = _capi.make_params(clip_negative_reflectance=clip)
    layers = ('diag', 'mndwi', 'ndvi', 'awesh')
    got = ctx.classify_host(bands, fm, p, layers=layers)
    ref_bands = [np.clip(b, 1, None) for b in bands] if clip else bands
    _check_indices(got, ref_bands)
    assert np.array_equal(got['diag'], c_oracle.classify(p, bands, fm, layers=('diag',))['diag'])
    # the same planes at odd addresses: int16 at +2 bytes, Fmask at +1, the float64 outputs at +8
    n = bands[0].size
    arena = ctx.malloc(n * 48 + 4096)
    try:
        pin, pout = _capi.PlanesIn(), _capi.PlanesOut()
        off = 2
        for i in range(6):
            arena.upload(bands[i].ravel(), off)
            pin.band[i] = arena.ptr + off
            off += 2 * n + 4
        off += 1
        arena.upload(fm.ravel(), off)
        pin.fmask = arena.ptr + off
        off += n
        off = (off + 255) // 256 * 256 + 8
        where = {}
        for k in ('mndwi', 'ndvi', 'awesh'):
            where[k] = off
            setattr(pout, k, arena.ptr + off)
            off += 8 * n + 8
        ctx.classify_device(p, 1, n, pin, pout)
        ctx.synchronize()
        got = {k: arena.download(np.float64, n, where[k]) for k in where}
        _check_indices(got, [b.ravel() for b in ref_bands])
    finally:
        arena.free()


# ---- 6. the clip-off vector fixtures on the direct and generic kernels --------------------------------------------------
@pytest.mark.parametrize('kernel', ['direct', 'generic'])
@pytest.mark.parametrize('fixture', ['diag_vectors.npz', 'diag_vectors_wide.npz'])
def test_diag_vector_fixtures(ctxs, fixture, kernel):
    """Every threshold set of the fixture with the clip off and no fills (the reference's DIAG), and with fills and the
    clip on or off (all layers against the C oracle); Fmask and LAND cycle through all bytes."""
    z = G.load(fixture)
    vec = z['bands']
    if kernel == 'generic' and fixture == 'diag_vectors.npz':
        # a tile per 7 vectors is slow on the host path: the tie vectors (the first 8000) and every 8th of the rest
        vec = vec[np.r_[0:8000, 8000:vec.shape[0]:8]]
    n = vec.shape[0]
    tags = [k[4:] for k in z.files if k.startswith('thr_')]
    cols = [np.ascontiguousarray(vec[:, i]) for i in range(6)]
    i = np.arange(n)
    fm0 = np.zeros(n, np.uint8)
    fm = ((i * 37) & 255).astype(np.uint8)
    masks = dict(land=((i * 11) & 255).astype(np.uint8), shad=(i % 3 != 0).astype(np.uint8),
                 ocean=(i % 17 != 0).astype(np.uint8))
    ctx = ctxs['direct' if kernel == 'direct' else 'lut']
    # the generic kernel: tiles of 1 x 7 pixels (the last n % 7 vectors are left out); the direct kernel: one row
    cut = (lambda a: a[:n - n % 7].reshape(-1, 1, 7)) if kernel == 'generic' else (lambda a: a.reshape(1, n))
    for tag in tags:
        thr = dict(zip(G.THR_KEYS, z['thr_' + tag].tolist()))
        p = _capi.make_params(thr, band_fills=[None] * 6, fmask_fill=None, clip_negative_reflectance=False)
        got = ctx.classify_host([cut(c) for c in cols], cut(fm0), p, layers=ALL_LAYERS)
        info = ctx.last_kernel_info()
        assert ('dswx_classify_v8' if kernel == 'direct' else 'dswx_classify_v1') in info, info
        want = binary_repr(z['diag_' + tag].ravel())
        if vec.shape[0] != z['bands'].shape[0]:
            want = want[np.r_[0:8000, 8000:z['bands'].shape[0]:8]]
        assert np.array_equal(got['diag'].ravel(), want[:got['diag'].size]), tag
        exp = c_oracle.classify(p, [cut(c) for c in cols], cut(fm0))
        check(got, exp, ALL_LAYERS, tag)
        for fills, clip in (([-32768.0, 0.0, 1.0, 32767.0, -9999.0, -1.0], False),
                            ([0.0, -32768.0, 32767.0, 1.0, -256.0, 2.0], True)):
            p = _capi.make_params(thr, band_fills=fills, fmask_fill=0.0, clip_negative_reflectance=clip)
            got = ctx.classify_host([cut(c) for c in cols], cut(fm), p, **{k: cut(v) for k, v in masks.items()})
            exp = c_oracle.classify(p, [cut(c) for c in cols], cut(fm), **{k: cut(v) for k, v in masks.items()})
            check(got, exp, ALL_LAYERS, (tag, fills, clip))
