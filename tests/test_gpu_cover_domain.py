"""mask_adjacent_to_cloud_mode 'cover' (proteus_amd/csrc/dswx_cover.hip, bind_cover_scratch and the chunk loop of
classify_device_impl) on every entry, geometry, address and Fmask byte.

The inputs are the named domains of oracle/cover_inputs.py, which tests/test_cover_domain.py shows on the CPU to do what
they are for: diamonds and walled corridors across every window seam, the 17-pixel dependency with its near pixel on the
first / last output row and column of a window and its far seed on the outermost halo row / column, all 256 Fmask bytes
in patches, saturated planes, diamonds cut by fill, ocean and shadow.  They run through the four stage-2 kernels of the
lab switch cover_kernel, both stage-1 kernels, dswx_classify_host, dswx_classify_device_2d and dswx_classify_batch at
odd tile strides and plane addresses, with subsets of the output planes, after launches that leave the scratch full of
set bits, and over more tiles than one chunk of the launch loop.

Everything is equality of integers against the numpy oracle and the reference-made fixtures: the eight layers, browse
where asked, and the three counters written over a sentinel."""
import functools

import numpy as np
import pytest

from oracle import cover_inputs as ci
from oracle import dswx_oracle as o
from proteus_amd import _capi
from tests import _golden as G
from tests.test_c_oracle import NAME, params_of_case, check_case
from tests.test_gpu_raster_domain import Dev, SENTINELS

pytestmark = pytest.mark.gpu

ALL_LAYERS = ('diag', 'wtr1', 'wtr1_aerosol', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud')
BROWSE_DEFAULT = (True, False, False, False, True)      # exclude_psw_aggressive, not_water, cloud, snow, ocean -> nodata


@pytest.fixture(scope='module')
def stage2():
    """A context per stage-2 kernel of the lab switch cover_kernel: words per window row | 16 = no LDS staging."""
    made = {'8': _capi.Context(0)}
    for name, switch in (('4', 4), ('8,direct', 8 + 16), ('4,direct', 4 + 16)):
        made[name] = _capi.Context(0)
        made[name].lab_configure(cover_kernel=switch)
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope='module')
def stage1():
    """The table-driven stage-1 kernel (the automatic choice) and the direct one (fused_variant = 0)."""
    made = {'lut': _capi.Context(0), 'direct': _capi.Context(0)}
    made['direct'].lab_configure(fused_variant=0)
    yield made
    for c in made.values():
        c.close()


def params(collapse=True, **kw):
    return _capi.make_params(mask_adjacent_to_cloud_mode='cover', collapse_wtr_classes=collapse, **kw)


def want(scene, collapse=True, browse=None, **kw):
    """The oracle's layers of a scene by C-ABI name, its three counters, and the browse layer for the five flags `browse`."""
    e = ci.expected(scene, collapse, **kw)
    out = {key: e[layer] for layer, key in NAME.items()}
    c = e['counters']
    out['counters'] = [c['n_valid'], c['n_cloud_and_valid'], c['n_not_ocean']]
    if browse is not None:
        raw = e['WTR'] if not collapse else ci.expected(scene, False, **kw)['WTR']
        out['browse'] = o.compute_browse_array(raw, collapse, *browse)
    return out


@functools.lru_cache(maxsize=None)
def scene_and_want(dom, h, w, nw, k, collapse, edge=False, seed=0):
    s = ci.scenes(dom, h, w, nw, seed)[k]
    if edge:
        s = ci.with_edge_rows(s)
    return s, want(s, collapse, BROWSE_DEFAULT)


def n_scenes(dom):
    return 4 if dom == 'saturated' else 1


def check_host(ctx, scene, exp, collapse, what, kernel=None):
    bands, fm, masks = ci.planes(scene)
    got = ctx.classify_host(bands, fm, params(collapse), layers=ALL_LAYERS + ('browse',), **masks)
    if kernel is not None:
        assert f'dswx_cover_dilate<{kernel}>' in ctx.last_kernel_info() and 'dswx_cover_finish' in ctx.last_kernel_info(), \
            ctx.last_kernel_info()
    for key in ALL_LAYERS + ('browse',):
        assert got[key].dtype == exp[key].dtype and np.array_equal(got[key], exp[key]), (what, key)
    assert got['counters'][0].tolist() == exp['counters'], what
    return got


# ---- a. domains x kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', list(ci.KERNELS))
@pytest.mark.parametrize('dom', ci.DOMAINS)
def test_domains_on_every_stage2_kernel(stage2, dom, kernel):
    nw = ci.KERNELS[kernel]
    for h, w in ci.KERNEL_SHAPES[nw]:
        for k in range(n_scenes(dom)):
            for collapse in (True, False):
                scene, exp = scene_and_want(dom, h, w, (nw,), k, collapse)
                got = check_host(stage2[kernel], scene, exp, collapse, (dom, kernel, h, w, k, collapse), kernel)
                if dom.startswith('chain17'):
                    assert len(scene['meta']) == 6 * len(ci.CHAIN_HALOS) * sum(len(s) for s in ci.seams(h, w, nw))
                    for p in scene['meta']:
                        # the near pixel (c4: first / last output row or column of a window, +-1) is snow exactly when
                        # the far seed (c21: the outermost halo row or column) is there
                        assert (got['cloud'][p['near']] == ci.SNOW) == p['far_seed'], (kernel, h, w, p)
                        assert got['cloud'][p['cells'][3]] == ci.SNOW and got['cloud'][p['far']] == \
                            (ci.SNOW if p['far_seed'] else ci.CLEAR)


COVER_FIXTURES = [n for n in G.tile_case_names() if '_cover_' in n and any(
    t in n for t in ('chain17', 'walled_corridors', 'bytes256', 'holes'))]
assert len(COVER_FIXTURES) == 5, COVER_FIXTURES


@pytest.mark.parametrize('kernel', list(ci.KERNELS))
@pytest.mark.parametrize('name', COVER_FIXTURES)
def test_reference_made_fixtures_on_every_stage2_kernel(stage2, name, kernel):
    c = G.tile_case(name)
    for collapse in (True, False):
        got = stage2[kernel].classify_host(c['bands'], c['fmask'], params_of_case(c, collapse), land=c['land'],
                                           shad=c['shad'], ocean=c['ocean'])
        assert f'dswx_cover_dilate<{kernel}>' in stage2[kernel].last_kernel_info()
        check_case(got, c, collapse, name)


# ---- b. thin and seam-sized rasters -------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ci.THIN_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_thin_and_seam_sized_rasters(stage2, shape):
    h, w = shape
    for dom in ('diamonds', 'corridors', 'speckle'):
        scene, exp = scene_and_want(dom, h, w, (8, 4), 0, True)
        for kernel in ci.KERNELS:
            check_host(stage2[kernel], scene, exp, True, (dom, kernel, shape), kernel)


# ---- c. entries, strides and addresses ----------------------------------------------------------------------------------
def entry_tiles(h, w, n_tiles, salt=0):
    """Tiles in turn from bytes256, diamonds, holes and speckle, seeds on the first and last row of each."""
    doms = ('bytes256', 'diamonds', 'holes', 'speckle')
    return [scene_and_want(doms[(t + salt) % 4], h, w, (8, 4), 0, True, True, t) for t in range(n_tiles)]


def strided(tiles, stride, dtype, junk):
    """[n_tiles][stride] with the tiles' pixels at the start of each slot and `junk` between them (the last slot ends
    with its tile)."""
    n = tiles[0].size
    out = np.full((len(tiles) - 1) * stride + n, junk, dtype)
    for t, a in enumerate(tiles):
        out[t * stride: t * stride + n] = np.asarray(a, dtype).ravel()
    return out


def device_run(ctx, p, tiles, h, w, extra=0, u8_off=0, i16_off=0, counters=True, entry='batch', layers=ALL_LAYERS,
               masks=True):
    """The scenes `tiles` through dswx_classify_batch (or _2d: extra = 0) with a tile stride of H * W + extra, byte
    planes `u8_off` and int16 planes / DIAG `i16_off` bytes into their allocations, every output between 256-byte guards
    and pre-filled with two sentinels in turn: guards and the pixels between the tiles keep the sentinel, the layers and
    counters are the same both times.  Returns ({layer: [T, h, w]}, counters [T, 3] or None)."""
    n, T = h * w, len(tiles)
    stride = n + extra
    span = (T - 1) * stride + n
    planes = [ci.planes(s) for s, _ in tiles]
    results = []
    with Dev(ctx) as d:
        pin, pout = _capi.PlanesIn(), _capi.PlanesOut()
        for i in range(6):
            pin.band[i] = d.put(strided([b[0][i] for b in planes], stride, np.int16, -9999), i16_off).ptr
        pin.fmask = d.put(strided([b[1] for b in planes], stride, np.uint8, ci.SEED), u8_off).ptr
        if masks:
            for m in ('shad', 'ocean'):
                vals = [b[2].get(m, np.ones((h, w), np.uint8)) for b in planes]
                setattr(pin, m, d.put(strided(vals, stride, np.uint8, 1), u8_off).ptr)
        outs = {k: d.span(span * (2 if k == 'diag' else 1), i16_off if k == 'diag' else u8_off) for k in layers}
        for k, s in outs.items():
            setattr(pout, k, s.ptr)
        cnt = d.span(T * 24) if counters else None
        for sent in SENTINELS:
            for s in list(outs.values()) + ([cnt] if counters else []):
                s.fill(sent)
            if entry == '2d':
                assert extra == 0
                ctx.classify_device_2d(p, T, h, w, pin, pout, counters_ptr=cnt.ptr if counters else None)
            else:
                geom = _capi.BatchGeom(n_tiles=T, height=h, width=w, tile_stride=stride)
                ctx.classify_batch(p, geom, pin, pout, counters_ptr=cnt.ptr if counters else None)
            ctx.synchronize()
            got = {}
            for k, s in outs.items():
                raw = s.get().view(np.uint16 if k == 'diag' else np.uint8)             # (the guards were checked)
                slots = np.full(T * stride, 0, raw.dtype)
                slots[:span] = raw
                slots = slots.reshape(T, stride)
                between = slots[:, n:].ravel()[:(T - 1) * extra]
                assert (between.view(np.uint8) == sent).all(), (k, 'pixels between the tiles were written')
                got[k] = slots[:, :n].reshape(T, h, w).copy()
            results.append((got, cnt.get().view(np.int64).reshape(T, 3).copy() if counters else None))
    (a, ca), (b, cb) = results
    for k in layers:
        assert np.array_equal(a[k], b[k]), (k, 'an output byte kept its sentinel')
    assert counters is False or np.array_equal(ca, cb)
    return a, ca


def check_tiles(got, cnt, tiles, layers, what):
    for t, (_, exp) in enumerate(tiles):
        for k in layers:
            assert np.array_equal(got[k][t], exp[k]), (what, t, k)
        if cnt is not None:
            assert cnt[t].tolist() == exp['counters'], (what, t)


STRIDE_EXTRAS = (0, 1, 4, 5, 8, 37)


@pytest.mark.parametrize('kernel', ['lut', 'direct'])
@pytest.mark.parametrize('shape', ci.ENTRY_SHAPES[:11], ids=lambda s: f'{s[0]}x{s[1]}')
def test_entries_strides_and_addresses(stage1, shape, kernel):
    """Every tile stride H * W + {0, 1, 4, 5, 8, 37} and n_tiles 1 .. 5 at every H * W % 8, byte planes at +1 / +3 and
    int16 planes at +2 (or all aligned), counters present and absent, both entries."""
    h, w = shape
    ctx, p = stage1[kernel], params()
    i, kernel_no = ci.ENTRY_SHAPES.index(shape), ('lut', 'direct').index(kernel)
    for j, extra in enumerate(STRIDE_EXTRAS):
        T = (i + j) % 5 + 1                              # (three rotations of their own: over the shapes every stride
        tiles = entry_tiles(h, w, T, salt=i)             # meets every tile count, offset pair and counter setting)
        u8_off, i16_off = ((1, 2), (3, 2), (0, 0))[(i + 2 * j) % 3]
        counters = (i // 2 + j) % 2 == 0
        entry = '2d' if extra == 0 and (i + kernel_no) % 2 else 'batch'
        got, cnt = device_run(ctx, p, tiles, h, w, extra, u8_off, i16_off, counters, entry)
        info = ctx.last_kernel_info()
        assert 'dswx_cover_dilate<8>' in info and 'dswx_cover_finish' in info, info
        if h * w >= 8:
            assert ('dswx_classify_lut' if kernel == 'lut' else 'dswx_classify_v8') in info, info
        check_tiles(got, cnt, tiles, ALL_LAYERS, (shape, kernel, extra, T, u8_off, entry))


# ---- d. output-plane subsets, the float32 chain, the browse options -----------------------------------------------------
SUBSETS = [('cloud',), ('browse',), ('bwtr', 'conf'), tuple(k for k in ALL_LAYERS + ('browse',) if k != 'wtr'),
           ('wtr', 'diag'), ALL_LAYERS + ('browse',)]


@pytest.mark.parametrize('kernel', ['lut', 'direct'])
@pytest.mark.parametrize('subset', SUBSETS, ids=['+'.join(s) if len(s) < 4 else f'{len(s)} planes' for s in SUBSETS])
def test_output_plane_subsets(stage1, subset, kernel):
    """The finishing kernel anchors its per-tile lead-in on the first plane that is given; three tiles of 97 x 99 at a
    stride of H * W + 5 and of 98 x 100 contiguous, byte planes at +1 and +3."""
    for (h, w), extra, u8_off in (((97, 99), 5, 1), ((98, 100), 0, 3), ((5, 5), 1, 1)):
        tiles = entry_tiles(h, w, 3, salt=len(subset))
        got, cnt = device_run(stage1[kernel], params(), tiles, h, w, extra, u8_off, 2, 'diag' in subset, 'batch', subset)
        check_tiles(got, cnt, tiles, subset, (subset, h, w))


@pytest.mark.parametrize('kernel', ['lut', 'direct'])
def test_float32_chain_in_cover_mode(stage1, kernel):
    """flag_offset_and_scale_inputs: 'cover' stage 1 of the float32 instantiations, on bytes256 and holes."""
    so = [(1.0, 0.0), (0.5, 0.0), (1.0, 0.0), (1.0, 0.0), (0.5, 0.0), (2.0, 1.0)]
    ctx = stage1[kernel]
    for dom, (h, w) in (('bytes256', (160, 112)), ('holes', (250, 250)), ('chain17', (250, 250))):
        scene = ci.scenes(dom, h, w, (8,))[0]
        bands, fm, masks = ci.planes(scene)
        for collapse in (True, False):
            exp = want(scene, collapse, offset_and_scale=so)
            got = ctx.classify_host(bands, fm, params(collapse, offset_and_scale=so), **masks)
            assert 'f32' in ctx.last_kernel_info() and 'dswx_cover_dilate' in ctx.last_kernel_info()
            for key in ALL_LAYERS:
                assert np.array_equal(got[key], exp[key]), (dom, kernel, collapse, key)
            assert got['counters'][0].tolist() == exp['counters']
        plain = ci.expected(scene, False, offset_and_scale=so, mode='ignore')['CLOUD']
        assert not np.array_equal(plain, exp['cloud'])               # the dilations still matter on the float32 chain


def test_all_browse_option_sets_on_bytes256(stage1):
    scene = ci.with_edge_rows(ci.scenes('bytes256', 160, 112, (8, 4))[0])
    scene['ocean'] = (np.arange(160 * 112).reshape(160, 112) % 7 != 0).astype(np.uint8)
    bands, fm, masks = ci.planes(scene)
    raw = ci.expected(scene, False)['WTR']
    assert set(np.unique(raw)) >= {0, 1, 252, 253, 254, 255}
    for bits in range(32):
        excl, nw, cl, sn, oc = [bool(bits >> i & 1) for i in range(5)]
        kw = dict(exclude_psw_aggressive_in_browse=excl, not_water_in_browse='nodata' if nw else 'white',
                  cloud_in_browse='nodata' if cl else 'gray', snow_in_browse='nodata' if sn else 'cyan',
                  set_ocean_masked_to_nodata=oc)
        for collapse in (True, False):
            got = stage1['lut'].classify_host(bands, fm, params(collapse, **kw), layers=('browse', 'cloud'), **masks)
            assert np.array_equal(got['browse'], o.compute_browse_array(raw, collapse, excl, nw, cl, sn, oc)), (bits, collapse)


# ---- e. stale scratch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', list(ci.KERNELS))
def test_launches_do_not_depend_on_stale_scratch(kernel):
    """On a fresh context: all snow and all area at 300 x 300, which leaves every state byte, bitmap and snow bit of the
    scratch set; then, back to back, the same geometry with no snow at all and smaller and differently shaped
    geometries, single and multi-tile, whose bitmaps, slack words and snow planes now lie on top of those set bits."""
    ctx = _capi.Context(0)
    ctx.lab_configure(cover_kernel={'8': 8, '4': 4, '8,direct': 24, '4,direct': 20}[kernel])
    try:
        nw = (ci.KERNELS[kernel],)
        h0, w0 = ci.STALE_SHAPES[0]
        launches = [[scene_and_want('saturated', h0, w0, nw, 0, True)], [scene_and_want('saturated', h0, w0, nw, 1, True)],
                    [scene_and_want('saturated', h0, w0, nw, 0, True)] * 2]
        for i, (h, w) in enumerate(ci.STALE_SHAPES[1:]):
            launches.append([scene_and_want('saturated', h, w, (8, 4), 1, True)])
            launches.append([scene_and_want(('diamonds', 'speckle')[t % 2], h, w, (8, 4), 0, True, True, t)
                             for t in range(1 + i % 3)])
            if i % 2:
                launches.append([scene_and_want('saturated', h0, w0, nw, 0, True)])      # set every bit again
        p = params()
        with Dev(ctx) as d:
            pending = []
            for tiles in launches:
                h, w = tiles[0][0]['fmask'].shape
                n, T = h * w, len(tiles)
                planes = [ci.planes(s) for s, _ in tiles]
                pin, pout = _capi.PlanesIn(), _capi.PlanesOut()
                for b in range(6):
                    pin.band[b] = d.put(np.stack([q[0][b] for q in planes])).ptr
                pin.fmask = d.put(np.stack([q[1] for q in planes])).ptr
                outs = {k: d.span(T * n * (2 if k == 'diag' else 1)) for k in ALL_LAYERS}
                cnt = d.span(T * 24)
                for k, s in list(outs.items()) + [('counters', cnt)]:
                    s.fill(SENTINELS[0])
                    if k != 'counters':
                        setattr(pout, k, s.ptr)
                pending.append((tiles, pin, pout, outs, cnt, h, w))
            for tiles, pin, pout, outs, cnt, h, w in pending:           # back to back: no synchronisation in between
                ctx.classify_device_2d(p, len(tiles), h, w, pin, pout, counters_ptr=cnt.ptr)
            ctx.synchronize()
            assert f'dswx_cover_dilate<{kernel}>' in ctx.last_kernel_info()
            for i, (tiles, pin, pout, outs, cnt, h, w) in enumerate(pending):
                T = len(tiles)
                got = {k: s.get().view(np.uint16 if k == 'diag' else np.uint8).reshape(T, h, w) for k, s in outs.items()}
                check_tiles(got, cnt.get().view(np.int64).reshape(T, 3), tiles, ALL_LAYERS, (kernel, i, h, w))
    finally:
        ctx.close()


# ---- f. more tiles than one chunk ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', ['lut', 'direct'])
@pytest.mark.parametrize('shape', [(3, 3), (4, 6)], ids=['3x3', '4x6'])
def test_more_tiles_than_one_chunk(stage1, shape, kernel):
    """65,537 tiles: the second chunk of the launch loop (65,535 tiles per launch) with its shifted scratch pointers.  The
    tiles repeat 64 distinct ones; every tile of every layer and every counter row is compared."""
    h, w = shape
    n, T, K = h * w, 65537, 64
    base = [scene_and_want('speckle', h, w, (8, 4), 0, True, t % 3 == 0, t) for t in range(K)]
    planes = [ci.planes(s) for s, _ in base]
    which = np.arange(T) % K
    ctx = stage1[kernel]
    with Dev(ctx) as d:
        pin, pout = _capi.PlanesIn(), _capi.PlanesOut()
        for b in range(6):
            pin.band[b] = d.put(np.stack([q[0][b] for q in planes])[which]).ptr
        pin.fmask = d.put(np.stack([q[1] for q in planes])[which]).ptr
        outs = {k: d.span(T * n * (2 if k == 'diag' else 1)) for k in ALL_LAYERS}
        cnt = d.span(T * 24)
        for k, s in outs.items():
            s.fill(SENTINELS[0])
            setattr(pout, k, s.ptr)
        cnt.fill(SENTINELS[1])
        ctx.classify_batch(params(), _capi.BatchGeom(n_tiles=T, height=h, width=w, tile_stride=0), pin, pout,
                           counters_ptr=cnt.ptr)
        ctx.synchronize()
        assert f'grid=(1,1,{T - 65535})' in ctx.last_kernel_info(), ctx.last_kernel_info()
        for k, s in outs.items():
            got = s.get().view(np.uint16 if k == 'diag' else np.uint8).reshape(T, h, w)
            exp = np.stack([e[k] for _, e in base])[which]
            bad = np.flatnonzero((got != exp).reshape(T, -1).any(axis=1))
            assert bad.size == 0, (k, bad[:8].tolist())
        got = cnt.get().view(np.int64).reshape(T, 3)
        assert np.array_equal(got, np.array([e['counters'] for _, e in base], np.int64)[which])
    assert len({e['cloud'].tobytes() for _, e in base}) > 40           # the 64 tiles are distinct
