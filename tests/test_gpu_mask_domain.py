"""The LAND / SHAD / OCEAN planes over the whole byte range, on every path that reads them or computes the counters.

The reference gives meaning to the whole byte of these uint8 planes: SHAD masks where it is 0 (dswx_hls.py:1333-1340),
OCEAN is ocean where it is 0 (:5245) but n_not_ocean = np.sum(ocean_mask) sums the byte VALUES (:5105), LAND is a
0..255 code.  synth_tile draws SHAD and OCEAN from {0, 1} only, so the rest of the suite never sees a byte above 1 in
those planes.  Here the planes of a synthetic tile are rewritten into other domains ({0, 255}, 0..255, all 255, all 0,
0..4) and every layer and the three counters of each path are compared with the scalar C oracle (the numpy oracle in
'cover' mode), the counters after a sentinel, so that a counter that was never written fails too."""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from oracle import dswx_oracle as o
from proteus_amd import _capi
from proteus_amd.synth import synth_tile, SEED

ALL_LAYERS = ('diag', 'wtr1', 'wtr1_aerosol', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud')
MASK_PLANES = ('land', 'shad', 'ocean')
SENTINEL = -7


def in_domain(plane, domain, rng):
    """A LAND / SHAD / OCEAN plane of synth_tile rewritten into a byte domain.  The recipe's zeros (shadow, ocean) stay
    zero where the domain has a zero, so the masking rules keep firing; the other pixels take the domain's values."""
    keep = plane != 0
    if domain == 'recipe':
        out = plane
    elif domain == '0/255':
        out = np.where(keep, 255, 0)
    elif domain == '0..255':
        out = np.where(keep, rng.integers(0, 256, size=plane.shape), 0)
    elif domain == '0..4':
        out = np.where(keep, rng.integers(1, 5, size=plane.shape), 0)
    elif domain == 'all 255':
        out = np.full(plane.shape, 255)
    elif domain == 'all 0':
        out = np.zeros(plane.shape)
    else:
        raise ValueError(domain)
    return np.ascontiguousarray(out, dtype=np.uint8)


def with_mask_domains(s, land='recipe', shad='recipe', ocean='recipe', seed=0):
    """A copy of synth_tile(..., with_masks=True) whose mask planes are in the given domains (test-only: synth.py's
    recipe, which the device generator matches bit for bit, stays as it is)."""
    rng = np.random.default_rng(seed)
    out = dict(s)
    for name, dom in (('land', land), ('shad', shad), ('ocean', ocean)):
        out[name] = in_domain(s[name], dom, rng)
    return out


# every domain of the issue at least once per plane; the first row is the recipe itself (the control)
DOMAINS = [
    dict(),
    dict(ocean='0/255', shad='0/255', land='0..255'),
    dict(ocean='0..255', shad='0..255', land='0..255'),
    dict(ocean='all 255', shad='0/255'),
    dict(ocean='all 0', shad='0..255'),
    dict(ocean='0..4', land='0..255'),
]
DOMAIN_IDS = ['-'.join(f'{k}={v}' for k, v in sorted(d.items())).replace(' ', '') or 'recipe' for d in DOMAINS]


@functools.lru_cache(maxsize=64)
def _recipe_tile(tile, h, w):
    return synth_tile(tile, h, w, with_masks=True)


def tile_in(dom, tile, h, w):
    return with_mask_domains(_recipe_tile(tile, h, w), seed=tile, **DOMAINS[dom])


def masks_of(s):
    return {m: s[m] for m in MASK_PLANES}


def check(got, exp, layers, what):
    for k in layers:
        assert np.array_equal(np.asarray(got[k]).reshape(exp[k].shape), exp[k]), (what, k)
    assert np.asarray(got['counters']).reshape(-1, 3)[0].tolist() == exp['counters'].tolist(), what


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def lab_ctx():
    """Contexts with a lab switch each: the staged host pipeline, the fold off, the direct kernel."""
    made = {}
    for name, settings in (('staged', dict(host_pipeline=1, host_chunks=3)), ('nofold', dict(tune_fold=0)),
                           ('direct', dict(fused_variant=0))):
        made[name] = _capi.Context(0)
        made[name].lab_configure(**settings)
    yield made
    for c in made.values():
        c.close()


def _pinned(c, a):
    q = c.pinned_empty(a.shape, a.dtype)
    q[...] = a
    return q


@pytest.mark.gpu
@pytest.mark.parametrize('dom', range(len(DOMAINS)), ids=DOMAIN_IDS)
@pytest.mark.parametrize('shape', [(400, 700), (37, 53)])
def test_classify_host_paths(ctx, lab_ctx, shape, dom):
    """dswx_classify_host from pageable arrays, from page-locked ones (zero copy) and through the staged pipeline in
    three pieces per tile: one tile, so the counters are folded into the table-driven kernel."""
    h, w = shape
    s = tile_in(dom, 900 + h, h, w)
    p = _capi.default_params()
    exp = c_oracle.classify(p, s['bands'], s['fmask'], **masks_of(s))
    check(ctx.classify_host(s['bands'], s['fmask'], p, **masks_of(s)), exp, ALL_LAYERS, 'pageable')
    for name, c, tag in (('zero copy', ctx, 'zero copy across PCIe'), ('staged', lab_ctx['staged'], 'pipelined over 3 streams')):
        got = c.classify_host([_pinned(c, b) for b in s['bands']], _pinned(c, s['fmask']), p,
                              **{m: _pinned(c, v) for m, v in masks_of(s).items()})
        assert tag in c.last_kernel_info(), c.last_kernel_info()
        check(got, exp, ALL_LAYERS, name)


@pytest.mark.gpu
@pytest.mark.parametrize('dom', range(len(DOMAINS)), ids=DOMAIN_IDS)
@pytest.mark.parametrize('align, shape', [(256, (400, 700)), (1, (37, 53)), (1, (301, 263))])
def test_device_batch_walks(ctx, align, shape, dom):
    """DeviceBatch.classify over 17 resident tiles walked at 17 (separate counters kernel), 16 and 1 (folded) and 5
    tiles, padded tiles and contiguous ragged ones (H * W % 8 != 0: the generic kernel does every tile's edges)."""
    n, (h, w) = 17, shape
    b = _capi.DeviceBatch(ctx, n, h, w, masks=True, extra_layers=('wtr1_aerosol',), tile_align=align)
    try:
        b.synth(SEED, tile0=600)
        p = _capi.default_params()
        exp = []
        for t in range(n):
            st = tile_in(dom, 600 + t, h, w)
            for m in MASK_PLANES:
                b.write_tile(m, t, st[m])
            exp.append(c_oracle.classify(p, st['bands'], st['fmask'], **masks_of(st)))
        for k in (17, 16, 1, 5):
            b.write_counters_sentinel(SENTINEL)
            b.classify(p, n_tiles=k)
            assert ('counters folded' in ctx.last_kernel_info()) == (k <= 16), (k, ctx.last_kernel_info())
            if align == 1 and k > 1:
                assert 'ragged tiles' in ctx.last_kernel_info()
            ctx.synchronize()
            cnt = b.read_counters()
            for t in range(k):
                assert cnt[t].tolist() == exp[t]['counters'].tolist(), (k, t)
            assert (cnt[k:] == SENTINEL).all(), k
            if k in (17, 1):
                for t in (range(n) if k == 17 else (0,)):
                    for key in ALL_LAYERS:
                        assert np.array_equal(b.read_tile(key, t), exp[t][key]), (k, t, key)
    finally:
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize('dom', range(len(DOMAINS)), ids=DOMAIN_IDS)
@pytest.mark.parametrize('switch', ['nofold', 'direct'])
def test_lab_switches(lab_ctx, switch, dom):
    """tune_fold = 0 (the separate counters kernel on small launches too) and fused_variant = 0 (dswx_classify_v8)."""
    c = lab_ctx[switch]
    n, h, w = 3, 400, 700
    b = _capi.DeviceBatch(c, n, h, w, masks=True, extra_layers=('wtr1_aerosol',))
    try:
        b.synth(SEED, tile0=700)
        p = _capi.default_params()
        exp = []
        for t in range(n):
            st = tile_in(dom, 700 + t, h, w)
            for m in MASK_PLANES:
                b.write_tile(m, t, st[m])
            exp.append(c_oracle.classify(p, st['bands'], st['fmask'], **masks_of(st)))
        b.write_counters_sentinel(SENTINEL)
        b.classify(p)
        info = c.last_kernel_info()
        assert 'counters folded' not in info, info
        if switch == 'direct':
            assert 'dswx_classify_v8' in info, info
        c.synchronize()
        cnt = b.read_counters()
        for t in range(n):
            assert cnt[t].tolist() == exp[t]['counters'].tolist(), t
            for key in ALL_LAYERS:
                assert np.array_equal(b.read_tile(key, t), exp[t][key]), (t, key)
        st = tile_in(dom, 700, h, w)
        check(c.classify_host(st['bands'], st['fmask'], p, **masks_of(st)), exp[0], ALL_LAYERS, 'host')
    finally:
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize('dom', range(len(DOMAINS)), ids=DOMAIN_IDS)
def test_float32_chain_browse_and_cover(ctx, dom):
    """The other instantiations of the table-driven kernel: the float32 chain (offset_and_scale), the browse plane and
    'cover' stage 1 (EXTRAS: fold groups of 16 blocks of 8192 pixels), on one tile (folded) and on a batch of two."""
    h, w = 400, 700
    s = tile_in(dom, 800, h, w)
    f32 = _capi.make_params(offset_and_scale=[(1e-4, 0.0)] * 6)
    exp = c_oracle.classify(f32, s['bands'], s['fmask'], **masks_of(s))
    check(ctx.classify_host(s['bands'], s['fmask'], f32, **masks_of(s)), exp, ALL_LAYERS, 'float32')
    assert 'f32' in ctx.last_kernel_info() and 'counters folded' in ctx.last_kernel_info(), ctx.last_kernel_info()
    p = _capi.default_params()
    layers = ALL_LAYERS + ('browse',)
    exp = c_oracle.classify(p, s['bands'], s['fmask'], layers=layers, **masks_of(s))
    check(ctx.classify_host(s['bands'], s['fmask'], p, layers=layers, **masks_of(s)), exp, layers, 'browse')
    assert 'extras' in ctx.last_kernel_info() and 'counters folded' in ctx.last_kernel_info(), ctx.last_kernel_info()
    pc = _capi.make_params(mask_adjacent_to_cloud_mode='cover')
    got = ctx.classify_host(s['bands'], s['fmask'], pc, **masks_of(s))
    with np.errstate(all='ignore'):
        e = o.classify_tile(s['bands'], s['fmask'], landcover=s['land'], shadow=s['shad'], ocean_mask=s['ocean'],
                            mask_adjacent_to_cloud_mode='cover')
    for key, layer in (('diag', 'DIAG'), ('wtr1', 'WTR-1'), ('wtr2', 'WTR-2'), ('wtr', 'WTR'), ('bwtr', 'BWTR'),
                       ('conf', 'CONF'), ('cloud', 'CLOUD')):
        want = e[layer + '.collapsed'] if layer + '.collapsed' in e else e[layer]
        assert np.array_equal(got[key], want), ('cover', key)
    c = e['counters']
    assert got['counters'][0].tolist() == [c['n_valid'], c['n_cloud_and_valid'], c['n_not_ocean']]
    # the same three parameter sets on a batch of two tiles
    n = 2
    b = _capi.DeviceBatch(ctx, n, h, w, masks=True, extra_layers=('wtr1_aerosol', 'browse'))
    try:
        b.synth(SEED, tile0=800)
        tiles = [tile_in(dom, 800 + t, h, w) for t in range(n)]
        for t, st in enumerate(tiles):
            for m in MASK_PLANES:
                b.write_tile(m, t, st[m])
        for params, what in ((f32, 'float32'), (p, 'browse')):
            b.write_counters_sentinel(SENTINEL)
            b.classify(params)
            assert 'counters folded' in ctx.last_kernel_info(), ctx.last_kernel_info()
            ctx.synchronize()
            cnt = b.read_counters()
            for t, st in enumerate(tiles):
                ex = c_oracle.classify(params, st['bands'], st['fmask'], layers=layers, **masks_of(st))
                assert cnt[t].tolist() == ex['counters'].tolist(), (what, t)
                for key in layers:
                    assert np.array_equal(b.read_tile(key, t), ex[key]), (what, t, key)
        b.write_counters_sentinel(SENTINEL)
        b.classify(pc)
        ctx.synchronize()
        cnt = b.read_counters()
        for t, st in enumerate(tiles):
            with np.errstate(all='ignore'):
                e = o.classify_tile(st['bands'], st['fmask'], landcover=st['land'], shadow=st['shad'],
                                    ocean_mask=st['ocean'], mask_adjacent_to_cloud_mode='cover')['counters']
            assert cnt[t].tolist() == [e['n_valid'], e['n_cloud_and_valid'], e['n_not_ocean']], ('cover', t)
    finally:
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize('dom', range(len(DOMAINS)), ids=DOMAIN_IDS)
def test_tile_engine_resident_masks(ctx, dom):
    """pipeline.TileEngine.classify (the product path) with the three mask planes resident as DevicePlanes."""
    from proteus_amd import pipeline
    h, w = 400, 700
    s = tile_in(dom, 850, h, w)
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


@pytest.mark.gpu
def test_largest_folded_tile_with_ocean_all_255(ctx):
    """4096 x 4095: the largest tile whose counters are folded (n_pixels < 2^24), every OCEAN byte 255, so that
    n_not_ocean = 4,277,145,600 > 2^31 -- a signed 32-bit truncation anywhere shows.  Plain outputs and with the browse plane
    (EXTRAS fold groups)."""
    h, w = 4096, 4095
    n_px = h * w
    assert n_px < 1 << 24 and 255 * n_px > 1 << 31
    p = _capi.default_params()
    layers = ALL_LAYERS + ('browse',)
    exp = None
    for extra in (('wtr1_aerosol',), ('wtr1_aerosol', 'browse')):
        b = _capi.DeviceBatch(ctx, 1, h, w, masks=True, extra_layers=extra)
        try:
            b.synth(SEED, tile0=77)
            b.write_tile('ocean', 0, np.full((h, w), 255, np.uint8))
            if exp is None:
                host = {k: b.read_tile(k, 0) for k in _capi.BAND_NAMES + ('fmask', 'land', 'shad')}
                exp = c_oracle.classify(p, [host[k] for k in _capi.BAND_NAMES], host['fmask'], land=host['land'],
                                        shad=host['shad'], ocean=np.full((h, w), 255, np.uint8), layers=layers)
                assert exp['counters'][2] == 255 * n_px
            b.write_counters_sentinel(SENTINEL)
            b.classify(p)
            assert 'counters folded' in ctx.last_kernel_info(), ctx.last_kernel_info()
            ctx.synchronize()
            assert b.read_counters()[0].tolist() == exp['counters'].tolist(), extra
            for key in ALL_LAYERS + (('browse',) if 'browse' in extra else ()):
                assert np.array_equal(b.read_tile(key, 0), exp[key]), (extra, key)
        finally:
            b.free()


@pytest.mark.gpu
def test_wide_ocean_launch_leaves_the_next_launch_clean(ctx):
    """A launch with a {0, 255} OCEAN plane, then -- on the same context, no synchronisation in between -- a launch with
    the recipe's {0, 1} plane of the same shape: both fold their counters through the context's accumulators, and the
    second launch's counters must be the oracle's (an accumulator left dirty by the first would corrupt them)."""
    h, w = 400, 700
    p = _capi.default_params()
    wide = _capi.DeviceBatch(ctx, 1, h, w, masks=True)
    plain = _capi.DeviceBatch(ctx, 1, h, w, masks=True)
    try:
        wide.synth(SEED, tile0=950)
        plain.synth(SEED, tile0=951)
        sw = with_mask_domains(_recipe_tile(950, h, w), ocean='0/255', seed=950)
        wide.write_tile('ocean', 0, sw['ocean'])
        sp = _recipe_tile(951, h, w)
        ew = c_oracle.classify(p, sw['bands'], sw['fmask'], **masks_of(sw))['counters'].tolist()
        ep = c_oracle.classify(p, sp['bands'], sp['fmask'], **masks_of(sp))['counters'].tolist()
        assert ew[2] > 1 << 19 and ep[2] < 1 << 19
        for rounds in (1, 3):
            wide.write_counters_sentinel(SENTINEL)
            plain.write_counters_sentinel(SENTINEL)
            for _ in range(rounds):
                wide.classify(p)
                assert 'counters folded' in ctx.last_kernel_info()
                plain.classify(p)
            ctx.synchronize()
            assert plain.read_counters()[0].tolist() == ep, rounds
            assert wide.read_counters()[0].tolist() == ew, rounds
    finally:
        wide.free()
        plain.free()
