"""Every aerosol-list bit and every cell of the post-test chain's decision tables, on every kernel that evaluates them.

The chain behind the five tests (aerosol remap, LAND / SHAD rules, cloud / snow, WTR, BWTR, CONF, 'cover' state, browse)
is a finite function; dswx_classify_lut reads it from the tables dswx_build_tables fills (lut1, fm16, land8, chain, pre16,
chainm, extra, extram), dswx_classify_v8 and dswx_classify_v1 evaluate it per pixel.  The aerosol lists reach the pixels
through fm16 (table-driven), a ds_bpermute of a lane register (direct) and an LDS copy (generic).  The tile of
oracle/chain_inputs.py holds every cell once -- tests/test_chain_domain.py shows on the CPU that every reachable cell of
pre16, chainm, extram and of the joint key is there and that every one of the 1,024 list bits decides a pixel -- and is
run here under the parameter sets S0 .. S8 of chain_inputs.SETS on every kernel form, through every entry, and four times
back to back with lists that differ in one bit (the table cache of a context).

Everything is bit for bit against the scalar C oracle (the numpy oracle in 'cover' mode): the eight layers, the browse
plane where produced, and the three counters (on the device entries written over a sentinel)."""
import ctypes
import functools

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py):
    import torch                                  # noqa: F401 -- loaded second, torch finds no device, and this file must pass on its own too
except ImportError:
    pass

from oracle import chain_inputs as ch
from proteus_amd import _capi

pytestmark = pytest.mark.gpu

ALL_LAYERS = ('diag', 'wtr1', 'wtr1_aerosol', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud')
MASK_PLANES = ('land', 'shad', 'ocean')
SENTINEL = -7


@pytest.fixture(scope='module')
def ctxs():
    """The automatic choice (table-driven, counters folded), the direct kernel (fused_variant = 0), the separate counters
    kernel (tune_fold = 0) and the staged host pipeline."""
    made = {'lut': _capi.Context(0)}
    for name, settings in (('direct', dict(fused_variant=0)), ('nofold', dict(tune_fold=0)),
                           ('staged', dict(host_pipeline=1, host_chunks=3))):
        made[name] = _capi.Context(0)
        made[name].lab_configure(**settings)
    yield made
    for c in made.values():
        c.close()


@functools.lru_cache(maxsize=8)
def expected(name, variant, collapse, masks=True):
    """The oracle's answer, once per (set, tile variant, collapse, with or without the mask planes)."""
    return ch.c_expected(name, ch.tile_of(name, variant), collapse, masks)


def check(got, exp, layers, what):
    for k in layers:
        g = np.asarray(got[k])
        assert g.dtype == exp[k].dtype and np.array_equal(g.reshape(exp[k].shape), exp[k]), (what, k)
    assert np.asarray(got['counters']).reshape(-1, 3).sum(axis=0).tolist() == list(exp['counters']), what


# ---- 1. every set on every kernel form ------------------------------------------------------------------------------------
# form -> (context, tile variant, mask planes, browse plane)
FORMS = {
    'lut plain': ('lut', 'full', False, False), 'lut masks': ('lut', 'full', True, False),
    'lut browse plain': ('lut', 'full', False, True), 'lut browse masks': ('lut', 'full', True, True),
    'lut masks unfolded': ('nofold', 'full', True, False),
    'direct plain': ('direct', 'full', False, False), 'direct masks': ('direct', 'full', True, False),
    'direct browse masks': ('direct', 'full', True, True),
    'generic': ('lut', 'reduced', True, True),
    'lut tail': ('lut', 'tail', True, False), 'direct tail': ('direct', 'tail', True, False),
}
COVER_FORMS = {'cover lut': ('lut', 'full', True, True), 'cover lut plain': ('lut', 'full', False, True),
               'cover direct': ('direct', 'full', True, True)}
CASES = [(name, form) for name in ch.SETS for form in (COVER_FORMS if name == 'S7' else FORMS)]


def kernel_name(ctx_key, variant, masks, extras, f32):
    """What last_kernel_info() says of the kernel that did the whole 8-pixel groups."""
    if variant == 'reduced':
        return 'dswx_classify_v1 '
    m, f = 'true' if masks else 'false', ',f32' if f32 else ''
    if ctx_key == 'direct':
        return f"dswx_classify_v8<{m},{'true' if extras else 'false'}{f}>"
    return f"dswx_classify_lut<{m}{',extras' if extras else ''}{f}>"


@pytest.mark.parametrize('name, form', CASES, ids=[f'{n}-{f.replace(" ", "_")}' for n, f in CASES])
def test_sets_on_every_kernel_form(ctxs, name, form):
    cover = name == 'S7'
    ctx_key, variant, masks, browse = (COVER_FORMS if cover else FORMS)[form]
    ctx = ctxs[ctx_key]
    tile = ch.tile_of(name, variant)
    layers = ALL_LAYERS + (('browse',) if browse else ())
    for collapse in (True, False):
        p = ch.params_of(name, collapse)
        exp = expected(name, variant, collapse, masks)
        got = ctx.classify_host(tile['bands'], tile['fmask'], p, layers=layers, **(ch.masks_of(tile) if masks else {}))
        info = ctx.last_kernel_info()
        assert kernel_name(ctx_key, variant, masks, browse or cover, 'offset_and_scale' in ch.SETS[name]['kw']) in info, info
        assert ('dswx_cover_dilate' in info and 'dswx_cover_finish' in info) == cover, info
        if variant == 'reduced':
            assert 'lut' not in info and 'v8' not in info, info
        elif ctx_key != 'direct':
            assert ('counters folded' in info) == (ctx_key == 'lut'), info
        check(got, exp, layers, (name, form, collapse))
        if variant == 'tail':
            # n % 8 == 5: the last five pixels belong to no 8-pixel group and go through dswx_classify_v1, which the info
            # string of a one-tile launch does not name (it names the kernel of the groups); they carry cells too
            assert tile['fmask'].size % 8 == 5
            for k in layers:
                assert np.array_equal(got[k].ravel()[-5:], exp[k].ravel()[-5:]), (name, form, collapse, k, 'tail pixels')
        if variant == 'reduced':            # a tile per seven pixels: the counters of every 97th tile as well
            from oracle import c_oracle
            assert got['counters'].shape == (tile['fmask'].shape[0], 3)
            want = [c_oracle.classify(p, [b[t] for b in tile['bands']], tile['fmask'][t],
                                      **{m: tile[m][t] for m in MASK_PLANES})['counters'].tolist()
                    for t in range(0, tile['fmask'].shape[0], 97)]
            assert got['counters'][::97].tolist() == want


# ---- 2. the entries -------------------------------------------------------------------------------------------------------
class Arena:
    """`copies` of a tile's planes, tile after tile, in one device allocation: int16 planes `band_off` bytes and byte planes
    `u8_off` bytes past a 256-byte boundary, and `out_sets` sets of output planes (browse included) and counters."""

    def __init__(self, ctx, tile, copies=1, band_off=0, u8_off=0, out_sets=1):
        self.ctx, self.t, self.n = ctx, copies, tile['fmask'].size
        self.size = size = self.n * copies
        self.buf = ctx.malloc(size * (16 + 11 * out_sets) + 512 * (12 + 12 * out_sets))
        self.off = 0
        self.pin = _capi.PlanesIn()
        rep = lambda a: np.concatenate([np.ascontiguousarray(a).ravel()] * copies)
        for i in range(6):
            self.pin.band[i] = self.buf.ptr + self._place(2 * size, band_off, rep(tile['bands'][i]))
        for name in ('fmask',) + MASK_PLANES:
            setattr(self.pin, name, self.buf.ptr + self._place(size, u8_off, rep(tile[name])))
        self.sets = []
        for _ in range(out_sets):
            pout, where = _capi.PlanesOut(), {}
            for name in ALL_LAYERS + ('browse',):
                where[name] = self._place(size * (2 if name == 'diag' else 1), band_off if name == 'diag' else u8_off)
                setattr(pout, name, self.buf.ptr + where[name])
            where['counters'] = self._place(24 * copies, 0)
            self.sets.append((pout, where))
        assert self.off <= self.buf.nbytes
        self.reset()

    def _place(self, nbytes, align_off, data=None):
        at = (self.off + 255) // 256 * 256 + align_off
        if data is not None:
            self.buf.upload(data, at)
        self.off = at + nbytes + 1
        return at

    def reset(self):
        """Every output plane to 0xEE bytes, every counter to the sentinel."""
        first = min(w['diag'] for _, w in self.sets)
        _capi._check(self.ctx.lib.dswx_memset_d(self.ctx.handle, ctypes.c_void_p(self.buf.ptr + first), 0xEE, self.off - first))
        for _, w in self.sets:
            self.buf.upload(np.full(3 * self.t, SENTINEL, np.int64), w['counters'])

    def launch(self, p, k=0, entry='device', stream=None):
        pout, w = self.sets[k]
        if entry == 'batch':
            self.ctx.classify_batch(p, _capi.BatchGeom(self.t, 1, self.n, self.n), self.pin, pout,
                                    self.buf.ptr + w['counters'], stream)
        else:
            self.ctx.classify_device(p, self.t, self.n, self.pin, pout, self.buf.ptr + w['counters'], stream)

    def read(self, k=0):
        _, w = self.sets[k]
        got = {name: self.buf.download(np.uint16 if name == 'diag' else np.uint8, self.size, w[name]).reshape(self.t, self.n)
               for name in ALL_LAYERS + ('browse',)}
        got['counters'] = self.buf.download(np.int64, 3 * self.t, w['counters']).reshape(self.t, 3)
        return got

    def free(self):
        self.buf.free()


def check_tiles(got, exp, what):
    """Every tile of an Arena's output (copies of one tile) against the expectation of that tile."""
    for t in range(got['counters'].shape[0]):
        for k in ALL_LAYERS + ('browse',):
            assert np.array_equal(got[k][t], exp[k].ravel()), (what, t, k)
        assert got['counters'][t].tolist() == list(exp['counters']), (what, t)


def _pinned(c, a):
    q = c.pinned_empty(a.shape, a.dtype)
    q[...] = a
    return q


@pytest.mark.parametrize('entry', ['device odd addresses', 'batch of three', 'DeviceBatch', 'staged host'])
@pytest.mark.parametrize('name', ['S1', 'S3'])
def test_sets_through_every_entry(ctxs, name, entry):
    ctx = ctxs['staged' if entry == 'staged host' else 'lut']
    layers = ALL_LAYERS + ('browse',)
    for collapse in (True, False):
        p = ch.params_of(name, collapse)
        if entry == 'device odd addresses':
            # dswx_classify_device, one tile, the int16 planes (DIAG too) at 2 bytes and the byte planes at 1 byte past a
            # 256-byte boundary: no plane aligned to its vector access
            tile, exp = ch.tile_of(name), expected(name, 'full', collapse)
            a = Arena(ctx, tile, band_off=2, u8_off=1)
            try:
                a.launch(p)
                ctx.synchronize()
                assert 'dswx_classify_lut<true,extras>' in ctx.last_kernel_info(), ctx.last_kernel_info()
                check_tiles(a.read(), exp, (name, entry, collapse))
            finally:
                a.free()
        elif entry == 'batch of three':
            # dswx_classify_batch, three copies of the reduced tile as one row each at a contiguous stride (n % 8 != 0)
            tile, exp = ch.tile_of(name, 'reduced'), expected(name, 'reduced', collapse)
            assert tile['fmask'].size % 8 != 0
            a = Arena(ctx, tile, copies=3)
            try:
                a.launch(p, entry='batch')
                ctx.synchronize()
                info = ctx.last_kernel_info()
                assert 'dswx_classify_lut<true,extras>' in info and 'ragged tiles: edges by dswx_classify_v1' in info, info
                check_tiles(a.read(), exp, (name, entry, collapse))
            finally:
                a.free()
        elif entry == 'DeviceBatch':
            tile, exp = ch.tile_of(name), expected(name, 'full', collapse)
            h, w = tile['fmask'].shape
            b = _capi.DeviceBatch(ctx, 1, h, w, masks=True, extra_layers=('wtr1_aerosol', 'browse'))
            try:
                for i, band in enumerate(_capi.BAND_NAMES):
                    b.write_tile(band, 0, tile['bands'][i])
                for m in ('fmask',) + MASK_PLANES:
                    b.write_tile(m, 0, tile[m])
                b.write_counters_sentinel(SENTINEL)
                b.classify(p)
                ctx.synchronize()
                assert 'dswx_classify_lut<true,extras>' in ctx.last_kernel_info(), ctx.last_kernel_info()
                for k in layers:
                    assert np.array_equal(b.read_tile(k, 0), exp[k]), (name, entry, collapse, k)
                assert b.read_counters()[0].tolist() == list(exp['counters'])
            finally:
                b.free()
        else:
            tile, exp = ch.tile_of(name), expected(name, 'full', collapse)
            got = ctx.classify_host([_pinned(ctx, x) for x in tile['bands']], _pinned(ctx, tile['fmask']), p, layers=layers,
                                    **{m: _pinned(ctx, tile[m]) for m in MASK_PLANES})
            assert 'pipelined over 3 streams' in ctx.last_kernel_info(), ctx.last_kernel_info()
            check(got, exp, layers, (name, entry, collapse))


# ---- 3. the table cache of a context --------------------------------------------------------------------------------------
FLIP_ROW, FLIP_BYTE = 2, 16            # class 3, the Fmask byte "snow and nothing else"


@functools.lru_cache(maxsize=1)
def _cache_runs():
    """Four (params, expectation) on the S1 tile: lists L = hashed(7), L with one bit flipped, L again, remapping off."""
    tile = ch.tile_of('S1')
    L = ch.hashed(7)
    flipped = ch.one_bit_flipped(L, FLIP_ROW, FLIP_BYTE)
    runs = []
    for lists, over in ((L, {}), (flipped, {}), (L, {}), (L, dict(apply_aerosol_class_remapping=False))):
        runs.append((ch.params_of('S1', True, lists, **over), ch.c_expected('S1', tile, True, True, lists, **over)))
    differ = lambda a, b: sum(int((a[k] != b[k]).sum()) for k in ALL_LAYERS + ('browse',))
    assert differ(runs[0][1], runs[1][1]) > 0 and differ(runs[2][1], runs[3][1]) > 0
    assert (runs[0][1]['cloud'] != runs[1][1]['cloud']).sum() == (runs[0][1]['wtr1_aerosol'] != runs[1][1]['wtr1_aerosol']).sum() > 0
    return runs


def test_table_cache_notices_one_list_bit_and_the_stream(ctxs):
    """The tables of a context are rebuilt when a memcmp of the device parameters, or the stream, says so.  On ONE context,
    nine launches with no synchronisation anywhere in between, each into output planes of its own and each with its own
    expectation.  On the context's stream: lists L, L with ONE bit flipped (class 3, a snow byte), L again, remapping off.
    Then on a caller's second stream: remapping off once more -- the parameters the cache holds, so that the stream is
    all that differs from the cached state while the first stream's work may still be running -- and the same four again.
    A cache that missed the bit gives the neighbouring launch's layers; the test does not claim to provoke a race between
    the streams, only that the results are right when the launches are issued this way."""
    torch = pytest.importorskip('torch')
    ctx = ctxs['lut']
    runs = _cache_runs()
    a = Arena(ctx, ch.tile_of('S1'), out_sets=9)
    try:
        caller = torch.cuda.Stream(device=0)
        plan = [(k, None) for k in range(4)] + [(3, caller.cuda_stream)] + [(k, caller.cuda_stream) for k in range(4)]
        for slot, (k, stream) in enumerate(plan):
            a.launch(runs[k][0], slot, stream=stream)
            assert 'dswx_classify_lut<true,extras>' in ctx.last_kernel_info(), ctx.last_kernel_info()
        ctx.synchronize()
        ctx.synchronize(caller.cuda_stream)
        for slot, (k, stream) in enumerate(plan):
            check_tiles(a.read(slot), runs[k][1], ('own stream' if stream is None else "caller's stream", slot, k))
    finally:
        a.free()
