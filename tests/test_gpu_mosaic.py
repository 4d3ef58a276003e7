"""The mosaic entries on the GPU: dswx_mosaic_device and dswx_batch_mosaic byte for byte against the library's scalar statement
(dswx_mosaic_host; tests/test_mosaic.py pins that to numpy and to two further statements) -- placements in all 16 residues
of a unit, tile and canvas widths either side of a unit and of a block's rectangle, canvas heights either side of its rows,
tile edges that cut a unit on either side and on both, plane addresses and strides, with every byte outside the output planes
checked and a plane buffer full of a padding byte that IS an observation; tile counts either side of a round of loads and of
the list of surviving tiles; 65535 random placements; contents chosen against the packed accumulators; every subset of
outputs; the identity placement against dswx_stack_device; on a caller's stream behind the kernel that writes the plane; the
batch forms; mosaic then label across a seam; DevicePlane.mosaic; bin/dswx_mosaic.py; the C example."""
import importlib.util
import json
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py)
    import torch
except ImportError:
    torch = None

from proteus_amd import _capi, geotiff
from proteus_amd.label import wtr_label_spec
from proteus_amd.mosaic import Spec, layout, mosaic_tiles, wtr_mosaic_spec
from proteus_amd.stack import NONE, NO_SHARE
from proteus_amd import stack as stack_mod
from proteus_amd.synth import SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, C, L, U, PPT = _capi.MOSAIC_RECT_H, _capi.MOSAIC_RECT_W, _capi.MOSAIC_LIST, _capi.MOSAIC_ROUND, 16
PAD = 0xA5                                        # every byte of a plane buffer that is not tile data; the specs below COUNT it
SENT = 0xEE                                       # every byte of an output buffer beforehand
KEYS = ('count', 'last', 'last_index', 'share')
GUARD = 512


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def random_spec(rng, n_cats):
    """Categories 0 .. 5 at random (4 and 5 are never observations); the padding byte is an observation of category 0."""
    cat = rng.integers(0, 6, size=256).astype(np.uint8)
    cat[PAD] = 0
    return Spec(n_cats, cat, int(rng.integers(0, 256)), int(rng.integers(0, 256)))


class Run:
    """One call of dswx_mosaic_device.  The plane lies guard | `off` bytes past a 256-byte boundary | guard in `sbuf`, every
    byte that is not tile data PAD (the last tile's padding does not exist); the table lies in `pbuf`; the wanted outputs lie
    in `obuf`, the uint16 planes 2 bytes and the byte planes 1 byte past a 16-byte boundary, every byte SENT beforehand."""

    def __init__(self, ctx, tiles, place, canvas, spec, stride=None, off=0, want=KEYS, sbuf=None, obuf=None, pbuf=None):
        self.ctx, self.spec, self.want, self.canvas = ctx, spec, want, canvas
        self.tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
        self.T, self.H, self.W = self.tiles.shape
        self.place = np.ascontiguousarray(place, dtype=np.int32).reshape(self.T, 2)
        n = self.H * self.W
        self.stride = n if stride is None else stride
        span = (self.T - 1) * self.stride + n if self.T else 0
        self.start = GUARD + off
        self.shost = np.full(self.start + span + GUARD, PAD, dtype=np.uint8)
        for t in range(self.T):
            self.shost[self.start + t * self.stride:self.start + t * self.stride + n] = self.tiles[t].reshape(-1)
        self.own = []
        self.sbuf = sbuf if sbuf is not None else self._malloc(self.shost.size)
        assert self.sbuf.nbytes >= self.shost.size and self.sbuf.ptr % 256 == 0
        self.sbuf.upload(self.shost)
        self.pbuf = pbuf if pbuf is not None else self._malloc(max(self.T, 1) * 8)
        assert self.pbuf.nbytes >= self.T * 8
        if self.T:
            self.pbuf.upload(self.place.view(np.uint8).reshape(-1))
        m = canvas[0] * canvas[1]
        self.m, self.where, cursor = m, {}, 0
        for key, eb, planes in (('count', 2, spec.n_cats), ('last_index', 2, 1), ('last', 1, 1), ('share', 1, 1)):
            for k in range(planes):
                begin = -(-cursor // 16) * 16 + eb
                self.where[(key, k)] = (begin, eb)
                cursor = begin + m * eb + 16
        self.osize = cursor + 16
        self.obuf = obuf if obuf is not None else self._malloc(self.osize)
        assert self.obuf.nbytes >= self.osize and self.obuf.ptr % 16 == 0
        self.obuf.upload(np.full(self.osize, SENT, dtype=np.uint8))
        at = lambda key, k=0: self.obuf.ptr + self.where[(key, k)][0] if key in want else None
        self.out = _capi.StackOut.of(count=[at('count', k) for k in range(spec.n_cats)] if 'count' in want else (),
                                     last=at('last'), last_index=at('last_index'), share=at('share'))

    def _malloc(self, n):
        self.own.append(self.ctx.malloc(n))
        return self.own[-1]

    def free(self):
        for b in self.own:
            b.free()

    def run(self, stream=None):
        self.ctx.mosaic_device(self.sbuf.ptr + self.start, self.spec, self.T, self.H, self.W, self.pbuf.ptr, self.canvas[0], self.canvas[1],
                               self.out, tile_stride=0 if self.stride == self.H * self.W else self.stride, stream=stream)

    def check(self, what):
        """The wanted planes are the host entry's, every other byte of the output buffer is still SENT, and the plane buffer
        is what was uploaded."""
        ref = _capi.mosaic_host(self.tiles, self.place, self.canvas, self.spec)
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for (key, k), (begin, eb) in self.where.items():
            if key not in self.want:
                continue
            got = raw[begin:begin + self.m * eb].copy().view(np.uint16 if eb == 2 else np.uint8)
            want = (ref[key][k] if key == 'count' else ref[key]).reshape(-1)
            assert np.array_equal(got, want), (what, key, k, np.flatnonzero(got != want)[:6], got[np.flatnonzero(got != want)[:6]],
                                               want[np.flatnonzero(got != want)[:6]])
            written[begin:begin + self.m * eb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted planes were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.array_equal(self.sbuf.download(np.uint8, self.shost.size), self.shost), (what, 'the plane was written')
        return ref


WIDTHS = (1, 15, 16, 17, C - 1, C, C + 1, 2 * C + 17)


@pytest.mark.parametrize('width', WIDTHS)
def test_device_entry_every_residue_width_height_stride_and_address(ctx, width):
    """This tile width x every canvas width of WIDTHS; canvas heights either side of the rows of a block; 20 tiles of three rows
    whose col0 runs through all 16 residues mod 16 (negative ones too), so that tile edges cut units on the left, on the
    right and, for widths below 16, on both sides, plus tiles over every edge of the canvas; the stride equal to the tile and
    above it, padding and guards full of a byte that is an observation; the plane 0, 1 and 6 bytes past a 256-byte boundary."""
    rng = np.random.default_rng(8100 + width)
    H, T = 3, 20
    big_w, big_h = WIDTHS[-1], 2 * R + 1
    sbuf = ctx.malloc(2 * GUARD + 256 + T * (H * width + 300))
    obuf = ctx.malloc(7 * (2 * big_w * big_h + 64) + 64)
    pbuf = ctx.malloc(T * 8)
    cases = 0
    for i, canvas_w in enumerate(WIDTHS):
        canvas_h = (R - 1, R, R + 1, 2 * R + 1)[(i + width) % 4]
        spec = random_spec(rng, 1 + (i + width) % 4)
        if i % 3 == 0:                                               # every byte an observation: the kernel has no neutral byte for cut units
            spec = Spec(spec.n_cats, rng.integers(0, spec.n_cats, size=256), spec.fill, spec.outside)
        tiles = rng.integers(0, 256, size=(T, H, width), dtype=np.uint8)
        tiles[tiles == PAD] = PAD - 1
        place = np.zeros((T, 2), dtype=np.int64)
        for r in range(16):                                          # every residue of col0, spread over the canvas and its left edge
            place[r] = (rng.integers(-2, canvas_h), (rng.integers(-1, max(canvas_w // 16, 1) + 1)) * 16 + r - (16 if r % 3 == 0 else 0))
        place[16] = (-1, -(width // 2) - 1)                          # over the top left corner
        place[17] = (canvas_h - 2, canvas_w - width // 2 - 1)        # over the bottom right corner
        place[18] = (1, canvas_w - width)                            # flush with the right edge
        place[19] = (canvas_h, 0)                                    # wholly below
        for j, stride in enumerate((H * width, H * width + 3 + 253 * (i & 1))):
            off = (0, 1, 6)[(i + j) % 3]
            r = Run(ctx, tiles, place, (canvas_h, canvas_w), spec, stride=stride, off=off, sbuf=sbuf, obuf=obuf, pbuf=pbuf)
            r.run()
            ctx.synchronize()
            r.check((width, canvas_h, canvas_w, stride, off, spec.n_cats))
            cases += 1
        info = ctx.last_kernel_info()
        assert 'dswx_mosaic_k' in info and f'grid=({-(-canvas_w // C) * -(-canvas_h // R)},1,1)' in info, info
        assert f'rect={R}x{C}' in info and f'pixels_per_thread={PPT}' in info and f'tiles_in_flight={U}' in info and f'list={L}' in info, info
    assert cases == 2 * len(WIDTHS)
    for b in (sbuf, obuf, pbuf):
        b.free()


def test_empty_inputs_on_the_device(ctx):
    rng = np.random.default_rng(8150)
    spec = random_spec(rng, 2)
    r = Run(ctx, np.zeros((0, 4, 5), dtype=np.uint8), np.zeros((0, 2)), (R + 1, C + 3), spec)      # no tile: the outside values
    r.run()
    ctx.synchronize()
    ref = r.check('no tile')
    assert np.all(ref['last'] == spec.outside) and np.all(ref['last_index'] == NONE) and np.all(ref['share'] == NO_SHARE)
    r.free()
    tiles = rng.integers(0, 256, size=(2, 4, 5), dtype=np.uint8)
    for canvas in ((0, 40), (40, 0)):                                                               # an empty canvas writes nothing
        r = Run(ctx, tiles, [(0, 0), (1, 1)], canvas, spec)
        r.run()
        ctx.synchronize()
        r.check(canvas)
        assert 'none' in ctx.last_kernel_info()
        r.free()
    for shape in ((3, 0, 5), (3, 4, 0)):                                                            # an empty raster covers nothing
        r = Run(ctx, np.zeros(shape, dtype=np.uint8), [(0, 0)] * 3, (5, 40), spec)
        r.run()
        ctx.synchronize()
        assert np.all(r.check(shape)['last'] == spec.outside)
        r.free()
    # the ends of int32 are ordinary placements
    i32 = (-(1 << 31), (1 << 31) - 1)
    place = [(a, b) for a in i32 + (0,) for b in i32 + (0,)]
    r = Run(ctx, rng.integers(0, 256, size=(len(place), 4, 20), dtype=np.uint8), place, (6, 50), spec)
    r.run()
    ctx.synchronize()
    ref = r.check('int32 ends')
    assert set(np.unique(ref['last_index']).tolist()) == {len(place) - 1, NONE}
    r.free()


@pytest.mark.parametrize('n_tiles', [1, U - 1, U, U + 1, L // 2 - 1, L // 2, L // 2 + 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1])
def test_tile_counts_around_a_round_of_loads_and_the_list(ctx, n_tiles):
    """Every tile intersects the first block of a canvas of two blocks (a few reach into the second, whose list stays short);
    the list is consumed when it holds more than L / 2 entries and at the end."""
    rng = np.random.default_rng(8200 + n_tiles)
    H, W = 2, 40
    spec = random_spec(rng, 4)
    tiles = rng.integers(0, 256, size=(n_tiles, H, W), dtype=np.uint8)
    place = np.stack([rng.integers(-1, R, size=n_tiles), rng.integers(-W + 1, C, size=n_tiles)], axis=1)
    r = Run(ctx, tiles, place, (R, C + 30), spec, off=1)
    r.run()
    ctx.synchronize()
    ref = r.check(n_tiles)
    assert int(ref['count'].sum(axis=0).max()) >= min(n_tiles, 2) - 1
    r.free()


def test_65535_random_placements(ctx):
    """65535 tiles of 4 x 20 on a canvas of 64 x 64, placements inside, over the edges and outside."""
    rng = np.random.default_rng(8300)
    T, H, W = 65535, 4, 20
    spec = random_spec(rng, 3)
    tiles = rng.integers(0, 256, size=(T, H, W), dtype=np.uint8)
    place = np.stack([rng.integers(-40, 104, size=T), rng.integers(-60, 124, size=T)], axis=1)
    r = Run(ctx, tiles, place, (64, 64), spec, stride=H * W + 1, off=6)
    r.run()
    ctx.synchronize()
    ref = r.check('65535 tiles')
    assert int(ref['count'].sum(axis=0).max()) > 20 and len(np.unique(ref['last_index'])) > 100     # the latest of ~100 tiles per pixel
    with pytest.raises(_capi.DswxError, match='65535') as e:
        ctx.mosaic_device(r.sbuf.ptr, spec, 65536, H, W, r.pbuf.ptr, 64, 64, r.out)
    assert e.value.code == _capi.ERR_ARG
    r.free()


def test_contents_that_break_accumulators(ctx):
    rng = np.random.default_rng(8400)
    T, H, W = 2 * U + 3, 5, 37
    canvas = (R + 3, 3 * W)
    place = np.stack([rng.integers(-2, 4, size=T), rng.integers(-5, 2 * W, size=T)], axis=1)
    n = H * W
    i = np.arange(n)
    two = Spec(2, [1, 0] + [255] * 254, 200, 201)                   # byte 0: category 1, byte 1: category 0
    cases = [(f'constant {v}', np.full((T, n), v, dtype=np.uint8), two) for v in (0, 1, 77, 255)]
    cases.append(('alternating within a unit', np.tile((i & 1).astype(np.uint8), (T, 1)), two))
    cases.append(('alternating across tiles', np.tile((np.arange(T) & 1).astype(np.uint8)[:, None], (1, n)), two))
    every = rng.integers(0, 2, size=(T, n)).astype(np.uint8)
    every[T // 2] = i % 256
    for n_cats in (1, 2, 3, 4):
        cases.append((f'all 256 byte values in one tile, {n_cats} categories', every, Spec(n_cats, (np.arange(256) * 7) % 6, 3, 4)))
        cases.append((f'noise, {n_cats} categories', rng.integers(0, 256, size=(T, n), dtype=np.uint8),
                      Spec(n_cats, rng.integers(0, 5, size=256), 9, 10)))
    # every byte an observation: a cut unit has no byte to put into the pixels that the tile does not cover
    cases.append(('noise, no byte that is not an observation', rng.integers(0, 256, size=(T, n), dtype=np.uint8), Spec(4, np.arange(256) % 4, 1, 2)))
    cases.append(('noise, one category, every byte observed', rng.integers(0, 256, size=(T, n), dtype=np.uint8), Spec(1, np.zeros(256), 1, 2)))
    sbuf, obuf, pbuf = ctx.malloc(2 * GUARD + T * n), ctx.malloc(7 * (2 * canvas[0] * canvas[1] + 64) + 64), ctx.malloc(T * 8)
    for label, tiles, spec in cases:
        r = Run(ctx, tiles.reshape(T, H, W), place, canvas, spec, sbuf=sbuf, obuf=obuf, pbuf=pbuf)
        r.run()
        ctx.synchronize()
        r.check(label)
    for b in (sbuf, obuf, pbuf):
        b.free()
    # 255 tiles of one category on one pixel, for each of the four fields of the accumulator
    four = Spec(4, [0, 1, 2, 3] + [255] * 252, 9, 8)
    for k in range(4):
        r = Run(ctx, np.full((255, 3, 19), k, dtype=np.uint8), [(1, 5)] * 255, (6, 40), four)
        r.run()
        ctx.synchronize()
        ref = r.check(('255 tiles', k))
        assert np.all(ref['count'][k, 1:4, 5:24] == 255) and int(ref['count'].sum()) == 255 * 3 * 19 and np.all(ref['last_index'][1:4, 5:24] == 254)
        r.free()


@pytest.mark.parametrize('key', KEYS)
def test_each_output_alone(ctx, key):
    rng = np.random.default_rng(8500)
    T, H, W = U + 3, 6, 300
    spec = random_spec(rng, 3)
    tiles = rng.integers(0, 256, size=(T, H, W), dtype=np.uint8)
    place = np.stack([rng.integers(-3, R + 2, size=T), rng.integers(-100, C, size=T)], axis=1)
    r = Run(ctx, tiles, place, (R + 2, C + 21), spec, stride=H * W + 5, off=1, want=(key,))
    r.run()
    ctx.synchronize()
    r.check(key)                                                     # the wanted plane is right, nothing else is written
    assert f"latest={int(key in ('last', 'last_index'))}" in ctx.last_kernel_info()
    if key == 'count':                                               # and one count plane of the three
        r.out.count[0] = r.out.count[2] = None
        r.obuf.upload(np.full(r.osize, SENT, dtype=np.uint8))
        del r.where[('count', 0)], r.where[('count', 2)]
        r.run()
        ctx.synchronize()
        ref = _capi.mosaic_host(tiles, place, r.canvas, spec)
        raw = r.obuf.download(np.uint8, r.osize)
        begin = r.where[('count', 1)][0]
        assert np.array_equal(raw[begin:begin + 2 * r.m].copy().view(np.uint16), ref['count'][1].reshape(-1))
        raw[begin:begin + 2 * r.m] = SENT
        assert np.all(raw == SENT)
    r.free()


def test_identity_placement_is_the_stack_entry_on_the_same_buffer(ctx):
    rng = np.random.default_rng(8600)
    T, H, W = U + 3, 7, 611
    n = H * W
    spec = random_spec(rng, 4)
    tiles = rng.integers(0, 256, size=(T, H, W), dtype=np.uint8)
    r = Run(ctx, tiles, np.zeros((T, 2)), (H, W), spec, stride=n + 9, off=1)
    r.run()
    ctx.synchronize()
    r.check('identity')
    mine = r.obuf.download(np.uint8, r.osize)
    r.obuf.upload(np.full(r.osize, SENT, dtype=np.uint8))
    ctx.stack_device(r.sbuf.ptr + r.start, stack_mod.Spec(spec.n_cats, spec.cat_of_byte, spec.fill), T, n, r.out, tile_stride=n + 9)
    ctx.synchronize()
    assert 'dswx_stack_k' in ctx.last_kernel_info()
    assert np.array_equal(r.obuf.download(np.uint8, r.osize), mine)
    r.free()


def test_on_a_callers_stream_behind_the_kernel_that_writes_the_plane(ctx):
    """Asynchronous on the caller's stream: the stream is held, a copy kernel that REPLACES the plane is queued on it, then the
    entry, with no synchronisation in between.  The entry returns while the hold is pending, and the planes are those of the
    replaced plane -- launched on any other stream it would read the old one."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(8700)
    T, H, W = 6, 90, 257
    n, stride = H * W, H * W + 5
    canvas = (140, 400)
    m = canvas[0] * canvas[1]
    spec = Spec(2, (np.arange(256) % 3), 7, 8)
    place_host = np.stack([rng.integers(-20, 80, size=T), rng.integers(-50, 250, size=T)], axis=1).astype(np.int32)
    old = rng.integers(0, 100, size=T * stride, dtype=np.uint8)
    new = rng.integers(100, 256, size=T * stride, dtype=np.uint8)
    plane = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    place = torch.from_numpy(place_host.copy()).to('cuda:0')
    share = torch.full((m,), SENT, dtype=torch.uint8, device='cuda:0')
    index = torch.full((m,), 0x1111, dtype=torch.int16, device='cuda:0')
    torch.cuda.synchronize()
    want_old = _capi.mosaic_host(old.reshape(T, stride), place_host, canvas, spec, raster=(H, W))
    want_new = _capi.mosaic_host(new.reshape(T, stride), place_host, canvas, spec, raster=(H, W))
    assert not np.array_equal(want_old['share'], want_new['share'])
    out = _capi.StackOut.of(share=share.data_ptr(), last_index=index.data_ptr())
    s = torch.cuda.Stream(device=0)
    call = lambda: ctx.mosaic_device(plane.data_ptr(), spec, T, H, W, place.data_ptr(), canvas[0], canvas[1], out, tile_stride=stride,
                                     stream=s.cuda_stream)
    call()
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(share.cpu().numpy(), want_old['share'].reshape(-1))
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(1.2e9))                       # some hundreds of milliseconds at any shader clock
        held = torch.cuda.Event()
        held.record(s)
        plane.copy_(src)
    t0 = time.perf_counter()
    call()
    dt = time.perf_counter() - t0
    assert not held.query(), f'the entry took {dt * 1e3:.1f} ms on the host: it waited for the stream'
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(share.cpu().numpy(), want_new['share'].reshape(-1))
    assert np.array_equal(index.cpu().numpy().view(np.uint16), want_new['last_index'].reshape(-1))
    assert torch.equal(plane, src)


def download(res, spec, m):
    got = {k: res[k].download(np.uint16 if k in ('count', 'last_index') else np.uint8, m * (spec.n_cats if k == 'count' else 1))
           for k in res}
    if 'count' in got:
        got['count'] = got['count'].reshape(spec.n_cats, m)
    for b in res.values():
        b.free()
    return got


@pytest.mark.parametrize('form', ['packed', 'padded'])
def test_batch_mosaic_on_a_packed_and_a_padded_batch(ctx, form):
    n_tiles, h, w = 6, 61, 67
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, tile_align=1 if form == 'packed' else 256)
    assert (batch.tile_stride == h * w) == (form == 'packed')
    rng = np.random.default_rng(8800)
    canvas = (150, 170)
    m = canvas[0] * canvas[1]
    place = np.stack([rng.integers(-20, 130, size=n_tiles), rng.integers(-20, 150, size=n_tiles)], axis=1).astype(np.int32)
    place[:2] = ((0, 0), (40, 50))
    pbuf = ctx.malloc(n_tiles * 8)
    pbuf.upload(place.view(np.uint8).reshape(-1))
    try:
        batch.synth(SEED, tile0=31)
        batch.classify(_capi.default_params())
        bwtr_spec = Spec(2, [1, 0] + [255] * 254, 255, 254)          # BWTR: 1 water, 0 not water
        for name, spec in (('wtr', wtr_mosaic_spec(outside=254)), ('wtr', wtr_mosaic_spec(partial_is_water=False, fill=0, outside=7)),
                           ('bwtr', bwtr_spec)):
            tiles = np.stack([batch.read_tile(name, t) for t in range(n_tiles)]).reshape(n_tiles, h, w)
            res = batch.mosaic(name, pbuf.ptr, canvas, spec)         # same stream as the classification; None = all tiles
            info = ctx.last_kernel_info()
            ctx.synchronize()
            assert info.count('dswx_mosaic_k') == 1 and f'grid=({-(-canvas[0] // R) * -(-canvas[1] // C)},1,1)' in info, info
            got, want = download(res, spec, m), _capi.mosaic_host(tiles, place, canvas, spec)
            assert list(got) == list(KEYS)
            for k in KEYS:
                assert np.array_equal(got[k], want[k].reshape(got[k].shape)), (name, k)
            assert int(want['count'].sum()) > 0 and len(np.unique(want['last'])) > 2, name           # the layer is not all fill
            # a tile range in the middle, and the other forms of a range: place[0] belongs to tile0, last_index counts from tile0
            for tile0, count in ((2, 3), (1, n_tiles - 1), (0, 1), (n_tiles - 1, None), (1, _capi.BATCH_ALL_TILES), (n_tiles, None), (0, 0)):
                res = batch.mosaic(name, pbuf.ptr, canvas, spec, tile0=tile0, n_tiles=count, want=('share', 'last_index'))
                ctx.synchronize()
                sub = tiles[tile0:] if count in (None, _capi.BATCH_ALL_TILES) else tiles[tile0:tile0 + count]
                got, want = download(res, spec, m), _capi.mosaic_host(sub, place[:len(sub)], canvas, spec)
                assert list(got) == ['last_index', 'share']
                for k in got:
                    assert np.array_equal(got[k], want[k].reshape(-1)), (name, tile0, count, k)
                if (tile0, count) == (2, 3):
                    seen = want['last_index'][want['last_index'] != NONE]
                    assert seen.size and int(seen.max()) <= 2 and int(seen.min()) == 0
        # planes that are not uint8, the counters, a plane this batch does not have; tile ranges outside the batch
        for name in ('blue', 'diag'):
            with pytest.raises(_capi.DswxError, match=r'band\[|diag') as e:
                batch.mosaic(name, pbuf.ptr, canvas, wtr_mosaic_spec())
            assert e.value.code == _capi.ERR_ARG and 'uint8' in str(e.value)
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.mosaic('counters', pbuf.ptr, canvas, wtr_mosaic_spec())
        assert e.value.code == _capi.ERR_ARG
        with pytest.raises(_capi.DswxError, match='land') as e:
            batch.mosaic('land', pbuf.ptr, canvas, wtr_mosaic_spec())
        assert e.value.code == _capi.ERR_ARG and 'no plane' in str(e.value)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside the batch'):
                batch.mosaic('wtr', pbuf.ptr, canvas, wtr_mosaic_spec(), tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(_capi.DswxError, match='place') as e:
            batch.mosaic('wtr', pbuf.ptr + 2, canvas, wtr_mosaic_spec())
        assert e.value.code == _capi.ERR_ALIGN
    finally:
        pbuf.free()
        batch.free()


def test_a_lake_on_a_seam_is_one_body_after_the_mosaic(ctx):
    """Two 64 x 96 tiles, each holding half of one lake, overlapping by 8 columns: the label of each tile finds one body, the
    mosaic followed by dswx_label_device on the canvas finds ONE body whose size is the union's."""
    from proteus_amd.pipeline import TileEngine
    H, W, over = 64, 96, 8
    CW = 2 * W - over
    yy, xx = np.mgrid[0:H, 0:CW]
    lake = ((yy - 31.5) / 20.0) ** 2 + ((xx - (CW - 1) / 2) / 60.0) ** 2 <= 1.0            # an ellipse across the seam
    scene = np.where(lake, 1, 0).astype(np.uint8)
    tiles = np.stack([scene[:, :W], scene[:, CW - W:]])
    tiles[0, :, W - 3:] = 253                                        # a cloud over the edge of the first tile, inside the overlap
    assert (tiles[0] == 1).any() and (tiles[1] == 1).any()
    eng = TileEngine(ctx)
    try:
        p = eng.upload(tiles)
        per_tile = p.label(wtr_label_spec(1), want=('summary',))
        s = per_tile['summary'].numpy()
        assert s[0, 0] == 1 and s[1, 0] == 1                          # one body in each tile
        halves = (int(s[0, 1]), int(s[1, 1]))
        res = p.mosaic([(0, 0), (0, W - over)], (H, CW), wtr_mosaic_spec(), want=('last',))
        canvas = res['last']
        assert np.array_equal(canvas.numpy(), scene)                 # the cloud filled from the second tile
        whole = canvas.label(wtr_label_spec(1), want=('summary',))
        t = whole['summary'].numpy()[0]
        assert t[0] == 1 and int(t[1]) == int(lake.sum()) == int(t[2])                     # ONE body, the union's size
        assert max(halves) < int(lake.sum()) < sum(halves) + 3 * H
        for d in (per_tile, res, whole):
            for plane in d.values():
                plane.release()
        p.release()
    finally:
        eng.close()


def test_device_plane_mosaic(ctx):
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(8900)
    try:
        a = rng.choice(np.array([0, 1, 2, 252, 253, 254, 255, 9], dtype=np.uint8), size=(4, 100, 130))
        place = [(0, 0), (0, 100), (70, 0), (70, 100)]
        p = eng.upload(a)
        for spec, want_keys in ((wtr_mosaic_spec(outside=254), KEYS), (Spec(3, np.arange(256) % 5, 1, 2), KEYS), (wtr_mosaic_spec(), ('share',))):
            got = p.mosaic(place, (180, 260), spec, want=want_keys)
            want = mosaic_tiles(a, place, (180, 260), spec)
            names = ([f'count{k}' for k in range(spec.n_cats)] if 'count' in want_keys else []) + [k for k in KEYS[1:] if k in want_keys]
            assert list(got) == names
            for name, plane in got.items():
                ref = want['count'][int(name[5:])] if name.startswith('count') else want[name]
                assert plane.shape == (180, 260) and plane.dtype == ref.dtype
                assert np.array_equal(plane.numpy(), ref), name
            # each is a plane like any other: counted on the device
            assert np.array_equal(got['share'].histogram(), np.bincount(want['share'].reshape(-1), minlength=256).astype(np.uint64))
            for plane in got.values():
                plane.release()
        with pytest.raises(ValueError):
            p.mosaic(place[:3], (180, 260), wtr_mosaic_spec())
        with pytest.raises(ValueError):
            p.mosaic(place, (180, -1), wtr_mosaic_spec())
        p.release()
        with pytest.raises(ValueError):
            eng.upload(np.zeros((4, 4), dtype=np.uint8)).mosaic([(0, 0)], (4, 4), wtr_mosaic_spec())
    finally:
        eng.close()


def test_the_command_line_tool(tmp_path, capsys):
    """bin/dswx_mosaic.py on four 100 x 130 WTR files of a 2 x 2 block with shifted geotransforms: every output band is the
    numpy statement's, every file a valid COG with the canvas geotransform and the first input's projection, the bodies of the
    canvas summarised; a file of another size, another projection, another pixel size or off the lattice is refused."""
    spec = importlib.util.spec_from_file_location('dswx_mosaic_tool', os.path.join(ROOT, 'bin', 'dswx_mosaic.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(9000)
    x0, y0, d = 600000.0, 4100040.0, 30.0
    H, W = 100, 130
    offsets = [(0, 100), (0, 0), (70, 100), (70, 0)]                 # rows, columns from the canvas origin; the first file is top RIGHT
    gt_of = lambda r, c: (x0 + c * d, d, 0.0, y0 - r * d, 0.0, -d)
    layers = rng.choice(np.array([0, 1, 2, 252, 253, 254, 255], dtype=np.uint8), size=(4, H, W), p=[.3, .2, .1, .05, .2, .05, .1])
    files = []
    for k, (r, c) in enumerate(offsets):
        files.append(str(tmp_path / f'tile{k}_WTR.tif'))
        geotiff.write_geotiff(files[-1], layers[k], geo_tags=geotiff.geo_tags_from_geotransform(gt_of(r, c), epsg=32611),
                              metadata={'SPACECRAFT_NAME': 'test'}, nodata=255)
    ch, cw, place, gt = layout([gt_of(r, c) for r, c in offsets], H, W)
    assert (ch, cw) == (170, 230) and place.tolist() == [list(o) for o in offsets] and gt == gt_of(0, 0)
    for flags, mspec in (([], wtr_mosaic_spec()), (['--no-partial'], wtr_mosaic_spec(partial_is_water=False))):
        prefix = str(tmp_path / ('out' + ''.join(flags)))
        bodies = str(tmp_path / ('bodies' + ''.join(flags) + '.json'))
        assert tool.main(flags + ['--bodies', bodies, '-o', prefix] + files) == 0
        want = mosaic_tiles(layers, place, (ch, cw), mspec)
        for suffix, ref, dtype, nodata in (('COUNT_WATER', want['count'][0], np.uint16, None), ('COUNT_LAND', want['count'][1], np.uint16, None),
                                           ('LAST', want['last'], np.uint8, 255), ('LAST_INDEX', want['last_index'], np.uint16, 65535),
                                           ('SHARE', want['share'], np.uint8, 255)):
            path = f'{prefix}_{suffix}.tif'
            arr, info = geotiff.read_geotiff(path)
            assert arr.dtype == dtype and arr.shape == (ch, cw) and np.array_equal(arr, ref), suffix
            assert geotiff.validate_cog(path) == [], suffix
            assert tuple(info.geotransform) == gt and info.nodata == nodata, (suffix, info.geotransform, info.nodata)
            assert list(info.geo_tags[geotiff.TAG_GEOKEYS][1])[-1] == 32611
            assert info.metadata['MOSAIC_INPUT_FILES'] == ', '.join(os.path.basename(f) for f in files)
            assert info.metadata['SPACECRAFT_NAME'] == 'test'
        text = capsys.readouterr().out
        said = json.loads(text.strip().splitlines()[-1])
        assert said == json.load(open(bodies))
        from proteus_amd.label import label_tiles
        ref = label_tiles(want['last'][None], wtr_label_spec(1, partial_is_water=not flags))
        assert said['bodies'] == int(ref['summary'][0, 0]) > 0 and said['member_pixels'] == int(ref['summary'][0, 1])
        assert (said['canvas_height'], said['canvas_width']) == (ch, cw)
    capsys.readouterr()
    tags = geotiff.geo_tags_from_geotransform(gt_of(0, 0), epsg=32611)
    other = str(tmp_path / 'other_size.tif')
    geotiff.write_geotiff(other, layers[0][:, :129], geo_tags=tags, nodata=255)
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], other]) == 1
    text = capsys.readouterr().out
    assert '[FAIL] Comparing size' in text and '130 x 100' in text and '129 x 100' in text
    zone = str(tmp_path / 'other_zone.tif')
    geotiff.write_geotiff(zone, layers[0], geo_tags=geotiff.geo_tags_from_geotransform(gt_of(0, 0), epsg=32612), nodata=255)
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], files[1], zone]) == 1
    text = capsys.readouterr().out
    assert '[FAIL] Comparing projection' in text and 'input 3' in text
    half = str(tmp_path / 'half_a_pixel.tif')
    geotiff.write_geotiff(half, layers[0], geo_tags=geotiff.geo_tags_from_geotransform((x0 + 15.0,) + gt_of(0, 0)[1:], epsg=32611), nodata=255)
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], half]) == 1
    text = capsys.readouterr().out
    assert '[FAIL] Comparing geotransform' in text and 'input 2 origin' in text and 'lattice' in text
    coarse = str(tmp_path / 'coarse.tif')
    geotiff.write_geotiff(coarse, layers[0], geo_tags=geotiff.geo_tags_from_geotransform((x0, 60.0, 0.0, y0, 0.0, -60.0), epsg=32611), nodata=255)
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], coarse]) == 1
    text = capsys.readouterr().out
    assert '[FAIL] Comparing geotransform' in text and 'input 2 pixel size' in text
    assert not os.path.exists(str(tmp_path / 'no_SHARE.tif'))
    assert tool.main(['-o', str(tmp_path / 'no'), '--band', '2'] + files) == 1


def test_mosaic_example_runs(tmp_path):
    """examples/batch_mosaic.c: its own checks (exit status 0: every pixel of the five device planes against its paste loop and
    against dswx_mosaic_host)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_mosaic')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_mosaic.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '301', '27'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr mosaic: device, paste loop and host entry agree in every pixel' in r.stdout
    assert '4 tiles of 90601 pixels on a canvas of 575 x 575' in r.stdout
