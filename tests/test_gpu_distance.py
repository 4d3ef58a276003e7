"""The distance entries on the GPU: dswx_distance_device and dswx_batch_distance bit for bit against the library's scalar
statement (dswx_distance_host, which tests/test_distance.py pins to the numpy statement, to a brute-force statement and to
scipy) on all four outputs -- heights and widths either side of every published geometry constant and of a 16-byte load, every
pattern of tests/_distance_cases.py at each, four radii, the plane at odd addresses, padded strides, every legal subset of the
outputs, with every byte outside the output planes checked; wide rows; the widest row and the refusal above it; more tiles
than grid.y has blocks; a caller's stream with the outputs reused; every form of batch; the results as device planes; the
summary against counts made another way; bin/dswx_distance.py; the C example."""
import ctypes
import importlib.util
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py)
    import torch
except ImportError:
    torch = None

from proteus_amd import _capi, geotiff
from proteus_amd.checksum import checksum
from proteus_amd.distance import NONE, SUMMARY_WORDS, Spec, distance_tiles, summary_of, wtr_distance_spec
from proteus_amd.synth import SEED
from tests import _distance_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BH, NC, BW, NEAR = _capi.DISTANCE_BAND_H, _capi.DISTANCE_COLS, _capi.DISTANCE_BLOCK_W, _capi.DISTANCE_NEAR
PAD = 200                                         # every byte of a plane buffer that is not tile data: a TARGET byte of C.plane_of
SENT = 0xEE                                       # every byte of an output buffer beforehand
KEYS = ('dist2', 'nearest', 'within', 'summary')
GUARD = 512
EB = {'dist2': 4, 'nearest': 4, 'within': 1, 'summary': 8}


def subsets(radius):
    """Every legal subset of the outputs: `within` needs a radius."""
    return (('dist2',), ('dist2', 'nearest'), KEYS if radius else ('dist2', 'nearest', 'summary'), ('dist2', 'summary'))


def host(tiles, spec):
    return _capi.distance_host(tiles, spec, want=KEYS if spec.max_radius else ('dist2', 'nearest', 'summary'))


def radius_above(tiles, table):
    """One above the largest distance present in the unbounded transform (1 for planes without a target)."""
    d = _capi.distance_host(tiles, Spec(table), want=('dist2',))['dist2']
    d = d[d != NONE]
    return math.isqrt(int(d.max())) + 1 if d.size else 1


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Run:
    """One call of dswx_distance_device.  The plane lies guard | `off` bytes past a 256-byte boundary | guard in `sbuf`, every
    byte that is not tile data PAD; the wanted outputs lie in `obuf`, dist2 and nearest 4 bytes, within 1 byte and summary 8
    bytes past a 16-byte boundary, every byte SENT beforehand."""

    def __init__(self, ctx, tiles, spec, stride=None, off=0, want=KEYS, sbuf=None, obuf=None):
        self.ctx, self.tiles, self.spec, self.want = ctx, tiles, spec, want
        self.T, self.H, self.W = tiles.shape
        n = self.H * self.W
        self.stride = n if stride is None else stride
        span = (self.T - 1) * self.stride + n if self.T else 0          # the last tile's padding need not exist
        self.start = GUARD + off
        self.shost = np.full(self.start + span + GUARD, PAD, dtype=np.uint8)
        for t in range(self.T):
            self.shost[self.start + t * self.stride:self.start + t * self.stride + n] = tiles[t].reshape(-1)
        self.sbuf = sbuf if sbuf is not None else ctx.malloc(self.shost.size)
        assert self.sbuf.nbytes >= self.shost.size and self.sbuf.ptr % 256 == 0
        self.sbuf.upload(self.shost)
        self.count = {k: self.T * (SUMMARY_WORDS if k == 'summary' else n) for k in KEYS}
        self.where, cursor = {}, 0
        for k in KEYS:
            begin = -(-cursor // 16) * 16 + EB[k]
            self.where[k] = begin
            cursor = begin + self.count[k] * EB[k] + 16
        self.osize = cursor + 16
        self.obuf = obuf if obuf is not None else ctx.malloc(self.osize)
        assert self.obuf.nbytes >= self.osize and self.obuf.ptr % 16 == 0
        self.poison()
        self.out = _capi.DistanceOut.of(**{k: self.obuf.ptr + self.where[k] for k in want})

    def poison(self):
        self.obuf.upload(np.full(self.osize, SENT, dtype=np.uint8))

    def run(self, stream=None):
        self.ctx.distance_device(self.sbuf.ptr + self.start, self.spec, self.T, self.H, self.W, self.out,
                                 tile_stride=0 if self.stride == self.H * self.W else self.stride, stream=stream)

    def check(self, what, ref=None):
        """The wanted planes are the host entry's, every other byte of the output buffer is still SENT, and the plane buffer is
        what was uploaded."""
        ref = host(self.tiles, self.spec) if ref is None else ref
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for k in self.want:
            begin, nb = self.where[k], self.count[k] * EB[k]
            got = raw[begin:begin + nb].copy().view(_capi.DISTANCE_DTYPES[k])
            want = ref[k].reshape(-1)
            assert np.array_equal(got, want), (what, k, np.flatnonzero(got != want)[:6], got[got != want][:6], want[got != want][:6])
            written[begin:begin + nb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted planes were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.array_equal(self.sbuf.download(np.uint8, self.shost.size), self.shost), (what, 'the plane was written')
        return ref

    def free(self):
        self.sbuf.free()
        self.obuf.free()


def around(c):
    return (c - 1, c, c + 1, 2 * c + 1)


HEIGHTS = tuple(sorted({1, 2, 15, 16, 17, *around(BH), *around(NC)}))
WIDTHS = tuple(sorted({1, 2, 15, 16, 17, *around(NC), *around(BW), *around(NEAR)}))


@pytest.mark.parametrize('W', WIDTHS)
def test_device_entry_against_the_host_entry_every_pattern_height_radius_address_and_subset(ctx, W):
    """This width x the heights either side of the band of the column pass, of its four columns and of a 16-byte load; the
    tiles of a call are the patterns of tests/_distance_cases.py; the radii 0, 1, 3 and one above the largest distance
    present; every legal subset of the outputs; the plane 0, 1 and 3 bytes past a 256-byte boundary, the stride equal to the
    raster and 5 above it with padding and guards full of a TARGET byte."""
    rng = np.random.default_rng(9100 + W)
    T = 15
    big = max(HEIGHTS) * W
    sbuf = ctx.malloc(2 * GUARD + 256 + T * (big + 5))
    obuf = ctx.malloc(T * (9 * big + 8 * SUMMARY_WORDS) + 256)
    cases = 0
    for H in HEIGHTS:
        tiles, table = C.plane_of(np.stack(list(C.patterns(H, W, rng).values())), rng)
        assert tiles.shape == (T, H, W)
        for radius in (0, 1, 3, radius_above(tiles, table)):
            spec = Spec(table, radius, mark=(9, 77, 255)[cases % 3])
            ref = host(tiles, spec)
            for want in subsets(radius):
                off = (0, 1, 3)[cases % 3]
                r = Run(ctx, tiles, spec, stride=H * W + (0 if off == 0 else 5), off=off, want=want, sbuf=sbuf, obuf=obuf)
                r.run()
                ctx.synchronize()
                r.check((H, W, radius, off, want), ref=ref)
                cases += 1
            info = ctx.last_kernel_info()
            assert 'dswx_distance_column_k' in info and 'dswx_distance_row_k' in info and f'band={BH}x{NC}' in info and f'radius={radius}' in info, info
            assert ('band,fill' in info) == (H > BH), info
    sbuf.free()
    obuf.free()


def test_a_table_where_only_byte_255_is_a_target(ctx):
    rng = np.random.default_rng(9150)
    plane, table = C.plane_of(np.stack([C.noise(BH + 3, BW + 9, d, rng) for d in C.DENSITIES]), rng, only_255=True)
    for radius in (0, 4):
        r = Run(ctx, plane, Spec(table, radius, mark=254), stride=plane[0].size + 7, off=1, want=subsets(radius)[2])
        r.run()
        ctx.synchronize()
        ref = r.check(('only 255', radius))
        assert np.array_equal(ref['dist2'] == 0, plane == 255)
        r.free()


@pytest.mark.parametrize('radius', [0, 40])
def test_wide_rows_where_a_wave_owns_several_blocks_and_the_search_goes_through_many(ctx, radius):
    """200 x 1100 and 3 x 1100: seventeen full blocks and a ragged one, so every wave owns several; sparse targets, so that
    the nearest one is many blocks away, in both directions, and most blocks are skipped by their minimum: one corner each,
    one full column, two equidistant targets, noise at one in 20000, and nothing; the radius 40 is above the outward look
    (NEAR) and ends the walk through the blocks early."""
    rng = np.random.default_rng(9200 + radius)
    for H, W in ((200, 1100), (3, 1100)):
        targets = np.stack([C.one_at(H, W, 0, 0), C.one_at(H, W, H - 1, W - 1), C.one_at(H, W, H // 2, W // 2), C.full_column(H, W),
                            C.two_equidistant(H, W), C.noise(H, W, 0.00005, rng), C.noise(H, W, 0.002, rng), C.empty(H, W),
                            C.diagonal(H, W)])
        tiles, table = C.plane_of(targets, rng)
        spec = Spec(table, radius, mark=5)
        r = Run(ctx, tiles, spec, stride=H * W + 5, off=3, want=subsets(radius)[2])
        r.run()
        ctx.synchronize()
        ref = r.check((H, W, radius))
        if radius == 0:                                                 # from a corner to the opposite one
            assert ref['dist2'][0, H - 1, W - 1] == (H - 1) ** 2 + (W - 1) ** 2 and ref['nearest'][1, 0, 0] == H * W - 1
        r.free()


def test_the_widest_row_and_the_refusal_one_above(ctx):
    W = _capi.DISTANCE_MAX_WIDTH
    rng = np.random.default_rng(9250)
    targets = np.stack([C.one_at(2, W, 1, 0), C.one_at(2, W, 0, W - 1), C.noise(2, W, 0.001, rng), C.empty(2, W)])
    tiles, table = C.plane_of(targets, rng)
    r = Run(ctx, tiles, Spec(table), off=1, want=('dist2', 'nearest', 'summary'))
    r.run()
    ctx.synchronize()
    ref = r.check('widest')
    assert ref['dist2'][0, 0, W - 1] == (W - 1) ** 2 + 1
    rc = ctx.lib.dswx_distance_device(ctx.handle, ctypes.c_void_p(r.sbuf.ptr + r.start), ctypes.byref(_capi.DistanceSpec.of(r.spec)), 1, 1,
                                      W + 1, 0, ctypes.byref(r.out), None)
    assert rc == _capi.ERR_ARG and 'DSWX_DISTANCE_MAX_WIDTH' in ctx.lib.dswx_last_error().decode()
    r.free()


def test_on_a_callers_stream_twice_with_the_same_outputs(ctx):
    """On a caller's stream, and a second call on the same stream that reuses the outputs of the first as they are (full of
    the first call's distances and summary): nothing depends on what the outputs held beyond the entry's own memset."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(9400)
    H, W = 2 * BH + 1, 2 * BW + 1
    first, table = C.plane_of(np.stack([C.full(H, W), C.noise(H, W, 0.05, rng), C.checkerboard(H, W)]), rng)
    second, _ = C.plane_of(np.stack([C.noise(H, W, 0.002, rng), C.one_at(H, W, H - 1, W - 1), C.empty(H, W)]), rng)
    s = torch.cuda.Stream(device=0)
    for radius in (0, 50):
        spec = Spec(table, radius, mark=0)
        r = Run(ctx, first, spec, stride=H * W + 5, off=3, want=subsets(radius)[2])
        r.run(stream=s.cuda_stream)
        ctx.synchronize(s.cuda_stream)
        r.check(('first', radius))
        r.tiles = second                                             # the same buffers, another plane, the outputs NOT poisoned again
        for t in range(3):
            r.shost[r.start + t * r.stride:r.start + t * r.stride + H * W] = second[t].reshape(-1)
        r.sbuf.upload(r.shost)
        r.run(stream=s.cuda_stream)
        r.run(stream=s.cuda_stream)
        ctx.synchronize(s.cuda_stream)
        r.check(('second', radius))
        r.free()


def test_a_workgroup_does_a_second_tile_past_the_blocks_of_grid_y(ctx):
    """65535 + 4 tiles of 3 x 5 pixels: grid.y is 65535, and the workgroups of tiles 0 .. 3 walk on to tiles 65535 .. 65538 with
    the LDS of the row pass as the first tile left it.  Every output of EVERY tile against the host entry, radius 2 (within
    changes bytes, some pixels are not reached), the stride 5 above the raster, the plane one byte past a 256-byte boundary."""
    rng = np.random.default_rng(9550)
    H, W = 3, 5
    targets = C.second_pass_targets(H, W, rng)
    T = len(targets)
    assert T == 65535 + 4
    tiles, table = C.plane_of(targets, rng)
    r = None
    for radius in (2, 0):
        spec = Spec(table, radius, mark=77)
        ref = host(tiles, spec)
        assert ref['summary'][65535, 2] == H * W and ref['summary'][0, 0] == H * W
        r = Run(ctx, tiles, spec, stride=H * W + 5, off=1, want=subsets(radius)[2], sbuf=r.sbuf if r else None, obuf=r.obuf if r else None)
        r.run()
        ctx.synchronize()
        info = ctx.last_kernel_info()
        assert info.count(',65535,1)') == 2, info
        r.check(radius, ref=ref)
    r.free()


def test_summary_counted_another_way(ctx):
    """Consistency without an oracle.  Word 0 (targets) is the plane's histogram -- dswx_histogram_device on the same bytes --
    folded through the target table; the histogram of `within` gains exactly word 1 pixels of the mark byte; the other words
    from the downloaded dist2 plane with bincount and argmax."""
    rng = np.random.default_rng(9600)
    H, W, T = 2 * BH + 3, 2 * BW + 5, 3
    tiles, table = C.plane_of(np.stack([C.noise(H, W, d, rng) for d in C.DENSITIES]), rng)
    spec = Spec(table, 6, mark=99)                                   # 99 is no byte of the plane
    r = Run(ctx, tiles, spec)
    r.run()
    hist = ctx.malloc(2 * T * 256 * 8)
    ctx.histogram_device(r.sbuf.ptr + r.start, _capi.HIST_U8, T, H * W, hist.ptr)
    ctx.histogram_device(r.obuf.ptr + r.where['within'], _capi.HIST_U8, T, H * W, hist.ptr + T * 256 * 8)
    ctx.synchronize()
    bins = hist.download(np.uint64, 2 * T * 256).reshape(2, T, 256)
    summary = r.obuf.download(np.uint64, T * SUMMARY_WORDS, r.where['summary']).reshape(T, SUMMARY_WORDS)
    dist2 = r.obuf.download(np.uint32, T * H * W, r.where['dist2']).reshape(T, H * W)
    for t in range(T):
        d = dist2[t].astype(np.int64)
        reached = d != NONE
        assert summary[t, 0] == bins[0, t, table != 0].sum() == np.count_nonzero(d == 0)
        assert summary[t, 1] == bins[1, t, 99] and summary[t, 0] + summary[t, 1] + summary[t, 2] == H * W
        assert summary[t, 2] == np.count_nonzero(~reached)
        assert summary[t, 3] == d[reached].max() and summary[t, 4] == np.argmax(np.where(reached, d, -1))
        assert summary[t, 5] == d[reached].sum() and summary[t, 6] == summary[t, 7] == 0
        ring = d[reached & (d > 0)]
        assert np.array_equal(summary[t, 8:], np.bincount(np.floor(np.log2(ring)).astype(int), minlength=32).astype(np.uint64))
    assert summary[0, 2] == 0 and summary[2, 2] > 0              # at one target in two every pixel is reached, at one in 500 not
    assert np.array_equal(summary, summary_of(dist2.reshape(T, H, W)))
    r.check('counted another way')
    hist.free()
    r.free()


def test_refusals_write_nothing(ctx):
    rng = np.random.default_rng(9700)
    tiles, table = C.plane_of(rng.random((2, 20, 30)) < 0.1, rng)
    spec = Spec(table, 3, mark=7)
    r = Run(ctx, tiles, spec)
    plane = r.sbuf.ptr + r.start
    lib, h = ctx.lib, ctx.handle

    def call(plane=plane, cspec=_capi.DistanceSpec.of(spec), n=2, H=20, W=30, stride=0, out=r.out, handle=h):
        return lib.dswx_distance_device(handle, ctypes.c_void_p(plane), ctypes.byref(cspec) if cspec is not None else None, n, H, W,
                                        stride, ctypes.byref(out) if out is not None else None, None)

    def cs(**kw):
        c = _capi.DistanceSpec.of(spec)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def outs(**kw):
        o = _capi.DistanceOut.of(**{k: r.obuf.ptr + r.where[k] for k in KEYS})
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    A, L = _capi.ERR_ARG, _capi.ERR_ALIGN
    for rc, kw in ((A, {'cspec': None}), (A, {'out': None}), (A, {'cspec': cs(mark=256)}), (A, {'cspec': cs(mark=-1)}),
                   (A, {'cspec': cs(max_radius=0)}),                 # within is wanted
                   (A, {'n': -1}), (A, {'H': -1}), (A, {'W': -1}), (A, {'stride': -1}), (A, {'stride': 599}),
                   (A, {'H': 46341, 'W': 1}), (A, {'H': 1, 'W': 46341}), (A, {'H': 1, 'W': _capi.DISTANCE_MAX_WIDTH + 1}),
                   (A, {'H': 46340, 'W': 8192, 'n': 1 << 33}), (A, {'plane': None}), (A, {'out': outs(dist2=None)}),
                   (L, {'out': outs(dist2=r.out.dist2 + 2)}), (L, {'out': outs(nearest=r.out.nearest + 1)}),
                   (L, {'out': outs(summary=r.out.summary + 4)}), (A, {'handle': None})):
        assert call(**kw) == rc, (kw, lib.dswx_last_error())
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    # arguments before the context: a bad spec AND no context names the spec
    assert call(cspec=cs(mark=300), handle=None) == A and 'mark' in lib.dswx_last_error().decode()
    # an empty raster and no tiles are legal and write nothing
    for kw in ({'n': 0}, {'H': 0}, {'W': 0}):
        assert call(**kw) == 0, kw
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    r.run()
    ctx.synchronize()
    r.check('after the refusals')
    r.free()


def download(res, n_tiles, h, w):
    got = {k: res[k].download(_capi.DISTANCE_DTYPES[k], n_tiles * (SUMMARY_WORDS if k == 'summary' else h * w)) for k in res}
    for k in got:
        got[k] = got[k].reshape((n_tiles, SUMMARY_WORDS) if k == 'summary' else (n_tiles, h, w))
    return got


FORMS = {'packed': {}, 'separate_outputs': {'separate_outputs': True}, 'slide_placed': {'sliding_outputs': True},
         'padded': {'tile_align': 256}, 'contiguous': {'tile_align': 1}}


@pytest.mark.parametrize('form', list(FORMS))
def test_batch_distance_on_the_wtr_plane_of_a_classified_batch(ctx, form):
    """The WTR plane of a classified batch of every form: every tile, tile ranges with tile0 > 0, DSWX_BATCH_ALL_TILES; the
    results checked by CHECKSUMS made on the device against the checksums of the host entry on the downloaded layer; DIAG, a
    band, the counters, a missing plane and ranges outside the batch refused."""
    n_tiles, h, w = 4, 2 * BH + 9, BW + 37
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, **FORMS[form])
    sums = ctx.malloc(8 * n_tiles)
    try:
        batch.synth(SEED, tile0=31)
        p = _capi.default_params()
        if form == 'slide_placed':
            batch.place_slide(p, slack_bytes=24 << 20, step_bytes=2 << 20, spread_gaps=2, refine_passes=1, launches=2, keep_free_bytes=0)
        batch.classify(p)
        tiles = np.stack([batch.read_tile('wtr', t) for t in range(n_tiles)])
        for spec in (wtr_distance_spec(), wtr_distance_spec(radius=5, partial_is_water=False)):
            keys = subsets(spec.max_radius)[2]
            ref = host(tiles, spec)
            assert ref['summary'][:, 0].min() > 1 and ref['summary'][:, 1].min() > 1        # the layer has water and land
            for tile0, count in ((0, None), (1, n_tiles - 1), (2, 1), (1, _capi.BATCH_ALL_TILES), (n_tiles, None), (0, 0)):
                res = batch.distance('wtr', spec, tile0=tile0, n_tiles=count, want=keys)
                assert list(res) == list(keys)
                last = tile0 + (n_tiles - tile0 if count in (None, _capi.BATCH_ALL_TILES) else count)
                nt = last - tile0
                for k in keys:
                    per = SUMMARY_WORDS if k == 'summary' else h * w
                    if nt:
                        ctx.checksum_device(res[k].ptr, EB[k], nt, per, sums.ptr)
                    ctx.synchronize()
                    got = sums.download(np.uint64, nt) if nt else np.zeros(0, dtype=np.uint64)
                    want = [checksum(ref[k][t].reshape(-1)) for t in range(tile0, last)]
                    assert got.tolist() == want, (form, k, tile0, count)
                for b in res.values():
                    b.free()
            res = batch.distance('wtr', spec, want=('dist2',))
            ctx.synchronize()
            assert list(res) == ['dist2'] and np.array_equal(download(res, n_tiles, h, w)['dist2'], ref['dist2'])
            res['dist2'].free()
        spec = wtr_distance_spec()
        for name in ('blue', 'swir2', 'diag'):
            with pytest.raises(_capi.DswxError, match=r'band\[|diag') as e:
                batch.distance(name, spec)
            assert e.value.code == _capi.ERR_ARG and 'uint8' in str(e.value)
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.distance('counters', spec)
        assert e.value.code == _capi.ERR_ARG
        for name in ('land', 'browse'):
            with pytest.raises(_capi.DswxError, match=name) as e:
                batch.distance(name, spec)
            assert e.value.code == _capi.ERR_ARG and 'no plane' in str(e.value)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside the batch'):
                batch.distance('wtr', spec, tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(ValueError):
            batch.distance('water', spec)
        with pytest.raises(ValueError):
            batch.distance('wtr', spec, want=('within',))                # no radius
    finally:
        sums.free()
        batch.free()


def test_device_plane_distance_feeds_histogram_and_checksum(ctx):
    """DevicePlane.distance, and its results as planes like any other: the within plane histogrammed on the device, dist2 and
    nearest checksummed, with no download in between."""
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9800)
    try:
        a = rng.choice(np.array([0, 1, 2, 252, 253, 255], dtype=np.uint8), size=(3, BH + 20, BW + 30), p=[0.9, 0.01, 0.01, 0.03, 0.03, 0.02])
        p = eng.upload(a)
        spec = wtr_distance_spec(radius=4)
        want = distance_tiles(a, spec)
        got = p.distance(spec, want=KEYS)
        assert list(got) == list(KEYS)
        assert np.array_equal(got['within'].histogram(), np.bincount(want['within'].reshape(-1), minlength=256).astype(np.uint64))
        assert got['dist2'].checksum() == checksum(want['dist2'].reshape(-1)) and got['nearest'].checksum() == checksum(want['nearest'].reshape(-1))
        assert got['within']._host is None and got['dist2']._host is None
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k].numpy(), want[k]), k
        only = p.distance(wtr_distance_spec(), want=('dist2',))
        assert list(only) == ['dist2'] and np.array_equal(only['dist2'].numpy(), distance_tiles(a, wtr_distance_spec())['dist2'])
        one = eng.upload(a[0]).distance(spec, want=('summary',))
        assert list(one) == ['dist2', 'summary'] and np.array_equal(one['summary'].numpy(), want['summary'][:1])
        with pytest.raises(ValueError):
            eng.upload(np.zeros((4,), dtype=np.uint8)).distance(spec)
        with pytest.raises(ValueError):
            eng.upload(np.zeros((2, 4, 4), dtype=np.uint16)).distance(spec)
        with pytest.raises(ValueError):
            p.distance(wtr_distance_spec(), want=('within',))
    finally:
        eng.close()


@pytest.fixture(scope='module')
def product_file(tmp_path_factory):
    """The multi-band product file of the suite's own synthetic product run (tools/make_synthetic_hls.py, 301 x 301)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    from proteus_amd import dswx_hls
    tmp = tmp_path_factory.mktemp('distance_product')
    _, files, _, _ = synth_hls.make(str(tmp), size=301, tile=4)
    out = str(tmp / 'product.tif')
    assert dswx_hls.generate_dswx_layers(files, out) is True
    return out


def test_the_command_line_tool(product_file, tmp_path, capsys):
    """bin/dswx_distance.py on a product file: the distance raster is pixel_size * sqrt(dist2) of the host entry on band 1 as
    a Float32 COG with the not-reached pixels nodata, the buffer a Byte COG that holds the host entry's within plane, the
    JSON the host entry's summary in metres."""
    spec = importlib.util.spec_from_file_location('dswx_distance_tool', os.path.join(ROOT, 'bin', 'dswx_distance.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    bands, info = geotiff.read_geotiff(product_file)
    wtr = bands[0] if bands.ndim == 3 else bands
    gt = tuple(info.geotransform)
    px = abs(gt[1])
    for metres in (None, 4 * px):
        dist, buf = str(tmp_path / f'dist{metres}.tif'), str(tmp_path / f'buf{metres}.tif')
        flags = ['--out-distance', dist] + ([] if metres is None else ['--radius-m', str(metres), '--out-buffer', buf])
        capsys.readouterr()
        assert tool.main(flags + [product_file]) == 0
        said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        dspec = wtr_distance_spec(radius=0 if metres is None else 4)
        ref = host(wtr[None], dspec)
        s = ref['summary'][0]
        assert (said['water_pixels'], said['reached_pixels'], said['not_reached_pixels']) == tuple(int(v) for v in s[:3])
        assert said['radius_pixels'] == dspec.max_radius and said['pixel_size_m'] == px
        assert said['largest_distance_m'] == px * math.sqrt(int(s[3])) and said['largest_distance_pixel'] == [int(s[4]) // wtr.shape[1], int(s[4]) % wtr.shape[1]]
        assert said['pixels_by_log2_dist2'] == [int(v) for v in s[8:]] and said['water_pixels'] > 1
        arr, meta = geotiff.read_geotiff(dist)
        d2 = ref['dist2'][0]
        want = np.where(d2 == NONE, tool.NODATA, px * np.sqrt(d2.astype(np.float64))).astype(np.float32)
        assert arr.dtype == np.float32 and np.array_equal(arr, want)
        assert geotiff.validate_cog(dist) == [] and tuple(meta.geotransform) == gt and meta.nodata == tool.NODATA
        if metres is not None:
            arr, meta = geotiff.read_geotiff(buf)
            assert arr.dtype == np.uint8 and np.array_equal(arr, ref['within'][0]) and np.count_nonzero(arr == dspec.mark) == int(s[1]) > 0
            assert geotiff.validate_cog(buf) == [] and tuple(meta.geotransform) == gt
    capsys.readouterr()
    assert tool.main(['--out-distance', str(tmp_path / 'no.tif'), '--out-buffer', str(tmp_path / 'nob.tif'), product_file]) == 1    # no radius
    assert tool.main(['--out-distance', str(tmp_path / 'no.tif'), '--band', '99', product_file]) == 1
    assert tool.main(['--out-distance', str(tmp_path / 'no.tif'), str(tmp_path / 'missing.tif')]) == 1
    assert not os.path.exists(str(tmp_path / 'no.tif'))


def test_distance_example_runs(tmp_path):
    """examples/batch_distance.c: its own checks (exit status 0: every output of two tiles of the device against its
    brute-force loop over the downloaded layer)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_distance')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_distance.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '3', '150'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr distance: device and brute force agree in every pixel' in r.stdout
    assert '3 tiles of 150 x 150 pixels' in r.stdout
