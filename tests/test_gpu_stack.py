"""The stack entries on the GPU: dswx_stack_device and dswx_batch_stack bit for bit against the numpy statement of the
definition (proteus_amd/stack.py) -- tile lengths either side of the kernel's 16-pixel units and of a block, tile counts
either side of a round of loads, strides and addresses, with every byte outside the output planes checked; contents chosen
against the packed accumulators; every subset of outputs; tile offsets past 2^32; on a caller's stream behind the kernel that
writes the stack; every form of batch; DevicePlane.stack; bin/dswx_stack.py; the C example."""
import importlib.util
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py):
    import torch                                  # loaded second, torch finds no device, and this file must pass on its own too
except ImportError:
    torch = None

from proteus_amd import _capi, geotiff
from proteus_amd.stack import NONE, NO_SHARE, Spec, stack_tiles, wtr_spec
from proteus_amd.synth import SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPT, BLOCK, U = 16, 256, 8                        # of dswx_stack.hip: pixels per thread, threads per block, tiles in flight
PASS = PPT * BLOCK                                # pixels of one block
PAD = 0xA5                                        # every byte of a stack buffer that is not tile data; the specs below COUNT it
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
    return Spec(n_cats, cat, int(rng.integers(0, 256)))


class Run:
    """One call of dswx_stack_device.  The stack lies guard | `off` bytes past a 256-byte boundary | guard in `sbuf`, every
    byte that is not tile data PAD; the wanted outputs lie in `obuf`, the uint16 planes 2 bytes and the byte planes 1 byte
    past a 16-byte boundary, every byte SENT beforehand."""

    def __init__(self, ctx, tiles, n, spec, stride=None, off=0, want=KEYS, sbuf=None, obuf=None):
        self.ctx, self.tiles, self.n, self.spec, self.want = ctx, tiles, n, spec, want
        self.T = len(tiles)
        self.stride = n if stride is None else stride
        span = (self.T - 1) * self.stride + n if self.T else 0          # the last tile's padding need not exist
        self.start = GUARD + off
        self.shost = np.full(self.start + span + GUARD, PAD, dtype=np.uint8)
        for t in range(self.T):
            self.shost[self.start + t * self.stride:self.start + t * self.stride + n] = tiles[t]
        self.sbuf = sbuf if sbuf is not None else ctx.malloc(self.shost.size)
        assert self.sbuf.nbytes >= self.shost.size and self.sbuf.ptr % 256 == 0
        self.sbuf.upload(self.shost)
        self.where, cursor = {}, 0
        for key, eb, planes in (('count', 2, spec.n_cats), ('last_index', 2, 1), ('last', 1, 1), ('share', 1, 1)):
            for k in range(planes):
                begin = -(-cursor // 16) * 16 + eb
                self.where[(key, k)] = (begin, eb)
                cursor = begin + n * eb + 16
        self.osize = cursor + 16
        self.obuf = obuf if obuf is not None else ctx.malloc(self.osize)
        assert self.obuf.nbytes >= self.osize and self.obuf.ptr % 16 == 0
        self.obuf.upload(np.full(self.osize, SENT, dtype=np.uint8))
        at = lambda key, k=0: self.obuf.ptr + self.where[(key, k)][0] if key in want else None
        self.out = _capi.StackOut.of(count=[at('count', k) for k in range(spec.n_cats)] if 'count' in want else (),
                                     last=at('last'), last_index=at('last_index'), share=at('share'))

    def run(self, stream=None):
        self.ctx.stack_device(self.sbuf.ptr + self.start, self.spec, self.T, self.n, self.out,
                              tile_stride=0 if self.stride == self.n else self.stride, stream=stream)

    def check(self, what):
        """The wanted planes are the numpy statement's, every other byte of the output buffer is still SENT, and the stack
        buffer is what was uploaded."""
        ref = stack_tiles(np.asarray(self.tiles, dtype=np.uint8).reshape(self.T, self.n), self.spec)
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for (key, k), (begin, eb) in self.where.items():
            if key not in self.want:
                continue
            got = raw[begin:begin + self.n * eb].copy().view(np.uint16 if eb == 2 else np.uint8)
            want = ref[key][k] if key == 'count' else ref[key]
            assert np.array_equal(got, want), (what, key, k, np.flatnonzero(got != want)[:6], got[:6], want[:6])
            written[begin:begin + self.n * eb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted planes were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.array_equal(self.sbuf.download(np.uint8, self.shost.size), self.shost), (what, 'the stack was written')
        return ref


SIZES = (0, 1, 15, 16, 17, PASS - 1, PASS, PASS + 1, 2 * PASS + 17)


@pytest.mark.parametrize('n_tiles', [0, 1, 2, U - 1, U, U + 1, 2 * U + 1, 255, 256, 257])
def test_device_entry_every_size_count_stride_and_address(ctx, n_tiles):
    """Every n_elems either side of a unit and of a block x this tile count; the stride equal to the tile and above it, the
    padding and the guards full of a byte that is an observation; the stack 0, 1 and 6 bytes past a 256-byte boundary; the
    uint16 outputs 2 and the byte outputs 1 byte past a 16-byte boundary; every byte outside the planes unchanged."""
    rng = np.random.default_rng(8100 + n_tiles)
    big = SIZES[-1]
    sbuf = ctx.malloc(2 * GUARD + 256 + max(n_tiles, 1) * (big + 300))
    obuf = ctx.malloc(7 * (2 * big + 64) + 64)
    cases = 0
    for i, n in enumerate(SIZES):
        spec = random_spec(rng, 1 + (i + n_tiles) % 4)
        tiles = rng.integers(0, 256, size=(n_tiles, n), dtype=np.uint8)
        tiles[tiles == PAD] = PAD - 1
        for j, stride in enumerate((n, n + 3 + 253 * (i & 1))):
            off = (0, 1, 6)[(i + j) % 3]
            r = Run(ctx, tiles, n, spec, stride=stride, off=off, sbuf=sbuf, obuf=obuf)
            r.run()
            ctx.synchronize()
            ref = r.check((n_tiles, n, stride, off, spec.n_cats))
            cases += 1
        if n:
            info = ctx.last_kernel_info()
            assert 'dswx_stack_k' in info and f'block={BLOCK}' in info and f'grid=({-(-(-(-n // PPT)) // BLOCK)},1,1)' in info, info
            assert f'pixels_per_thread={PPT}' in info and f'tiles_in_flight={U}' in info, info
        if n_tiles == 0 and n:
            assert np.all(ref['last'] == spec.fill) and np.all(ref['last_index'] == NONE) and np.all(ref['share'] == NO_SHARE)
    assert cases == 2 * len(SIZES)
    sbuf.free()
    obuf.free()


def contents(n, T):
    """(label, tiles [T, n], spec): stacks chosen against the packed accumulators and the select of the latest observation."""
    i = np.arange(n)
    two = Spec(2, [1, 0] + [255] * 254, 200)                        # byte 0: category 1, byte 1: category 0
    rng = np.random.default_rng(8200)
    out = []
    for v in (0, 1, 77, 255):
        out.append((f'constant {v}', np.full((T, n), v, dtype=np.uint8), two))
    out.append(('two bytes alternating within a unit', np.tile((i & 1).astype(np.uint8), (T, 1)), two))
    out.append(('two bytes alternating across units', np.tile(((i // PPT) & 1).astype(np.uint8), (T, 1)), two))
    out.append(('two bytes alternating across tiles', np.tile((np.arange(T) & 1).astype(np.uint8)[:, None], (1, n)), two))
    every = rng.integers(0, 2, size=(T, n)).astype(np.uint8)
    every[T // 2] = i % 256
    for n_cats in (1, 2, 3, 4):
        out.append((f'all 256 byte values in one tile, {n_cats} categories', every, Spec(n_cats, (np.arange(256) * 7) % 6, 3)))
        out.append((f'noise, {n_cats} categories', rng.integers(0, 256, size=(T, n), dtype=np.uint8),
                    Spec(n_cats, rng.integers(0, 5, size=256), 9)))
    first = np.full((T, n), 255, dtype=np.uint8)
    first[0] = rng.integers(0, 2, size=n)
    out.append(('only tile 0 is an observation', first, two))
    final = np.full((T, n), 255, dtype=np.uint8)
    final[T - 1] = rng.integers(0, 2, size=n)
    out.append(('only the last tile is an observation', final, two))
    return out


def test_contents_that_break_accumulators(ctx):
    n, T = PASS + 4 * PPT + 5, 2 * U + 3
    sbuf = ctx.malloc(2 * GUARD + T * n)
    obuf = ctx.malloc(7 * (2 * n + 64) + 64)
    for label, tiles, spec in contents(n, T):
        r = Run(ctx, tiles, n, spec, sbuf=sbuf, obuf=obuf)
        r.run()
        ctx.synchronize()
        ref = r.check(label)
        if label == 'only tile 0 is an observation':
            assert np.all(ref['last_index'] == 0) and np.array_equal(ref['last'], tiles[0])
        if label == 'only the last tile is an observation':
            assert np.all(ref['last_index'] == T - 1) and np.array_equal(ref['last'], tiles[T - 1])
    sbuf.free()
    obuf.free()


def test_65535_tiles_do_not_carry_between_the_packed_counts(ctx):
    """65535 tiles x 16 pixels, pixels alternating between always category 0 and always category 1: counts of 65535 beside
    counts of 0, last_index 65534, share in {0, 100}; and the four fields of the accumulator all at 65535 side by side."""
    T = 65535
    tiles = np.zeros((T, 16), dtype=np.uint8)
    tiles[:, 1::2] = 1
    r = Run(ctx, tiles, 16, Spec(2, [1, 0] + [255] * 254, 9))
    r.run()
    ctx.synchronize()
    ref = r.check('65535 x 16')
    assert np.all(ref['count'][1, 0::2] == 65535) and np.all(ref['count'][0, 0::2] == 0) and np.all(ref['count'][0, 1::2] == 65535)
    assert np.all(ref['last_index'] == 65534) and set(ref['share'].tolist()) == {0, 100}
    tiles4 = np.tile(np.arange(16, dtype=np.uint8) % 4, (T, 1))
    r4 = Run(ctx, tiles4, 16, Spec(4, [0, 1, 2, 3] + [255] * 252, 9), sbuf=r.sbuf)
    r4.run()
    ctx.synchronize()
    ref = r4.check('65535 x 16, four categories')
    assert all(np.all(ref['count'][k, k::4] == 65535) and int(ref['count'][k].sum()) == 4 * 65535 for k in range(4))
    with pytest.raises(_capi.DswxError, match='65535') as e:
        ctx.stack_device(r.sbuf.ptr, r.spec, 65536, 16, r.out)
    assert e.value.code == _capi.ERR_ARG


@pytest.mark.parametrize('key', KEYS)
def test_each_output_alone(ctx, key):
    rng = np.random.default_rng(8300)
    n, T = PASS + 21, U + 3
    spec = random_spec(rng, 3)
    tiles = rng.integers(0, 256, size=(T, n), dtype=np.uint8)
    r = Run(ctx, tiles, n, spec, stride=n + 5, off=1, want=(key,))
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
        ref = stack_tiles(tiles, spec)
        raw = r.obuf.download(np.uint8, r.osize)
        begin = r.where[('count', 1)][0]
        assert np.array_equal(raw[begin:begin + 2 * n].copy().view(np.uint16), ref['count'][1])
        raw[begin:begin + 2 * n] = SENT
        assert np.all(raw == SENT)


def test_tile_offsets_past_2_32(ctx):
    """5 tiles of 4097 bytes at a stride of 2^30 + 256: the span is allocated, only the tiles are uploaded."""
    rng = np.random.default_rng(8400)
    n, T, stride = 4097, 5, (1 << 30) + 256
    spec = random_spec(rng, 4)
    tiles = rng.integers(0, 256, size=(T, n), dtype=np.uint8)
    sbuf = ctx.malloc((T - 1) * stride + n)
    obuf = ctx.malloc(7 * 2 * n)
    try:
        for t in range(T):
            sbuf.upload(tiles[t], t * stride)
        obuf.upload(np.full(7 * 2 * n, SENT, dtype=np.uint8))
        out = _capi.StackOut.of(count=[obuf.ptr + 2 * n * k for k in range(4)], last_index=obuf.ptr + 8 * n,
                                last=obuf.ptr + 10 * n, share=obuf.ptr + 11 * n)
        ctx.stack_device(sbuf.ptr, spec, T, n, out, tile_stride=stride)
        ctx.synchronize()
        ref = stack_tiles(tiles, spec)
        assert np.array_equal(obuf.download(np.uint16, 4 * n).reshape(4, n), ref['count'])
        assert np.array_equal(obuf.download(np.uint16, n, 8 * n), ref['last_index'])
        assert np.array_equal(obuf.download(np.uint8, n, 10 * n), ref['last'])
        assert np.array_equal(obuf.download(np.uint8, n, 11 * n), ref['share'])
        assert np.all(obuf.download(np.uint8, 2 * n, 12 * n) == SENT)
        assert len(set(ref['last_index'].tolist())) > 2              # the tiles far apart were all read
    finally:
        sbuf.free()
        obuf.free()


def test_on_a_callers_stream_behind_the_kernel_that_writes_the_stack(ctx):
    """Asynchronous on the caller's stream: the stream is held, a copy kernel that REPLACES the stack is queued on it, then the
    entry, with no synchronisation in between.  The entry returns while the hold is pending, and the planes are those of the
    replaced stack -- launched on any other stream it would read the old one."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(8500)
    n, T, stride = 300 * 257, 6, 300 * 257 + 5
    spec = Spec(2, (np.arange(256) % 3), 7)
    old = rng.integers(0, 100, size=T * stride, dtype=np.uint8)
    new = rng.integers(100, 256, size=T * stride, dtype=np.uint8)
    plane = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    share = torch.full((n,), SENT, dtype=torch.uint8, device='cuda:0')
    index = torch.full((n,), 0x1111, dtype=torch.int16, device='cuda:0')
    torch.cuda.synchronize()
    want_old = stack_tiles(np.stack([old[t * stride:t * stride + n] for t in range(T)]), spec)
    want_new = stack_tiles(np.stack([new[t * stride:t * stride + n] for t in range(T)]), spec)
    assert not np.array_equal(want_old['share'], want_new['share'])
    out = _capi.StackOut.of(share=share.data_ptr(), last_index=index.data_ptr())
    s = torch.cuda.Stream(device=0)
    ctx.stack_device(plane.data_ptr(), spec, T, n, out, tile_stride=stride, stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(share.cpu().numpy(), want_old['share'])
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(1.2e9))                       # some hundreds of milliseconds at any shader clock
        held = torch.cuda.Event()
        held.record(s)
        plane.copy_(src)
    t0 = time.perf_counter()
    ctx.stack_device(plane.data_ptr(), spec, T, n, out, tile_stride=stride, stream=s.cuda_stream)
    dt = time.perf_counter() - t0
    assert not held.query(), f'the entry took {dt * 1e3:.1f} ms on the host: it waited for the stream'
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(share.cpu().numpy(), want_new['share'])
    assert np.array_equal(index.cpu().numpy().view(np.uint16), want_new['last_index'])
    assert torch.equal(plane, src)


def download(res, spec, n):
    got = {k: res[k].download(np.uint16 if k in ('count', 'last_index') else np.uint8, n * (spec.n_cats if k == 'count' else 1))
           for k in res}
    if 'count' in got:
        got['count'] = got['count'].reshape(spec.n_cats, n)
    for b in res.values():
        b.free()
    return got


@pytest.mark.parametrize('form', ['packed', 'separate_outputs', 'slide_placed'])
@pytest.mark.parametrize('n_tiles,h,w', [(5, 61, 67), (2, 400, 700)])
def test_batch_stack_on_every_form_of_batch(ctx, form, n_tiles, h, w):
    kw = {'separate_outputs': form == 'separate_outputs', 'sliding_outputs': form == 'slide_placed'}
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, **kw)
    n = h * w
    try:
        batch.synth(SEED, tile0=31)
        p = _capi.default_params()
        if form == 'slide_placed':
            batch.place_slide(p, slack_bytes=24 << 20, step_bytes=2 << 20, spread_gaps=2, refine_passes=1, launches=2,
                              keep_free_bytes=0)
        batch.classify(p)
        bwtr_spec = Spec(2, [1, 0] + [255] * 254, 255)               # BWTR: 1 water, 0 not water
        for name, spec in (('wtr', wtr_spec()), ('wtr', wtr_spec(partial_is_water=False, fill=0)), ('bwtr', bwtr_spec)):
            tiles = np.stack([batch.read_tile(name, t).reshape(-1) for t in range(n_tiles)])
            res = batch.stack(name, spec)                            # same stream as the classification; None = all tiles
            info = ctx.last_kernel_info()
            ctx.synchronize()
            assert info.count('dswx_stack_k') == 1 and f'grid=({-(-(-(-n // PPT)) // BLOCK)},1,1)' in info, info
            got, want = download(res, spec, n), stack_tiles(tiles, spec)
            assert list(got) == list(KEYS)
            for k in KEYS:
                assert np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:4])
            assert int(want['count'].sum()) > 0 and len(np.unique(want['share'])) > 1, name   # the layer is not all fill
            for tile0, count in ((1, n_tiles - 1), (0, 1), (n_tiles - 1, None), (1, _capi.BATCH_ALL_TILES), (n_tiles, None), (0, 0)):
                res = batch.stack(name, spec, tile0=tile0, n_tiles=count, want=('share', 'last_index'))
                ctx.synchronize()
                sub = tiles[tile0:] if count in (None, _capi.BATCH_ALL_TILES) else tiles[tile0:tile0 + count]
                got, want = download(res, spec, n), stack_tiles(sub, spec)
                assert list(got) == ['last_index', 'share']
                for k in got:
                    assert np.array_equal(got[k], want[k]), (name, tile0, count, k)
        # planes that are not uint8, the counters, a plane this batch does not have; tile ranges outside the batch
        for name in ('blue', 'swir2', 'diag'):
            with pytest.raises(_capi.DswxError, match=r'band\[|diag') as e:
                batch.stack(name, wtr_spec())
            assert e.value.code == _capi.ERR_ARG and 'uint8' in str(e.value)
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.stack('counters', wtr_spec())
        assert e.value.code == _capi.ERR_ARG
        for name in ('land', 'browse'):
            with pytest.raises(_capi.DswxError, match=name) as e:
                batch.stack(name, wtr_spec())
            assert e.value.code == _capi.ERR_ARG and 'no plane' in str(e.value)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside the batch'):
                batch.stack('wtr', wtr_spec(), tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(ValueError):
            batch.stack('water', wtr_spec())
    finally:
        batch.free()


def test_device_plane_stack(ctx):
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(8600)
    try:
        a = rng.choice(np.array([0, 1, 2, 252, 253, 254, 255, 9], dtype=np.uint8), size=(4, 100, 130))
        p = eng.upload(a)
        for spec, want_keys in ((wtr_spec(), KEYS), (Spec(3, np.arange(256) % 5, 1), KEYS), (wtr_spec(), ('share',))):
            got = p.stack(spec, want=want_keys)
            want = stack_tiles(a, spec)
            names = ([f'count{k}' for k in range(spec.n_cats)] if 'count' in want_keys else []) + [k for k in KEYS[1:] if k in want_keys]
            assert list(got) == names
            for name, plane in got.items():
                ref = want['count'][int(name[5:])] if name.startswith('count') else want[name]
                assert plane.shape == (100, 130) and plane.dtype == ref.dtype
                assert np.array_equal(plane.numpy(), ref), name
            # each is a plane like any other: counted on the device
            assert np.array_equal(got['share'].histogram(), np.bincount(want['share'].reshape(-1), minlength=256).astype(np.uint64))
            for plane in got.values():
                plane.release()
        p.release()
        with pytest.raises(ValueError):
            eng.upload(np.zeros((4, 4), dtype=np.uint8)).stack(wtr_spec())
        with pytest.raises(ValueError):
            eng.upload(np.zeros((2, 4, 4), dtype=np.uint16)).stack(wtr_spec())
    finally:
        eng.close()


def test_the_command_line_tool(tmp_path, capsys):
    """bin/dswx_stack.py on four 100 x 130 WTR files: every output band is the numpy statement's, every file a valid COG with
    the first input's geo tags, the inputs named in the metadata; a file of another size, or another geotransform, is refused."""
    spec = importlib.util.spec_from_file_location('dswx_stack_tool', os.path.join(ROOT, 'bin', 'dswx_stack.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(8700)
    gt = (600000.0, 30.0, 0.0, 4100040.0, 0.0, -30.0)
    tags = geotiff.geo_tags_from_geotransform(gt, epsg=32611)
    layers = rng.choice(np.array([0, 1, 2, 252, 253, 254, 255], dtype=np.uint8), size=(4, 100, 130), p=[.3, .2, .1, .05, .2, .05, .1])
    files = []
    for k in range(4):
        files.append(str(tmp_path / f'date{k}_WTR.tif'))
        geotiff.write_geotiff(files[-1], layers[k], geo_tags=tags, metadata={'SPACECRAFT_NAME': 'test'}, nodata=255)
    for flags, stack_spec in (([], wtr_spec()), (['--no-partial'], wtr_spec(partial_is_water=False))):
        prefix = str(tmp_path / ('out' + ''.join(flags)))
        assert tool.main(flags + ['-o', prefix] + files) == 0
        want = stack_tiles(layers, stack_spec)
        for suffix, ref, dtype, nodata in (('COUNT_WATER', want['count'][0], np.uint16, None), ('COUNT_LAND', want['count'][1], np.uint16, None),
                                           ('LAST', want['last'], np.uint8, 255), ('LAST_INDEX', want['last_index'], np.uint16, 65535),
                                           ('SHARE', want['share'], np.uint8, 255)):
            path = f'{prefix}_{suffix}.tif'
            arr, info = geotiff.read_geotiff(path)
            assert arr.dtype == dtype and arr.shape == (100, 130) and np.array_equal(arr, ref), suffix
            assert geotiff.validate_cog(path) == [], suffix
            assert tuple(info.geotransform) == gt and info.nodata == nodata, (suffix, info.geotransform, info.nodata)
            assert info.metadata['STACK_INPUT_FILES'] == ', '.join(os.path.basename(f) for f in files)
            assert info.metadata['SPACECRAFT_NAME'] == 'test'
            assert (info.colormap is not None) == (suffix == 'LAST')
    capsys.readouterr()
    other = str(tmp_path / 'other_size.tif')
    geotiff.write_geotiff(other, layers[0][:, :129], geo_tags=tags, nodata=255)
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], other]) == 1
    text = capsys.readouterr().out
    assert '[FAIL] Comparing size' in text and '130 x 100' in text and '129 x 100' in text
    moved = str(tmp_path / 'moved.tif')
    geotiff.write_geotiff(moved, layers[0], geo_tags=geotiff.geo_tags_from_geotransform((600030.0,) + gt[1:], epsg=32611), nodata=255)
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], files[1], moved]) == 1
    text = capsys.readouterr().out
    assert '[FAIL] Comparing geotransform' in text and 'differs from input 3 geotransform' in text
    assert not os.path.exists(str(tmp_path / 'no_SHARE.tif'))
    assert tool.main(['-o', str(tmp_path / 'no'), '--band', '2'] + files) == 1


def test_stack_example_runs(tmp_path):
    """examples/batch_stack.c: its own checks (exit status 0: every pixel of the five device planes against its loop and
    against dswx_stack_host)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_stack')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_stack.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '5', '301'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr stack: device, loop and host entry agree in every pixel' in r.stdout
    assert '5 tiles of 90601 pixels' in r.stdout
