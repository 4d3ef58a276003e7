"""The histogram entries on the GPU: dswx_histogram_device and dswx_batch_histogram bit for bit against the numpy statement
of the definition (proteus_amd/histogram.py) -- every kind, tile lengths either side of the kernel's 16-byte units, of an
unrolled round and of a block's chunk, tile counts, strides and plane addresses; contents chosen against the accumulator
(constant planes, two values, every value, runs, noise); a tile of more than 2^32 elements; more tiles than one launch takes, every kind; on a caller's stream behind
the kernel that writes the plane; every form of batch; DevicePlane.histogram; the C example."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from oracle import dswx_oracle as o
from proteus_amd import _capi
from proteus_amd.histogram import BINS, DTYPES, HIST_DIAG, HIST_I16, HIST_U16, HIST_U8, bin_of, histogram, histogram_tiles
from proteus_amd.synth import SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, UNROLL, MAX_PASSES = 256, 4, 64            # of dswx_histogram.hip: threads, loads in flight, passes of a block's largest chunk
PAD = 0xA5                                        # every byte that is not tile data; as an element it is counted by every BINNING below
# (kind, lo, shift): the linear kinds with a range that holds the padding element 0xA5A5 (42405 / -23131), so that a kernel
# that read the padding would count it
BINNINGS = {'u8': (HIST_U8, 0, 0), 'u16': (HIST_U16, 40000, 4), 'i16': (HIST_I16, -32768, 7), 'diag': (HIST_DIAG, 0, 0)}
PATTERNS = o.get_binary_representation(np.arange(32, dtype=np.uint16))
SENT_OUT = 0x1111111111111111


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def tile_data(rng, name, n):
    """n elements of the kind's dtype: over the whole domain and around the counted range, never the padding element."""
    kind, lo, shift = BINNINGS[name]
    dt = DTYPES[kind]
    if kind == HIST_U8:
        a = rng.integers(0, 256, size=n).astype(dt)
    elif kind == HIST_DIAG:
        a = np.where(rng.random(n) < 0.8, PATTERNS[rng.integers(0, 32, size=n)],
                     np.where(rng.random(n) < 0.5, 65535, rng.integers(0, 65536, size=n))).astype(dt)
    else:
        info = np.iinfo(dt)
        near = np.clip(rng.integers(lo - 64, lo + (256 << shift) + 64, size=n), info.min, info.max)
        a = np.where(rng.random(n) < 0.7, near, rng.integers(info.min, info.max + 1, size=n)).astype(dt)
    pad = np.array([PAD, PAD], dtype=np.uint8).view(dt)[0] if dt.itemsize == 2 else dt.type(PAD)
    a[a == pad] = pad - 1
    return a


class Plane:
    """A device buffer holding guard | plane at byte offset `off` past a 256-byte boundary | guard, every byte that is not
    tile data PAD; the records follow, prefilled with a sentinel.  `tiles` are the host copies the expected counts come from."""
    GUARD = 512

    def __init__(self, ctx, name, tiles, stride, off, buf=None):
        self.ctx, self.name, self.tiles, self.stride, self.off = ctx, name, tiles, stride, off
        self.kind, self.lo, self.shift = BINNINGS[name]
        self.eb = DTYPES[self.kind].itemsize
        self.n, self.n_tiles = (len(tiles[0]) if tiles else 0), len(tiles)
        span = ((self.n_tiles - 1) * stride + self.n) * self.eb if self.n_tiles else 0       # the last tile's padding need not exist
        self.start = self.GUARD + off
        self.nbytes = self.start + span + self.GUARD
        host = np.full(self.nbytes, PAD, dtype=np.uint8)
        for t, data in enumerate(tiles):
            a = self.start + t * stride * self.eb
            host[a:a + self.n * self.eb] = data.view(np.uint8)
        self.host = host
        self.out_off = -(-self.nbytes // 256) * 256
        need = self.out_off + 8 * BINS * max(self.n_tiles, 1)
        self.buf = buf if buf is not None else ctx.malloc(need)
        assert self.buf.nbytes >= need and self.buf.ptr % 256 == 0
        self.buf.upload(host)
        self.buf.upload(np.full(BINS * max(self.n_tiles, 1), SENT_OUT, dtype=np.uint64), self.out_off)

    def run(self, stream=None):
        self.ctx.histogram_device(self.buf.ptr + self.start, self.kind, self.n_tiles, self.n, self.buf.ptr + self.out_off,
                                  lo=self.lo, shift=self.shift, tile_stride=self.stride, stream=stream)

    def result(self):
        return self.buf.download(np.uint64, BINS * self.n_tiles, self.out_off).reshape(self.n_tiles, BINS)

    def expected(self):
        return histogram_tiles(self.tiles, self.kind, self.lo, self.shift)


def unit_elems(name):
    return 16 // DTYPES[BINNINGS[name][0]].itemsize


@pytest.mark.parametrize('name', list(BINNINGS))
def test_device_entry_every_size_count_stride_and_address(ctx, name):
    """Tile lengths around the 16-byte unit, the 4 KiB pass, one unrolled round of a block (+- 1) and a block's largest chunk
    + 17 bytes (several blocks flush into one record); 1 and 3 tiles; the stride equal to the tile and above it, the padding
    full of an element that would be counted; the plane at its address, one element on and 6 bytes on."""
    rng = np.random.default_rng(7100 + len(name))
    epu = unit_elems(name)
    eb = 16 // epu
    one_round = UNROLL * BLOCK * epu
    chunk = MAX_PASSES * BLOCK * epu
    sizes = [0, 1, 15, 16, 17, 4095, 4096, 4097, one_round - 1, one_round, one_round + 1, chunk + -(-17 // eb)]
    buf = ctx.malloc(2 * Plane.GUARD + 256 + 3 * (sizes[-1] + 300) * eb + 8 * BINS * 3 + 512)
    cases = 0
    for n in sizes:
        for n_tiles in (1, 3):
            tiles = [tile_data(rng, name, n) for _ in range(n_tiles)]
            for stride, off in ((n, 0), (n + 3, eb), (-(-(n + 1) // 256) * 256, 6), (n + 1, 0)):
                p = Plane(ctx, name, tiles, stride, off, buf=buf)
                p.run()
                ctx.synchronize()
                got, want = p.result(), p.expected()
                assert np.array_equal(got, want), (name, n, n_tiles, stride, off, np.argwhere(got != want)[:4])
                cases += 1
        if n:
            assert 'dswx_histogram_k' in ctx.last_kernel_info() and f'block={BLOCK}' in ctx.last_kernel_info()
    assert cases == len(sizes) * 2 * 4
    # what is counted is what is in range: U8 and DIAG count every element
    if name in ('u8', 'diag'):
        assert int(got.sum()) == 3 * sizes[-1]
    if name == 'u8':                                          # a byte plane at address + 1 byte is the + 1 element case above
        assert eb == 1
    else:                                                     # a 16-bit plane one byte off its elements is refused
        with pytest.raises(_capi.DswxError) as e:
            ctx.histogram_device(buf.ptr + 1, BINNINGS[name][0], 1, 16, buf.ptr + 4096)
        assert e.value.code == _capi.ERR_ALIGN
    buf.free()


def contents(n):
    """Byte-valued contents (int64 0 .. 255) chosen against a private accumulator."""
    rng = np.random.default_rng(7200)
    i = np.arange(n)
    return {'constant 0': np.zeros(n, dtype=np.int64), 'constant 255': np.full(n, 255), 'constant 0x80': np.full(n, 0x80),
            'two values alternating': np.where(i & 1, 3, 200), 'every value equally often': i % 256,
            'every value in runs of 16': (i // 16) % 256, 'ramp with runs of 1000': (i // 1000) % 256,
            'one value nine times in ten': np.where(rng.random(n) < 0.9, 1, rng.integers(0, 256, size=n))}


@pytest.mark.parametrize('name', list(BINNINGS))
def test_contents_that_break_accumulators(ctx, name):
    """One tile of 2^20 + 5 elements: what makes the lanes of a wave meet in one counter, or never."""
    n = (1 << 20) + 5
    kind = BINNINGS[name][0]
    # the byte-valued content as elements of the kind, and a binning under which bin = the byte (DIAG: the byte mod 34)
    diag_values = np.concatenate([PATTERNS, [65535, 2]]).astype(np.uint16)
    as_kind = {'u8': (lambda c: c.astype(np.uint8), 0, 0), 'u16': (lambda c: (c * 64 + 17).astype(np.uint16), 0, 6),
               'i16': (lambda c: ((c - 128) * 64 + 63).astype(np.int16), -8192, 6),
               'diag': (lambda c: diag_values[c % 34], 0, 0)}[name]
    buf = ctx.malloc(n * 2 + 256 + 8 * BINS)
    out_off = -(-n * 2 // 256) * 256
    for label, c in contents(n).items():
        a = as_kind[0](c)
        buf.upload(a)
        buf.upload(np.full(BINS, SENT_OUT, dtype=np.uint64), out_off)
        ctx.histogram_device(buf.ptr, kind, 1, n, buf.ptr + out_off, lo=as_kind[1], shift=as_kind[2])
        ctx.synchronize()
        got = buf.download(np.uint64, BINS, out_off)
        want = histogram(a, kind, as_kind[1], as_kind[2])
        assert np.array_equal(got, want), (name, label, np.flatnonzero(got != want)[:8])
        assert int(got.sum()) == n, (name, label)
        if name != 'diag':
            assert np.array_equal(got, np.bincount(c, minlength=BINS).astype(np.uint64)), (name, label)
    buf.free()


def test_noise_like_planes_of_synth(ctx):
    """The generated input planes of one tile of 2^20 + 5 pixels (2367 x 443): bands linearly, Fmask by the byte, through the
    device entry on the batch's own planes and through the batch entry."""
    h, w = 2367, 443
    n = h * w
    assert n == (1 << 20) + 5
    batch = _capi.DeviceBatch(ctx, 1, h, w)
    out = ctx.malloc(8 * BINS)
    try:
        batch.synth(SEED, tile0=3)
        batch.classify(_capi.default_params())
        both = batch.histogram(band_lo=-512, band_shift=5)
        for name in batch.plane_names():
            ptr, dt = batch._plane(name)
            kind, lo, shift = (HIST_DIAG, 0, 0) if name == 'diag' else (HIST_I16, -512, 5) if dt == np.int16 else (HIST_U8, 0, 0)
            ctx.histogram_device(ptr, kind, 1, n, out.ptr, lo=lo, shift=shift)
            ctx.synchronize()
            want = histogram(batch.read_tile(name, 0), kind, lo, shift)
            assert np.array_equal(out.download(np.uint64, BINS), want), name
            assert np.array_equal(both[name][0], want), name
            if dt == np.int16:
                assert np.count_nonzero(want) > 8, name                        # noise: many bins
    finally:
        out.free()
        batch.free()


def test_a_tile_of_more_than_2_32_elements(ctx):
    """One byte plane of 2^32 + 4096 elements set with a memset, three bytes changed: as one tile (a block's largest chunk,
    16385 blocks into one record, a count past 2^32) and as two tiles of half the size."""
    n = (1 << 32) + 4096
    value, other = 0x5A, 7
    buf = ctx.malloc(n + 2 * 8 * BINS)
    try:
        _capi._check(ctx.lib.dswx_memset_d(ctx.handle, buf.ptr, value, n))
        changed = (0, (1 << 32) - 1, n - 1)
        for i in changed:
            buf.upload(np.array([other], dtype=np.uint8), i)
        ctx.histogram_device(buf.ptr, HIST_U8, 1, n, buf.ptr + n)
        ctx.synchronize()
        assert f'passes={MAX_PASSES}' in ctx.last_kernel_info() and 'grid=(16385,1,1)' in ctx.last_kernel_info(), ctx.last_kernel_info()
        got = buf.download(np.uint64, BINS, n)
        want = np.zeros(BINS, dtype=np.uint64)
        want[value], want[other] = n - 3, 3
        assert np.array_equal(got, want), (int(got[value]), int(got[other]))
        ctx.histogram_device(buf.ptr, HIST_U8, 2, n // 2, buf.ptr + n)
        ctx.synchronize()
        assert f'passes={MAX_PASSES}' in ctx.last_kernel_info() and 'grid=(8193,2,1)' in ctx.last_kernel_info(), ctx.last_kernel_info()
        got = buf.download(np.uint64, 2 * BINS, n).reshape(2, BINS)
        want = np.zeros((2, BINS), dtype=np.uint64)
        want[0, value], want[0, other], want[1, value], want[1, other] = n // 2 - 1, 1, n // 2 - 2, 2
        assert np.array_equal(got, want)
    finally:
        buf.free()


def test_65537_one_element_tiles_cross_the_launch_split(ctx):
    T = 65537
    rng = np.random.default_rng(7300)
    a = rng.integers(0, 256, size=T).astype(np.uint8)
    host = np.full((T, 3), PAD, dtype=np.uint8)
    host[:, 0] = a
    buf = ctx.malloc(host.nbytes + 256 + 8 * BINS * T)
    out_off = -(-host.nbytes // 256) * 256
    buf.upload(host)
    ctx.histogram_device(buf.ptr, HIST_U8, T, 1, buf.ptr + out_off, tile_stride=3)
    ctx.synchronize()
    got = buf.download(np.uint64, BINS * T, out_off).reshape(T, BINS)
    want = np.zeros((T, BINS), dtype=np.uint64)
    want[np.arange(T), a] = 1
    assert np.array_equal(got, want)
    buf.free()


@pytest.fixture(scope='module')
def split_buffer(ctx):
    """One buffer for the four calls of the test below (their records alone are 134 MB)."""
    T, n = 65535 + 4, 17
    buf = ctx.malloc(2 * Plane.GUARD + 512 + T * (n + 3) * 2 + 8 * BINS * T + 4096)
    yield buf
    buf.free()


@pytest.mark.parametrize('name', list(BINNINGS))
def test_more_tiles_than_one_launch_takes_every_kind(ctx, split_buffer, name):
    """65535 + 4 tiles of 17 elements (one 16-byte unit and a tail for the byte kind, two units and a tail for the others),
    the stride 3 above the tile, the plane one element past a 256-byte boundary, the linear kinds with a non-zero lo and
    shift: the second launch starts at tile 65535.  Random elements, so that a tile read one stride off or a record written
    one slot off differs: EVERY record against the numpy statement (a few also against the library's scalar entry), and every
    other byte of the buffer -- guards, padding, tiles, the bytes behind the records -- as it was."""
    rng = np.random.default_rng(7350 + len(name))
    T, n = 65535 + 4, 17
    kind, lo, shift = BINNINGS[name]
    assert name in ('u8', 'diag') or (lo != 0 and shift != 0)
    tiles = tile_data(rng, name, T * n).reshape(T, n)
    bins = bin_of(tiles, kind, lo, shift)
    flat = (bins + np.arange(T)[:, None] * BINS)[bins >= 0]
    want = np.bincount(flat, minlength=T * BINS).astype(np.uint64).reshape(T, BINS)
    for t in (0, 1, 65534, 65535, 65536, T - 1):
        assert np.array_equal(want[t], histogram(tiles[t], kind, lo, shift)) and np.array_equal(want[t], _capi.histogram_host(tiles[t], kind, lo, shift))
    eb = tiles.dtype.itemsize
    p = Plane(ctx, name, list(tiles), n + 3, eb, buf=split_buffer)
    behind = p.out_off + 8 * BINS * T
    split_buffer.upload(np.full(split_buffer.nbytes - behind, PAD, dtype=np.uint8), behind)
    split_buffer.upload(np.full(p.out_off - p.nbytes + 8, PAD, dtype=np.uint8), p.nbytes - 8)
    p.run()
    ctx.synchronize()
    assert ',65535,1)' in ctx.last_kernel_info(), ctx.last_kernel_info()
    got = p.result()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, bad[:4], got[tuple(bad[:4].T)], want[tuple(bad[:4].T)])
    assert np.array_equal(split_buffer.download(np.uint8, p.nbytes), p.host), 'the plane was written'
    assert np.all(split_buffer.download(np.uint8, p.out_off - p.nbytes + 8, p.nbytes - 8) == PAD)
    assert np.all(split_buffer.download(np.uint8, split_buffer.nbytes - behind, behind) == PAD), 'bytes behind the records were written'


def test_on_a_callers_stream_behind_the_kernel_that_writes_the_plane(ctx):
    """Asynchronous on the caller's stream: the stream is held, a copy kernel that REPLACES the plane is queued on it, then
    the entry, with no synchronisation in between.  The entry returns while the hold is pending, and the counts are those
    of the replaced plane -- launched on any other stream it would read the old one."""
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(7400)
    n, n_tiles, stride = 300 * 257, 6, 300 * 257 + 5
    old = rng.integers(0, 100, size=n_tiles * stride, dtype=np.uint8)
    new = rng.integers(100, 256, size=n_tiles * stride, dtype=np.uint8)
    plane = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    out = torch.full((n_tiles, BINS), 0x1111, dtype=torch.int64, device='cuda:0')
    torch.cuda.synchronize()
    want_old = histogram_tiles([old[t * stride:t * stride + n] for t in range(n_tiles)])
    want_new = histogram_tiles([new[t * stride:t * stride + n] for t in range(n_tiles)])
    s = torch.cuda.Stream(device=0)
    ctx.histogram_device(plane.data_ptr(), HIST_U8, n_tiles, n, out.data_ptr(), tile_stride=stride, stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want_old)
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(1.2e9))                       # some hundreds of milliseconds at any shader clock
        held = torch.cuda.Event()
        held.record(s)
        plane.copy_(src)
    t0 = time.perf_counter()
    ctx.histogram_device(plane.data_ptr(), HIST_U8, n_tiles, n, out.data_ptr(), tile_stride=stride, stream=s.cuda_stream)
    dt = time.perf_counter() - t0
    assert not held.query(), f'the entry took {dt * 1e3:.1f} ms on the host: it waited for the stream'
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want_new)
    assert torch.equal(plane, src)


def _kind_of_plane(name, band_lo, band_shift):
    return (HIST_DIAG, 0, 0) if name == 'diag' else (HIST_I16, band_lo, band_shift) if name in _capi.BAND_NAMES else (HIST_U8, 0, 0)


@pytest.mark.parametrize('form', ['packed', 'separate_outputs', 'slide_placed'])
@pytest.mark.parametrize('masks,extra', [(False, ()), (True, ('wtr1_aerosol',)), (True, ('wtr1_aerosol', 'browse'))],
                         ids=['plain', 'masks_aerosol', 'masks_all_layers'])
@pytest.mark.parametrize('tile_align', [256, 1])
@pytest.mark.parametrize('n_tiles,h,w', [(5, 61, 67), (2, 400, 700)])
def test_batch_histogram_on_every_form_of_batch(ctx, form, masks, extra, tile_align, n_tiles, h, w):
    kw = {'separate_outputs': form == 'separate_outputs', 'sliding_outputs': form == 'slide_placed'}
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, masks=masks, extra_layers=extra, tile_align=tile_align, **kw)
    try:
        batch.synth(SEED, tile0=31)
        p = _capi.default_params()
        if form == 'slide_placed':
            batch.place_slide(p, slack_bytes=24 << 20, step_bytes=2 << 20, spread_gaps=2, refine_passes=1, launches=2,
                              keep_free_bytes=0)
        batch.classify(p)
        names = batch.plane_names()
        assert len(names) == 7 + (3 if masks else 0) + 7 + len(extra)
        hist = batch.histogram()                              # same stream as the classification; None = DSWX_BATCH_ALL_TILES
        info = ctx.last_kernel_info()
        assert info.count('dswx_histogram_k') == 1 and f',{n_tiles},{len(names)})' in info, info     # ONE launch, all planes
        assert list(hist) == names
        for name in names:
            kind, lo, shift = _kind_of_plane(name, 0, 6)
            assert hist[name].shape == (n_tiles, BINS) and hist[name].dtype == np.uint64
            for t in range(n_tiles):
                want = histogram(batch.read_tile(name, t), kind, lo, shift)
                assert np.array_equal(hist[name][t], want), (name, t, np.flatnonzero(hist[name][t] != want)[:8])
            if kind != HIST_I16:
                assert np.all(hist[name].sum(axis=1) == h * w), name
        assert np.count_nonzero(hist['diag'][:, 34:]) == 0 and np.count_nonzero(hist['diag'][:, 33]) == 0
        # a few planes, from tile0 > 0, the bands binned otherwise
        some = ['wtr', 'nir', 'diag'] + (['ocean'] if masks else [])
        part = batch.histogram(names=some, tile0=1, n_tiles=n_tiles - 1, band_lo=-100, band_shift=3)
        assert list(part) == sorted(some, key=_capi.PLANE_INDEX.get)
        for name in some:
            assert part[name].shape == (n_tiles - 1, BINS)
            if name == 'nir':
                want = histogram_tiles([batch.read_tile(name, t) for t in range(1, n_tiles)], HIST_I16, -100, 3)
                assert np.array_equal(part[name], want)
            else:
                assert np.array_equal(part[name], hist[name][1:]), name
        assert np.array_equal(batch.histogram(names=['cloud'], tile0=n_tiles - 1)['cloud'], hist['cloud'][n_tiles - 1:])
        assert np.array_equal(batch.histogram(names=['cloud'], tile0=0, n_tiles=_capi.BATCH_ALL_TILES)['cloud'], hist['cloud'])
        assert batch.histogram(names=['cloud'], tile0=n_tiles)['cloud'].shape == (0, BINS)
        # planes this batch does not have; the counters
        for name in [v for v in ('land', 'wtr1_aerosol', 'browse') if v not in names]:
            with pytest.raises(_capi.DswxError, match=name) as e:
                batch.histogram(names=['wtr', name])
            assert e.value.code == _capi.ERR_ARG
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.histogram(names=['wtr', 'counters'])
        assert e.value.code == _capi.ERR_ARG
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError):
                batch.histogram(names=['wtr'], tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(_capi.DswxError, match='shift'):
            batch.histogram(names=['wtr'], band_shift=9)
    finally:
        batch.free()


def test_device_plane_histogram_of_the_product_run(ctx):
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(7500)
    try:
        for a, kw in ((rng.integers(0, 256, size=(211, 97)).astype(np.uint8), {}),
                      ((rng.normal(size=(211, 97)) * 3000).astype(np.int16), {'lo': -4000, 'shift': 5}),
                      (rng.integers(0, 65536, size=(97, 211)).astype(np.uint16), {'lo': 1, 'shift': 8}),
                      (PATTERNS[rng.integers(0, 32, size=(211, 97))], {'kind': HIST_DIAG})):
            p = eng.upload(a)
            got = p.histogram(**kw)
            assert got.dtype == np.uint64 and np.array_equal(got, histogram(a, **kw)), (a.dtype, kw)
            p.release()
        with pytest.raises(ValueError):
            eng.upload(np.zeros((4, 4), dtype=np.float32)).histogram()
    finally:
        eng.close()


def test_histogram_example_runs(tmp_path):
    """examples/batch_histogram.c: its own checks (exit status 0: every WTR bin of the device against its loop and against
    dswx_histogram_host, the DIAG bins sum to the pixels), and the WTR classes it prints against the same batch made here."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_histogram')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_histogram.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    n_tiles, size = 3, 301
    r = subprocess.run([exe, str(n_tiles), str(size)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr: device, loop and host entry agree in every bin' in r.stdout
    c = _capi.Context(0)
    batch = _capi.DeviceBatch(c, n_tiles, size, size)
    try:
        batch.synth(20251010)
        batch.classify(_capi.default_params())
        for t in range(n_tiles):
            want = histogram(batch.read_tile('wtr', t))
            line = 'tile %d: wtr classes' % t + ''.join(' %d:%d' % (b, want[b]) for b in np.flatnonzero(want))
            assert line in r.stdout.splitlines(), (line, r.stdout[-1500:])
    finally:
        batch.free()
        c.close()
