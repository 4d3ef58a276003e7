"""The checksum entries of ABI v7 on the GPU: dswx_checksum_device and dswx_batch_checksum against the numpy statement of
the definition (proteus_amd/checksum.py) on downloaded copies -- every element size, tile lengths either side of the
kernel's 16-byte units and 4 KiB passes, tile counts (also past the 65535 of one launch), strides and plane addresses; on a caller's stream behind the
kernel that writes the plane; the batch forms; and the two headline batches with EVERY tile checked against the C oracle
through the checksums (tests/test_gpu_parity.py compares 5 of 256 and 3 of 512 tiles byte by byte)."""
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import c_oracle
from proteus_amd import _capi
from proteus_amd.checksum import checksum, checksum_tiles
from proteus_amd.synth import SEED

pytestmark = pytest.mark.gpu

SENT = 0xA5
N_ELEMS = (0, 1, 7, 8, 9, 63, 64, 65, 4095, 4097, 3660 * 3659, 3660 * 3660)
N_TILES = (1, 2, 16, 17, 64)


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def _stride(kind, n):
    """Tile strides in elements: the tile itself, padded to 256, and odd."""
    return {'n': n, 'pad256': -(-n // 256) * 256 if n else 256, 'odd': (n + 3) | 1}[kind]


class Plane:
    """A device buffer holding guard | plane at byte offset `off` past a 256-byte boundary | guard, every byte that is
    not tile data the sentinel; `tiles` are the host copies the expected values come from."""
    GUARD = 512

    def __init__(self, ctx, rng, eb, n, n_tiles, stride, off, sentinel=SENT, buf=None, values=256, tiles=None):
        self.ctx, self.eb, self.n, self.n_tiles, self.stride, self.off = ctx, eb, n, n_tiles, stride, off
        span = ((n_tiles - 1) * stride + n) * eb if n_tiles else 0           # the last tile's padding need not exist
        self.nbytes = self.GUARD + off + span + self.GUARD
        self.host = np.full(self.nbytes, sentinel, dtype=np.uint8)
        self.start = self.GUARD + off
        if tiles is not None:                             # the bytes of every tile, uint8 [n_tiles, n * eb], placed in one step
            assert tiles.shape == (n_tiles, n * eb) and tiles.dtype == np.uint8 and n_tiles > 0
            rows = np.lib.stride_tricks.as_strided(self.host[self.start:], shape=tiles.shape, strides=(stride * eb, 1))
            rows[...] = tiles
            self.tiles = tiles
        else:
            self.tiles = []
        for t in range(n_tiles if tiles is None else 0):
            data = rng.integers(0, values, size=n * eb, dtype=np.uint8)
            a = self.start + t * stride * eb
            self.host[a:a + n * eb] = data
            self.tiles.append(data)
        self.buf = buf if buf is not None else ctx.malloc(self.nbytes + 8 * max(n_tiles, 1) + 256)
        assert self.buf.nbytes >= self.nbytes + 8 * n_tiles + 256 and self.buf.ptr % 256 == 0
        self.buf.upload(self.host)
        self.out_off = -(-self.nbytes // 256) * 256
        self.buf.upload(np.full(max(n_tiles, 1), 0x1111111111111111, dtype=np.uint64), self.out_off)

    def run(self, stream=None):
        self.ctx.checksum_device(self.buf.ptr + self.start, self.eb, self.n_tiles, self.n, self.buf.ptr + self.out_off,
                                 tile_stride=self.stride, stream=stream)

    def result(self):
        return self.buf.download(np.uint64, self.n_tiles, self.out_off)

    def expected(self):
        return np.array([checksum(d) for d in self.tiles], dtype=np.uint64)

    def assert_untouched(self):
        """The kernel only reads: guards, padding between tiles and the tiles themselves are what was uploaded."""
        assert np.array_equal(self.buf.download(np.uint8, self.nbytes), self.host)


def test_device_entry_small_tiles_every_size_count_stride_and_address(ctx):
    """The full product of element sizes, the tile lengths up to 4097 elements, tile counts, the three strides and every
    plane address from 0 to 15 bytes past a 256-byte boundary that the element size allows."""
    rng = np.random.default_rng(9001)
    buf = ctx.malloc(2 * Plane.GUARD + 16 + 64 * (4097 + 256) * 8 + 8 * 64 + 512)
    cases = 0
    for eb in (1, 2, 4, 8):
        for n in [v for v in N_ELEMS if v <= 4097]:
            for n_tiles in N_TILES:
                for kind in ('n', 'pad256', 'odd'):
                    for off in range(0, 16, eb):
                        p = Plane(ctx, rng, eb, n, n_tiles, _stride(kind, n), off, buf=buf)
                        p.run()
                        ctx.synchronize()
                        got, want = p.result(), p.expected()
                        assert np.array_equal(got, want), (eb, n, n_tiles, kind, off, got[:4], want[:4])
                        if cases % 16 == 0:
                            p.assert_untouched()
                            # the same tiles under another sentinel: what lies between and around them does not count
                            q = Plane(ctx, np.random.default_rng(1), eb, n, n_tiles, p.stride, off, sentinel=0x3C, buf=buf)
                            r = Plane(ctx, np.random.default_rng(1), eb, n, n_tiles, p.stride, off, sentinel=0xC3, buf=buf)
                            q.run()
                            ctx.synchronize()
                            got_q = q.result()
                            r.run()
                            ctx.synchronize()
                            assert np.array_equal(got_q, r.result()) and np.array_equal(got_q, q.expected())
                        cases += 1
    assert cases == (16 + 8 + 4 + 2) * 10 * 5 * 3
    assert 'dswx_checksum_k' in ctx.last_kernel_info()
    buf.free()


@pytest.mark.parametrize('n', [3660 * 3659, 3660 * 3660])
def test_device_entry_full_size_tiles(ctx, n):
    """Tiles of the product's own size (3660 x 3660 = 144 mod 256 elements; 3660 x 3659 is odd in units of 4): every
    element size, stride and tile count, the plane at addresses that exercise the unaligned 16-byte loads."""
    rng = np.random.default_rng(9002 + n % 7)
    cases = 0
    for eb, tile_counts in ((1, N_TILES), (2, (1, 2, 17)), (4, (1, 2)), (8, (1, 2))):
        buf = ctx.malloc(2 * Plane.GUARD + 16 + max(tile_counts) * (n + 256) * eb + 8 * 64 + 512)
        for n_tiles in tile_counts:
            for kind in ('n', 'pad256', 'odd'):
                offs = [o for o in (0, 1, 2, 4, 8, 15 // eb * eb) if o % eb == 0]
                off = offs[cases % len(offs)]
                p = Plane(ctx, rng, eb, n, n_tiles, _stride(kind, n), off, buf=buf, values=5)
                p.run()
                ctx.synchronize()
                got, want = p.result(), p.expected()
                assert np.array_equal(got, want), (eb, n, n_tiles, kind, off)
                if n_tiles <= 2:
                    p.assert_untouched()
                cases += 1
        buf.free()
    assert cases == (5 + 3 + 2 + 2) * 3


def test_every_plane_address_at_full_size(ctx):
    """One full-size tile at every byte offset 0 .. 15 that its element size allows."""
    rng = np.random.default_rng(9003)
    n = 3660 * 3660
    for eb in (1, 2, 4, 8):
        buf = ctx.malloc(2 * Plane.GUARD + 16 + 2 * (n + 256) * eb + 1024)
        for off in range(0, 16, eb):
            p = Plane(ctx, rng, eb, n // eb, 2, _stride('odd', n // eb), off, buf=buf)
            p.run()
            ctx.synchronize()
            assert np.array_equal(p.result(), p.expected()), (eb, off)
        buf.free()


SPLIT = 65535                                             # the blocks of grid.y: one launch takes this many tiles


@pytest.mark.parametrize('eb', [1, 2, 4, 8])
def test_more_tiles_than_one_launch_takes(ctx, eb):
    """Tile counts either side of the 65535 tiles of one launch and past two launches (65535, 65536, 65535 + 4, 2 x 65535 + 1:
    a third launch), tiles of 1 element (a tail only) and of 17 (one 16-byte unit and a tail with eb 1), the stride equal
    to the tile and 3 above it, the plane one element past a 256-byte boundary.  Random bytes, so that a tile read one
    stride off or a word written one slot off differs: EVERY checksum against the numpy statement (a few of them also
    against the library's scalar entry), and every other byte of the buffer -- guards, padding, tiles, the words around the
    table -- as it was."""
    rng = np.random.default_rng(9010 + eb)
    counts = (SPLIT, SPLIT + 1, SPLIT + 4, 2 * SPLIT + 1)
    tail = 64                                                                  # sentinel words behind the table
    buf = ctx.malloc(2 * Plane.GUARD + 256 + max(counts) * (17 + 3) * eb + 256 + 8 * (max(counts) + tail))
    cases = 0
    for n in (1, 17):
        pool = rng.integers(0, 256, size=(max(counts), n * eb), dtype=np.uint8)
        sums = checksum_tiles(pool)
        for k in (0, 1, SPLIT - 1, SPLIT, SPLIT + 1, 2 * SPLIT, len(pool) - 1):
            assert int(sums[k]) == _capi.checksum_host(pool[k]) == checksum(pool[k])
        for n_tiles in counts:
            for stride in (n, n + 3):
                p = Plane(ctx, rng, eb, n, n_tiles, stride, eb, buf=buf, tiles=pool[:n_tiles])
                words = n_tiles + tail
                buf.upload(np.full(words, 0x1111111111111111, dtype=np.uint64), p.out_off)
                buf.upload(np.full(p.out_off - p.nbytes + 8, SENT, dtype=np.uint8), p.nbytes - 8)
                p.run()
                ctx.synchronize()
                assert f',{SPLIT},1)' in ctx.last_kernel_info(), ctx.last_kernel_info()
                got = buf.download(np.uint64, words, p.out_off)
                bad = np.flatnonzero(got[:n_tiles] != sums[:n_tiles])
                assert bad.size == 0, (eb, n, n_tiles, stride, bad[:4], got[bad[:4]], sums[bad[:4]])
                assert np.all(got[n_tiles:] == 0x1111111111111111), (eb, n, n_tiles, stride, 'words behind the table were written')
                p.assert_untouched()
                assert np.all(buf.download(np.uint8, p.out_off - p.nbytes + 8, p.nbytes - 8) == SENT)     # (up to the table)
                cases += 1
    assert cases == 2 * 4 * 2
    buf.free()


def test_on_a_callers_stream_behind_the_kernel_that_writes_the_plane(ctx):
    """Asynchronous on the caller's stream: the stream is held, a copy kernel that REPLACES the plane is queued on it, then
    the entry, with no synchronisation in between.  The entry returns while the hold is pending, and the checksums are
    those of the replaced plane -- launched on any other stream it would read the old one."""
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(9004)
    n, n_tiles, stride = 300 * 257, 6, 300 * 257 + 5
    old = rng.integers(0, 256, size=n_tiles * stride, dtype=np.uint8)
    new = rng.integers(0, 256, size=n_tiles * stride, dtype=np.uint8)
    plane = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    out = torch.full((n_tiles,), 0x1111, dtype=torch.int64, device='cuda:0')
    torch.cuda.synchronize()
    want_old = [checksum(old[t * stride:t * stride + n]) for t in range(n_tiles)]
    want_new = [checksum(new[t * stride:t * stride + n]) for t in range(n_tiles)]
    assert want_old != want_new
    s = torch.cuda.Stream(device=0)
    ctx.checksum_device(plane.data_ptr(), 1, n_tiles, n, out.data_ptr(), tile_stride=stride, stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    assert out.cpu().numpy().view(np.uint64).tolist() == want_old
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(1.2e9))                       # some hundreds of milliseconds at any shader clock
        held = torch.cuda.Event()
        held.record(s)
        plane.copy_(src)
    t0 = time.perf_counter()
    ctx.checksum_device(plane.data_ptr(), 1, n_tiles, n, out.data_ptr(), tile_stride=stride, stream=s.cuda_stream)
    dt = time.perf_counter() - t0
    assert not held.query(), f'the entry took {dt * 1e3:.1f} ms on the host: it waited for the stream'
    ctx.synchronize(s.cuda_stream)
    assert out.cpu().numpy().view(np.uint64).tolist() == want_new
    assert torch.equal(plane, src)


def test_same_call_twenty_times_same_values(ctx):
    """The sum is commutative: the order of the blocks and of their atomic adds does not show."""
    rng = np.random.default_rng(9005)
    p = Plane(ctx, rng, 2, 1000 * 1003, 9, _stride('odd', 1000 * 1003), 2)
    want = p.expected()
    for _ in range(20):
        p.run()
        ctx.synchronize()
        assert np.array_equal(p.result(), want)
    p.buf.free()
    batch = _capi.DeviceBatch(ctx, 12, 700, 900, masks=True, extra_layers=('wtr1_aerosol', 'browse'))
    try:
        batch.synth(SEED, tile0=5)
        batch.classify(_capi.default_params())
        first = batch.checksums()
        assert len(first) == 10 + 9
        for _ in range(19):
            again = batch.checksums()
            for name in first:
                assert np.array_equal(again[name], first[name]), name
    finally:
        batch.free()


def _host_sums(batch, names, t):
    return {n: checksum(batch.read_tile(n, t)) for n in names}


@pytest.mark.parametrize('form', ['packed', 'separate_outputs', 'slide_placed'])
@pytest.mark.parametrize('masks,extra', [(False, ()), (True, ('wtr1_aerosol',)), (True, ('wtr1_aerosol', 'browse'))],
                         ids=['plain', 'masks_aerosol', 'masks_all_layers'])
@pytest.mark.parametrize('tile_align', [256, 1])
def test_batch_checksums_on_every_form_of_batch(ctx, form, masks, extra, tile_align):
    n_tiles, h, w = 7, 301, 257
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
        sums = batch.checksums()                              # same stream as the classification: ordered behind it
        assert 'dswx_checksum_k' in ctx.last_kernel_info() and f',{len(names)})' in ctx.last_kernel_info()
        assert list(sums) == names
        for t in range(n_tiles):
            want = _host_sums(batch, names, t)
            for n in names:
                assert int(sums[n][t]) == want[n], (n, t)
        # a few planes, from tile0 > 0
        some = ['wtr', 'nir', 'diag'] + (['ocean'] if masks else [])
        part = batch.checksums(names=some, tile0=3, n_tiles=3)
        assert list(part) == sorted(some, key=_capi.PLANE_INDEX.get)
        for n in some:
            assert part[n].shape == (3,) and np.array_equal(part[n], sums[n][3:6]), n
        assert np.array_equal(batch.checksums(names=['cloud'], tile0=6)['cloud'], sums['cloud'][6:])
        assert batch.checksums(names=['cloud'], tile0=7)['cloud'].shape == (0,)
        # the counters plane, by name: [n_tiles][3] int64
        cnt = batch.read_counters()
        got = batch.checksums(names=['counters'])['counters']
        assert [int(v) for v in got] == [checksum(cnt[t]) for t in range(n_tiles)]
        # planes this batch does not have
        absent = [n for n in ('land', 'wtr1_aerosol', 'browse') if n not in names]
        for n in absent:
            with pytest.raises(_capi.DswxError, match=n) as e:
                batch.checksums(names=['wtr', n])
            assert e.value.code == _capi.ERR_ARG
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError):
                batch.checksums(names=['wtr'], tile0=bad[0], n_tiles=bad[1])
    finally:
        batch.free()


def test_device_plane_checksum_of_the_product_run(ctx):
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9006)
    for dt in (np.uint8, np.int16, np.float32, np.float64):
        a = (rng.normal(size=(211, 97)) * 100).astype(dt)
        p = eng.upload(a)
        assert p.checksum() == checksum(a)
        p.release()
    eng.close()


def _workers():
    """Threads for the host side of the whole-batch tests: no more than the CPUs this process may use."""
    quota = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    env = os.environ.get('OMP_NUM_THREADS', '')
    return max(1, min(16, quota, int(env) if env.isdigit() and int(env) > 0 else 16))


def _whole_batch_every_tile(ctx, n_tiles, masks, extra, tile_align, detect_tile=None):
    """Synthesise and classify the batch, ONE checksums() call for all planes, then for EVERY tile: download the input
    planes only, checksum them on the host (the checksum kernel's addressing, through an independent path), run the C
    oracle on them and checksum its layers (every output layer of every tile, without downloading one)."""
    h, w = 3660, 3660
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, masks=masks, extra_layers=extra, tile_align=tile_align)
    try:
        batch.synth(SEED, tile0=0)
        p = _capi.default_params()
        batch.classify(p)
        ctx.synchronize()
        names = batch.plane_names()
        inputs = [n for n in names if _capi.PLANE_INDEX[n] < _capi.PLANE_INDEX['diag']]
        layers = [n for n in names if n not in inputs]
        t0 = time.perf_counter()
        sums = batch.checksums()
        wall = {'device_call_s': time.perf_counter() - t0, 'download_s': 0.0, 'oracle_s': 0.0, 'host_checksums_s': 0.0}
        assert ctx.last_kernel_info().count('dswx_checksum_k') == 1 and f',{n_tiles},{len(names)})' in ctx.last_kernel_info()
        c_oracle.load()

        def one_tile(t):
            a = time.perf_counter()
            planes = {n: batch.read_tile(n, t) for n in inputs}
            b = time.perf_counter()
            bad = [n for n in inputs if checksum(planes[n]) != int(sums[n][t])]
            c = time.perf_counter()
            exp = c_oracle.classify(p, [planes[n] for n in _capi.BAND_NAMES], planes['fmask'], layers=tuple(layers),
                                    **{m: planes[m] for m in ('land', 'shad', 'ocean') if m in planes})
            d = time.perf_counter()
            for n in layers:
                if checksum(exp[n]) != int(sums[n][t]):
                    got = batch.read_tile(n, t)
                    diff = np.flatnonzero(got.ravel() != exp[n].ravel())
                    bad.append(f'{n}: first differing index {int(diff[0]) if diff.size else None} of {diff.size} '
                               f'(device checksum {int(sums[n][t]):016x}, host checksum of the download {checksum(got):016x})')
            e = time.perf_counter()
            return t, bad, (b - a, d - c, (c - b) + (e - d))

        t0 = time.perf_counter()
        tiles_checked, failures = 0, []
        with ThreadPoolExecutor(max_workers=_workers()) as pool:
            for t, bad, (dl, orc, cks) in pool.map(one_tile, range(n_tiles)):
                tiles_checked += 1
                wall['download_s'] += dl
                wall['oracle_s'] += orc
                wall['host_checksums_s'] += cks
                if bad:
                    failures.append((t, bad))
        wall['host_phase_wall_s'] = time.perf_counter() - t0
        wall.update(n_tiles=n_tiles, masks=masks, tile_align=tile_align, planes=len(names), threads=_workers(),
                    note='download / oracle / host_checksums are summed over the threads')
        print('CHECKSUM_WALL ' + json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in wall.items()}))
        assert not failures, failures[:3]
        assert tiles_checked == n_tiles
        if detect_tile is not None:
            # one byte of one layer of one tile: exactly that word of the table changes
            tile = batch.read_tile('wtr', detect_tile)
            tile[1234, 2345] ^= 1
            batch.write_tile('wtr', detect_tile, tile)
            after = batch.checksums()
            changed = [(n, t) for n in names for t in range(n_tiles) if after[n][t] != sums[n][t]]
            assert changed == [('wtr', detect_tile)]
            assert sum(len(after[n]) for n in layers) == n_tiles * len(layers)
        return tiles_checked
    finally:
        batch.free()


@pytest.mark.parametrize('masks,extra,tile_align', [(False, (), 256), (True, ('wtr1_aerosol',), 1)],
                         ids=['padded', 'masks_aerosol_contiguous'])
def test_headline_batch_256_tiles_every_tile(ctx, masks, extra, tile_align):
    """The batch of tests/test_gpu_parity.py::test_headline_batch_256_tiles_past_2_31 (72 / 82 GB; tile offsets pass 2^31
    pixels at tile 161 and 2^32 bytes at tile 160) with all 256 tiles compared, inputs and every layer.  In the plain
    run one byte of WTR of tile 200 is then overwritten: of the 256 x 7 layer checksums exactly that one changes."""
    assert _whole_batch_every_tile(ctx, 256, masks, extra, tile_align, detect_tile=None if masks else 200) == 256


def test_batch_512_tiles_every_tile(ctx):
    """The batch of test_batch_512_tiles_past_2_32_pixels (144 GB; tile offsets pass 2^32 pixels at tile 321), all 512."""
    assert _whole_batch_every_tile(ctx, 512, False, (), 256) == 512
