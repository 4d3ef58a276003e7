"""The crosstab entries on the GPU: dswx_crosstab_device and dswx_batch_crosstab bit for bit against the numpy statement of
the definition (proteus_amd/crosstab.py) -- every kind of plane A, tile lengths either side of the kernel's 16-pair steps, of
an unrolled round and of a block's chunk, tile counts, the strides and the addresses of the two planes chosen independently;
contents chosen against the accumulator and its one-value shortcut; more tiles than one launch takes; on a caller's stream behind the kernel that replaces
plane B; every form of batch, two batches of different strides; DevicePlane.crosstab; the product comparison's tables; the
C example."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from oracle import dswx_oracle as o
from proteus_amd import _capi
from proteus_amd.crosstab import CELLS, WTR_CLASSES, WTR_VALUES, Spec, cell_of, classes, crosstab, crosstab_tiles, fold
from proteus_amd.histogram import DTYPES, HIST_DIAG, HIST_I16, HIST_U16, HIST_U8, bin_of
from proteus_amd.synth import SEED
from tests.test_crosstab import check_printed_tables

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, UNROLL, MAX_PASSES, STEP = 256, 4, 64, 16     # of dswx_crosstab.hip: threads, steps in flight, passes of a block's largest chunk, pairs per step
PAD = 0xA5                                           # every byte that is not tile data; as an element of A and as a byte of B it WOULD be counted
# (kind, lo, shift): the linear kinds with a range that holds the padding element 0xA5A5 (42405 / -23131)
BINNINGS = {'u8': (HIST_U8, 0, 0), 'u16': (HIST_U16, 40000, 4), 'i16': (HIST_I16, -32768, 7), 'diag': (HIST_DIAG, 0, 0)}
PATTERNS = o.get_binary_representation(np.arange(32, dtype=np.uint16))
SENT_OUT = 0x1111111111111111


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def pad_element(name):
    dt = DTYPES[BINNINGS[name][0]]
    return np.array([PAD, PAD], dtype=np.uint8).view(dt)[0] if dt.itemsize == 2 else dt.type(PAD)


def a_data(rng, name, n):
    """n elements of plane A: over the whole domain and around the counted range, never the padding element."""
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
    pad = pad_element(name)
    a[a == pad] = pad - 1
    return a


def b_data(rng, n):
    b = rng.integers(0, 256, size=n).astype(np.uint8)
    b[b == PAD] = PAD - 1
    return b


def spec_with_counted_padding(rng, name, col_bits=3):
    """Random tables, a fifth of the entries excluded on each side -- but the padding element of A and the padding byte of B
    are counted, so that a kernel that read the padding would count it."""
    kind, lo, shift = BINNINGS[name]
    n_rows, n_cols = 256 >> col_bits, 1 << col_bits
    rows = np.where(rng.random(256) < 0.2, rng.integers(n_rows, 256, size=256), rng.integers(0, n_rows, size=256)).astype(np.uint8)
    cols = np.where(rng.random(256) < 0.2, rng.integers(n_cols, 256, size=256), rng.integers(0, n_cols, size=256)).astype(np.uint8)
    pad_bin = int(bin_of(np.array([pad_element(name)]), kind, lo, shift)[0])
    assert pad_bin >= 0
    rows[pad_bin], cols[PAD] = n_rows - 1, n_cols - 1
    spec = Spec(kind, lo, shift, col_bits, rows, cols)
    assert crosstab(np.array([pad_element(name)]), np.array([PAD], dtype=np.uint8), spec).sum() == 1
    return spec


class Pair:
    """A device buffer holding guard | plane A at byte offset `a_off` past a 256-byte boundary | guard | plane B at byte offset
    `b_off` past a 256-byte boundary | guard, every byte that is not tile data PAD; the records follow, prefilled with a
    sentinel.  `a_tiles` / `b_tiles` are the host copies the expected counts come from."""
    GUARD = 512

    def __init__(self, ctx, spec, a_tiles, b_tiles, a_stride, b_stride, a_off, b_off, buf=None):
        self.ctx, self.spec, self.a_tiles, self.b_tiles = ctx, spec, a_tiles, b_tiles
        self.a_stride, self.b_stride = a_stride, b_stride
        eb = DTYPES[spec.a_kind].itemsize
        self.n, self.n_tiles = (len(a_tiles[0]) if a_tiles else 0), len(a_tiles)
        span = lambda stride, e: ((self.n_tiles - 1) * stride + self.n) * e if self.n_tiles else 0   # noqa: E731 (the last tile's padding need not exist)
        self.a_start = self.GUARD + a_off
        a_end = self.a_start + span(a_stride, eb)
        self.b_start = -(-(a_end + self.GUARD) // 256) * 256 + b_off
        self.nbytes = self.b_start + span(b_stride, 1) + self.GUARD
        host = np.full(self.nbytes, PAD, dtype=np.uint8)
        for t in range(self.n_tiles):
            at = self.a_start + t * a_stride * eb
            host[at:at + self.n * eb] = a_tiles[t].view(np.uint8)
            at = self.b_start + t * b_stride
            host[at:at + self.n] = b_tiles[t]
        self.host = host
        self.out_off = -(-self.nbytes // 256) * 256
        need = self.out_off + 8 * CELLS * max(self.n_tiles, 1)
        self.buf = buf if buf is not None else ctx.malloc(need)
        assert self.buf.nbytes >= need and self.buf.ptr % 256 == 0
        self.buf.upload(host)
        self.buf.upload(np.full(CELLS * max(self.n_tiles, 1), SENT_OUT, dtype=np.uint64), self.out_off)

    def run(self, stream=None):
        self.ctx.crosstab_device(self.buf.ptr + self.a_start, self.buf.ptr + self.b_start, self.spec, self.n_tiles, self.n,
                                 self.buf.ptr + self.out_off, a_stride=self.a_stride, b_stride=self.b_stride, stream=stream)

    def result(self):
        return self.buf.download(np.uint64, CELLS * self.n_tiles, self.out_off).reshape(self.n_tiles, CELLS)


@pytest.mark.parametrize('name', list(BINNINGS))
def test_device_entry_every_size_count_stride_and_address(ctx, name):
    """Tile lengths around the 16-pair step, the 4096-pair pass, one unrolled round of a block (+- 1) and a block's largest
    chunk + 17 pairs (several blocks flush into one record); 1 and 3 tiles; the strides of A and B equal to the tile and above
    it, independently, the padding full of elements that would be counted; A and B at independent offsets past a 256-byte
    boundary."""
    rng = np.random.default_rng(9600 + len(name))
    spec = spec_with_counted_padding(rng, name)
    eb = DTYPES[spec.a_kind].itemsize
    one_round = UNROLL * BLOCK * STEP
    chunk = MAX_PASSES * BLOCK * STEP
    sizes = [0, 1, 15, 16, 17, 4095, 4096, 4097, one_round - 1, one_round, one_round + 1, chunk + 17]
    buf = ctx.malloc(4 * Pair.GUARD + 1024 + 3 * (sizes[-1] + 300) * (eb + 1) + 8 * CELLS * 3 + 512)
    cases = 0
    for n in sizes:
        for n_tiles in (1, 3):
            a_tiles, b_tiles = [a_data(rng, name, n) for _ in range(n_tiles)], [b_data(rng, n) for _ in range(n_tiles)]
            want = crosstab_tiles(a_tiles, b_tiles, spec)
            for a_stride, b_stride, a_off, b_off in ((n, n, 0, 0), (n + 3, n, eb, 0), (n, n + 5, 0, 3),
                                                     (-(-(n + 1) // 256) * 256, n + 1, 6, 5)):
                p = Pair(ctx, spec, a_tiles, b_tiles, a_stride, b_stride, a_off, b_off, buf=buf)
                p.run()
                ctx.synchronize()
                got = p.result()
                assert np.array_equal(got, want), (name, n, n_tiles, a_stride, b_stride, a_off, b_off, np.argwhere(got != want)[:4])
                cases += 1
        if n:
            info = ctx.last_kernel_info()
            assert 'dswx_crosstab_k' in info and f'block={BLOCK}' in info and 'replicas=32' in info and 'passes=' in info, info
    assert cases == len(sizes) * 2 * 4
    assert 0 < int(want.sum()) < 3 * sizes[-1]                # something is counted, something excluded
    if name != 'u8':                                          # a 16-bit plane A one byte off its elements is refused
        with pytest.raises(_capi.DswxError) as e:
            ctx.crosstab_device(buf.ptr + 1, buf.ptr + 4096, spec, 1, 16, buf.ptr + 8192)
        assert e.value.code == _capi.ERR_ALIGN
    # a == b is legal: a byte plane against itself is its histogram on the diagonal
    if name == 'u8':
        a = a_data(rng, name, 5000)
        buf.upload(a)
        ident = Spec(HIST_U8, col_bits=4, row_of_bin=np.arange(256) % 16, col_of_byte=np.arange(256) % 16)
        ctx.crosstab_device(buf.ptr, buf.ptr, ident, 1, 5000, buf.ptr + 8192)
        ctx.synchronize()
        got = ident.table(buf.download(np.uint64, CELLS, 8192))
        assert np.array_equal(np.diag(got), np.bincount(a % 16, minlength=16)) and got.sum() == 5000
    buf.free()


# ---- contents against the accumulator ----------------------------------------------------------------------------------
PERM = np.array([5, 12, 0, 9, 3, 15, 7, 1, 14, 2, 11, 6, 8, 13, 4, 10], dtype=np.uint8)


def contents(n):
    """(class of A, class of B) per pair, both int64 0 .. 15, chosen against a private accumulator and its shortcut."""
    rng = np.random.default_rng(9700)
    i = np.arange(n)
    noise_a, noise_b = rng.integers(0, 16, size=n), rng.integers(0, 16, size=n)
    five, two = np.full(n, 5), np.full(n, 2)
    nine_in_ten = rng.random(n) < 0.9
    return {'both constant': (five, two),
            'A constant, B noise': (five, noise_b), 'A noise, B constant': (noise_a, two),
            'A constant, B changes in the middle of a unit': (five, np.where(i % 16 < 8, 2, 9)),
            'A constant, B changes in its last byte': (five, np.where(i % 16 < 15, 2, 9)),
            'B constant, A changes in the middle of a step': (np.where(i % 16 < 8, 5, 11), two),
            'B constant, A changes in its last element': (np.where(i % 16 < 15, 5, 11), two),
            'two alternating values': (np.where(i & 1, 3, 13), np.where(i & 1, 13, 3)),
            'every cell equally often': (i % 16, (i // 16) % 16),
            'every cell in runs of 16': ((i // 16) % 16, (i // 256) % 16),
            'one cell nine times in ten': (np.where(nine_in_ten, 1, noise_a), np.where(nine_in_ten, 7, noise_b))}


@pytest.mark.parametrize('name', list(BINNINGS))
def test_contents_that_break_accumulators(ctx, name):
    """One tile of 2^20 + 5 pairs: what makes the lanes of a wave meet in one counter, or never, and what the one-value
    shortcut must not take for constant."""
    n = (1 << 20) + 5
    kind = BINNINGS[name][0]
    # class c of A as an element of the kind, under a binning whose bin is c; class c of B as the byte 16 c + 3
    as_kind = {'u8': (lambda c: c.astype(np.uint8), 0, 0), 'u16': (lambda c: (c * 64 + 17).astype(np.uint16), 0, 6),
               'i16': (lambda c: ((c - 128) * 64 + 63).astype(np.int16), -8192, 6), 'diag': (lambda c: PATTERNS[c], 0, 0)}[name]
    rows = np.full(256, 255, dtype=np.uint8)
    rows[:16] = PERM
    cols = np.full(256, 255, dtype=np.uint8)
    cols[np.arange(16) * 16 + 3] = PERM[::-1]
    spec = Spec(kind, as_kind[1], as_kind[2], 4, rows, cols)
    none_a = Spec(kind, as_kind[1], as_kind[2], 4, np.full(256, 255, dtype=np.uint8), cols)
    none_b = Spec(kind, as_kind[1], as_kind[2], 4, rows, np.full(256, 255, dtype=np.uint8))
    b_off = -(-n * 2 // 256) * 256 + 256
    out_off = b_off + -(-n // 256) * 256 + 256
    buf = ctx.malloc(out_off + 8 * CELLS)

    def run(sp):
        buf.upload(np.full(CELLS, SENT_OUT, dtype=np.uint64), out_off)
        ctx.crosstab_device(buf.ptr, buf.ptr + b_off, sp, 1, n, buf.ptr + out_off)
        ctx.synchronize()
        return buf.download(np.uint64, CELLS, out_off)

    for label, (ca, cb) in contents(n).items():
        a, b = as_kind[0](ca), (cb * 16 + 3).astype(np.uint8)
        buf.upload(a)
        buf.upload(b, b_off)
        got = run(spec)
        want = crosstab(a, b, spec)
        assert np.array_equal(got, want), (name, label, np.flatnonzero(got != want)[:8])
        assert int(got.sum()) == n, (name, label)
        assert np.array_equal(got, np.bincount(PERM[ca].astype(np.int64) * 16 + PERM[::-1][cb], minlength=CELLS).astype(np.uint64)), (name, label)
    assert run(none_a).sum() == 0 and run(none_b).sum() == 0          # everything excluded on one side (the last content: skewed noise)
    buf.free()


def test_65537_one_element_tiles_cross_the_launch_split(ctx):
    T = 65537
    rng = np.random.default_rng(9800)
    a, b = rng.integers(0, 16, size=T).astype(np.uint8), rng.integers(0, 16, size=T).astype(np.uint8)
    host_a, host_b = np.full((T, 3), 7, dtype=np.uint8), np.full((T, 2), 7, dtype=np.uint8)      # (the padding would be counted)
    host_a[:, 0], host_b[:, 0] = a, b
    b_off = -(-host_a.nbytes // 256) * 256
    out_off = b_off + -(-host_b.nbytes // 256) * 256
    buf = ctx.malloc(out_off + 8 * CELLS * T)
    buf.upload(host_a)
    buf.upload(host_b, b_off)
    ctx.crosstab_device(buf.ptr, buf.ptr + b_off, Spec(), T, 1, buf.ptr + out_off, a_stride=3, b_stride=2)
    ctx.synchronize()
    got = buf.download(np.uint64, CELLS * T, out_off).reshape(T, CELLS)
    want = np.zeros((T, CELLS), dtype=np.uint64)
    want[np.arange(T), a.astype(np.int64) * 16 + b] = 1
    assert np.array_equal(got, want)
    buf.free()


@pytest.mark.parametrize('name', ['u8', 'u16'])
def test_more_tiles_than_one_launch_takes_with_two_strides(ctx, name):
    """65535 + 4 tiles of 17 pairs (one 16-pair step and a tail), plane A with a stride 3 above the tile and one element past
    a 256-byte boundary, plane B with a stride 5 above it and 3 bytes past one: the second launch starts at tile 65535 of
    BOTH, each by its own stride, so a swapped or shared offset shows.  Random elements and a random spec under which the
    padding would be counted: EVERY record against the numpy statement (a few also against the library's scalar entry), and
    every other byte of the buffer -- guards, padding, tiles, the bytes behind the records -- as it was."""
    rng = np.random.default_rng(9850 + len(name))
    T, n = 65535 + 4, 17
    spec = spec_with_counted_padding(rng, name)
    a, b = a_data(rng, name, T * n).reshape(T, n), b_data(rng, T * n).reshape(T, n)
    cells = cell_of(a, b, spec)
    want = np.bincount((cells + np.arange(T)[:, None] * CELLS)[cells >= 0], minlength=T * CELLS).astype(np.uint64).reshape(T, CELLS)
    for t in (0, 1, 65534, 65535, 65536, T - 1):
        assert np.array_equal(want[t], crosstab(a[t], b[t], spec)) and np.array_equal(want[t], _capi.crosstab_host(a[t], b[t], spec))
    assert 0 < int(want.sum()) < T * n                        # something is counted, something excluded
    eb = a.dtype.itemsize
    buf = ctx.malloc(4 * Pair.GUARD + 1024 + T * (n + 3) * eb + T * (n + 5) + 8 * CELLS * T + 4096)
    p = Pair(ctx, spec, list(a), list(b), n + 3, n + 5, eb, 3, buf=buf)
    behind = p.out_off + 8 * CELLS * T
    tail = np.full(p.buf.nbytes - behind, PAD, dtype=np.uint8)
    p.buf.upload(tail, behind)
    p.buf.upload(np.full(p.out_off - p.nbytes + 8, PAD, dtype=np.uint8), p.nbytes - 8)
    p.run()
    ctx.synchronize()
    assert ',65535,1)' in ctx.last_kernel_info(), ctx.last_kernel_info()
    got = p.result()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, bad[:4], got[tuple(bad[:4].T)], want[tuple(bad[:4].T)])
    assert np.array_equal(p.buf.download(np.uint8, p.nbytes), p.host), 'a plane was written'
    assert np.all(p.buf.download(np.uint8, p.out_off - p.nbytes + 8, p.nbytes - 8) == PAD)
    assert np.all(p.buf.download(np.uint8, tail.size, behind) == PAD), 'bytes behind the records were written'
    p.buf.free()


def test_on_a_callers_stream_behind_the_kernel_that_replaces_plane_b(ctx):
    """Asynchronous on the caller's stream: the stream is held, a copy kernel that REPLACES plane B is queued on it, then the
    entry, with no synchronisation in between.  The entry returns while the hold is pending, and the table is that of the
    replaced plane -- launched on any other stream it would read the old one."""
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(9900)
    n, n_tiles, a_stride, b_stride = 300 * 257, 6, 300 * 257 + 5, 300 * 257 + 2
    a = rng.integers(0, 16, size=n_tiles * a_stride, dtype=np.uint8)
    old = rng.integers(0, 8, size=n_tiles * b_stride, dtype=np.uint8)
    new = rng.integers(8, 16, size=n_tiles * b_stride, dtype=np.uint8)
    plane_a = torch.from_numpy(a.copy()).to('cuda:0')
    plane_b = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    out = torch.full((n_tiles, CELLS), 0x1111, dtype=torch.int64, device='cuda:0')
    torch.cuda.synchronize()
    spec = Spec()
    tiles = lambda x, stride: [x[t * stride:t * stride + n] for t in range(n_tiles)]             # noqa: E731
    want_old = crosstab_tiles(tiles(a, a_stride), tiles(old, b_stride), spec)
    want_new = crosstab_tiles(tiles(a, a_stride), tiles(new, b_stride), spec)
    assert not np.array_equal(want_old, want_new)
    s = torch.cuda.Stream(device=0)
    kw = {'a_stride': a_stride, 'b_stride': b_stride, 'stream': s.cuda_stream}
    ctx.crosstab_device(plane_a.data_ptr(), plane_b.data_ptr(), spec, n_tiles, n, out.data_ptr(), **kw)
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want_old)
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(1.2e9))                       # some hundreds of milliseconds at any shader clock
        held = torch.cuda.Event()
        held.record(s)
        plane_b.copy_(src)
    t0 = time.perf_counter()
    ctx.crosstab_device(plane_a.data_ptr(), plane_b.data_ptr(), spec, n_tiles, n, out.data_ptr(), **kw)
    dt = time.perf_counter() - t0
    assert not held.query(), f'the entry took {dt * 1e3:.1f} ms on the host: it waited for the stream'
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want_new)
    assert torch.equal(plane_b, src)


# ---- the batch entry ---------------------------------------------------------------------------------------------------
SWIR1_SPEC = Spec(HIST_I16, 0, 6, 4, fold(16), classes(WTR_VALUES, other=7))         # reflectances 0 .. 16383 in 16 rows of 1024
DIAG_SPEC = Spec(HIST_DIAG, col_bits=3, row_of_bin=np.minimum(np.arange(256), 31), col_of_byte=classes(WTR_VALUES, other=7))


def other_params():
    p = _capi.default_params()
    p.wigt, p.pswt_1_nir = 0.2, 1400.0                # two of the five tests move: some pixels change class
    return p


@pytest.mark.parametrize('form', ['packed', 'separate_outputs', 'slide_placed'])
@pytest.mark.parametrize('masks,extra', [(False, ()), (True, ('wtr1_aerosol',)), (True, ('wtr1_aerosol', 'browse'))],
                         ids=['plain', 'masks_aerosol', 'masks_all_layers'])
def test_batch_crosstab_on_every_form_of_batch(ctx, form, masks, extra):
    n_tiles, h, w = 4, 61, 67
    kw = {'separate_outputs': form == 'separate_outputs', 'sliding_outputs': form == 'slide_placed'}
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, masks=masks, extra_layers=extra, tile_align=256, **kw)
    other = _capi.DeviceBatch(ctx, n_tiles + 1, h, w, masks=masks, tile_align=1)               # another stride, one tile more
    small = _capi.DeviceBatch(ctx, n_tiles, h, w + 1)
    try:
        assert batch.tile_stride != other.tile_stride
        p = _capi.default_params()
        batch.synth(SEED, tile0=31)
        other.synth(SEED, tile0=31)
        if form == 'slide_placed':
            batch.place_slide(p, slack_bytes=24 << 20, step_bytes=2 << 20, spread_gaps=2, refine_passes=1, launches=2,
                              keep_free_bytes=0)
        batch.classify(p)
        other.classify(other_params())
        names_before = batch.plane_names()
        # ONE call, four pairs of one batch, three kinds of plane A
        pairs = [('wtr2', 'wtr', WTR_CLASSES), ('wtr1', 'wtr2', WTR_CLASSES), ('swir1', 'wtr', SWIR1_SPEC), ('diag', 'wtr1', DIAG_SPEC)]
        got = batch.crosstab(pairs)                           # same stream as the classification; None = DSWX_BATCH_ALL_TILES
        info = ctx.last_kernel_info()
        assert info.count('dswx_crosstab_k') == 1 and f',{n_tiles},{len(pairs)})' in info and 'replicas=32' in info, info
        assert got.shape == (len(pairs), n_tiles, CELLS) and got.dtype == np.uint64
        for k, (na, nb, spec) in enumerate(pairs):
            for t in range(n_tiles):
                want = crosstab(batch.read_tile(na, t), batch.read_tile(nb, t), spec)
                assert np.array_equal(got[k, t], want), (na, nb, t, np.flatnonzero(got[k, t] != want)[:8])
        assert np.all(got[[0, 1, 3]].sum(axis=2) == h * w)                                      # nothing excluded in the class pairs
        # row and column sums are the histograms of the two planes
        hist = batch.histogram(names=['wtr2', 'wtr', 'swir1'])
        table = WTR_CLASSES.table(got[0])                                                        # [t, 32, 8]
        for k, v in enumerate(WTR_VALUES):
            assert np.array_equal(table[:, k, :].sum(axis=1), hist['wtr2'][:, v]) and np.array_equal(table[:, :, k].sum(axis=1), hist['wtr'][:, v])
        assert np.all(table[:, 7:, :] == 0) and np.all(table[:, :, 7] == 0)                      # no other byte in either layer
        swir = SWIR1_SPEC.table(got[2])                                                          # [t, 16, 16]: rows of 16 bins (lo 0, shift 6)
        assert np.array_equal(swir.sum(axis=2), hist['swir1'].reshape(n_tiles, 16, 16).sum(axis=2))
        # the reference's own rule: cloud masking only overwrites WTR-2 with snow (column 3) or cloud (column 4)
        off = table[:, :8, :].copy()
        off[:, np.arange(8), np.arange(8)] = 0
        assert np.all(np.delete(off, [3, 4], axis=2) == 0)
        # two batches with different strides; tile0 > 0; DSWX_BATCH_ALL_TILES; the empty range
        two = [('wtr', 'wtr', WTR_CLASSES), ('swir1', 'wtr', SWIR1_SPEC)]
        got2 = batch.crosstab(two, other=other, n_tiles=n_tiles)
        assert got2.shape == (2, n_tiles, CELLS)
        for k, (na, nb, spec) in enumerate(two):
            want = crosstab_tiles([batch.read_tile(na, t) for t in range(n_tiles)], [other.read_tile(nb, t) for t in range(n_tiles)], spec)
            assert np.array_equal(got2[k], want), (na, nb)
        moved = WTR_CLASSES.table(got2[0])[:, :8, :].sum(axis=0)
        assert moved.sum() == n_tiles * h * w and moved.sum() > np.trace(moved) > 0               # the parameter sets differ somewhere
        assert np.array_equal(batch.crosstab(two, other=other, tile0=1, n_tiles=n_tiles - 1), got2[:, 1:])
        assert np.array_equal(batch.crosstab(two, other=other, tile0=2, n_tiles=1), got2[:, 2:3])
        assert np.array_equal(batch.crosstab(pairs, tile0=1), got[:, 1:])
        assert np.array_equal(batch.crosstab(pairs, tile0=0, n_tiles=_capi.BATCH_ALL_TILES), got)
        assert batch.crosstab(pairs, tile0=n_tiles).shape == (len(pairs), 0, CELLS)
        assert batch.crosstab([]).shape == (0, n_tiles, CELLS)
        # refused: 7 pairs, a kind that does not fit its plane, a 16-bit plane as B, planes the batch does not have, the counters
        with pytest.raises(_capi.DswxError, match='pairs') as e:
            batch.crosstab([pairs[0]] * 7)
        assert e.value.code == _capi.ERR_ARG
        assert batch.crosstab([pairs[0]] * 6).shape == (6, n_tiles, CELLS)
        for na, spec in (('wtr', SWIR1_SPEC), ('swir1', WTR_CLASSES), ('swir1', DIAG_SPEC), ('diag', WTR_CLASSES), ('diag', SWIR1_SPEC),
                         ('fmask', Spec(HIST_U16))):
            with pytest.raises(_capi.DswxError, match='a_kind') as e:
                batch.crosstab([(na, 'wtr', spec)])
            assert e.value.code == _capi.ERR_ARG and ('band[4]' if na == 'swir1' else na) in str(e.value), str(e.value)
        assert batch.crosstab([('diag', 'wtr', Spec(HIST_U16, 0, 8))]).shape == (1, n_tiles, CELLS)      # DIAG takes U16 too
        for nb in ('diag', 'nir'):
            with pytest.raises(_capi.DswxError, match='uint8') as e:
                batch.crosstab([('wtr', nb, WTR_CLASSES)])
            assert e.value.code == _capi.ERR_ARG and ('band[3]' if nb == 'nir' else nb) in str(e.value)
        for name in [v for v in ('land', 'wtr1_aerosol', 'browse') if v not in names_before]:
            for pr in ((name, 'wtr', WTR_CLASSES), ('wtr', name, WTR_CLASSES)):
                with pytest.raises(_capi.DswxError, match=name) as e:
                    batch.crosstab([pairs[0], pr])
                assert e.value.code == _capi.ERR_ARG
        if extra:                                             # `other` has no extra layers: batch b is named
            with pytest.raises(_capi.DswxError, match='batch b has no plane .*wtr1_aerosol'):
                batch.crosstab([('wtr', 'wtr1_aerosol', WTR_CLASSES)], other=other)
        for pr in (('counters', 'wtr', WTR_CLASSES), ('wtr', 'counters', WTR_CLASSES)):
            with pytest.raises(_capi.DswxError, match='counters') as e:
                batch.crosstab([pr])
            assert e.value.code == _capi.ERR_ARG
        with pytest.raises(_capi.DswxError, match='tile size'):
            batch.crosstab(two, other=small)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside'):
                batch.crosstab(two, tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(_capi.DswxError, match='outside'):
            other.crosstab(two, other=batch, tile0=0, n_tiles=n_tiles + 1)                        # inside a, outside b
        bad_spec = Spec()
        bad_spec.col_bits = 9
        with pytest.raises(_capi.DswxError, match='col_bits'):
            batch.crosstab([('wtr', 'wtr', bad_spec)])
        with pytest.raises(ValueError):
            batch.crosstab([('wtr', 'no such plane', WTR_CLASSES)])
        assert batch.plane_names() == names_before
    finally:
        small.free()
        other.free()
        batch.free()


# ---- the layers above --------------------------------------------------------------------------------------------------
def test_device_plane_crosstab(ctx):
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(10000)
    try:
        b = rng.choice(np.array(WTR_VALUES, dtype=np.uint8), size=(211, 97))
        for a, spec in ((rng.choice(np.array(WTR_VALUES + (9,), dtype=np.uint8), size=(211, 97)), WTR_CLASSES),
                        ((rng.normal(size=(211, 97)) * 3000).astype(np.int16), Spec(HIST_I16, -4000, 5, 3, fold(32), classes(WTR_VALUES))),
                        (rng.integers(0, 65536, size=(211, 97)).astype(np.uint16), Spec(HIST_U16, 1, 8, 4, fold(16), classes(WTR_VALUES))),
                        (PATTERNS[rng.integers(0, 32, size=(211, 97))], DIAG_SPEC)):
            pa, pb = eng.upload(a), eng.upload(b)
            got = pa.crosstab(pb, spec)
            assert got.dtype == np.uint64 and got.shape == (1, CELLS) and np.array_equal(got[0], crosstab(a, b, spec)), (a.dtype, spec)
            pa.release()
            pb.release()
        # a stack: one record per leading index, or one index alone
        a3, b3 = rng.choice(np.array(WTR_VALUES, dtype=np.uint8), size=(3, 50, 41)), rng.choice(np.array(WTR_VALUES, dtype=np.uint8), size=(3, 50, 41))
        pa, pb = eng.upload(a3), eng.upload(b3)
        assert np.array_equal(pa.crosstab(pb, WTR_CLASSES), crosstab_tiles(a3, b3, WTR_CLASSES))
        assert np.array_equal(pa.crosstab(pb, WTR_CLASSES, index=2)[0], crosstab(a3[2], b3[2], WTR_CLASSES))
        assert np.array_equal(pa.crosstab(pa, WTR_CLASSES)[1], crosstab(a3[1], a3[1], WTR_CLASSES))       # a plane against itself
        with pytest.raises(ValueError):
            pa.crosstab(pb, WTR_CLASSES, index=3)
        with pytest.raises(ValueError):
            pa.crosstab(pb, SWIR1_SPEC)                       # a kind of another dtype
        with pytest.raises(ValueError):
            pa.crosstab(eng.upload(b3[:2]), WTR_CLASSES)
        with pytest.raises(ValueError):
            pa.crosstab(eng.upload(b3.astype(np.uint16)), WTR_CLASSES)
    finally:
        eng.close()


def _product(path, array, descriptions):
    from proteus_amd import geotiff
    geotiff.write_geotiff(str(path), array, metadata={'PRODUCT': 'DSWx-HLS', 'SPACECRAFT_NAME': 'test'}, descriptions=descriptions,
                          nodata=255, geo_tags=geotiff.geo_tags_from_geotransform((500000.0, 30.0, 0.0, 4000000.0, 0.0, -30.0), 32611))


def test_product_crosstab_on_the_device_prints_the_tables(ctx, tmp_path, capsys):
    """Two small products that differ in a known number of pixels: compare_dswx_hls_products(..., device=0, crosstab=True)
    prints what the host path prints, every cell is checked against a count made here, and everything printed without the
    flag and the return value stay as they are; the command-line tool takes the flag."""
    from proteus_amd.dswx_hls import compare_dswx_hls_products, get_context
    rng = np.random.default_rng(10100)
    H, W = 70, 53
    base = rng.choice(np.array([0, 1, 2, 252, 254, 255], dtype=np.uint8), size=(2, H, W))
    other = base.copy()
    for y, x in ((3, 4), (33, 17), (69, 52), (40, 0), (0, 52)):                                  # five pixels of band 2: open water -> cloud
        base[1, y, x], other[1, y, x] = 1, 253
    desc = ['WTR', 'WTR-2']
    f1, f2 = str(tmp_path / 'base.tif'), str(tmp_path / 'other.tif')
    _product(f1, base, desc)
    _product(f2, other, desc)
    capsys.readouterr()
    plain = compare_dswx_hls_products(f1, f2, device=0)
    plain_text = capsys.readouterr().out
    host = compare_dswx_hls_products(f1, f2, crosstab=True)
    host_text = capsys.readouterr().out
    dev = compare_dswx_hls_products(f1, f2, device=0, crosstab=True)
    dev_text = capsys.readouterr().out
    assert 'dswx_crosstab_k' in get_context(0).last_kernel_info()                                # the tables were made in HBM
    assert plain is False and host is False and dev is False
    assert dev_text == host_text
    extra = [line for line in dev_text.splitlines() if line not in plain_text.splitlines()]
    assert [line for line in dev_text.splitlines() if line not in extra] == plain_text.splitlines()
    check_printed_tables(extra, base, other, desc)
    n = H * W
    assert f'Band 2 - WTR-2: agreement {(n - 5) / n:.6f} ({n - 5} of {n} pixels)' in dev_text
    assert f'Band 1 - WTR: agreement {1:.6f} ({n} of {n} pixels)' in dev_text
    # identical files: the diagonal alone, and the return value stays True
    assert compare_dswx_hls_products(f1, f1, device=0, crosstab=True) is True
    assert 'agreement 1.000000' in capsys.readouterr().out
    # the command-line tool
    import importlib.util
    spec = importlib.util.spec_from_file_location('dswx_compare_cli', os.path.join(ROOT, 'bin', 'dswx_compare.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.main([f1, f2, '--device', '0', '--crosstab']) == 1
    assert capsys.readouterr().out == dev_text
    assert cli.main([f1, f1, '--crosstab']) == 0
    assert cli.main([f1, f2, '--device', '0']) == 1
    assert capsys.readouterr().out.endswith(plain_text)


def test_crosstab_example_runs(tmp_path):
    """examples/batch_crosstab.c: its own checks (exit status 0: every cell of the device against its loop and against
    dswx_crosstab_host), and the cells it prints against the same two batches made here."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_crosstab')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_crosstab.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    n_tiles, size = 3, 301
    r = subprocess.run([exe, str(n_tiles), str(size)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr x wtr: device, loop and host entry agree in every cell' in r.stdout
    c = _capi.Context(0)
    a, b = _capi.DeviceBatch(c, n_tiles, size, size), _capi.DeviceBatch(c, n_tiles, size, size, tile_align=1)
    try:
        a.synth(20251010)
        b.synth(20251010)
        a.classify(_capi.default_params())
        b.classify(other_params())
        for t in range(n_tiles):
            want = crosstab(a.read_tile('wtr', t), b.read_tile('wtr', t), WTR_CLASSES)
            line = 'tile %d: wtr x wtr cells' % t + ''.join(' %d,%d:%d' % (cell // 8, cell % 8, want[cell]) for cell in np.flatnonzero(want))
            assert line in r.stdout.splitlines(), (line, r.stdout[-1500:])
    finally:
        b.free()
        a.free()
        c.close()
