"""The grid entries on the GPU: dswx_grid_device and dswx_batch_grid bit for bit against the numpy statement of the definition
(proteus_amd/grid.py) -- widths and cell widths either side of a 16-byte load and of a cell boundary inside one, heights and
cell heights either side of a cell row, rasters either side of what one workgroup owns, tile counts, strides and addresses,
with every byte outside the output planes checked; cells chosen against the packed counters; every subset of outputs; on a
caller's stream behind the kernel that writes the plane; every form of batch; DevicePlane.grid feeding histogram and stack;
bin/dswx_grid.py; the C example."""
import importlib.util
import itertools
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
from proteus_amd.grid import NO_SHARE, NONE, Spec, grid_shape, grid_tiles, wtr_grid_spec
from proteus_amd.stack import Spec as StackSpec, stack_tiles
from proteus_amd.synth import SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# of dswx_grid.hip: columns per unit (= bytes per load), threads per block, rows in flight, units summed before widening,
# cells of a job at most, columns of a job when cell_w < 16, pixel rows a job should have
PPU, BLOCK, U, ROWS_PACKED, MAX_CELLS, SMALL_COLS, TARGET_ROWS = 16, 256, 4, 15, 2048, 1024, 32
PAD = 0xA5                                        # every byte of a plane buffer that is not tile data; the specs below COUNT it
SENT = 0xEE                                       # every byte of an output buffer beforehand
KEYS = ('count', 'share', 'coverage', 'major')
GUARD = 512


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def random_spec(rng, n_cats, cell_h, cell_w, every_byte_observed=False):
    """Categories 0 .. 5 at random (4 and 5 are never observations); the padding byte is an observation of category 0."""
    cat = rng.integers(0, n_cats if every_byte_observed else 6, size=256).astype(np.uint8)
    cat[PAD] = 0
    return Spec(n_cats, cell_h, cell_w, cat)


class Run:
    """One call of dswx_grid_device.  The plane lies guard | `off` bytes past a 256-byte boundary | guard in `sbuf`, every byte
    that is not tile data PAD; the wanted outputs lie in `obuf`, the count planes 4 bytes and the byte planes 1 byte past a
    16-byte boundary, every byte SENT beforehand."""

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
        gh, gw = grid_shape(self.H, self.W, spec)
        self.cells = self.T * gh * gw
        self.where, cursor = {}, 0
        for key, eb, planes in (('count', 4, spec.n_cats), ('share', 1, 1), ('coverage', 1, 1), ('major', 1, 1)):
            for k in range(planes):
                begin = -(-cursor // 16) * 16 + eb
                self.where[(key, k)] = (begin, eb)
                cursor = begin + self.cells * eb + 16
        self.osize = cursor + 16
        self.obuf = obuf if obuf is not None else ctx.malloc(self.osize)
        assert self.obuf.nbytes >= self.osize and self.obuf.ptr % 16 == 0
        self.obuf.upload(np.full(self.osize, SENT, dtype=np.uint8))
        at = lambda key, k=0: self.obuf.ptr + self.where[(key, k)][0] if key in want else None
        self.out = _capi.GridOut.of(count=[at('count', k) for k in range(spec.n_cats)] if 'count' in want else (),
                                    share=at('share'), coverage=at('coverage'), major=at('major'))

    def run(self, stream=None):
        self.ctx.grid_device(self.sbuf.ptr + self.start, self.spec, self.T, self.H, self.W, self.out,
                             tile_stride=0 if self.stride == self.H * self.W else self.stride, stream=stream)

    def check(self, what, ref=None):
        """The wanted planes are the numpy statement's, every other byte of the output buffer is still SENT, and the plane
        buffer is what was uploaded."""
        ref = grid_tiles(self.tiles, self.spec) if ref is None else ref
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for (key, k), (begin, eb) in self.where.items():
            if key not in self.want:
                continue
            got = raw[begin:begin + self.cells * eb].copy().view(np.uint32 if eb == 4 else np.uint8)
            want = (ref[key][k] if key == 'count' else ref[key]).reshape(-1)
            assert np.array_equal(got, want), (what, key, k, np.flatnonzero(got != want)[:6], got[:6], want[:6])
            written[begin:begin + self.cells * eb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted planes were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.array_equal(self.sbuf.download(np.uint8, self.shost.size), self.shost), (what, 'the plane was written')
        return ref


WIDTHS = (1, 15, 16, 17, 31, 33, 61, 100, 257)
HEIGHTS = (1, 2, 5, 31, 64, 65)
TILE_COUNTS = (0, 1, 3, 17)


def cell_widths(W):
    return (1, 2, 3, 7, 16, 17, 30, 64, W, W + 5)


def cell_heights(H):
    return (1, 3, 30, H, H + 1)


@pytest.mark.parametrize('W', WIDTHS)
def test_device_entry_every_width_height_cell_count_stride_and_address(ctx, W):
    """This width x every cell width either side of a 16-byte load and of a cell boundary inside one x every height x every
    cell height; the tile counts, the stride equal to the raster and above it, the padding and the guards full of a byte that
    is an observation, the plane 0, 1 and 6 bytes past a 256-byte boundary, cycling so that every cell width meets every
    one of them; the count outputs 4 and the byte outputs 1 byte past a 16-byte boundary; every byte outside the planes
    unchanged."""
    rng = np.random.default_rng(9100 + W)
    big = max(HEIGHTS) * W
    sbuf = ctx.malloc(2 * GUARD + 256 + max(TILE_COUNTS) * (big + 3))
    obuf = ctx.malloc(7 * (4 * max(TILE_COUNTS) * big + 64) + 64)
    combos = list(itertools.product(TILE_COUNTS, (0, 3), (0, 1, 6)))
    seen, cases = set(), 0
    for H in HEIGHTS:
        for cell_h in cell_heights(H):
            for cell_w in cell_widths(W):
                n_tiles, extra, off = combos[(cases * 7 + cases // len(combos)) % len(combos)]
                spec = random_spec(rng, 1 + cases % 4, cell_h, cell_w, every_byte_observed=cases % 5 == 0)
                tiles = rng.integers(0, 256, size=(n_tiles, H, W), dtype=np.uint8)
                tiles[tiles == PAD] = PAD - 1
                r = Run(ctx, tiles, spec, stride=H * W + extra, off=off, sbuf=sbuf, obuf=obuf)
                r.run()
                ctx.synchronize()
                r.check((n_tiles, H, W, cell_h, cell_w, extra, off, spec.n_cats))
                if n_tiles:
                    info = ctx.last_kernel_info()
                    gh, gw = grid_shape(H, W, spec)
                    assert 'dswx_grid_k' in info and f'block={BLOCK}' in info and f'cells={gh}x{gw}' in info, info
                    assert f'small={int(min(cell_w, W) < PPU)}' in info and f'rows_in_flight={U}' in info, info
                seen.add((n_tiles, extra, off))
                cases += 1
    assert cases == len(HEIGHTS) * 5 * 10 and seen == set(combos)
    sbuf.free()
    obuf.free()


# Either side of what one workgroup owns.  cell_w >= 16: the whole cells that fit BLOCK units of PPU columns; cell_w < 16: the
# whole cells that fit SMALL_COLS columns; down: the cell rows that make TARGET_ROWS pixel rows, within MAX_CELLS cells; and a
# single cell wider than BLOCK units, whose threads walk several units.
JOB_SHAPES = [
    # (H, W, cell_h, cell_w)
    (3, BLOCK * PPU - 1, 2, PPU), (3, BLOCK * PPU, 2, PPU), (3, BLOCK * PPU + 1, 2, PPU),          # 256 cells of 16 columns +- 1
    (5, 30 * (BLOCK // 2) - 1, 30, 30), (5, 30 * (BLOCK // 2) + 1, 30, 30),                        # 128 cells of two units +- 1
    (3, SMALL_COLS - 1, 1, 1), (3, SMALL_COLS, 1, 1), (3, SMALL_COLS + 1, 1, 1),                    # 1024 cells of one column +- 1
    (7, 3 * (SMALL_COLS // 3) + 1, 3, 3), (4, 7 * (SMALL_COLS // 7) + 8, 2, 7),
    (TARGET_ROWS - 1, 40, 1, 40), (TARGET_ROWS, 40, 1, 40), (TARGET_ROWS + 1, 40, 1, 40),           # 32 cell rows of one row +- 1
    (2 * TARGET_ROWS + 1, 33, 2, 16), (67, 21, 11, 5),
    (2, PPU * BLOCK + 21, 2, PPU * BLOCK + 16), (3, PPU * (BLOCK + 1) + 3, 3, PPU * (BLOCK + 1) + 3),  # one cell of 257 and 258 units
    (4 * ROWS_PACKED + 1, 40, 2 * ROWS_PACKED, 20), (4 * ROWS_PACKED + 1, 40, 2 * ROWS_PACKED + 1, 20),  # widening inside a cell
]


def test_more_tiles_than_a_grid_dimension(ctx):
    """More tiles than grid.y has blocks (65535): a block walks on to tile blockIdx.y + 65535."""
    rng = np.random.default_rng(9250)
    T, H, W = 65535 + 4, 2, 3
    spec = random_spec(rng, 3, 2, 2)
    tiles = rng.integers(0, 256, size=(T, H, W), dtype=np.uint8)
    tiles[tiles == PAD] = PAD - 1
    r = Run(ctx, tiles, spec, stride=H * W + 3, off=1)
    r.run()
    ctx.synchronize()
    r.check((T, H, W))
    assert ',65535,1)' in ctx.last_kernel_info()
    r.sbuf.free()
    r.obuf.free()


@pytest.mark.parametrize('H,W,cell_h,cell_w', JOB_SHAPES)
def test_either_side_of_what_one_workgroup_owns(ctx, H, W, cell_h, cell_w):
    rng = np.random.default_rng(9200 + H + W)
    for n_cats, observed in ((2, False), (4, True)):
        spec = random_spec(rng, n_cats, cell_h, cell_w, every_byte_observed=observed)
        tiles = rng.integers(0, 256, size=(2, H, W), dtype=np.uint8)
        tiles[tiles == PAD] = PAD - 1
        r = Run(ctx, tiles, spec, stride=H * W + 3, off=1)
        r.run()
        ctx.synchronize()
        r.check((H, W, cell_h, cell_w, n_cats))
        r.sbuf.free()
        r.obuf.free()


def test_cells_that_break_packed_counters(ctx):
    """Constant planes of every category and of no category, columns and rows alternating within a unit and across units,
    on cells that are widened several times (cell_h above ROWS_PACKED) and cells with a short last unit."""
    H, W = 4 * ROWS_PACKED + 7, 75
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    rng = np.random.default_rng(9300)
    planes = [np.full((H, W), v, dtype=np.uint8) for v in (0, 1, 2, 3, 77, 255)]
    planes += [(j & 1).astype(np.uint8), ((j // PPU) & 1).astype(np.uint8), (i & 1).astype(np.uint8), ((i + j) % 4).astype(np.uint8),
               (np.arange(H * W) % 256).astype(np.uint8).reshape(H, W)]
    tiles = np.stack(planes)
    sbuf = ctx.malloc(2 * GUARD + tiles.size)
    obuf = ctx.malloc(7 * (4 * tiles.size + 64) + 64)
    for cell_h, cell_w in ((H, W), (2 * ROWS_PACKED + 3, 30), (ROWS_PACKED, 17), (ROWS_PACKED + 1, 16), (1, 1), (3, 3), (H, 5)):
        for n_cats, table in ((4, [0, 1, 2, 3] + [255] * 252), (4, list(np.arange(256) % 4)), (1, [0] * 256), (2, [1, 0] + [9] * 254),
                              (3, list(rng.integers(0, 5, size=256)))):
            r = Run(ctx, tiles, Spec(n_cats, cell_h, cell_w, table), sbuf=sbuf, obuf=obuf)
            r.run()
            ctx.synchronize()
            ref = r.check((cell_h, cell_w, n_cats))
            if (cell_h, cell_w) == (H, W) and table[:5] == [0, 1, 2, 3, 255]:
                for v in range(4):                                    # a constant tile as one cell: everything in one field
                    assert ref['count'][v, v, 0, 0] == H * W and ref['count'][:, v].sum() == H * W
                    assert ref['coverage'][v, 0, 0] == 100 and ref['major'][v, 0, 0] == v
                assert ref['share'][4, 0, 0] == NO_SHARE and ref['major'][5, 0, 0] == NONE and ref['coverage'][4, 0, 0] == 0
    sbuf.free()
    obuf.free()


def constant_tile_as_one_cell(ctx, H, W, cell_h, cell_w):
    """One constant H x W tile; the reference is stated directly (every pixel is category 1 of 2)."""
    spec = Spec(2, cell_h, cell_w, [9, 1] + [9] * 254)
    tiles = np.ones((1, H, W), dtype=np.uint8)
    gh, gw = grid_shape(H, W, spec)
    n_pix = np.outer(np.diff(np.append(np.arange(0, H, min(cell_h, H)), H)), np.diff(np.append(np.arange(0, W, min(cell_w, W)), W)))
    ref = {'count': np.stack([np.zeros((1, gh, gw), dtype=np.uint32), n_pix[None].astype(np.uint32)]),
           'share': np.zeros((1, gh, gw), dtype=np.uint8), 'coverage': np.full((1, gh, gw), 100, dtype=np.uint8),
           'major': np.ones((1, gh, gw), dtype=np.uint8)}
    r = Run(ctx, tiles, spec)
    r.run()
    ctx.synchronize()
    r.check((H, W, cell_h, cell_w), ref=ref)
    r.sbuf.free()
    r.obuf.free()
    return ref


def test_field_widths_a_cell_above_uint16(ctx):
    """One 300 x 300 cell of a single category, 90,000 pixels, beside ragged neighbours, against the numpy statement."""
    rng = np.random.default_rng(9400)
    tiles = rng.integers(0, 3, size=(1, 430, 450), dtype=np.uint8)
    tiles[0, :300, :300] = 1
    r = Run(ctx, tiles, Spec(3, 300, 300, [0, 1, 2] + [255] * 253))
    r.run()
    ctx.synchronize()
    ref = r.check('300 x 300')
    assert ref['count'][1, 0, 0, 0] == 90000 and ref['count'][0, 0, 0, 0] == 0 and ref['major'][0, 0, 0] == 1
    assert ref['count'].shape == (3, 1, 2, 2)


def test_field_widths_1024_x_1024_as_one_cell(ctx):
    ref = constant_tile_as_one_cell(ctx, 1024, 1024, 1024, 1024)
    assert ref['count'][1, 0, 0, 0] == 1 << 20


def test_field_widths_4096_x_4096_as_one_cell_and_the_refusal_above(ctx):
    """A cell of 2^24 pixels of one category: count 16,777,216, and 100 x that still fits 32 bits (the category of interest
    here, so share is 100); one row more is refused with nothing written."""
    H = W = 4096
    spec = Spec(2, H, W, [0, 1] + [9] * 254)
    tiles = np.zeros((1, H, W), dtype=np.uint8)
    r = Run(ctx, tiles, spec)
    r.run()
    ctx.synchronize()
    ref = {'count': np.array([1 << 24, 0], dtype=np.uint32).reshape(2, 1, 1, 1), 'share': np.full((1, 1, 1), 100, dtype=np.uint8),
           'coverage': np.full((1, 1, 1), 100, dtype=np.uint8), 'major': np.zeros((1, 1, 1), dtype=np.uint8)}
    r.check('4096 x 4096', ref=ref)
    assert r.obuf.download(np.uint32, 1, r.where[('count', 0)][0])[0] == 16777216
    r.obuf.upload(np.full(r.osize, SENT, dtype=np.uint8))
    with pytest.raises(_capi.DswxError, match='DSWX_GRID_MAX_CELL_PIXELS') as e:      # (the refusal reads no byte of the plane)
        ctx.grid_device(r.sbuf.ptr + r.start, Spec(2, 4097, 4096, spec.cat_of_byte), 1, 4097, 4096, r.out)
    assert e.value.code == _capi.ERR_ARG
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)


SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(KEYS, n)]


@pytest.mark.parametrize('n_cats', [1, 2, 3, 4])
def test_every_subset_of_the_outputs(ctx, n_cats):
    rng = np.random.default_rng(9500 + n_cats)
    tiles = rng.integers(0, 256, size=(3, 65, 100), dtype=np.uint8)
    spec = random_spec(rng, n_cats, 30, 17)
    sbuf = ctx.malloc(2 * GUARD + 8 + 3 * (65 * 100 + 5))
    r = None
    for want in SUBSETS:
        r = Run(ctx, tiles, spec, stride=65 * 100 + 5, off=1, want=want, sbuf=sbuf, obuf=r.obuf if r else None)
        r.run()
        ctx.synchronize()
        r.check(want)                                                # the wanted planes are right, nothing else is written
    # one count plane of several
    if n_cats > 1:
        r = Run(ctx, tiles, spec, want=('count',), sbuf=sbuf, obuf=r.obuf)
        for k in range(n_cats):
            if k != n_cats - 1:
                r.out.count[k] = None
                del r.where[('count', k)]
        r.run()
        ctx.synchronize()
        ref = grid_tiles(tiles, spec)
        raw = r.obuf.download(np.uint8, r.osize)
        begin = r.where[('count', n_cats - 1)][0]
        assert np.array_equal(raw[begin:begin + 4 * r.cells].copy().view(np.uint32), ref['count'][n_cats - 1].reshape(-1))
        raw[begin:begin + 4 * r.cells] = SENT
        assert np.all(raw == SENT)
    sbuf.free()
    r.obuf.free()


def test_refusals_write_nothing(ctx):
    rng = np.random.default_rng(9600)
    tiles = rng.integers(0, 256, size=(2, 20, 30), dtype=np.uint8)
    spec = random_spec(rng, 2, 7, 7)
    r = Run(ctx, tiles, spec)
    plane = r.sbuf.ptr + r.start
    lib, h = ctx.lib, ctx.handle
    cspec = _capi.GridSpec.of(spec)

    def call(plane=plane, cspec=cspec, n=2, H=20, W=30, stride=0, out=r.out, handle=h):
        import ctypes
        return lib.dswx_grid_device(handle, ctypes.c_void_p(plane), ctypes.byref(cspec) if cspec is not None else None, n, H, W,
                                    stride, ctypes.byref(out) if out is not None else None, None)

    def cs(**kw):
        c = _capi.GridSpec.of(spec)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    three = _capi.GridOut.of(count=[r.out.count[0], r.out.count[1], r.out.count[0]])
    off = _capi.GridOut.of(count=[r.out.count[0] + 2])
    for rc, kw in ((_capi.ERR_ARG, {'cspec': None}), (_capi.ERR_ARG, {'out': None}), (_capi.ERR_ARG, {'cspec': cs(n_cats=0)}),
                   (_capi.ERR_ARG, {'cspec': cs(n_cats=5)}), (_capi.ERR_ARG, {'cspec': cs(cell_h=0)}), (_capi.ERR_ARG, {'cspec': cs(cell_w=-1)}),
                   (_capi.ERR_ARG, {'n': -1}), (_capi.ERR_ARG, {'H': -1}), (_capi.ERR_ARG, {'W': -1}), (_capi.ERR_ARG, {'stride': -1}),
                   (_capi.ERR_ARG, {'stride': 599}), (_capi.ERR_ARG, {'out': _capi.GridOut.of()}), (_capi.ERR_ARG, {'out': three}),
                   (_capi.ERR_ARG, {'plane': None}), (_capi.ERR_ALIGN, {'out': off}), (_capi.ERR_ARG, {'handle': None})):
        assert call(**kw) == rc, kw
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    # arguments before the context: a bad spec AND no context names the spec
    assert call(cspec=cs(n_cats=9), handle=None) == _capi.ERR_ARG and 'n_cats' in lib.dswx_last_error().decode()
    # an empty raster and no tiles are legal and write nothing
    for kw in ({'n': 0}, {'H': 0}, {'W': 0}):
        assert call(**kw) == 0, kw
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    r.run()
    ctx.synchronize()
    r.check('after the refusals')


def test_on_a_callers_stream_behind_the_kernel_that_writes_the_plane(ctx):
    """Asynchronous on the caller's stream: the stream is held, a copy kernel that REPLACES the plane is queued on it, then the
    entry, with no synchronisation in between.  The entry returns while the hold is pending, and the planes are those of the
    replaced plane -- launched on any other stream it would read the old one."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(9700)
    T, H, W = 6, 300, 257
    n, stride = H * W, H * W + 5
    spec = Spec(2, 30, 30, np.arange(256) % 3)
    old = rng.integers(0, 100, size=T * stride, dtype=np.uint8)
    new = rng.integers(100, 256, size=T * stride, dtype=np.uint8)
    plane = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    gh, gw = grid_shape(H, W, spec)
    cells = T * gh * gw
    share = torch.full((cells,), SENT, dtype=torch.uint8, device='cuda:0')
    count1 = torch.full((cells,), 0x11111111, dtype=torch.int32, device='cuda:0')
    torch.cuda.synchronize()
    rasters = lambda a: np.stack([a[t * stride:t * stride + n].reshape(H, W) for t in range(T)])
    want_old, want_new = grid_tiles(rasters(old), spec), grid_tiles(rasters(new), spec)
    assert not np.array_equal(want_old['share'], want_new['share'])
    out = _capi.GridOut.of(count=[None, count1.data_ptr()], share=share.data_ptr())
    s = torch.cuda.Stream(device=0)
    ctx.grid_device(plane.data_ptr(), spec, T, H, W, out, tile_stride=stride, stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(share.cpu().numpy(), want_old['share'].reshape(-1))
    with torch.cuda.stream(s):
        torch.cuda._sleep(int(1.2e9))                       # some hundreds of milliseconds at any shader clock
        held = torch.cuda.Event()
        held.record(s)
        plane.copy_(src)
    t0 = time.perf_counter()
    ctx.grid_device(plane.data_ptr(), spec, T, H, W, out, tile_stride=stride, stream=s.cuda_stream)
    dt = time.perf_counter() - t0
    assert not held.query(), f'the entry took {dt * 1e3:.1f} ms on the host: it waited for the stream'
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(share.cpu().numpy(), want_new['share'].reshape(-1))
    assert np.array_equal(count1.cpu().numpy().view(np.uint32), want_new['count'][1].reshape(-1))
    assert torch.equal(plane, src)


def download(res, spec, shape):
    got = {k: res[k].download(np.uint32 if k == 'count' else np.uint8, int(np.prod(shape)) * (spec.n_cats if k == 'count' else 1))
           for k in res}
    for k in got:
        got[k] = got[k].reshape(((spec.n_cats,) if k == 'count' else ()) + tuple(shape))
    for b in res.values():
        b.free()
    return got


FORMS = {'packed': {}, 'separate_outputs': {'separate_outputs': True}, 'slide_placed': {'sliding_outputs': True},
         'padded': {'tile_align': 256}, 'contiguous': {'tile_align': 1}}


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('n_tiles,h,w', [(5, 100, 37), (3, 129, 97)])
def test_batch_grid_on_every_form_of_batch(ctx, form, n_tiles, h, w):
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, **FORMS[form])
    try:
        batch.synth(SEED, tile0=31)
        p = _capi.default_params()
        if form == 'slide_placed':
            batch.place_slide(p, slack_bytes=24 << 20, step_bytes=2 << 20, spread_gaps=2, refine_passes=1, launches=2,
                              keep_free_bytes=0)
        batch.classify(p)
        assert (batch.tile_stride == h * w) == (form == 'contiguous')
        bwtr = Spec(2, 16, 5, [1, 0] + [255] * 254)                  # BWTR: 1 water, 0 not water
        for name, spec in (('wtr', wtr_grid_spec(30)), ('wtr', wtr_grid_spec(7, partial_is_water=False)), ('bwtr', bwtr),
                           ('fmask', Spec(4, 33, 64, np.arange(256) % 5))):
            tiles = np.stack([batch.read_tile(name, t) for t in range(n_tiles)])
            gh, gw = grid_shape(h, w, spec)
            res = batch.grid(name, spec)                             # same stream as the classification; None = all tiles
            info = ctx.last_kernel_info()
            ctx.synchronize()
            assert info.count('dswx_grid_k') == 1 and f'cells={gh}x{gw}' in info, info
            got, want = download(res, spec, (n_tiles, gh, gw)), grid_tiles(tiles, spec)
            assert list(got) == list(KEYS)
            for k in KEYS:
                assert np.array_equal(got[k], want[k]), (name, k, np.argwhere(got[k] != want[k])[:4])
            assert int(want['count'].sum()) > 0, name                # the layer is not all fill
            for tile0, count in ((1, n_tiles - 1), (0, 1), (n_tiles - 1, None), (1, _capi.BATCH_ALL_TILES), (n_tiles, None), (0, 0)):
                res = batch.grid(name, spec, tile0=tile0, n_tiles=count, want=('share', 'major'))
                ctx.synchronize()
                sub = tiles[tile0:] if count in (None, _capi.BATCH_ALL_TILES) else tiles[tile0:tile0 + count]
                got, want = download(res, spec, (len(sub), gh, gw)), grid_tiles(sub, spec)
                assert list(got) == ['share', 'major']
                for k in got:
                    assert np.array_equal(got[k], want[k]), (name, tile0, count, k)
        # planes that are not uint8, the counters, a plane this batch does not have; tile ranges outside the batch
        spec = wtr_grid_spec(30)
        for name in ('blue', 'swir2', 'diag'):
            with pytest.raises(_capi.DswxError, match=r'band\[|diag') as e:
                batch.grid(name, spec)
            assert e.value.code == _capi.ERR_ARG and 'uint8' in str(e.value)
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.grid('counters', spec)
        assert e.value.code == _capi.ERR_ARG
        for name in ('land', 'browse'):
            with pytest.raises(_capi.DswxError, match=name) as e:
                batch.grid(name, spec)
            assert e.value.code == _capi.ERR_ARG and 'no plane' in str(e.value)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside the batch'):
                batch.grid('wtr', spec, tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(ValueError):
            batch.grid('water', spec)
    finally:
        batch.free()


def test_device_plane_grid_feeds_histogram_and_stack(ctx):
    """DevicePlane.grid, and its results as planes like any other: the share plane histogrammed on the device, and stacked
    through a thresholding table (cells at least half water / less / without an observation), with no download in between."""
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9800)
    try:
        a = rng.choice(np.array([0, 1, 2, 252, 253, 254, 255, 9], dtype=np.uint8), size=(4, 100, 130))
        p = eng.upload(a)
        for spec, want_keys in ((wtr_grid_spec(30), KEYS), (Spec(3, 7, 16, np.arange(256) % 5), KEYS), (wtr_grid_spec(3), ('share',))):
            got = p.grid(spec, want=want_keys)
            want = grid_tiles(a, spec)
            gh, gw = grid_shape(100, 130, spec)
            names = ([f'count{k}' for k in range(spec.n_cats)] if 'count' in want_keys else []) + [k for k in KEYS[1:] if k in want_keys]
            assert list(got) == names
            for name, plane in got.items():
                ref = want['count'][int(name[5:])] if name.startswith('count') else want[name]
                assert plane.shape == (4, gh, gw) and plane.dtype == ref.dtype
                assert np.array_equal(plane.numpy(), ref), name
            share = p.grid(spec, want=('share',))['share']           # (a fresh plane: nothing of it has been downloaded)
            assert np.array_equal(share.histogram(), np.bincount(want['share'].reshape(-1), minlength=256).astype(np.uint64))
            half = StackSpec(2, np.where(np.arange(256) >= 50, 0, 1).astype(np.uint8) + 254 * (np.arange(256) > 100).astype(np.uint8), 255)
            often = share.stack(half, want=('count', 'share'))
            ref = stack_tiles(want['share'], half)
            assert np.array_equal(often['count0'].numpy(), ref['count'][0]) and np.array_equal(often['count1'].numpy(), ref['count'][1])
            assert np.array_equal(often['share'].numpy(), ref['share'])
            assert share._host is None
            for plane in list(got.values()) + list(often.values()) + [share]:
                plane.release()
        one = eng.upload(a[0])                                       # a single raster [H, W]
        got = one.grid(wtr_grid_spec(30), want=('major',))
        assert got['major'].shape == (1, 4, 5) and np.array_equal(got['major'].numpy(), grid_tiles(a[:1], wtr_grid_spec(30))['major'])
        p.release()
        with pytest.raises(ValueError):
            eng.upload(np.zeros((4,), dtype=np.uint8)).grid(wtr_grid_spec(2))
        with pytest.raises(ValueError):
            eng.upload(np.zeros((2, 4, 4), dtype=np.uint16)).grid(wtr_grid_spec(2))
    finally:
        eng.close()


@pytest.fixture(scope='module')
def product_file(tmp_path_factory):
    """The multi-band product file of the suite's own synthetic product run (tools/make_synthetic_hls.py, 301 x 301)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    from proteus_amd import dswx_hls
    tmp = tmp_path_factory.mktemp('grid_product')
    _, files, _, _ = synth_hls.make(str(tmp), size=301, tile=4)
    out = str(tmp / 'product.tif')
    assert dswx_hls.generate_dswx_layers(files, out) is True
    return out


def test_the_command_line_tool(product_file, tmp_path, capsys):
    """bin/dswx_grid.py on a product file: the three files are the numpy statement of band 1, Byte COGs with nodata 255, the
    input's tie point and N times its pixel scale."""
    spec = importlib.util.spec_from_file_location('dswx_grid_tool', os.path.join(ROOT, 'bin', 'dswx_grid.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    bands, info = geotiff.read_geotiff(product_file)
    wtr = bands[0] if bands.ndim == 3 else bands
    H, W = wtr.shape
    gt = tuple(info.geotransform)
    for flags, cell, partial in (([], 30, True), (['--no-partial'], 7, False)):
        prefix = str(tmp_path / f'out{cell}')
        assert tool.main(flags + ['--cell', str(cell), '-o', prefix, product_file]) == 0
        gspec = wtr_grid_spec(cell, partial_is_water=partial)
        want = grid_tiles(wtr[None], gspec)
        gh, gw = grid_shape(H, W, gspec)
        for suffix, key in (('SHARE', 'share'), ('COVERAGE', 'coverage'), ('MAJOR', 'major')):
            path = f'{prefix}_{suffix}.tif'
            arr, out = geotiff.read_geotiff(path)
            assert arr.dtype == np.uint8 and arr.shape == (gh, gw) and np.array_equal(arr, want[key][0]), suffix
            assert geotiff.validate_cog(path) == [], suffix
            assert out.nodata == 255
            assert tuple(out.geotransform) == (gt[0], gt[1] * cell, gt[2], gt[3], gt[4], gt[5] * cell), (out.geotransform, gt)
            assert out.geo_tags.get(geotiff.TAG_GEOKEYS) == info.geo_tags.get(geotiff.TAG_GEOKEYS)
            assert out.metadata['GRID_CELL_PIXELS'] == str(cell) and out.metadata['GRID_INPUT_FILE'] == os.path.basename(product_file)
        assert len(np.unique(want['share'])) > 2
    capsys.readouterr()
    assert tool.main(['--cell', '0', '-o', str(tmp_path / 'no'), product_file]) == 1
    assert tool.main(['--cell', '30', '--band', '99', '-o', str(tmp_path / 'no'), product_file]) == 1
    assert tool.main(['--cell', '30', '-o', str(tmp_path / 'no'), str(tmp_path / 'missing.tif')]) == 1
    assert not os.path.exists(str(tmp_path / 'no_SHARE.tif'))


def test_grid_example_runs(tmp_path):
    """examples/batch_grid.c: its own checks (exit status 0: every cell of the device planes against its loop over the
    downloaded layer and against dswx_grid_host)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_grid')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_grid.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '5', '301'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr grid: device, loop and host entry agree in every cell' in r.stdout
    assert '5 tiles of 301 x 301 pixels, 11 x 11 cells of 30 x 30' in r.stdout
