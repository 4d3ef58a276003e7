"""The ABI v6 raster-format entries (proteus_amd/csrc/dswx_writer.hip) over their whole sample domain and at awkward
addresses: the named domains of oracle/raster_inputs.py through dswx_cog_blocks_device, dswx_untile_device,
dswx_convolve_axis_device, dswx_rgb_planes_device, dswx_to_byte_device, dswx_gather_2d_device and dswx_copy_2d_device,
against the host writer's whole-array statements (proteus_amd/geotiff.py, dswx_hls._gdal_byte) and the element-by-element
ones of oracle/cog_oracle.py, which tests/test_raster_domain.py shows to agree with each other on these inputs.

Everything is bit-exact.  The one rule about NaN: entries that move bytes (PREDICTOR=3 both ways, gather, 2-D copy) must
reproduce NaN bits; an invalid RGB pixel is exactly the quiet NaN np.nan stores; arithmetic outputs (the CUBICSPLINE
pyramid, the Byte conversion) must have NaN at the same positions, and everything else is compared as unsigned integers,
the sign of zero included.

Addresses: planes sit at sample-aligned but otherwise odd offsets inside their allocation (+1 / +3 bytes for 8-bit, +2 / +6
for 16-bit, +4 / +12 for 32-bit samples), every output lies between two guards of 256 bytes, and every call runs twice
over outputs pre-filled with two different sentinels: the guards must keep the sentinel, and the two results must be the
same bytes, so that no output byte was left unwritten."""
import ctypes

import numpy as np
import pytest

from oracle import cog_oracle as co, raster_inputs as R
from proteus_amd import _capi, dswx_hls as D, geotiff
from tests import test_gpu_streams as S          # (imports torch before this process opens the GPU, as that module needs it)
from tests.test_raster_domain import host_pyramid, same_floats

pytestmark = pytest.mark.gpu

FACTORS = geotiff.COG_OVERVIEW_FACTORS
GUARD = 256
SENTINELS = (0xA5, 0x5A)
OFFS = {1: (1, 3), 2: (2, 6), 4: (4, 12), 8: (8, 24)}
ERR_ALIGN = -5                                   # DSWX_ERR_ALIGN (include/dswx_hip.h)
PLANES = R.f32_planes()
PLANE_IDS = [p[0] for p in PLANES]


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Span:
    """`nbytes` at a chosen offset past a 256-byte boundary, a guard of 256 bytes either side."""

    def __init__(self, ctx, nbytes, off=0):
        self.ctx, self.nbytes, self.lo = ctx, int(nbytes), GUARD + int(off)
        self.buf = ctx.malloc(self.nbytes + 2 * GUARD + 32)
        self.ptr = self.buf.ptr + self.lo
        self.sent = None

    def fill(self, sent):
        self.sent = sent
        _capi._check(self.ctx.lib.dswx_memset_d(self.ctx.handle, ctypes.c_void_p(self.buf.ptr), sent, self.buf.nbytes))

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        if arr.nbytes:
            self.buf.upload(arr.reshape(-1).view(np.uint8), self.lo)
        return self

    def get(self):
        """The payload, after the guards were seen untouched."""
        whole = self.buf.download(np.uint8, self.buf.nbytes)
        assert (whole[:self.lo] == self.sent).all(), 'bytes before the output were written'
        assert (whole[self.lo + self.nbytes:] == self.sent).all(), 'bytes after the output were written'
        return whole[self.lo: self.lo + self.nbytes]

    def untouched(self):
        return bool((self.buf.download(np.uint8, self.buf.nbytes) == self.sent).all())


class Dev:
    """The spans of one case; freed together."""

    def __init__(self, ctx):
        self.ctx, self.spans = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        for s in self.spans:
            s.buf.free()

    def span(self, nbytes, off=0):
        s = Span(self.ctx, max(int(nbytes), 1), off)
        self.spans.append(s)
        return s

    def put(self, arr, off=0):
        s = self.span(np.asarray(arr).nbytes, off)
        s.fill(0xEE)
        return s.put(arr)

    def run(self, outs, launch, twice=True):
        """launch() over `outs` filled with each sentinel in turn -> their payloads (uint8)."""
        res = []
        for sent in SENTINELS[:2 if twice else 1]:
            for o in outs:
                o.fill(sent)
            launch()
            self.ctx.synchronize()
            res.append([o.get() for o in outs])
        if twice:
            for a, b in zip(*res):
                assert np.array_equal(a, b), 'an output byte kept its sentinel: not every byte was written'
        return res[0]


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _plane(k, shape, salt=0):
    name, domain, variant = PLANES[k]
    return R.f32_plane(domain, _rng(k, shape[0], shape[1], salt), shape, variant)


# ---- PREDICTOR=3 both ways ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(PLANES)), ids=PLANE_IDS)
def test_predictor_3_moves_bits_both_ways(ctx, k):
    """Tiles of 16 and 512, a block larger than the raster, strips; widths of every residue mod 4."""
    cases = [((37, 52 + r), 16, True) for r in range(4)] + [((21, 50), 64, True), ((530, 1027 + k % 4), 512, False)]
    for i, (shape, tile, small) in enumerate(cases):
        a = _plane(k, shape)
        h, w = shape
        lay = _capi.cog_layout(h, w, 4, (), tile)
        with Dev(ctx) as d:
            src, out = d.put(a, OFFS[4][i % 2]), d.span(lay['total_bytes'])
            got, = d.run([out], lambda: ctx.cog_blocks_device(src.ptr, 4, h, w, out.ptr, (), tile, 3))
            host = geotiff.blocked_level(a[None], tile, 3)
            assert np.array_equal(got, np.asarray(host.data).reshape(-1).view(np.uint8)), (shape, tile)
            if small:
                assert np.array_equal(got, co.blocks(a, tile, 3)), (shape, tile)
            blk, back = d.put(got, OFFS[4][(i + 1) % 2]), d.span(a.nbytes, OFFS[4][i % 2])
            res, = d.run([back], lambda: ctx.untile_device(blk.ptr, 4, h, w, tile, tile, 3, back.ptr))
            assert res.tobytes() == a.tobytes(), (shape, tile)
            # strips: the raster's own width, 7 rows each, the last one short (its slot padded)
            bh = 7
            pad = np.zeros((-(-h // bh) * bh, w), np.float32)
            pad[:h] = a
            strips = np.frombuffer(geotiff._fp_predictor_encode(pad), np.uint8)
            if small:
                assert co.unblocks(strips, np.float32, h, w, w, bh, 3).tobytes() == a.tobytes()
            blk2 = d.put(strips, OFFS[4][i % 2])
            res, = d.run([back], lambda: ctx.untile_device(blk2.ptr, 4, h, w, w, bh, 3, back.ptr))
            assert res.tobytes() == a.tobytes(), (shape, 'strips')


# ---- PREDICTOR 2 / 1 ----------------------------------------------------------------------------------------------------
BLOCK_WIDTHS = (1, 7, 511, 512, 513, 1024, 1031, 3660)       # one to eight chunks of 512 elements; 3660: strips


@pytest.mark.parametrize('dtype', R.INT_DTYPES, ids=[np.dtype(t).name for t in R.INT_DTYPES])
@pytest.mark.parametrize('domain', R.INT_DOMAINS)
def test_untile_predictor_2_and_1(ctx, domain, dtype):
    """The running sum of every block row (wave scan + the carry across chunks of 512 elements) in 8, 16 and 32 bits."""
    es = np.dtype(dtype).itemsize
    bh, H = 3, 5                                              # two rows of blocks, the second one short
    for i, bw in enumerate(BLOCK_WIDTHS):
        W = bw if bw == 3660 else 2 * bw + (bw + 1) // 2      # three blocks across, the last one cut
        across, down = -(-W // bw), -(-H // bh)
        vals = R.int_rows(domain, _rng(R.INT_DOMAINS.index(domain), es, bw), across * down * bh, bw, dtype)
        want = vals.reshape(down, across, bh, bw).transpose(0, 2, 1, 3).reshape(down * bh, across * bw)[:H, :W]
        for predictor in (2, 1):
            staged = R.differenced(vals) if predictor == 2 else vals
            raw = np.ascontiguousarray(staged).reshape(-1).view(np.uint8)
            assert np.array_equal(co.unblocks(raw, dtype, H, W, bw, bh, predictor), want), (bw, predictor)
            with Dev(ctx) as d:
                blk, out = d.put(raw, OFFS[es][i % 2]), d.span(H * W * es, OFFS[es][(i + 1) % 2])
                got, = d.run([out], lambda: ctx.untile_device(blk.ptr, es, H, W, bw, bh, predictor, out.ptr))
                assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (domain, dtype, bw, predictor)


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16], ids=['uint8', 'uint16'])
def test_cog_blocks_predictor_2_across_block_boundaries(ctx, dtype):
    """The forward direction: rows whose differences wrap run across the block boundaries of tiles of 512 and 16."""
    es = np.dtype(dtype).itemsize
    i = 0
    for H, W, tile, oracle in ((20, 1100, 512, True), (37, 1100, 16, True), (9, 3660, 512, False)):
        for domain in ('wrap', 'carry', 'full', 'runs'):
            a = R.int_rows(domain, _rng(H, W, es, R.INT_DOMAINS.index(domain)), H, W, dtype)
            lay = _capi.cog_layout(H, W, es, (), tile)
            i += 1
            with Dev(ctx) as d:
                src, out = d.put(a, OFFS[es][i % 2]), d.span(lay['total_bytes'])
                for predictor in (2, 1):
                    got, = d.run([out], lambda: ctx.cog_blocks_device(src.ptr, es, H, W, out.ptr, (), tile, predictor))
                    host = geotiff.blocked_level(a[None], tile, predictor)
                    assert np.array_equal(got, np.asarray(host.data).reshape(-1).view(np.uint8)), (H, W, tile, domain, predictor)
                    if oracle and predictor == 2 and domain != 'runs':
                        assert np.array_equal(got, co.blocks(a, tile, 2)), (H, W, tile, domain)


# ---- the NEAREST pick, every size ---------------------------------------------------------------------------------------
SWEEP_MAX = 4200
# a call takes DSWX_COG_MAX_LEVELS - 1 = 7 factors: (2, 3, 4, 5, 7, 16, 64, 128) goes in two calls, the second one the reference's
FACTOR_SETS = ((2, 3, 4, 5, 7, 16, 64), FACTORS)
SWEEP_TILE = 8
SWEEP_BATCH = 200


def _sweep_plane(n, axis):
    """A plane of 2 x n (axis 'width') or n x 2 whose values are their own index along the swept axis."""
    row = np.arange(n, dtype=np.uint16)
    a = np.stack([row, 65535 - row])
    return a if axis == 'width' else np.ascontiguousarray(a.T)


def _blocks_u16(r, tile):
    h, w = r.shape
    down, across = -(-h // tile), -(-w // tile)
    pad = np.zeros((down * tile, across * tile), np.uint16)
    pad[:h, :w] = r
    return pad.reshape(down, tile, across, tile).transpose(0, 2, 1, 3).tobytes()


@pytest.mark.parametrize('axis', ['width', 'height'])
def test_nearest_pick_at_every_size(ctx, axis):
    """Every width 1 .. 4200 (height 2) and every height 1 .. 4200 (width 2), factors 2, 3, 4, 5, 7, 16, 64, 128 and the
    reference's: each level of each size against geotiff.overview_nearest, one size in eight (and every size to 64) against
    cog_oracle.nearest_overview as well.  The launches of 200 sizes go out together; no size is left out."""
    sizes = list(range(1, SWEEP_MAX + 1))
    assert 128 * 7 < SWEEP_MAX <= 65535
    planes = {n: _sweep_plane(n, axis) for n in sizes}
    at, cur = {}, 0
    for n in sizes:
        at[n] = cur
        cur += planes[n].nbytes
    with Dev(ctx) as d:
        src = d.put(np.concatenate([planes[n].reshape(-1) for n in sizes]), OFFS[2][0])
        checked = 0
        for b0 in range(0, len(sizes), SWEEP_BATCH):
            batch = sizes[b0: b0 + SWEEP_BATCH]
            jobs, total = [], 0
            for n in batch:
                h, w = planes[n].shape
                for fs in FACTOR_SETS:
                    lay = _capi.cog_layout(h, w, 2, fs, SWEEP_TILE)
                    assert total % 16 == 0
                    jobs.append((n, fs, lay, total))
                    total += lay['total_bytes']
            out = d.span(total)
            out.fill(SENTINELS[0])
            for n, fs, lay, off in jobs:
                h, w = planes[n].shape
                ctx.cog_blocks_device(src.ptr + at[n], 2, h, w, out.ptr + off, fs, SWEEP_TILE, 1)
            ctx.synchronize()
            got = out.get()
            d.spans.remove(out)
            out.buf.free()
            for n, fs, lay, off in jobs:
                a = planes[n]
                want = [a] + [geotiff.overview_nearest(a, f) for f in fs if a.shape != (1, 1)]
                assert lay['n_levels'] == len(want), (n, fs)
                for lv, r, f in zip(lay['levels'], want, (1,) + tuple(fs)):
                    assert (lv['height'], lv['width']) == r.shape, (n, f)
                    exp = _blocks_u16(r, SWEEP_TILE)
                    lo = off + lv['offset_bytes']
                    assert got[lo: lo + len(exp)].tobytes() == exp, (axis, n, f)
                    if f > 1 and (n % 8 == 0 or n <= 64):
                        assert np.array_equal(co.nearest_overview(a, f), r), (axis, n, f)
                    checked += 1
        assert checked >= (SWEEP_MAX - 1) * (len(FACTOR_SETS[0]) + len(FACTOR_SETS[1]) + 2)


# ---- the CUBICSPLINE pyramid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(len(PLANES)), ids=PLANE_IDS)
def test_cubicspline_pyramid_over_the_float32_domains(ctx, k):
    from proteus_amd import pipeline
    eng = pipeline.TileEngine(ctx)
    try:
        for shape in ((700, 333), (513, 1025), (129, 4097), (37, 53), (5, 3)):
            a = _plane(k, shape)
            got = [g.numpy() for g in eng._float_pyramid(eng.upload(a), FACTORS)]
            want = host_pyramid(a)
            assert len(got) == len(want)
            for lvl, (g, w) in enumerate(zip(got, want)):
                assert same_floats(np.asarray(g), w), (PLANES[k][0], shape, lvl)
            if shape[0] < 100:
                for lvl, (g, w) in enumerate(zip(got, co.cubicspline_pyramid(a, FACTORS))):
                    assert same_floats(np.asarray(g), w), (PLANES[k][0], shape, lvl, 'oracle')
    finally:
        eng.close()


# ---- dswx_convolve_axis_device itself -----------------------------------------------------------------------------------
def _odd_taps(rng, n_in, n_out, taps):
    """Taps that are not a B-spline: windows that start before the line and end after it (clamped reads), zero weights, one
    output with no weight at all."""
    first = rng.integers(-taps, n_in, size=n_out)
    w = rng.random((n_out, taps))
    w[rng.random((n_out, taps)) < 0.3] = 0.0
    w[0] = 0.0
    return first, w


GUARD_VALUE = 3.0e4                              # what surrounds the window in the source raster


@pytest.mark.parametrize('src64,dst64', [(False, False), (False, True), (True, False), (True, True)],
                         ids=['f32-f32', 'f32-f64', 'f64-f32', 'f64-f64'])
def test_convolve_axis_type_pairs_windows_and_strides(ctx, src64, dst64):
    """All four instantiations on a window inside a larger raster, rows as lines (line stride > element stride) and columns
    as lines (line stride 1: the vertical pass), B-spline taps up to the 513 of a direct factor-128 level and taps of another
    shape, against the float64 statement evaluated in tap order from the same `first` and `weights`."""
    ti, to = (np.float64 if src64 else np.float32), (np.float64 if dst64 else np.float32)
    es_i, es_o = np.dtype(ti).itemsize, np.dtype(to).itemsize
    rng = _rng(7, src64, dst64)
    geoms = [(9, 70, geotiff.convolve_weights(70, 18)), (6, 70, _odd_taps(rng, 70, 23, 9)), (5, 1536, geotiff.convolve_weights(1536, 12)),
             (300, 40, geotiff.convolve_weights(40, 40))]
    assert geoms[2][2][1].shape[1] == 513
    case = 0
    for n_lines, n_in, (first, w) in geoms:
        n_out, taps = w.shape
        inputs = [R.f32_plane(dom, rng, (n_lines, n_in), var) for _, dom, var in PLANES if n_lines < 100 or dom in ('bits', 'tiny')]
        with np.errstate(invalid='ignore'):
            inputs = [v.astype(ti) for v in inputs]
        if src64:
            inputs += [R.f64_lines(dom, rng, (n_lines, n_in)) for dom in R.F64_DOMAINS]
        for lines in inputs:
            ref = co.convolve_axis(lines, first, w)
            with np.errstate(over='ignore', invalid='ignore'):
                want = ref.astype(to)
            for vertical in (False, True):
                case += 1
                y0, x0 = 3, 5
                win = lines.T if vertical else lines
                raster = np.full((win.shape[0] + 6, win.shape[1] + 11), GUARD_VALUE, ti)
                raster[y0: y0 + win.shape[0], x0: x0 + win.shape[1]] = win
                RW = raster.shape[1]
                res = want.T if vertical else want
                DH, DW = res.shape[0] + 6, res.shape[1] + 9
                with Dev(ctx) as d:
                    src = d.put(raster, OFFS[es_i][case % 2])
                    d_first = d.put(first.astype(np.int32), OFFS[4][case % 2])
                    d_w = d.put(np.ascontiguousarray(w.T), OFFS[8][case % 2])
                    out = d.span(DH * DW * es_o, OFFS[es_o][(case + 1) % 2])
                    sp, dp = src.ptr + (y0 * RW + x0) * es_i, out.ptr + (3 * DW + 4) * es_o
                    if vertical:
                        launch = lambda: ctx.convolve_axis_device(sp, src64, n_lines, n_in, 1, RW, n_out, taps, d_first.ptr, d_w.ptr,  # noqa: E731
                                                                  dp, dst64, 1, DW)
                    else:
                        launch = lambda: ctx.convolve_axis_device(sp, src64, n_lines, n_in, RW, 1, n_out, taps, d_first.ptr, d_w.ptr,  # noqa: E731
                                                                  dp, dst64, DW, 1)
                    for sent in SENTINELS:           # (the window's surroundings keep the sentinel: each run is checked on its own)
                        out.fill(sent)
                        launch()
                        ctx.synchronize()
                        img = out.get().reshape(DH, DW * es_o).copy()
                        cut = img[3: 3 + res.shape[0], 4 * es_o: (4 + res.shape[1]) * es_o]
                        assert same_floats(np.ascontiguousarray(cut).view(to), np.ascontiguousarray(res)), (n_lines, n_in, taps, vertical)
                        cut[:] = sent
                        assert (img == sent).all(), 'written outside the destination window'
    # a float32 store that overflows, and one that lands in the denormal range, did happen (float64 source)
    if src64 and not dst64:
        first, w = geotiff.convolve_weights(70, 18)
        with np.errstate(over='ignore'):
            big = co.convolve_axis(R.f64_lines('beyond_f32', rng, (9, 70)), first, w).astype(np.float32)
        assert np.isinf(big).any()


# ---- RGB planes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('band', range(3))
def test_rgb_planes_over_every_int16_value(ctx, band):
    n = 65536
    for k in range(len(R.RGB_SCALE_OFFSET)):
        bands, diag, scales, offsets = R.rgb_case(band, k)
        with Dev(ctx) as d:
            db = [d.put(b, OFFS[2][(c + k) % 2]) for c, b in enumerate(bands)]
            dd = d.put(diag, OFFS[2][k % 2])
            out = d.span(3 * n * 4, OFFS[4][k % 2])
            for clip in (True, False):
                for use_diag in (True, False):
                    got, = d.run([out], lambda: ctx.rgb_planes_device(db[0].ptr, db[1].ptr, db[2].ptr, dd.ptr if use_diag else None, n,
                                                                      scales, offsets, clip, out.ptr))
                    got = got.view(np.uint32).reshape(3, n)
                    oracle = co.rgb_planes(bands, diag if use_diag else None, scales, offsets, clip=clip)
                    for c in range(3):
                        want = R.rgb_statement(bands[c], scales[c], offsets[c], clip, diag if use_diag else None)
                        assert np.array_equal(got[c], want.view(np.uint32)), (band, k, clip, use_diag, c)
                        assert np.array_equal(got[c], oracle[c].view(np.uint32)), (band, k, clip, use_diag, c, 'oracle')
                        if use_diag:
                            assert (got[c][diag == 65535] == R.QUIET_NAN_BITS).all()


# ---- the Byte conversion ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['edges', 'exponents', 'random'])
def test_to_byte_float32(ctx, which):
    a = {'edges': R.byte_edges, 'exponents': R.byte_exponent_sweep, 'random': R.byte_random}[which]()
    with Dev(ctx) as d:
        src, out = d.put(a, OFFS[4][which == 'edges']), d.span(a.size, OFFS[1][which != 'edges'])
        got, = d.run([out], lambda: ctx.to_byte_device(src.ptr, np.float32, a.size, out.ptr), twice=which != 'random')
    assert np.array_equal(got, co.gdal_byte_vec(a)), which
    assert np.array_equal(got, D._gdal_byte(a)), which
    if which == 'edges':
        assert np.array_equal(got, co.gdal_byte(a))


@pytest.mark.parametrize('dtype', [np.uint16, np.int16], ids=['uint16', 'int16'])
def test_to_byte_every_16_bit_value_at_an_offset_address(ctx, dtype):
    a = np.arange(65536, dtype=np.uint16).view(dtype)
    for i in range(2):
        with Dev(ctx) as d:
            src, out = d.put(a, OFFS[2][i]), d.span(a.size, OFFS[1][i])
            got, = d.run([out], lambda: ctx.to_byte_device(src.ptr, dtype, a.size, out.ptr))
        assert np.array_equal(got, co.gdal_byte(a)) and np.array_equal(got, D._gdal_byte(a))


# ---- gather and 2-D copy ------------------------------------------------------------------------------------------------
def _bit_planes(shape):
    return [R.f32_plane('bits', _rng(1, *shape), shape).view(np.uint32), R.f32_plane('edges', _rng(2, *shape), shape).view(np.uint32),
            R.int_rows('full', _rng(3, *shape), shape[0], shape[1], np.uint8), R.int_rows('full', _rng(4, *shape), shape[0], shape[1], np.uint16)]


def test_gather_2d_preserves_bits(ctx):
    H, W = 61, 83
    rng = _rng(5)
    rows = np.concatenate([[0, 0, H - 1, H - 1, 17, 0, H - 1], rng.integers(0, H, size=40)]).astype(np.int32)
    cols = np.concatenate([[W - 1, W - 1, 0, 0, 31, W - 1, 0], rng.integers(0, W, size=300)]).astype(np.int32)
    for i, a in enumerate(_bit_planes((H, W))):
        es = a.dtype.itemsize
        want = a[rows][:, cols]
        with Dev(ctx) as d:
            src, dr, dc = d.put(a, OFFS[es][i % 2]), d.put(rows, OFFS[4][i % 2]), d.put(cols, OFFS[4][(i + 1) % 2])
            out = d.span(want.nbytes, OFFS[es][(i + 1) % 2])
            got, = d.run([out], lambda: ctx.gather_2d_device(src.ptr, es, H, W, dr.ptr, rows.size, dc.ptr, cols.size, out.ptr))
        assert got.tobytes() == np.ascontiguousarray(want).tobytes(), a.dtype


def test_copy_2d_odd_pitches_preserve_bits(ctx):
    rows = 50
    for i, a in enumerate(_bit_planes((rows, 64))):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(rows, -1)
        src_pitch, dst_pitch = raw.shape[1] + 1 + 2 * (i % 2), raw.shape[1] + 7
        width = raw.shape[1] - (0 if a.dtype.itemsize == 4 else 5)
        pitched = np.full((rows, src_pitch), 0x11, np.uint8)
        pitched[:, :raw.shape[1]] = raw
        with Dev(ctx) as d:
            src, out = d.put(pitched, OFFS[1][i % 2]), d.span(rows * dst_pitch, OFFS[1][(i + 1) % 2])
            sent = SENTINELS[0]
            got, = d.run([out], lambda: ctx.copy_2d_device(out.ptr, dst_pitch, src.ptr, src_pitch, width, rows), twice=False)
        got = got.reshape(rows, dst_pitch)
        assert np.array_equal(got[:, :width], raw[:, :width]), a.dtype
        assert (got[:, width:] == sent).all(), 'written between the rows'


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _refused(ctx, outs, call):
    for o in outs:
        o.fill(SENTINELS[0])
    with pytest.raises(_capi.DswxError) as e:
        call()
    ctx.synchronize()
    assert e.value.code == ERR_ALIGN, e.value
    assert all(o.untouched() for o in outs), 'a refused call wrote its output'


def test_misaligned_pointers_are_refused_and_nothing_is_written(ctx):
    """`blocks` off a 16-byte boundary, and any 16- / 32- / 64-bit plane or index array off its sample alignment:
    DSWX_ERR_ALIGN, the output untouched.  (The same calls at aligned addresses are the tests above.)"""
    h, w, tile = 20, 24, 16
    n = h * w
    with Dev(ctx) as d:
        big = d.span(1 << 16)
        src = d.put(np.zeros(1 << 14, np.uint8))
        idx = d.put(np.zeros(64, np.int32))
        wts = d.put(np.ones(64, np.float64))
        p, o, ix, wp = src.ptr, big.ptr, idx.ptr, wts.ptr
        for off in (1, 2, 4, 8, 15):
            _refused(ctx, [big], lambda: ctx.cog_blocks_device(p, 1, h, w, o + off, (), tile, 2))
            _refused(ctx, [big], lambda: ctx.cog_blocks_device(p, 2, h, w, o + off, (2,), tile, 2))
            _refused(ctx, [big], lambda: ctx.cog_blocks_device(p, 4, h, w, o + off, (), tile, 3))
        _refused(ctx, [big], lambda: ctx.cog_blocks_device(p + 1, 2, h, w, o, (), tile, 2))
        for off in (1, 2, 3):
            _refused(ctx, [big], lambda: ctx.cog_blocks_device(p + off, 4, h, w, o, (), tile, 3))
            for predictor in (1, 2, 3):
                _refused(ctx, [big], lambda: ctx.untile_device(p + off, 4, h, w, tile, tile, predictor, o))
                _refused(ctx, [big], lambda: ctx.untile_device(p, 4, h, w, tile, tile, predictor, o + off))
            _refused(ctx, [big], lambda: ctx.to_byte_device(p + off, np.float32, n, o))
            _refused(ctx, [big], lambda: ctx.gather_2d_device(p + off, 4, h, w, ix, 4, ix, 4, o))
            _refused(ctx, [big], lambda: ctx.gather_2d_device(p, 4, h, w, ix, 4, ix, 4, o + off))
            _refused(ctx, [big], lambda: ctx.gather_2d_device(p, 1, h, w, ix + off, 4, ix, 4, o))
            _refused(ctx, [big], lambda: ctx.gather_2d_device(p, 1, h, w, ix, 4, ix + off, 4, o))
            _refused(ctx, [big], lambda: ctx.rgb_planes_device(p, p, p, None, n, [1.0] * 3, [0.0] * 3, True, o + off))
            _refused(ctx, [big], lambda: ctx.convolve_axis_device(p + off, False, 4, 8, 8, 1, 4, 2, ix, wp, o, False, 4, 1))
            _refused(ctx, [big], lambda: ctx.convolve_axis_device(p, False, 4, 8, 8, 1, 4, 2, ix, wp, o + off, False, 4, 1))
            _refused(ctx, [big], lambda: ctx.convolve_axis_device(p, False, 4, 8, 8, 1, 4, 2, ix + off, wp, o, False, 4, 1))
        for off in (1, 2, 4, 7):
            _refused(ctx, [big], lambda: ctx.convolve_axis_device(p, False, 4, 8, 8, 1, 4, 2, ix, wp + off, o, False, 4, 1))
            _refused(ctx, [big], lambda: ctx.convolve_axis_device(p + off, True, 4, 8, 8, 1, 4, 2, ix, wp, o, False, 4, 1))
            _refused(ctx, [big], lambda: ctx.convolve_axis_device(p, False, 4, 8, 8, 1, 4, 2, ix, wp, o + off, True, 4, 1))
        _refused(ctx, [big], lambda: ctx.untile_device(p + 1, 2, h, w, tile, tile, 2, o))
        _refused(ctx, [big], lambda: ctx.untile_device(p, 2, h, w, tile, tile, 2, o + 1))
        _refused(ctx, [big], lambda: ctx.to_byte_device(p + 1, np.uint16, n, o))
        _refused(ctx, [big], lambda: ctx.to_byte_device(p + 1, np.int16, n, o))
        _refused(ctx, [big], lambda: ctx.gather_2d_device(p + 1, 2, h, w, ix, 4, ix, 4, o))
        _refused(ctx, [big], lambda: ctx.gather_2d_device(p, 2, h, w, ix, 4, ix, 4, o + 1))
        for j in range(4):                       # red, green, blue, DIAG
            ptrs = [p + (1 if c == j else 0) for c in range(4)]
            _refused(ctx, [big], lambda: ctx.rgb_planes_device(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, [1.0] * 3, [0.0] * 3, True, o))


# ---- on a caller's stream -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def env(ctx):
    e = S.Env(ctx)
    yield e
    S.torch.cuda.synchronize()
    ctx.synchronize()


STREAM_ENTRIES = ('cog_blocks', 'untile', 'convolve_axis', 'rgb_planes', 'to_byte', 'gather_2d', 'copy_2d')


@pytest.mark.parametrize('entry', STREAM_ENTRIES)
def test_on_a_held_stream(ctx, env, entry):
    """One case per entry on a caller's stream that is held (tests/test_gpu_streams.py's protocol): the call returns while
    the hold is pending, the output keeps its sentinel until the hold ends, and is then bit for bit the reference's."""
    e = env
    h, w = 61, 83
    n = h * w
    if entry == 'cog_blocks':
        a = R.f32_plane('edges', _rng(21), (h, w))
        want = co.blocks(a, 16, 3)
        d_in, out = S._dev(a), S._pinned(ctx, want.size + 64)
        launch = lambda st: ctx.cog_blocks_device(d_in.data_ptr(), 4, h, w, out.ctypes.data, (), 16, 3, stream=st)      # noqa: E731
        check = lambda: (np.array_equal(out[:want.size], want), (out[want.size:] == S.SENT).all())                     # noqa: E731
    elif entry == 'untile':
        vals = R.int_rows('carry', _rng(22), 6, 1031, np.uint16)
        d_in, out = S._dev(R.differenced(vals)), S._pinned(ctx, vals.nbytes + 64)
        launch = lambda st: ctx.untile_device(d_in.data_ptr(), 2, 6, 1031, 1031, 3, 2, out.ctypes.data, stream=st)     # noqa: E731
        check = lambda: (out[:vals.nbytes].tobytes() == vals.tobytes(), (out[vals.nbytes:] == S.SENT).all())           # noqa: E731
    elif entry == 'convolve_axis':              # float32 -> float32: an instantiation the pipeline does not use
        a = R.f32_plane('tiny', _rng(23), (h, w))
        first, wt = geotiff.convolve_weights(w, 21)
        want = co.convolve_axis(a.astype(np.float64), first, wt).astype(np.float32)
        d_in, d_f, d_w = S._dev(a), S._dev(first.astype(np.int32)), S._dev(np.ascontiguousarray(wt.T))
        out = S._pinned(ctx, want.nbytes + 64)
        launch = lambda st: ctx.convolve_axis_device(d_in.data_ptr(), False, h, w, w, 1, 21, wt.shape[1], d_f.data_ptr(),   # noqa: E731
                                                     d_w.data_ptr(), out.ctypes.data, False, 21, 1, stream=st)
        check = lambda: (same_floats(out[:want.nbytes].view(np.float32).reshape(want.shape), want),                    # noqa: E731
                         (out[want.nbytes:] == S.SENT).all())
    elif entry == 'rgb_planes':
        bands, diag, scales, offsets = R.rgb_case(1, 2)
        d_b, d_d = [S._dev(b) for b in bands], S._dev(diag)
        want = np.stack([R.rgb_statement(bands[c], scales[c], offsets[c], True, diag) for c in range(3)]).view(np.uint32)
        out = S._pinned(ctx, want.nbytes + 64)
        launch = lambda st: ctx.rgb_planes_device(d_b[0].data_ptr(), d_b[1].data_ptr(), d_b[2].data_ptr(), d_d.data_ptr(), 65536,  # noqa: E731
                                                  scales, offsets, True, out.ctypes.data, stream=st)
        check = lambda: (np.array_equal(out[:want.nbytes].view(np.uint32).reshape(3, -1), want),                       # noqa: E731
                         (out[want.nbytes:] == S.SENT).all())
    elif entry == 'to_byte':
        a = R.byte_edges()
        want = co.gdal_byte_vec(a)
        d_in, out = S._dev(a), S._pinned(ctx, a.size + 64)
        launch = lambda st: ctx.to_byte_device(d_in.data_ptr(), np.float32, a.size, out.ctypes.data, stream=st)        # noqa: E731
        check = lambda: (np.array_equal(out[:a.size], want), (out[a.size:] == S.SENT).all())                           # noqa: E731
    elif entry == 'gather_2d':
        a = R.f32_plane('bits', _rng(24), (h, w)).view(np.uint32)
        rows, cols = np.int32([0, h - 1, h - 1, 0, 5]), np.int32([w - 1, 0, 0, w - 1] * 70)
        want = a[rows][:, cols]
        d_in, d_r, d_c = S._dev(a), S._dev(rows), S._dev(cols)
        out = S._pinned(ctx, want.nbytes + 64)
        launch = lambda st: ctx.gather_2d_device(d_in.data_ptr(), 4, h, w, d_r.data_ptr(), rows.size, d_c.data_ptr(), cols.size,  # noqa: E731
                                                 out.ctypes.data, stream=st)
        check = lambda: (out[:want.nbytes].tobytes() == want.tobytes(), (out[want.nbytes:] == S.SENT).all())           # noqa: E731
    else:
        a = R.f32_plane('bits', _rng(25), (h, w)).view(np.uint8).reshape(h, -1)
        width, dst_pitch = a.shape[1] - 3, a.shape[1] + 5
        d_in, out = S._dev(a), S._pinned(ctx, h * dst_pitch)
        launch = lambda st: ctx.copy_2d_device(out.ctypes.data, dst_pitch, d_in.data_ptr(), a.shape[1], width, h, stream=st)   # noqa: E731
        check = lambda: (np.array_equal(out.reshape(h, dst_pitch)[:, :width], a[:, :width]),                           # noqa: E731
                         (out.reshape(h, dst_pitch)[:, width:] == S.SENT).all())

    def checked():
        assert all(check()), entry
    S.held_call(e, launch, [out], checked)
