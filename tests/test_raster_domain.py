"""The sample domains of oracle/raster_inputs.py on the CPU, before any GPU time is spent on them: (1) the domains are
not vacuous -- each reaches, by the reference statements alone, the condition it is named for; (2) the two CPU
restatements of every raster-format step (proteus_amd/geotiff.py + dswx_hls._gdal_byte, whole arrays; oracle/cog_oracle.py,
element by element) agree on them, bits equal wherever the value is not NaN and NaN at the same positions; (3) the RGB
statement with explicit float32 scalars is the reference's expression under the installed numpy; (4) the vectorised
references tests/test_gpu_raster_domain.py uses for speed are pinned against their element-wise forms.

One thing the float32 domains CANNOT reach, and why: a CUBICSPLINE level value that is finite in the float64 accumulator
and overflows at the float32 store.  Every weight of the cubic B-spline is >= 0 and the sum is normalised, so an output is
a convex combination of float32 inputs: |out| <= max |in| <= FLT_MAX up to a relative 1e-14 of float64 rounding, while the
float32 store only overflows from FLT_MAX * (1 + 2^-25).  test_huge_stays_finite_and_the_store_overflows_from_float64
asserts exactly that for `huge`, and reaches the overflowing store where it can be reached: dswx_convolve_axis_device
with a float64 source (raster_inputs.f64_lines('beyond_f32'))."""
import numpy as np
import pytest

from oracle import cog_oracle as co, raster_inputs as R
from proteus_amd import dswx_hls as D, geotiff

FACTORS = geotiff.COG_OVERVIEW_FACTORS


def same_floats(got, want):
    """NaN at the same positions, every other value equal by bits (the sign of zero included)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(np.ascontiguousarray(got).view(u)[~gn], np.ascontiguousarray(want).view(u)[~wn]))


def host_pyramid(a, factors=FACTORS):
    """write_geotiff's cascade of geotiff.overview_cubicspline."""
    shape = a.shape
    out, prev = [a], 1
    with np.errstate(over='ignore', invalid='ignore'):
        for f in factors:
            if f <= 1 or shape == (1, 1):
                continue
            lv = geotiff.overview_cubicspline(out[-1], f // prev) if prev > 1 and f % prev == 0 else geotiff.overview_cubicspline(a, f)
            if lv.shape != tuple(-(-n // f) for n in shape):
                lv = geotiff.overview_cubicspline(a, f)
            out.append(lv)
            prev = f
    return out


def _plane(name, domain, variant, shape, salt=0):
    return R.f32_plane(domain, np.random.default_rng([len(name), shape[0], shape[1], variant, salt]), shape, variant)


# ---- (1) the domains are not vacuous ------------------------------------------------------------------------------------
def test_bits_and_edges_hold_what_they_are_named_for():
    b = _plane('bits', 'bits', 0, (300, 257)).view(np.uint32).ravel()
    exp, man = (b >> 23) & 0xff, b & 0x7fffff
    nan = (exp == 255) & (man != 0)
    assert 0.5 / 256 < nan.mean() < 2.0 / 256
    assert ((b[nan] >> 31) == 1).any() and ((b[nan] >> 31) == 0).any()
    assert (nan & ((man >> 22) == 0)).any(), 'no signalling NaN'
    assert len(set(man[nan].tolist())) > 50, 'NaN payloads not arbitrary'
    assert ((exp == 0) & (man != 0)).any() and (b == 0).any() and (b == 0x80000000).any()
    assert (b == 0x7f800000).any() and (b == 0xff800000).any()
    e = _plane('edges', 'edges', 0, (37, 53)).view(np.uint32)
    assert set(e.ravel().tolist()) == set(R.EDGE_BITS)
    assert np.float32(np.nan).view(np.uint32) == R.QUIET_NAN_BITS


def test_huge_stays_finite_and_the_store_overflows_from_float64():
    a = _plane('huge', 'huge', 0, (129, 260))
    assert np.isfinite(a).all() and np.abs(a).min() >= np.float32(9.9e37) and (a > 0).any() and (a < 0).any()
    assert (np.abs(a) == np.float32(R.FLT_MAX)).any()
    lv = host_pyramid(a)[1]
    # a convex combination of float32 values (module docstring): no level value can leave the float32 range
    assert np.isfinite(lv).all() and np.abs(lv.astype(np.float64)).max() <= R.FLT_MAX
    assert (np.abs(lv) > np.float32(1e37)).any()
    # the overflowing store itself: a float64 source
    lines = R.f64_lines('beyond_f32', np.random.default_rng(3), (9, 64))
    first, w = geotiff.convolve_weights(64, 16)
    acc = co.convolve_axis(lines, first, w)
    assert np.isfinite(acc).all()
    with np.errstate(over='ignore'):
        stored = acc.astype(np.float32)
    assert np.isposinf(stored).any() and np.isneginf(stored).any() and np.isfinite(stored).any()


def test_tiny_produces_float32_denormal_outputs():
    a = _plane('tiny', 'tiny', 0, (129, 260))
    den_in = (a != 0) & (np.abs(a) < np.finfo(np.float32).tiny)
    assert den_in.any() and (np.abs(a) >= np.finfo(np.float32).tiny).any()
    for lv in host_pyramid(a)[1:3]:
        assert ((lv != 0) & (np.abs(lv) < np.finfo(np.float32).tiny)).any()
    acc = co.convolve_axis(R.f64_lines('below_f32', np.random.default_rng(4), (9, 64)), *geotiff.convolve_weights(64, 16))
    stored = acc.astype(np.float32)
    assert ((stored != 0) & (np.abs(stored) < np.finfo(np.float32).tiny)).any()


def test_inf_signs_produces_nan_where_the_normalising_sum_is_positive():
    a = _plane('inf_signs', 'inf_signs', 0, (300, 257))
    assert not np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
    lv = host_pyramid(a)[1]
    # no input is NaN, so every normalising sum is positive: a NaN output is +inf and -inf inside one support
    assert np.isnan(lv).any() and np.isposinf(lv).any() and np.isneginf(lv).any() and np.isfinite(lv).any()
    ys, xs = np.nonzero(np.isinf(a))
    d = [max(abs(int(ys[i]) - int(ys[j])), abs(int(xs[i]) - int(xs[j]))) for i in range(len(ys)) for j in range(i)
         if a[ys[i], xs[i]] != a[ys[j], xs[j]]]
    assert min(d) < R.LEVEL1_SUPPORT // 2 and any(v > 2 * R.LEVEL1_SUPPORT for v in d)


def test_nan_structures_produce_nan_and_non_nan_outputs():
    seen_nan = seen_val = 0
    for k, s in enumerate(R.NAN_STRUCTURES):
        a = _plane(f'nan_{s}', 'nan_structures', k, (129, 260))
        assert np.isnan(a).any() and not np.isnan(a).all()
        lv = host_pyramid(a)[1]
        seen_nan += int(np.isnan(lv).any())
        seen_val += int((~np.isnan(lv)).any())
        if s in ('rows', 'columns', 'survivor'):
            assert np.isnan(lv).any() and (~np.isnan(lv)).any(), s
        if s == 'survivor':
            assert np.isnan(a).sum() == a.size - 1 and 0 < (~np.isnan(lv)).sum() < lv.size / 2
        if s in ('frame', 'checkerboard'):
            assert not np.isnan(lv).any(), s            # renormalised around the missing taps
    assert seen_nan >= 3 and seen_val == len(R.NAN_STRUCTURES)


@pytest.mark.parametrize('dtype', R.INT_DTYPES)
@pytest.mark.parametrize('n', [1031, 3660, 513])
def test_wrap_and_carry_meet_their_definitions(dtype, n):
    bits = 8 * np.dtype(dtype).itemsize
    m = 1 << bits
    rng = np.random.default_rng(n + bits)
    d = R.wrap_differences(rng, 9, n, dtype)
    wide = np.cumsum(d.astype(np.uint64), axis=1, dtype=np.uint64)              # the running sum without a modulus
    passes = np.zeros(d.shape, bool)
    passes[:, 1:] = (wide[:, 1:] // m) > (wide[:, :-1] // m)
    for c0 in range(0, n, R.CHUNK):
        seg = passes[:, c0: c0 + R.CHUNK]
        if seg.shape[1] >= 16:
            assert seg.any(axis=1).all(), (dtype, n, c0)
        every = seg[0::3, (1 if c0 == 0 else 0):]            # rows 0, 3, ...: every step but one in 2^bits
        assert ((~every).sum(axis=1) <= every.shape[1] // m + 1).all(), (dtype, n, c0)
    v = R.int_rows('wrap', np.random.default_rng(n + bits), 9, n, dtype)
    assert v.dtype == np.dtype(dtype) and np.array_equal(R.differenced(v), d)
    assert np.array_equal(v.view(d.dtype), (wide % m).astype(d.dtype))
    c = R.int_rows('carry', rng, 9, n, dtype)
    ends = c.view(d.dtype)[:, R.CHUNK - 1::R.CHUNK].astype(np.int64)
    assert ends.size == 9 * (n // R.CHUNK)
    dist = np.minimum(ends, m - ends)
    assert (dist <= 2).all() and len(set(((ends + 2) % m).ravel().tolist())) == 5, 'all of -2 .. 2 at the chunk ends'
    for dom in ('full', 'runs'):
        r = R.int_rows(dom, rng, 9, n, dtype)
        assert r.dtype == np.dtype(dtype) and r.shape == (9, n)
    full = R.int_rows('full', rng, 64, 4096, dtype).view(d.dtype)
    assert full.min() < m // 64 and full.max() >= m - m // 64


def test_byte_sets_hold_both_sides_of_every_rounding_edge():
    e = R.byte_edges()
    assert e.dtype == np.float32 and e.size == 258 * 2 * 129
    for k in range(-1, 257):
        for c in (k, k + 0.5):
            near = e[np.abs(e.astype(np.float64) - c) < 5e-3]
            assert (near < c).sum() >= 64 and (near > c).sum() >= 64 and (near == c).any(), (k, c)
    want = co.gdal_byte(e)
    assert set(want.tolist()) == set(range(256))
    for k in range(0, 255):                        # the value just under k + 0.5 rounds down, k + 0.5 itself up
        edge = np.float32(k + 0.5)
        below = np.nextafter(edge, np.float32(-np.inf))
        assert co.gdal_byte(np.array([below, edge]))[0] == k and co.gdal_byte(np.array([below, edge]))[1] == k + 1
    s = R.byte_exponent_sweep().view(np.uint32)
    assert s.size == 1 << 20 and len(set(((s >> 23) & 0x1ff).tolist())) == 512 and not (s & 0xfff).any()
    r = R.byte_random(n=1 << 12)
    assert r.dtype == np.float32 and np.isnan(r).any() is not None


def test_rgb_cases_cover_what_they_are_named_for():
    for band in range(3):
        bands, diag, scales, offsets = R.rgb_case(band, 0)
        assert np.array_equal(np.sort(bands[band]), np.arange(-32768, 32768))
        for c in range(3):
            if c != band:
                assert set(bands[c].tolist()) == set(R.RGB_BAND_EDGES)
        assert set(diag.tolist()) == set(R.RGB_DIAG_CYCLE)
        assert ((diag[:-1] == 65534) & (diag[1:] == 65535)).any() or ((diag[:-1] == 65535) & (diag[1:] == 65534)).any()
    pairs = set()
    for k in range(len(R.RGB_SCALE_OFFSET)):
        _, _, scales, offsets = R.rgb_case(1, k)
        pairs.add((scales[1], offsets[1]))
        assert all(abs(v) <= R.FLT_MAX for v in scales + offsets)
    assert pairs == set(R.RGB_SCALE_OFFSET)


# ---- (2) the two CPU restatements agree ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name,domain,variant', R.f32_planes(), ids=[p[0] for p in R.f32_planes()])
def test_predictor_3_restatements_move_bits(name, domain, variant):
    """geotiff.blocked_level (and its inverse) against cog_oracle.blocks / unblocks: by bytes, NaN payloads included."""
    for shape, tile in (((37, 53), 16), ((21, 50), 64), ((5, 51), 16)):
        a = _plane(name, domain, variant, shape)
        lv = geotiff.blocked_level(a[None], tile, 3)
        data = co.blocks(a, tile, 3)
        assert np.array_equal(np.asarray(lv.data).reshape(-1).view(np.uint8), data), (shape, tile)
        assert co.unblocks(data, np.float32, shape[0], shape[1], tile, tile, 3).tobytes() == a.tobytes()
        rows = -(-shape[0] // tile) * -(-shape[1] // tile) * tile
        back = geotiff._fp_predictor_decode(np.asarray(lv.data).reshape(-1).view(np.uint8), rows, tile, 1, np.float32)
        # the host reader's inverse gives the padded block rows back, bit for bit: encoding them again gives the same bytes
        assert back.dtype == np.float32 and geotiff._fp_predictor_encode(back) == data.tobytes()


@pytest.mark.parametrize('dtype', R.INT_DTYPES)
@pytest.mark.parametrize('domain', R.INT_DOMAINS)
def test_predictor_2_restatements_agree(domain, dtype):
    rng = np.random.default_rng([R.INT_DOMAINS.index(domain), np.dtype(dtype).itemsize])
    a = R.int_rows(domain, rng, 19, 1100, dtype)
    for tile in (16, 512):
        lv = geotiff.blocked_level(a[None], tile, 2)
        data = co.blocks(a, tile, 2)
        assert np.array_equal(np.asarray(lv.data).reshape(-1).view(np.uint8), data), tile
        assert np.array_equal(co.unblocks(data, dtype, 19, 1100, tile, tile, 2), a)


@pytest.mark.parametrize('name,domain,variant', R.f32_planes(), ids=[p[0] for p in R.f32_planes()])
def test_cubicspline_restatements_agree(name, domain, variant):
    for shape in ((37, 53), (5, 3), (66, 21)):
        a = _plane(name, domain, variant, shape)
        got, want = host_pyramid(a), co.cubicspline_pyramid(a, FACTORS)
        assert len(got) == len(want) == 5
        for k, (g, w) in enumerate(zip(got, want)):
            assert same_floats(g, w), (shape, k)


def test_byte_restatements_agree():
    for a in (R.byte_edges(), R.byte_exponent_sweep(), R.f32_plane('edges', np.random.default_rng(1), (40, 50)),
              R.f32_plane('bits', np.random.default_rng(2), (300, 257))):
        want = co.gdal_byte(a)
        assert np.array_equal(D._gdal_byte(a), want)
        assert np.array_equal(co.gdal_byte_vec(a), want)
    r = R.byte_random()
    assert np.array_equal(D._gdal_byte(r), co.gdal_byte_vec(r))
    for dt in (np.uint16, np.int16):
        a = np.arange(65536, dtype=np.uint16).view(dt)
        assert np.array_equal(D._gdal_byte(a), co.gdal_byte(a)) and np.array_equal(co.gdal_byte_vec(a), co.gdal_byte(a))


def test_nearest_restatements_agree_on_every_size_to_300():
    for n in range(1, 301):
        row = np.arange(n, dtype=np.uint16)
        for a in (np.stack([row, 65535 - row]), np.stack([row, 65535 - row]).T.copy()):
            for f in (2, 3, 4, 5, 7, 16, 64, 128):
                assert np.array_equal(geotiff.overview_nearest(a, f), co.nearest_overview(a, f)), (n, f)


# ---- (3) the RGB statement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [True, False])
def test_rgb_float32_statement_is_the_references_expression(clip):
    for band in range(3):
        for k in range(len(R.RGB_SCALE_OFFSET)):
            bands, diag, scales, offsets = R.rgb_case(band, k)
            want = co.rgb_planes(bands, diag, scales, offsets, clip=clip)
            plain = co.rgb_planes(bands, None, scales, offsets, clip=clip)
            for c in range(3):
                b = np.clip(bands[c], 1, None) if clip else bands[c]
                with np.errstate(over='ignore', invalid='ignore'):
                    ref = scales[c] * (np.asarray(b, dtype=np.float32) - offsets[c])        # the reference's expression
                assert ref.dtype == np.float32
                mine = R.rgb_statement(bands[c], scales[c], offsets[c], clip)
                assert not np.isnan(ref).any()
                assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), (band, k, c)
                assert np.array_equal(plain[c].view(np.uint32), ref.view(np.uint32))
                masked = R.rgb_statement(bands[c], scales[c], offsets[c], clip, diag)
                assert np.array_equal(masked.view(np.uint32), want[c].view(np.uint32))
                assert (masked.view(np.uint32)[diag == 65535] == R.QUIET_NAN_BITS).all()
                assert not np.isnan(masked[diag != 65535]).any()
    # the cases reach the clip boundary, overflow, denormal products and both signs of zero
    bands, diag, scales, offsets = R.rgb_case(0, 5)
    assert np.isinf(R.rgb_statement(bands[0], 3e38, 0.0, False)).any()
    v = R.rgb_statement(bands[0], 1e-42, 0.0, False)
    assert ((v != 0) & (np.abs(v) < np.finfo(np.float32).tiny)).any()
    z = R.rgb_statement(bands[0], 0.0, 7.0, False).view(np.uint32)
    assert (z == 0).any() and (z == 0x80000000).any()
    on, off = R.rgb_statement(bands[0], 1e-4, 0.0, True), R.rgb_statement(bands[0], 1e-4, 0.0, False)
    i = {int(v): j for j, v in enumerate(bands[0])}
    assert on[i[0]] == on[i[1]] == on[i[-1]] == on[i[-32768]] != on[i[2]] and off[i[0]] == 0 and off[i[-1]] < 0


# ---- (4) the vectorised references --------------------------------------------------------------------------------------
def test_generic_convolution_reference_against_its_element_wise_form():
    rng = np.random.default_rng(11)
    for name, domain, variant in R.f32_planes():
        with np.errstate(invalid='ignore'):             # (a signalling NaN raises the flag when it is widened)
            lines = _plane(name, domain, variant, (6, 70)).astype(np.float64)
        for first, w in (geotiff.convolve_weights(70, 18), geotiff.convolve_weights(70, 70), _odd_taps(rng, 70, 23, 9)):
            got = co.convolve_axis(lines, first, w)
            want = np.array([co.convolve_line_generic([float(v) for v in ln], first, w) for ln in lines])
            assert same_floats(got, want), name
    for domain in R.F64_DOMAINS:
        lines = R.f64_lines(domain, rng, (5, 40))
        first, w = geotiff.convolve_weights(40, 10)
        want = np.array([co.convolve_line_generic([float(v) for v in ln], first, w) for ln in lines])
        assert same_floats(co.convolve_axis(lines, first, w), want)
    # with the B-spline taps it is the oracle's own pass
    a = _plane('dem', 'dem', 0, (4, 61)).astype(np.float64)
    first, w = geotiff.convolve_weights(61, 16)
    assert same_floats(co.convolve_axis(a, first, w), np.array([co._convolve_line([float(v) for v in ln], 16) for ln in a]))


def _odd_taps(rng, n_in, n_out, taps):
    """Taps that are not a B-spline: windows that start before the line and end after it (clamped reads), zero weights."""
    first = rng.integers(-taps, n_in, size=n_out)
    w = rng.random((n_out, taps))
    w[rng.random((n_out, taps)) < 0.3] = 0.0
    w[0] = 0.0                                   # no weight left: NaN
    return first, w
