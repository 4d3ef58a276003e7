"""TEST INFRASTRUCTURE -- seeded, named sample domains for the raster-format entries (dswx_cog_blocks_device,
dswx_untile_device, dswx_convolve_axis_device, dswx_rgb_planes_device, dswx_to_byte_device, dswx_gather_2d_device,
dswx_copy_2d_device), shared by tests/test_raster_domain.py (CPU) and tests/test_gpu_raster_domain.py.  Only tests/ may
import it.

Float32 planes (f32_plane):
  bits            uniform random 32-bit patterns: about 1 in 256 a NaN of arbitrary payload and sign; denormals, +-0 and
                  +-inf are put in by construction
  edges           per pixel a pick from EDGE_BITS
  tiny            magnitudes 1e-45 ... 1e-37, mixed signs (float32 denormals and the smallest normals)
  huge            magnitudes 1e38 ... FLT_MAX, mixed signs
  inf_signs       a finite field with isolated +inf / -inf pairs, alternately closer together than the support of a
                  level-1 (factor 4) CUBICSPLINE pixel and farther apart
  nan_structures  NAN_STRUCTURES[variant]: whole rows, whole columns, a frame, a checkerboard, one survivor in an all-NaN
                  raster
  dem             the recipe of tests/test_gpu_writer.py
Float64 lines for dswx_convolve_axis_device with a float64 source (f64_lines): beyond_f32 (finite in float64, outside the
float32 range: the (float) store overflows) and below_f32 (inside and under the float32 denormal range).

Byte conversion (dswx_to_byte_device, float32): byte_edges, byte_exponent_sweep, byte_random.

Integer rows (int_rows; uint8, uint16, int16, uint32) as the VALUES a PREDICTOR=2 running sum must give back;
differenced() makes the rows that go into the blocks:
  full   uniform over the whole range
  runs   class-map-like: few values in runs
  wrap   the running sum of the differences, taken without a modulus, passes a multiple of 2^bits in every chunk of 512
         elements: at every step (but one in 2^bits) in rows 0, 3, 6, ..., at least every second step in rows 1, 4, ..., once per 8 elements
         (one lane of the device's wave scan) in rows 2, 5, ...
  carry  the value at the end of every chunk of 512 elements -- the carry into the next chunk -- is within +-2 of the
         wrap point (2^bits - 2 ... 2^bits + 2, i.e. -2 ... 2 in the sample's width)

RGB composites (rgb_case): all 65,536 int16 values in the band under test.
"""
import numpy as np

F32_DOMAINS = ('bits', 'edges', 'tiny', 'huge', 'inf_signs', 'nan_structures', 'dem')
NAN_STRUCTURES = ('rows', 'columns', 'frame', 'checkerboard', 'survivor')
FLT_MAX = float(np.finfo(np.float32).max)
QUIET_NAN_BITS = 0x7fc00000                      # what np.float32(np.nan) stores
# +-0, +-smallest denormal, +-largest denormal, +-FLT_MIN, +-FLT_MAX, +-inf, quiet / signalling / negative NaN, NaN payload 1
EDGE_BITS = (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
             0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, QUIET_NAN_BITS, 0x7fa00000, 0xffc00000, 0x7f800001)
LEVEL1_SUPPORT = 17                              # taps of one pass at factor 4: ceil(2 * 2 * 4) + 1


def f32_planes():
    """(name, domain, variant) of every float32 plane the tests run: each domain once, nan_structures once per structure."""
    out = []
    for d in F32_DOMAINS:
        if d == 'nan_structures':
            out += [(f'nan_{s}', d, k) for k, s in enumerate(NAN_STRUCTURES)]
        else:
            out.append((d, d, 0))
    return out


def _finite_field(rng, shape):
    return (rng.normal(size=shape) * 1000).astype(np.float32)


def f32_plane(domain, rng, shape, variant=0):
    """One float32 plane [H, W] of `domain`."""
    h, w = shape
    n = h * w
    if domain == 'bits':
        bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        seed = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x7f800001, 0xffffffff],
                        np.uint32)
        at = rng.permutation(n)[:min(n, seed.size)]
        bits[at] = seed[:at.size]
        return bits.view(np.float32).reshape(shape)
    if domain == 'edges':
        return rng.choice(np.array(EDGE_BITS, np.uint32), size=shape).view(np.float32)
    if domain == 'tiny':
        mag = 10.0 ** rng.uniform(-45.0, -37.0, size=shape)
        return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    if domain == 'huge':
        mag = np.minimum(10.0 ** rng.uniform(38.0, np.log10(FLT_MAX), size=shape), FLT_MAX)
        a = (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
        a.reshape(-1)[:2] = [FLT_MAX, -FLT_MAX][:min(n, 2)]
        return a
    if domain == 'inf_signs':
        a = _finite_field(rng, shape)
        for k in range(max(2, n // 1500)):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            gap = int(rng.integers(1, 7)) if k % 2 == 0 else int(rng.integers(3 * LEVEL1_SUPPORT, 6 * LEVEL1_SUPPORT))
            y2, x2 = (y, min(x + gap, w - 1)) if k % 4 < 2 else (min(y + gap, h - 1), x)
            a[y, x] = np.inf
            if (y2, x2) != (y, x):
                a[y2, x2] = -np.inf
        return a
    if domain == 'nan_structures':
        a = _finite_field(rng, shape)
        s = NAN_STRUCTURES[variant]
        if s == 'rows':
            a[::7] = np.nan
            a[h // 4: h // 4 + LEVEL1_SUPPORT + 8] = np.nan     # a band taller than a level-1 support
        elif s == 'columns':
            a[:, ::7] = np.nan
            a[:, w // 4: w // 4 + LEVEL1_SUPPORT + 8] = np.nan
        elif s == 'frame':
            a[:2], a[-2:], a[:, :2], a[:, -2:] = np.nan, np.nan, np.nan, np.nan
        elif s == 'checkerboard':
            a[(np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 0] = np.nan
        else:
            keep = a[h // 2, w // 2]
            a[:] = np.nan
            a[h // 2, w // 2] = keep
        return a
    if domain == 'dem':
        a = (rng.normal(size=shape) * 300 + 500).astype(np.float32)
        a[rng.random(shape) < 0.02] = np.nan
        a.reshape(-1)[:3] = np.float32([np.inf, -0.0, 1e-40])[:min(n, 3)]
        return a
    raise ValueError(domain)


F64_DOMAINS = ('beyond_f32', 'below_f32')


def f64_lines(domain, rng, shape):
    """float64 [n_lines, n_in] for a float64 source: values no float32 plane can hold."""
    if domain == 'beyond_f32':                   # finite in float64; most weighted means overflow the float32 store
        # lines 0, 3, ...: far outside; lines 1, 4, ...: one sign, just past the boundary at which the float32 store rounds to
        # infinity (FLT_MAX * (1 + 2^-25)); lines 2, 5, ...: either side of that boundary, so that some means stay finite
        mag = 10.0 ** rng.uniform(38.6, 300.0, size=shape)
        sign = rng.choice([-1.0, 1.0], size=shape)
        mag[1::3] = FLT_MAX * (1.0 + 2.0 ** -25 * rng.uniform(1.0, 32.0, size=mag[1::3].shape))
        mag[2::3] = FLT_MAX * (1.0 + 2.0 ** -25 * rng.uniform(-4.0, 4.0, size=mag[2::3].shape))
        sign[1::3] = rng.choice([-1.0, 1.0], size=(sign[1::3].shape[0], 1))
        sign[2::3] = rng.choice([-1.0, 1.0], size=(sign[2::3].shape[0], 1))
        return mag * sign
    if domain == 'below_f32':                    # the float32 denormal range and under it
        return 10.0 ** rng.uniform(-60.0, -37.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
    raise ValueError(domain)


# ---- the Byte conversion ------------------------------------------------------------------------------------------------
def byte_edges(steps=64):
    """For every k in -1 .. 256: k and k + 0.5 and the `steps` float32 values either side of each (nextafter)."""
    out = []
    for k in range(-1, 257):
        for c in (np.float32(k), np.float32(k + 0.5)):
            up, down = [c], []
            for _ in range(steps):
                up.append(np.nextafter(up[-1], np.float32(np.inf)))
            lo = c
            for _ in range(steps):
                lo = np.nextafter(lo, np.float32(-np.inf))
                down.append(lo)
            out += down[::-1] + up
    return np.array(out, np.float32)


def byte_exponent_sweep():
    """Every float32 pattern whose low 12 mantissa bits are zero: 2^20 patterns, every sign and exponent."""
    return (np.arange(1 << 20, dtype=np.uint32) << np.uint32(12)).view(np.float32)


def byte_random(seed=20261016, n=1 << 24):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


# ---- integer rows -------------------------------------------------------------------------------------------------------
INT_DTYPES = (np.uint8, np.uint16, np.int16, np.uint32)
INT_DOMAINS = ('full', 'runs', 'wrap', 'carry')
CHUNK = 512                                      # elements one pass of the device's wave scan covers


def _unsigned(dtype):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32}[np.dtype(dtype).itemsize]


def differenced(rows):
    """Rows of values -> the rows PREDICTOR=2 stores (libtiff horDiff: wrap-around in the sample's width, the first sample
    as it is), in the unsigned type of that width."""
    u = np.ascontiguousarray(rows).view(_unsigned(rows.dtype))
    d = u.copy()
    d[..., 1:] = u[..., 1:] - u[..., :-1]
    return d


def wrap_differences(rng, n_rows, n, dtype):
    """The differences of the 'wrap' domain (unsigned, [n_rows, n]); row r is of kind r % 3."""
    u = _unsigned(dtype)
    m = 1 << (8 * np.dtype(u).itemsize)
    d = np.empty((n_rows, n), np.uint64)
    for r in range(n_rows):
        if r % 3 == 0:
            d[r] = m - 1                                                 # every step but one in 2^bits passes a multiple of 2^bits
        elif r % 3 == 1:
            d[r] = rng.integers(m // 2, m, size=n, dtype=np.uint64)      # at least every second step
        else:
            d[r] = m // 8 + rng.integers(0, max(m // 64, 2), size=n, dtype=np.uint64)    # once per lane of 8
    return d.astype(u)


def int_rows(domain, rng, n_rows, n, dtype):
    """[n_rows, n] values of `dtype` in `domain`."""
    dtype = np.dtype(dtype)
    u = _unsigned(dtype)
    m = 1 << (8 * dtype.itemsize)
    if domain == 'full':
        v = rng.integers(0, m, size=(n_rows, n), dtype=np.uint64).astype(u)
    elif domain == 'runs':
        base = rng.integers(0, 5, size=(n_rows, -(-n // 16)), dtype=np.uint64)
        v = (np.repeat(base, 16, axis=1)[:, :n] * (1 if dtype.itemsize == 1 else 1111)).astype(u)
        v[::5] = 3
    elif domain == 'wrap':
        v = np.cumsum(wrap_differences(rng, n_rows, n, dtype).astype(np.uint64), axis=1, dtype=np.uint64).astype(u)
    elif domain == 'carry':
        v = rng.integers(0, m, size=(n_rows, n), dtype=np.uint64)
        ends = np.arange(CHUNK - 1, n, CHUNK)
        v[:, ends] = (m + (np.arange(n_rows * ends.size).reshape(n_rows, ends.size) + int(rng.integers(0, 5))) % 5 - 2) % m
        v = v.astype(u)
    else:
        raise ValueError(domain)
    return v.view(dtype)


# ---- RGB composites -----------------------------------------------------------------------------------------------------
RGB_SCALE_OFFSET = ((1e-4, 0.0), (2.75e-5, -0.2), (-1e-4, 16384.0), (0.0, 7.0), (1e-42, 0.0), (3e38, 0.0), (1.0, 32767.5),
                    (1.0 / 3.0, 1e9))
RGB_DIAG_CYCLE = (0, 11111, 65534, 65535)
RGB_BAND_EDGES = (-32768, -1, 0, 1, 2, 32767)


def rgb_case(band, k):
    """Case (band under test, index k into RGB_SCALE_OFFSET) -> (three int16 bands [65536], DIAG uint16 [65536], scales,
    offsets): the band under test runs over every int16 value with the pair k, the other two are held at edge values (a
    different one per stretch of 6 / 7 pixels) with the next pairs of the list; DIAG cycles through RGB_DIAG_CYCLE."""
    n = 65536
    i = np.arange(n)
    edges = np.array(RGB_BAND_EDGES, np.int16)
    bands, scales, offsets = [], [], []
    for c in range(3):
        if c == band:
            bands.append(np.arange(-32768, 32768, dtype=np.int32).astype(np.int16))
        else:
            bands.append(edges[(i // (6 + c)) % edges.size])
        sc, of = RGB_SCALE_OFFSET[(k + (c - band) % 3) % len(RGB_SCALE_OFFSET)]
        scales.append(sc)
        offsets.append(of)
    # the cycle shifted by one every 4 pixels: 65534 and 65535 lie side by side, and no code keeps to one residue of the value
    diag = np.array(RGB_DIAG_CYCLE, np.uint16)[(i + i // 4) % 4]
    return bands, diag, scales, offsets


def rgb_statement(band, scale, offset, clip, diag=None):
    """_save_output_rgb_file's arithmetic on one band with explicit float32 scalars: float32 [n]; invalid pixels carry the
    quiet NaN np.nan stores."""
    b = np.clip(band, 1, None) if clip else band
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.float32(scale) * (b.astype(np.float32) - np.float32(offset))
    assert v.dtype == np.float32
    if diag is not None:
        v = v.copy()
        v[diag == 65535] = np.float32(np.nan)
    return v
