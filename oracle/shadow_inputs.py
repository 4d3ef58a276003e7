"""TEST INFRASTRUCTURE -- named input domains for the terrain shadow layer (_compute_opera_shadow_layer :4215-4283),
shared by tests/test_shadow_domain.py (the oracle alone: what each domain is for) and tests/test_gpu_shadow_domain.py
(dswx_shadow_v3 / dswx_shadow_v2 against the oracle on every C-ABI entry).  Pure numpy, fixed seeds.

    shadow = ~(low_inc | ~backslope)      low_inc:   degrees(arccos(q)) <= max_sun_local_inc_angle
                                          backslope: degrees(arctan(t)) <= min_slope_angle
    n0 = -grad_x / sx,  n1 = -grad_y / -|sy|,  q = (n0 s0 + n1 s1 + s2) / sqrt(n0^2 + n1^2 + 1),  t = n0 sin az + n1 cos az

The filter kernel (dswx_shadow_v3) evaluates q and t approximately in float32, decides a pixel when it clears its
threshold by more than a host-computed bound, and recomputes it exactly otherwise, or when S = n0^2 + n1^2 + 1 is not
below 2^60.  The domains walk what that argument rests on: the magnitude of the height differences (`magnitudes`), the
pixel spacings and their signs (`spacings`), the sun vector and the thresholds at and past their edges (`sun`), data
lying ON the thresholds at large magnitudes and odd spacings (`on_threshold`), and the launch geometry (`geometry`).

A case is `Case(name, dem, az, el, min_slope, max_inc, sx, sy)`: a float32 DEM [H][W] and the six arguments of the
reference's function, the spacings as Python floats (as the reference's caller passes them)."""
import collections
import functools

import numpy as np

from oracle import dswx_oracle as o

Case = collections.namedtuple('Case', 'name dem az el min_slope max_inc sx sy')

DOMAINS = ('magnitudes', 'spacings', 'sun', 'on_threshold', 'geometry')
H0, W0 = 40, 72                       # every raster but the geometry tiles
SUN0, THR0 = (141.0, 35.0), (-5.0, 40.0)
FLT_MAX = float(np.finfo(np.float32).max)
S_SANE = 2.0 ** 60                    # the filter's `sane` gate: S < 2^60

SCALES = (1e-30, 1e-12, 1e-3, 1.0, 1e3, 1e6, 1e9, 1e12, 1e15, 1e18, 1e19, 1e25)
SPACINGS = ((30.0, -30.0), (-30.0, 30.0), (-30.0, -30.0), (2.77e-4, 2.77e-4), (30.1, 1 / 3), (1e-20, 1e20), (1e30, 1e30),
            (3e38, 1e-38), (0.0, 30.0))
SUN_ELEVATIONS = (0.0, 1e-6, 45.0, 89.999, 90.0, -10.0, 100.0)
SUN_AZIMUTHS = (0.0, 90.0, 180.0, 270.0, 360.0, -45.0, 720.5)
SUN_MAX_INC = (0.0, 'zenith', 90.0, 180.0, -1.0)             # 'zenith' = 90 - el: flat ground sits on the threshold
SUN_MIN_SLOPE = (0.0, -5.0, 5.0, -90.0, 90.0, 1e-30, -1e-30)  # the last two: the t_tiny branch, threshold not 0
# geometry: output shapes around one quad, the overlapping last quad, the 8 rows of a block and the second block in x
GEOMETRY_OH = tuple(range(1, 18))
GEOMETRY_OW = tuple(range(1, 10)) + (255, 256, 257, 260, 261)
GEOMETRY_SHAPES = tuple((oh, ow) for oh in GEOMETRY_OH for ow in GEOMETRY_OW)
GEOMETRY_MARGINS = (0, 1, 2, 3, 50)
GEOMETRY_TILES = 3


# ---- surfaces (float64) ------------------------------------------------------------------------------------------------
def rough(h=H0, w=W0, seed=11):
    """A random-walk surface in metres: steps of ~20 m per pixel along both axes (slopes of tens of degrees at 30 m
    spacing) and 5 m of pixel noise."""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.normal(0, 20, w))[None, :] + np.cumsum(rng.normal(0, 20, h))[:, None] +
            rng.normal(0, 5, (h, w)))


def terraced(h=H0, w=W0, seed=12, unit=15.0):
    """Integer random walks along both axes times `unit` metres: the central differences take five values per axis, so
    q and t take a few dozen values, each on many pixels -- a threshold placed on one of them has all of those pixels
    exactly on it (also exact zero differences next to steps)."""
    rng = np.random.default_rng(seed)
    return unit * (np.cumsum(rng.integers(-1, 2, w))[None, :] + np.cumsum(rng.integers(-1, 2, h))[:, None]).astype(np.float64)


def _f32(z):
    with np.errstate(over='ignore', under='ignore'):
        return np.ascontiguousarray(z, dtype=np.float32)


def _neg_nan():
    return np.array([0xffc00000], np.uint32).view(np.float32)[0]


SPECIALS = collections.OrderedDict([
    ('pzero', np.float32(0.0)), ('nzero', np.float32(-0.0)), ('denormal', np.float32(1e-44)), ('flt_max', np.float32(FLT_MAX)),
    ('neg_flt_max', np.float32(-FLT_MAX)), ('nan', np.float32(np.nan)), ('neg_nan', _neg_nan()), ('inf', np.float32(np.inf)),
    ('neg_inf', np.float32(-np.inf)), ('nodata_32768', np.float32(-32768.0)), ('nodata_9999', np.float32(-9999.0))])


# ---- the reference's arguments -----------------------------------------------------------------------------------------
def sun_scalars(az, el):
    """(sun vector, sin az, cos az) formed exactly as the reference forms them (:4246-4253, :4276-4277)."""
    a, zen = np.radians(az), np.radians(90 - el)
    return [np.sin(a) * np.sin(zen), np.cos(a) * np.sin(zen), np.cos(zen)], np.sin(a), np.cos(a)


def arguments(case, float64=True):
    """(q, t, n0, n1) of every pixel.  float64=True: the real-number values as closely as float64 gives them (the DEM
    widened first).  float64=False: the float64 arrays that the reference's expressions give under numpy >= 2 (gradient,
    normal and norm in float32, the products with the sun scalars in float64), which is what 'nep50' compares."""
    sun, sa, ca = sun_scalars(case.az, case.el)
    dem = case.dem.astype(np.float64) if float64 else case.dem
    with np.errstate(all='ignore'):
        gy, gx = np.gradient(dem)
        n0, n1 = -gx / case.sx, -gy / - abs(case.sy)
        norm = np.sqrt(n0 ** 2 + n1 ** 2 + 1)
        q = (n0 * sun[0] + n1 * sun[1] + sun[2]) / norm
        t = n0 * sa + n1 * ca
    return q, t, n0, n1


def expected(case, legacy, margin=0):
    """The oracle's layer of a case as uint8 (1 = not shadow), cropped by `margin`."""
    with np.errstate(all='ignore'):
        full = o.compute_opera_shadow_layer(case.dem, case.az, case.el, case.min_slope, case.max_inc, case.sx, case.sy,
                                            legacy_promotion=legacy)
    h, w = case.dem.shape
    return np.ascontiguousarray(full[margin:h - margin, margin:w - margin], dtype=np.uint8)


def band_counts(case, margin=3):
    """Pixels of the cropped raster inside the filter's uncertainty band, counted in float64: (|q - inc_q_min| <= 4e-6,
    |t - slope_arg_max| <= 2^-18 (|n0 sin| + |n1 cos|), either)."""
    q, t, n0, n1 = (a[margin:-margin, margin:-margin] for a in arguments(case))
    _, sa, ca = sun_scalars(case.az, case.el)
    inc_q_min, slope_arg_max = np.cos(np.radians(case.max_inc)), np.tan(np.radians(case.min_slope))
    with np.errstate(all='ignore'):
        in_q = np.abs(q - inc_q_min) <= 4e-6
        in_t = np.abs(t - slope_arg_max) <= 2.0 ** -18 * (np.abs(n0 * sa) + np.abs(n1 * ca))
    return int(in_q.sum()), int(in_t.sum()), int((in_q | in_t).sum())


# ---- the domains -------------------------------------------------------------------------------------------------------
def _case(name, dem, az=SUN0[0], el=SUN0[1], min_slope=THR0[0], max_inc=THR0[1], sx=30.0, sy=30.0):
    return Case(name, _f32(dem), float(az), float(el), float(min_slope), float(max_inc), float(sx), float(sy))


def mixed_scales():
    """Patches of several scales side by side (widths that are no multiple of 4, the order rotated half way down), so
    that neighbouring quads -- and the pixels of one quad -- sit on both sides of S = 2^60 and of the float32 overflow
    of n0 * n0 in the exact path."""
    base = rough(seed=13)
    scales = [1.0, 1e9, 1e12, 1e6, 1e19, 1e22]
    edges = [0, 11, 24, 33, 47, 59, W0]
    z = np.empty_like(base)
    for k in range(6):
        z[:H0 // 2, edges[k]:edges[k + 1]] = base[:H0 // 2, edges[k]:edges[k + 1]] * scales[k]
        z[H0 // 2:, edges[k]:edges[k + 1]] = base[H0 // 2:, edges[k]:edges[k + 1]] * scales[(k + 3) % 6]
    return z


def _magnitudes():
    base = rough()
    out = [_case(f'scale_{s:g}', base * s) for s in SCALES]
    out.append(_case('mixed_scales', mixed_scales()))
    rng = np.random.default_rng(14)
    out.append(_case('offset_8000', 8000.0 + 0.01 * rng.uniform(-1, 1, (H0, W0))))
    # +-0 and float32 denormal steps: exact zero differences and differences of 1e-44, at the default thresholds and at a
    # zero slope threshold (t_tiny) with flat ground on the incidence threshold
    zeros = np.zeros((H0, W0), np.float32)
    zeros[::2, 1::2] = -0.0
    zeros[::3, ::5] = np.float32(1e-44)
    zeros[1::7, 2::3] = np.float32(-3e-39)
    out.append(_case('zeros_denormals', zeros))
    out.append(_case('zeros_denormals_tiny', zeros, min_slope=0.0, max_inc=90.0 - SUN0[1]))
    vals = list(SPECIALS.values())
    pix = _f32(base)
    for k in range(6 * len(vals)):
        pix[int(rng.integers(0, H0)), int(rng.integers(0, W0))] = vals[k % len(vals)]
    out.append(_case('special_pixels', pix))
    lines = _f32(base)
    for k, v in enumerate(vals):                       # rows 2, 9, 16, ...; columns 3, 15, 27, ... (odd values)
        if k % 2 == 0:
            lines[2 + 7 * (k // 2), :] = v
        else:
            lines[:, 3 + 12 * (k // 2)] = v
    out.append(_case('special_rows_columns', lines))
    blocks = _f32(base)
    for k, v in enumerate(vals):                       # 5 x 7 blocks on a 3 x 4 grid, none touching another
        y, x = 3 + 12 * (k // 4), 5 + 17 * (k % 4)
        blocks[y:y + 5, x:x + 7] = v
    out.append(_case('special_blocks', blocks))
    return out


def _spacings():
    base = rough()
    return [_case(f'spacing_{sx:g}_{sy:g}', base, sx=sx, sy=sy) for sx, sy in SPACINGS]


def _sun():
    """Every (elevation, azimuth) pair on the rough and on the gentle terrain; max_inc and min_slope walk their lists in
    shuffled order, so every value of either meets many sun vectors."""
    rng = np.random.default_rng(15)
    terrains = (('rough', rough()), ('gentle', rough() * 0.05))
    pairs = [(el, az, tn) for el in SUN_ELEVATIONS for az in SUN_AZIMUTHS for tn in range(2)]
    n = len(pairs)
    inc_order = np.concatenate([rng.permutation(len(SUN_MAX_INC)) for _ in range(-(-n // len(SUN_MAX_INC)))])
    slope_order = np.concatenate([rng.permutation(len(SUN_MIN_SLOPE)) for _ in range(-(-n // len(SUN_MIN_SLOPE)))])
    out = []
    for i, (el, az, tn) in enumerate(pairs):
        max_inc = SUN_MAX_INC[inc_order[i]]
        max_inc = 90.0 - el if max_inc == 'zenith' else max_inc
        min_slope = SUN_MIN_SLOPE[slope_order[i]]
        out.append(_case(f'el{el:g}_az{az:g}_{terrains[tn][0]}_inc{max_inc:g}_slope{min_slope:g}', terrains[tn][1],
                         az=az, el=el, min_slope=min_slope, max_inc=max_inc))
    return out


ON_THRESHOLD_TERRAINS = (     # (name, scale, sx, sy, quantile of q, quantile of t)
    ('scale_1e3', 1e3, 30.0, 30.0, 0.5, 0.3), ('scale_1e6', 1e6, 30.0, 30.0, 0.3, 0.5), ('scale_1e9', 1e9, 30.0, 30.0, 0.7, 0.7),
    ('scale_1e12', 1e12, 30.0, 30.0, 0.5, 0.7), ('scale_1e19', 1e19, 30.0, 30.0, 0.3, 0.3),
    ('spacing_30.1_third', 1.0, 30.1, 1 / 3, 0.5, 0.5), ('spacing_neg30_neg30', 1.0, -30.0, -30.0, 0.7, 0.3),
    ('spacing_neg30_30', 1.0, -30.0, 30.0, 0.3, 0.7), ('spacing_geographic', 1.0, 2.77e-4, 2.77e-4, 0.5, 0.3))


def _on_threshold():
    """Thresholds at quantiles (the nearest data value) of the case's own q and t on terraced terrain: the most
    populated values of the distribution lie on the decision boundaries."""
    out = []
    for k, (name, scale, sx, sy, qq, tq) in enumerate(ON_THRESHOLD_TERRAINS):
        az, el = (141.0, 35.0) if k % 2 == 0 else (233.0, 52.5)
        c = _case(name, terraced(seed=20 + k) * scale, az=az, el=el, sx=sx, sy=sy)
        q, t, _, _ = arguments(c)
        max_inc = float(np.degrees(np.arccos(np.clip(np.quantile(q, 1 - qq, method='nearest'), -1, 1))))
        min_slope = float(np.degrees(np.arctan(np.quantile(t, tq, method='nearest'))))
        out.append(c._replace(min_slope=min_slope, max_inc=max_inc))
    # NEAR the incidence threshold, not on it: terraces with micrometres of noise spread a populated value of q over a few
    # 1e-7 around the threshold -- inside the filter's bound, where the approximate value itself is on the wrong side for
    # some.  A slope threshold of 90 degrees holds for every pixel, so the layer is the incidence test alone.
    for name, scale, sx in (('near_scale_1e6', 1e6, 30.0), ('near_geographic', 1.0, 2.77e-4)):
        rng = np.random.default_rng(40)
        c = _case(name, (terraced(seed=40) + rng.uniform(-3e-6, 3e-6, (H0, W0))) * scale, sx=sx, sy=sx, min_slope=90.0)
        q = arguments(c)[0]
        out.append(c._replace(max_inc=float(np.degrees(np.arccos(np.clip(np.quantile(q, 0.5, method='nearest'), -1, 1))))))
    return out


def _geometry():
    """The tiles that every geometry case is cut from (its top left corner): rough terrain at scale 1e3, on which about
    half the pixels are shadow."""
    h, w = max(GEOMETRY_OH) + 2 * max(GEOMETRY_MARGINS), max(GEOMETRY_OW) + 2 * max(GEOMETRY_MARGINS)
    return [_case(f'tile_{t}', rough(h, w, seed=30 + t) * 1e3) for t in range(GEOMETRY_TILES)]


_BUILDERS = dict(magnitudes=_magnitudes, spacings=_spacings, sun=_sun, on_threshold=_on_threshold, geometry=_geometry)


@functools.lru_cache(maxsize=None)
def cases(domain):
    """The cases of a domain (built once; treat the arrays as read-only)."""
    out = _BUILDERS[domain]()
    for c in out:
        c.dem.setflags(write=False)
    return tuple(out)


def case(domain, name):
    return next(c for c in cases(domain) if c.name == name)


def geometry_dems(oh, ow, margin):
    """The GEOMETRY_TILES DEMs [n][oh + 2 margin][ow + 2 margin] of one geometry case."""
    return np.ascontiguousarray(np.stack([c.dem[:oh + 2 * margin, :ow + 2 * margin] for c in cases('geometry')]))


@functools.lru_cache(maxsize=None)
def _geometry_full(legacy):
    return tuple(expected(c, legacy) for c in cases('geometry'))


def geometry_expected(oh, ow, margin, legacy):
    """The oracle's layers [n][oh][ow] of one geometry case.  With a margin every output pixel is an interior pixel of
    the cut as of the whole tile (central differences over the same neighbours), so the layers are cut from the
    oracle's layer of the whole tile, computed once; without one the borders take one-sided differences and the oracle
    runs on the cut itself."""
    if margin == 0:
        return np.stack([expected(c._replace(dem=c.dem[:oh, :ow]), legacy) for c in cases('geometry')])
    return np.ascontiguousarray(np.stack([f[margin:margin + oh, margin:margin + ow] for f in _geometry_full(legacy)]))
