"""Planes resampled onto another lattice through a mesh of source coordinates, include/dswx_hip.h ("warp"), stated in numpy --
and the meshes themselves, which are made on the host: the device sees integers and never a projection.

THE DEFINITION.  The input is [n_tiles, H, W] of 1-, 2- or 4-byte elements, the destination dst_h x dst_w per tile.  The mesh is
int32 [mesh_h, mesh_w, 2] = (x, y) in 1/256 SOURCE pixel (source pixel (c, r) has its centre at (256 c + 128, 256 r + 128)),
one node every step = 1 << shift destination pixels: node (i, j) is the source position of the CENTRE of destination pixel
(X, Y) = (j * step, i * step); mesh_h = ((dst_h + step - 1) >> shift) + 1.  With i = Y >> shift, fy = Y & (step - 1) and j, fx
likewise, in 64-bit integers for x and for y

    num = (step - fy) * ((step - fx) * x[i, j] + fx * x[i, j + 1]) + fy * ((step - fx) * x[i + 1, j] + fx * x[i + 1, j + 1])
    sx  = (num + (1 << (2 * shift - 1))) >> (2 * shift)               (arithmetic; shift 0: sx = x[i, j])

and the nearest source pixel is c = sx >> 8, r = sy >> 8, INSIDE iff 0 <= c < W and 0 <= r < H.

    dst         the element of source pixel (c, r) of the same tile where inside, else `outside`        the plane's dtype
    src_index   r * W + c where inside, else OUTSIDE (0xFFFFFFFF)                                       uint32
    head        [pixels, inside, outside, min row, max row, min col, max col, 0] (H, 0, W, 0 if none)   uint64 [n_tiles, 8]

warp_tiles calls neither dswx_warp_host nor the device: the tests pin the three to each other.

THE MESHES.  affine_mesh: two north-up geotransforms of one SRS.  utm_mesh: two WGS 84 / UTM zones (EPSG 326zz / 327zz) through
this module's own transverse Mercator -- the Krueger series in the third flattening n to order n^6, forward and inverse, in
numpy float64.  UNPINNED: GDAL and PROJ are not part of this project's environment, so gdal.Warp's own choice of the nearest
pixel, its approximate transformer (0.125 pixel error threshold) and its handling of a centre exactly on a pixel boundary
are not pinned by execution; the projection is pinned to independent statements of its own instead (tests/test_warp.py: round
trip, meridian arc by quadrature, conformality, the Redfearn series).  Still refused: bilinear / cubic / mode / average
resampling, SRSs other than WGS 84 / UTM, the antimeridian.
"""
import numpy as np

from . import geotiff

OUTPUTS = ('dst', 'src_index', 'head')
HEAD_WORDS, MAX_SHIFT, OUTSIDE, MAX_PIXELS = 8, 8, 0xFFFFFFFF, 1 << 30
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# WGS 84 / UTM
WGS84_A, WGS84_INV_F = 6378137.0, 298.257223563
UTM_K0, UTM_FALSE_EASTING, UTM_FALSE_NORTHING_SOUTH = 0.9996, 500000.0, 10000000.0


class Spec:
    """dswx_warp_spec_t: elem_bytes 1 / 2 / 4, shift 0 .. 8, `outside` (its low elem_bytes bytes are the element of a pixel that
    is not inside), and the two strides (0 = packed plane, 0 = one mesh for all tiles)."""

    def __init__(self, elem_bytes, shift, outside=0, src_tile_stride=0, mesh_tile_stride_nodes=0):
        self.elem_bytes, self.shift, self.outside = int(elem_bytes), int(shift), int(outside) & 0xFFFFFFFF
        self.src_tile_stride, self.mesh_tile_stride_nodes = int(src_tile_stride), int(mesh_tile_stride_nodes)
        self.reserved = 0
        if self.elem_bytes not in (1, 2, 4):
            raise ValueError(f'elem_bytes {self.elem_bytes}: not 1, 2 or 4')
        if not 0 <= self.shift <= MAX_SHIFT:
            raise ValueError(f'shift {self.shift} outside 0 .. {MAX_SHIFT}')


def mesh_shape(dst_shape, shift):
    """(mesh_h, mesh_w) of a destination of dst_shape = (dst_h, dst_w)."""
    step = 1 << shift
    return ((int(dst_shape[0]) + step - 1) >> shift) + 1, ((int(dst_shape[1]) + step - 1) >> shift) + 1


def positions(mesh, shift, dst_shape):
    """(sx, sy) int64 [dst_h, dst_w]: the source position of every destination pixel in 1/256 pixel, by the definition."""
    dh, dw = (int(v) for v in dst_shape)
    mh, mw = mesh_shape((dh, dw), shift)
    mesh = np.asarray(mesh)
    if mesh.shape != (mh, mw, 2):
        raise ValueError(f'a mesh for {dh} x {dw} at shift {shift} is [{mh}, {mw}, 2], not {mesh.shape}')
    m = mesh.astype(np.int64)
    step = 1 << shift
    Y, X = np.arange(dh, dtype=np.int64)[:, None], np.arange(dw, dtype=np.int64)[None, :]
    i, fy, j, fx = Y >> shift, Y & (step - 1), X >> shift, X & (step - 1)
    half = (1 << (2 * shift - 1)) if shift else 0
    out = []
    for k in range(2):
        v = m[:, :, k]
        num = (step - fy) * ((step - fx) * v[i, j] + fx * v[i, j + 1]) + fy * ((step - fx) * v[i + 1, j] + fx * v[i + 1, j + 1])
        out.append((num + half) >> (2 * shift))
    return out[0], out[1]


def warp_tiles(tiles, mesh, shift, dst_shape, outside=0):
    """{'dst': [n, dst_h, dst_w] of the tiles' dtype, 'src_index': uint32 [n, dst_h, dst_w], 'head': uint64 [n, 8]} of tiles
    [n_tiles, H, W] warped through `mesh` -- int32 [mesh_h, mesh_w, 2] for all tiles, or [n_tiles, mesh_h, mesh_w, 2]."""
    tiles = np.asarray(tiles)
    if tiles.ndim != 3 or tiles.dtype.itemsize not in (1, 2, 4):
        raise ValueError(f'the tiles are [n_tiles, H, W] of 1-, 2- or 4-byte elements, not {tiles.dtype} {tiles.shape}')
    n, H, W = tiles.shape
    dh, dw = (int(v) for v in dst_shape)
    if H * W > MAX_PIXELS or dh * dw > MAX_PIXELS:
        raise ValueError('more than 2^30 pixels')
    mesh = np.asarray(mesh)
    bits = 8 * tiles.dtype.itemsize
    fill = np.array([int(outside) & ((1 << bits) - 1)], dtype=f'<u{tiles.dtype.itemsize}').view(tiles.dtype)[0]
    dst = np.full((n, dh, dw), fill, dtype=tiles.dtype)
    index = np.full((n, dh, dw), OUTSIDE, dtype=np.uint32)
    head = np.zeros((n, HEAD_WORDS), dtype=np.uint64)
    shared = positions(mesh, shift, (dh, dw)) if mesh.ndim == 3 else None
    for t in range(n):
        sx, sy = shared if shared is not None else positions(mesh[t], shift, (dh, dw))
        c, r = sx >> 8, sy >> 8
        inside = (c >= 0) & (c < W) & (r >= 0) & (r < H)
        idx = (r * W + c)[inside]
        if idx.size:
            dst[t][inside] = tiles[t].reshape(-1)[idx]
            index[t][inside] = idx
        k = int(inside.sum())
        head[t] = [dh * dw, k, dh * dw - k, int(r[inside].min()) if k else H, int(r[inside].max()) if k else 0,
                   int(c[inside].min()) if k else W, int(c[inside].max()) if k else 0, 0]
    return {'dst': dst, 'src_index': index, 'head': head}


# ---- meshes -------------------------------------------------------------------------------------------------------------

def _north_up(gt, what):
    gt = tuple(float(v) for v in gt)
    if len(gt) != 6:
        raise ValueError(f'a geotransform has six numbers, not {len(gt)}')
    if gt[2] != 0.0 or gt[4] != 0.0:
        raise ValueError(f'{what} geotransform {gt} is rotated')
    if gt[1] == 0.0 or gt[5] == 0.0:
        raise ValueError(f'{what} geotransform {gt} has an empty pixel')
    return gt


def _node_pixels(dst_shape, shift):
    """(Y [mesh_h, 1], X [1, mesh_w]) float64: the destination pixels whose centres the nodes describe."""
    mh, mw = mesh_shape(dst_shape, shift)
    step = 1 << shift
    return (np.arange(mh, dtype=np.float64) * step)[:, None], (np.arange(mw, dtype=np.float64) * step)[None, :]


def _quantise(col, row):
    """Continuous source pixel coordinates (pixel c covers [c, c + 1)) -> int32 [.., 2] in 1/256 pixel, clamped to int32."""
    q = np.stack(np.broadcast_arrays(np.rint(256.0 * col), np.rint(256.0 * row)), axis=-1)
    q = np.where(np.isfinite(q), q, INT32_MAX)
    return np.clip(q, INT32_MIN, INT32_MAX).astype(np.int64).astype(np.int32)


def _affine_exact(src_gt, dst_gt, Y, X):
    """Continuous source pixel coordinates (col, row) of the centres of destination pixels (X, Y) (floats allowed)."""
    x = dst_gt[0] + (X + 0.5) * dst_gt[1]
    y = dst_gt[3] + (Y + 0.5) * dst_gt[5]
    return (x - src_gt[0]) / src_gt[1], (y - src_gt[3]) / src_gt[5]


def affine_mesh(src_gt, dst_gt, dst_shape, shift):
    """The mesh int32 [mesh_h, mesh_w, 2] that lays a source raster with GDAL geotransform src_gt (x0, dx, 0, y0, 0, dy) onto a
    destination of dst_shape with dst_gt in the SAME SRS: a shifted origin, another pixel size.  Rotated geotransforms are
    refused.  An affine map is reproduced by the mesh interpolation up to the rounding of the nodes."""
    s, d = _north_up(src_gt, 'the source'), _north_up(dst_gt, 'the destination')
    Y, X = _node_pixels(dst_shape, shift)
    return _quantise(*_affine_exact(s, d, Y, X))


def _kruger(n):
    """(A / a, alpha [6], beta [6]) of the Krueger series to order n^6 (Karney 2011, eqs. 35 and 36)."""
    n2, n3, n4, n5, n6 = n ** 2, n ** 3, n ** 4, n ** 5, n ** 6
    A = (1 + n2 / 4 + n4 / 64 + n6 / 256) / (1 + n)
    alpha = (n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800,
             13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360,
             61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440,
             49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600,
             34729 * n5 / 80640 - 3418889 * n6 / 1995840,
             212378941 * n6 / 319334400)
    beta = (n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800,
            n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720,
            17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720,
            4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600,
            4583 * n5 / 161280 - 108847 * n6 / 3991680,
            20648693 * n6 / 638668800)
    return A, alpha, beta


_F = 1.0 / WGS84_INV_F
_E2 = _F * (2.0 - _F)
_E = np.sqrt(_E2)
_A_OVER_A, _ALPHA, _BETA = _kruger(_F / (2.0 - _F))


def _taup(tau):
    """tan of the conformal latitude from tan of the geographic one."""
    sigma = np.sinh(_E * np.arctanh(_E * tau / np.sqrt(1.0 + tau * tau)))
    return tau * np.sqrt(1.0 + sigma * sigma) - sigma * np.sqrt(1.0 + tau * tau)


def tm_forward(lon_deg, lat_deg, lon0_deg):
    """WGS 84 transverse Mercator, central meridian lon0: (easting, northing) in metres WITHOUT false easting / northing, scale
    k0 = 0.9996 on the central meridian; numpy float64, any shape."""
    lam = np.radians(np.asarray(lon_deg, dtype=np.float64) - lon0_deg)
    tp = _taup(np.tan(np.radians(np.asarray(lat_deg, dtype=np.float64))))
    xi_p = np.arctan2(tp, np.cos(lam))
    eta_p = np.arcsinh(np.sin(lam) / np.sqrt(tp * tp + np.cos(lam) ** 2))
    xi, eta = xi_p.copy(), eta_p.copy()
    for j, a in enumerate(_ALPHA, 1):
        xi = xi + a * np.sin(2 * j * xi_p) * np.cosh(2 * j * eta_p)
        eta = eta + a * np.cos(2 * j * xi_p) * np.sinh(2 * j * eta_p)
    k = UTM_K0 * WGS84_A * _A_OVER_A
    return k * eta, k * xi


def tm_inverse(easting, northing, lon0_deg):
    """The inverse of tm_forward: (lon, lat) in degrees."""
    k = UTM_K0 * WGS84_A * _A_OVER_A
    xi, eta = np.asarray(northing, dtype=np.float64) / k, np.asarray(easting, dtype=np.float64) / k
    xi_p, eta_p = xi.copy(), eta.copy()
    for j, b in enumerate(_BETA, 1):
        xi_p = xi_p - b * np.sin(2 * j * xi) * np.cosh(2 * j * eta)
        eta_p = eta_p - b * np.cos(2 * j * xi) * np.sinh(2 * j * eta)
    tp = np.sin(xi_p) / np.sqrt(np.sinh(eta_p) ** 2 + np.cos(xi_p) ** 2)
    lam = np.arctan2(np.sinh(eta_p), np.cos(xi_p))
    tau = tp.copy()
    for _ in range(6):                       # Newton on taup(tau) = tp: quadratic, three steps reach the last bit below 89 degrees
        ti = _taup(tau)
        tau = tau + (tp - ti) / np.sqrt(1.0 + ti * ti) * (1.0 + (1.0 - _E2) * tau * tau) / ((1.0 - _E2) * np.sqrt(1.0 + tau * tau))
    return np.degrees(lam) + lon0_deg, np.degrees(np.arctan(tau))


def utm_zone(epsg):
    """(central meridian in degrees, false northing) of EPSG 326zz (north) / 327zz (south); anything else is refused."""
    code = int(epsg) if epsg is not None else 0
    zone = code % 100
    if code // 100 not in (326, 327) or not 1 <= zone <= 60:
        raise ValueError(f'EPSG {epsg} is not WGS 84 / UTM (EPSG 32601 .. 32660, 32701 .. 32760): only those are reprojected')
    return -183.0 + 6.0 * zone, UTM_FALSE_NORTHING_SOUTH if code // 100 == 327 else 0.0


def utm_to_utm(x, y, src_epsg, dst_epsg):
    """Map coordinates (x, y) of one WGS 84 / UTM zone (EPSG 326zz / 327zz) in another: through lon / lat; equal codes: as given."""
    lon0_s, fn_s = utm_zone(src_epsg)
    lon0_d, fn_d = utm_zone(dst_epsg)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if (lon0_s, fn_s) == (lon0_d, fn_d):
        return x, y
    lon, lat = tm_inverse(x - UTM_FALSE_EASTING, y - fn_s, lon0_s)
    e, n = tm_forward(lon, lat, lon0_d)
    return e + UTM_FALSE_EASTING, n + fn_d


def _utm_exact(src_gt, src_epsg, dst_gt, dst_epsg, Y, X):
    """Continuous source pixel coordinates (col, row) of the centres of destination pixels (X, Y) (floats allowed): destination
    pixel centre -> lon / lat -> source zone -> source pixel."""
    x, y = utm_to_utm(dst_gt[0] + (X + 0.5) * dst_gt[1] + 0.0 * Y, dst_gt[3] + (Y + 0.5) * dst_gt[5] + 0.0 * X, dst_epsg, src_epsg)
    return (x - src_gt[0]) / src_gt[1], (y - src_gt[3]) / src_gt[5]


def _mesh_and_deviation(exact, dst_shape, shift):
    """(mesh, deviation) of exact(Y, X) -> continuous source pixel coordinates (col, row): the nodes quantised, and the largest
    deviation of the interpolated mesh from the exact mapping at the CENTRES of the mesh cells, in 1/256 source pixel."""
    Y, X = _node_pixels(dst_shape, shift)
    col, row = exact(Y, X)
    mesh = _quantise(col, row)
    half = (1 << shift) / 2.0
    ccol, crow = exact(Y[:-1] + half, X[:, :-1] + half)
    m = mesh.astype(np.float64)
    mid = (m[:-1, :-1] + m[:-1, 1:] + m[1:, :-1] + m[1:, 1:]) / 4.0
    dev = np.maximum(np.abs(mid[..., 0] - 256.0 * ccol), np.abs(mid[..., 1] - 256.0 * crow))
    return mesh, float(dev.max()) if dev.size else 0.0


def utm_mesh(src_gt, src_epsg, dst_gt, dst_epsg, dst_shape, shift):
    """(mesh int32 [mesh_h, mesh_w, 2], deviation): the mesh that lays a source raster (north-up geotransform src_gt, EPSG
    326zz / 327zz) onto a destination of dst_shape with dst_gt in another -- or the same -- WGS 84 / UTM zone, and the largest
    deviation of the interpolated mesh from the exact mapping at the CENTRES of the mesh cells, in 1/256 source pixel, so that a
    caller can choose `shift`.  Positions beyond int32 are clamped to INT32_MIN / INT32_MAX."""
    s, d = _north_up(src_gt, 'the source'), _north_up(dst_gt, 'the destination')
    return _mesh_and_deviation(lambda Y, X: _utm_exact(s, src_epsg, d, dst_epsg, Y, X), dst_shape, shift)


GEOGRAPHIC_EPSG = 4326


def _geographic_exact(src_gt, dst_gt, dst_epsg, Y, X):
    """Continuous source pixel coordinates (col, row) in a north-up raster in degrees (EPSG:4326) of the centres of destination
    pixels (X, Y) of a WGS 84 / UTM grid (floats allowed), and the longitudes: destination pixel centre -> tm_inverse -> pixel."""
    lon0, fn = utm_zone(dst_epsg)
    lon, lat = tm_inverse(dst_gt[0] + (X + 0.5) * dst_gt[1] + 0.0 * Y - UTM_FALSE_EASTING, dst_gt[3] + (Y + 0.5) * dst_gt[5] + 0.0 * X - fn, lon0)
    return (lon - src_gt[0]) / src_gt[1], (lat - src_gt[3]) / src_gt[5], lon


def geographic_mesh(src_gt, dst_gt, dst_epsg, dst_shape, shift):
    """(mesh int32 [mesh_h, mesh_w, 2], deviation) as utm_mesh reports them, for a source raster in EPSG:4326 (north-up
    geotransform src_gt in degrees: a DEM) laid onto a destination of dst_shape with dst_gt in a WGS 84 / UTM zone (dst_epsg
    326zz / 327zz).  A destination whose nodes leave -180 .. 180 degrees of longitude is refused: the antimeridian is out of
    scope."""
    s, d = _north_up(src_gt, 'the source'), _north_up(dst_gt, 'the destination')
    Y, X = _node_pixels(dst_shape, shift)
    lon = _geographic_exact(s, d, dst_epsg, Y, X)[2]
    if lon.size and (float(lon.min()) < -180.0 or float(lon.max()) > 180.0):
        raise ValueError(f'the destination reaches {float(lon.min()):.4f} .. {float(lon.max()):.4f} degrees of longitude: the source window '
                         'would cross the antimeridian, which is not handled')
    return _mesh_and_deviation(lambda Y, X: _geographic_exact(s, d, dst_epsg, Y, X)[:2], dst_shape, shift)


def in_degrees(src_gt):
    """Whether the origin of a north-up geotransform can be one in degrees: a longitude in -180 .. 180, a latitude in -90 ..
    90, and a pixel smaller than a degree.  A geotransform in metres that merely carries the code 4326 is not."""
    gt = tuple(float(v) for v in src_gt)
    return len(gt) == 6 and -180.0 <= gt[0] <= 180.0 and -90.0 <= gt[3] <= 90.0 and 0.0 < abs(gt[1]) < 1.0 and 0.0 < abs(gt[5]) < 1.0


def epsg_of(geo_tags):
    """The EPSG code of the GeoKey directory (ProjectedCSTypeGeoKey 3072, else GeographicTypeGeoKey 2048), or None."""
    if geotiff.TAG_GEOKEYS not in geo_tags:
        return None
    keys = [int(v) for v in geo_tags[geotiff.TAG_GEOKEYS][1]]
    found = {keys[i]: keys[i + 3] for i in range(4, len(keys) - 3, 4) if keys[i + 1] == 0}
    code = found.get(3072, found.get(2048))
    return code if code and code != 32767 else None


def mesh_between(src_gt, src_epsg, dst_gt, dst_epsg, dst_shape, shift):
    """(mesh, deviation) for two rasters by their geotransforms and EPSG codes: affine_mesh when the codes are equal (any SRS,
    None included), geographic_mesh for a source in EPSG:4326 whose geotransform is in degrees (in_degrees) under a WGS 84 / UTM
    destination, utm_mesh for two WGS 84 / UTM zones; refused otherwise -- a source that carries the code 4326 over a
    geotransform in metres included."""
    if src_epsg == dst_epsg:
        return affine_mesh(src_gt, dst_gt, dst_shape, shift), 0.0
    if src_epsg == GEOGRAPHIC_EPSG and in_degrees(src_gt):
        return geographic_mesh(src_gt, dst_gt, dst_epsg, dst_shape, shift)
    return utm_mesh(src_gt, src_epsg, dst_gt, dst_epsg, dst_shape, shift)
