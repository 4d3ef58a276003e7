"""Inputs shared by tests/test_land_mesh.py (CPU) and tests/test_gpu_land_mesh.py: maps, meshes and the cases built from them."""
import math

import numpy as np

from proteus_amd import landmesh, warp

WC_PIXEL, CG_PIXEL = 1.0 / 12000.0, 1.0 / 1008.0          # ESA WorldCover 10 m and Copernicus CGLS-100 m, degrees
FOREST = (111, 113, 115, 121, 300, -1)                     # (classes outside 0 .. 255 name no byte)
WC_BYTES = np.array([10, 10, 10, 50, 50, 80, 90, 95, 0, 20, 30, 40, 60, 100, 255], dtype=np.uint8)
CG_BYTES = np.array([111, 111, 113, 115, 121, 20, 30, 0, 200, 255], dtype=np.uint8)
LATITUDES = (0.5, 45.0, 70.0)


def maps(rng, n, wc_shape, cg_shape):
    """Patchy maps: classes drawn per block of a few pixels, so that 3 x 3 counts take every value."""
    def one(codes, shape, block):
        h, w = shape
        small = rng.integers(0, codes.size, size=(n, -(-h // block) + 1, -(-w // block) + 1))
        big = np.repeat(np.repeat(small, block, axis=1), block, axis=2)[:, :h, :w]
        noise = rng.integers(0, codes.size, size=(n, h, w))
        return codes[np.where(rng.random((n, h, w)) < 0.15, noise, big)].astype(np.uint8)
    return one(WC_BYTES, wc_shape, 5), one(CG_BYTES, cg_shape, 3)


def identity_mesh(dst_shape, shift, scale=(256, 256), offset=(128, 128)):
    """Destination pixel (x, y) -> (scale x + offset) in 1/256 source pixel; the default puts it on the centre of source pixel (x, y)."""
    mh, mw = warp.mesh_shape(dst_shape, shift)
    step = 1 << shift
    x = np.arange(mw, dtype=np.int64)[None, :] * step * scale[0] + offset[0] + np.zeros((mh, 1), dtype=np.int64)
    y = np.arange(mh, dtype=np.int64)[:, None] * step * scale[1] + offset[1] + np.zeros((1, mw), dtype=np.int64)
    return np.stack([x, y], axis=-1).astype(np.int32)


def garbage_mesh(rng, dst_shape, shift, n=None):
    """Any int32, the extremes included, and a share of nodes near a small raster so that some taps are inside."""
    mh, mw = warp.mesh_shape(dst_shape, shift)
    shape = ((n,) if n else ()) + (mh, mw, 2)
    m = rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64)
    near = rng.integers(-3000, 30000, size=shape, dtype=np.int64)
    pick = rng.random(shape)
    m = np.where(pick < 0.5, near, m)
    m = np.where(pick > 0.97, -(1 << 31), m)
    m = np.where(pick > 0.985, (1 << 31) - 1, m)
    return m.astype(np.int32)


def hls_grid(lat, shape, zone=32, pixel=30.0):
    """(geotransform of an HLS lattice of `shape` pixels centred on the central meridian of the zone at latitude `lat`, EPSG)."""
    lon0 = -183.0 + 6.0 * zone
    _, north = warp.tm_forward(lon0, lat, lon0)
    h, w = shape
    return (500000.0 - w // 2 * pixel, pixel, 0.0, round(float(north) / pixel) * pixel + h // 2 * pixel, 0.0, -pixel), 32600 + zone


def map_gt(lat, pixel, zone=32):
    """A north-up geotransform in degrees of a map that covers the lattice of hls_grid generously."""
    lon0 = -183.0 + 6.0 * zone
    return (lon0 - 1.0, pixel, 0.0, math.floor(lat) + 2.0, 0.0, -pixel)


def geographic_case(rng, lat, shape=(40, 52), shift_wc=5, shift_cg=3, n=1):
    """Maps in EPSG:4326 at their real pixel sizes under an HLS lattice at `lat`: (wc [n, h, w], cg, mesh_wc, mesh_cg) with the
    meshes relative to the source windows that the nodes need."""
    H, W = shape
    gt, epsg = hls_grid(lat, shape)
    fine_gt = (gt[0], gt[1] / 3, 0.0, gt[3], 0.0, gt[5] / 3)
    m_wc, d_wc = warp.geographic_mesh(map_gt(lat, WC_PIXEL), fine_gt, epsg, (3 * H, 3 * W), shift_wc)
    m_cg, d_cg = warp.geographic_mesh(map_gt(lat, CG_PIXEL), gt, epsg, (H, W), shift_cg)
    big = 1 << 24
    win_wc, m_wc = landmesh.source_window(m_wc, d_wc, big, big)
    win_cg, m_cg = landmesh.source_window(m_cg, d_cg, big, big)
    wc, cg = maps(rng, n, (win_wc[3], win_wc[2]), (win_cg[3], win_cg[2]))
    return wc, cg, m_wc, m_cg


def spec_of(shift_wc, shift_cg, **kw):
    kw.setdefault('forest_classes', FOREST)
    return landmesh.Spec(shift_wc, shift_cg, **kw)


def numpy_land(wc, cg, m_wc, m_cg, shape, spec):
    """proteus_amd.landmesh.land_tiles for the fields of a Spec."""
    return landmesh.land_tiles(wc, cg, m_wc, m_cg, shape, spec.shift_wc, spec.shift_cg, spec.outside_wc, spec.outside_cg,
                               spec.thresholds, spec.year_offset, spec.forest_classes)
