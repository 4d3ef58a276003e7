"""The LAND layer from land-cover maps that are NOT on the HLS grid, include/dswx_hip.h ("land mesh"), stated in numpy -- and the
plan that lays a map file onto a product: source window, mesh, shift.

THE DEFINITION.  For every tile, land == landcover_mask(W3, CG): W3 uint8 [3 H, 3 W] is warp.warp_tiles of the WorldCover tiles
[n, wc_h, wc_w] through mesh_wc (shift_wc, outside_wc) onto the lattice three times finer than the HLS lattice, CG uint8 [H, W]
warp.warp_tiles of the CGLS tiles [n, cg_h, cg_w] through mesh_cg (shift_cg, outside_cg) onto the HLS lattice.  Then the 3 x 3
counts of W3 -- water {80, 90, 95}, urban 50, tree 10, the last only where CG is a forest class -- and the hierarchy, later
rules winning: 255; tree >= thresholds[0]: 201; urban >= thresholds[1]: year_offset; urban >= thresholds[2]: 100 + year_offset;
water >= thresholds[3]: 200, the two developed classes stored modulo 256.

    land    uint8 [n, H, W]
    head    uint64 [n, 8]: HLS pixels; fine pixels whose WorldCover tap was inside, outside; HLS pixels whose CGLS tap was inside,
            outside; HLS pixels whose nine WorldCover taps were all outside; LAND pixels equal to 255; 0

land_tiles calls neither dswx_land_mesh_host nor the device: the tests pin the three to each other and to the chain of the
existing entries.  UNPINNED: GDAL is not part of this project's environment, so gdal.Warp's own choice of the nearest pixel and
its handling of a centre exactly on a pixel boundary are not pinned by execution.
"""
import numpy as np

from . import warp

OUTPUTS = ('land', 'head')
HEAD_WORDS = 8
MAX_LATTICE_PIXELS = (1 << 30) // 9
MESH_SHIFTS = (6, 5, 4)                    # the DEM's rule: tried in this order until the mesh deviates by at most 1/256 source pixel


class Spec:
    """dswx_land_mesh_spec_t: the two shifts 0 .. 8, the two `outside` bytes, thresholds [4], year_offset, the forest classes,
    and the strides (0 = packed planes, 0 = one mesh for all tiles, 0 = packed LAND)."""

    def __init__(self, shift_wc, shift_cg, outside_wc=0, outside_cg=0, thresholds=(6, 3, 7, 3), year_offset=0, forest_classes=(),
                 wc_tile_stride=0, cg_tile_stride=0, mesh_wc_tile_stride_nodes=0, mesh_cg_tile_stride_nodes=0, land_tile_stride=0):
        self.shift_wc, self.shift_cg = int(shift_wc), int(shift_cg)
        self.outside_wc, self.outside_cg = int(outside_wc), int(outside_cg)
        self.thresholds = tuple(int(v) for v in thresholds)
        self.year_offset = int(year_offset)
        self.forest_classes = [int(v) for v in (forest_classes if forest_classes is not None else ())]
        self.wc_tile_stride, self.cg_tile_stride = int(wc_tile_stride), int(cg_tile_stride)
        self.mesh_wc_tile_stride_nodes, self.mesh_cg_tile_stride_nodes = int(mesh_wc_tile_stride_nodes), int(mesh_cg_tile_stride_nodes)
        self.land_tile_stride = int(land_tile_stride)
        self.reserved = self.reserved2 = 0
        if len(self.thresholds) != 4:
            raise ValueError(f'thresholds are four numbers, not {len(self.thresholds)}')
        for name in ('shift_wc', 'shift_cg'):
            if not 0 <= getattr(self, name) <= warp.MAX_SHIFT:
                raise ValueError(f'{name} {getattr(self, name)} outside 0 .. {warp.MAX_SHIFT}')
        for name in ('outside_wc', 'outside_cg'):
            if not 0 <= getattr(self, name) <= 255:
                raise ValueError(f'{name} {getattr(self, name)} outside 0 .. 255')


def _sum3(a):
    """uint8 [3 H, 3 W] of 0 / 1 -> the 3 x 3 sums, int64 [H, W]."""
    h, w = a.shape[0] // 3, a.shape[1] // 3
    return a.reshape(h, 3, w, 3).astype(np.int64).sum(axis=(1, 3))


def land_of_warped(w3, cg, thresholds, year_offset, forest_classes):
    """LAND uint8 [H, W] of W3 uint8 [3 H, 3 W] and CG uint8 [H, W]: the counts and the hierarchy of the definition."""
    water = _sum3(np.isin(w3, (80, 90, 95)))
    urban = _sum3(w3 == 50)
    forest = np.isin(cg, [c for c in forest_classes if 0 <= c <= 255])
    tree = np.where(forest, _sum3(w3 == 10), 0)
    land = np.full(cg.shape, 255, dtype=np.uint8)
    land[tree >= thresholds[0]] = 201
    land[urban >= thresholds[1]] = year_offset & 0xFF
    land[urban >= thresholds[2]] = (100 + year_offset) & 0xFF
    land[water >= thresholds[3]] = 200
    return land


def land_tiles(worldcover, copernicus, mesh_wc, mesh_cg, shape, shift_wc, shift_cg, outside_wc=0, outside_cg=0,
               thresholds=(6, 3, 7, 3), year_offset=0, forest_classes=()):
    """{'land': uint8 [n, H, W], 'head': uint64 [n, 8]} of WorldCover tiles uint8 [n, wc_h, wc_w] and CGLS tiles uint8 [n, cg_h,
    cg_w] read through mesh_wc (int32 [mesh_h, mesh_w, 2] of the lattice 3 H x 3 W at shift_wc, or one per tile) and mesh_cg (of
    H x W at shift_cg)."""
    wc, cg = np.asarray(worldcover), np.asarray(copernicus)
    if wc.dtype != np.uint8 or cg.dtype != np.uint8 or wc.ndim != 3 or cg.ndim != 3 or wc.shape[0] != cg.shape[0]:
        raise ValueError(f'the maps are uint8 [n_tiles, h, w] with one n_tiles, not {wc.dtype} {wc.shape} and {cg.dtype} {cg.shape}')
    H, W = (int(v) for v in shape)
    if H * W > MAX_LATTICE_PIXELS:
        raise ValueError('more than 2^30 / 9 pixels')
    n = wc.shape[0]
    w3 = warp.warp_tiles(wc, mesh_wc, shift_wc, (3 * H, 3 * W), outside_wc)
    c1 = warp.warp_tiles(cg, mesh_cg, shift_cg, (H, W), outside_cg)
    land = np.zeros((n, H, W), dtype=np.uint8)
    head = np.zeros((n, HEAD_WORDS), dtype=np.uint64)
    for t in range(n):
        land[t] = land_of_warped(w3['dst'][t], c1['dst'][t], thresholds, int(year_offset), forest_classes or ())
        none_inside = _sum3(w3['src_index'][t] != warp.OUTSIDE) == 0
        head[t] = [H * W, w3['head'][t, 1], w3['head'][t, 2], c1['head'][t, 1], c1['head'][t, 2], int(none_inside.sum()),
                   int((land[t] == 255).sum()), 0]
    return {'land': land, 'head': head}


def source_window(mesh, deviation, height, width, pad=1):
    """(window (xoff, yoff, xsize, ysize) of a source raster of height x width, the mesh relative to that window): the extent
    of the nodes, widened by `pad` pixels and the deviation and clipped to the raster; (0, 0, 0, 0) if they miss it.  The
    nodes bound every interpolated position, so the window covers every tap that is inside the raster."""
    pad = int(pad) + int(np.ceil(deviation / 256.0))
    x, y = mesh[..., 0].astype(np.int64), mesh[..., 1].astype(np.int64)
    x0, x1 = max(int(x.min() >> 8) - pad, 0), min(int(x.max() >> 8) + pad + 1, int(width))
    y0, y1 = max(int(y.min() >> 8) - pad, 0), min(int(y.max() >> 8) + pad + 1, int(height))
    window = (x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else (0, 0, 0, 0)
    moved = np.clip(np.stack([x - 256 * window[0], y - 256 * window[1]], axis=-1), warp.INT32_MIN, warp.INT32_MAX).astype(np.int32)
    return window, moved


def choose_mesh(src_gt, src_epsg, dst_gt, dst_epsg, dst_shape, shifts=MESH_SHIFTS):
    """(mesh, shift, deviation): warp.mesh_between at the first of `shifts` whose mesh deviates by at most 1/256 source pixel,
    else at the last.  ValueError (warp's) for what mesh_between refuses."""
    for shift in shifts:
        mesh, deviation = warp.mesh_between(src_gt, src_epsg, dst_gt, dst_epsg, dst_shape, shift)
        if deviation <= 1.0:
            break
    return mesh, shift, deviation


def plan(info, geotransform, geo_tags, length, width, scale, on_grid=False):
    """What lays a land-cover map that is NOT on its grid onto the HLS grid refined `scale` times (3: WorldCover, 1: CGLS):
    (window (xoff, yoff, xsize, ysize) of the file to read, mesh int32 relative to that window, shift, deviation in 1/256 source
    pixel).  Taken: a north-up raster of ONE uint8 band in EPSG:4326 under a product in a WGS 84 / UTM zone, in a WGS 84 / UTM
    zone, or in the product's own SRS (warp.mesh_between decides); nearest pixel, no margin.  `on_grid`: the map lies on its
    grid already (the other one does not) and takes the identity through warp.affine_mesh, whatever SRS it names.
    NotImplementedError says what is taken for anything else: a rotated geotransform, another SRS, the antimeridian, a window
    above 2^30 pixels."""
    taken = ('a land-cover map is taken on its grid (CGLS: the HLS grid; WorldCover: 3x finer), or as a north-up raster of one '
             'uint8 band in EPSG:4326, in a WGS 84 / UTM zone or in the SRS of the product, of which a window of at most 2^30 '
             'pixels is read and laid onto the grid on the device, nearest pixel; not across the antimeridian')
    src_gt = info.geotransform
    src_epsg, dst_epsg = warp.epsg_of(info.geo_tags), warp.epsg_of(geo_tags)
    if on_grid:
        src_epsg = dst_epsg
    if src_gt is None:
        raise NotImplementedError(f'the map has no geotransform: {taken}')
    if getattr(info, 'dtype', np.dtype(np.uint8)) != np.dtype(np.uint8) or getattr(info, 'bands', 1) != 1:
        raise NotImplementedError(f'the map is not one uint8 band: {taken}')
    if src_epsg != dst_epsg and (src_epsg is None or dst_epsg is None):
        raise NotImplementedError(f'the map (EPSG {src_epsg}) or the product (EPSG {dst_epsg}) names no SRS: {taken}')
    dst_gt = (geotransform[0], geotransform[1] / scale, 0.0, geotransform[3], 0.0, geotransform[5] / scale)
    if geotransform[2] != 0 or geotransform[4] != 0:
        raise NotImplementedError(f'the product geotransform is rotated: {taken}')
    try:
        mesh, shift, deviation = choose_mesh(src_gt, src_epsg, dst_gt, dst_epsg, (scale * length, scale * width))
    except ValueError as e:
        raise NotImplementedError(f'{e}: {taken}')
    window, moved = source_window(mesh, deviation, info.height, info.width)
    if window[2] * window[3] > warp.MAX_PIXELS:
        raise NotImplementedError(f'the source window {window} has more than 2^30 pixels: {taken}')
    return window, moved, shift, deviation
