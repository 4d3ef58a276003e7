"""Every pixel whose centre lies within a radius of a polygon edge, include/dswx_hip.h ("reach"), stated in numpy.

Records, `tile_first`, the count of a tile, legality and malformed records are those of proteus_amd.burn (VERTEX_DTYPE, int32
coordinates in 1/256 pixel, the centre of pixel (c, r) at P = (256 c + 128, 256 r + 128)); `word` is ignored and nothing is
dropped: a horizontal edge takes part, and an edge whose endpoints coincide is a point.  `radius` R is in 1/256 pixel, 0 ..
MAX_RADIUS = 2^20.  Pixel (c, r) is reached by the well-formed edge A -> B iff, with d = B - A, u = P - A, D = d.d, t = u.d,

    D == 0 or t <= 0:  u.u <= R^2        t >= D:  |P - B|^2 <= R^2        otherwise:  (u x d)^2 <= R^2 D

in unbounded integers (at the extreme coordinates u x d passes 2^63 and R^2 D reaches 2^103).

    acc     uint32 [n_tiles, H, W]: the number of well-formed edges of the tile that reach the pixel, modulo 2^32
    mask    uint8 [n_tiles, H, W]: spec.burn where acc != 0, else src (when given) or spec.background
    head    uint64 [n_tiles, 8]: records, malformed records, edges that reach a pixel of the tile, (edge, row) intervals
            applied (the capsule of an edge is convex: one interval per row), those of them whose edge also reaches the centre
            of column -1, those whose edge also reaches the centre of column W, pixels with acc != 0, 0

`reach_tiles` tests all edges against the pixels of their bounding boxes grown by R (and by one column either side, for the
two cut counts): in int64 where every intermediate provably fits, in Python ints (object arrays) otherwise.  It calls neither
dswx_reach_host nor the device, and has no interval, square root or floating point in it: the tests pin the three to each
other, to a per-pixel loop in Python ints and to a floating-point distance.  GEOS is not available to this project, so the
chords by which OGR's Buffer replaces the circle at a convex vertex (inside it by at most 3.4e-4 R) are UNPINNED.
"""
import numpy as np

from . import burn as _burn
from .burn import MAX_COORD, VERTEX_DTYPE

HEAD_WORDS = 8
MAX_RADIUS = 1 << 20
OUTPUTS = ('acc', 'mask', 'head')


class Spec(_burn.Spec):
    """dswx_reach_spec_t: the fields of burn.Spec, then `radius` in 1/256 pixel, 0 .. MAX_RADIUS."""

    def __init__(self, radius, burn=1, background=0, mask_tile_stride=0, src_tile_stride=0):
        super().__init__(burn, background, mask_tile_stride, src_tile_stride)
        self.radius, self.reserved = int(radius), 0
        if not 0 <= self.radius <= MAX_RADIUS:
            raise ValueError(f'radius {self.radius} outside 0 .. {MAX_RADIUS} (1/256 pixel)')


def reached(px, py, ax, ay, bx, by, R):
    """THE PREDICATE on arrays (int64, or object arrays of Python ints) or scalars that broadcast."""
    dx, dy, ux, uy = bx - ax, by - ay, px - ax, py - ay
    D, t = dx * dx + dy * dy, ux * dx + uy * dy
    vx, vy, cross = ux - dx, uy - dy, ux * dy - uy * dx
    return np.where((D == 0) | (t <= 0), ux * ux + uy * uy <= R * R, np.where(t >= D, vx * vx + vy * vy <= R * R, cross * cross <= R * R * D))


def edge_pixels(ax, ay, bx, by, R, height, width):
    """bool [rows, cols + 2] of one well-formed edge over its bounding box grown by R and clipped to the rows 0 .. height - 1
    and the columns -1 .. width, with the first row and (r0, c0) -- None when the box misses them."""
    r0, r1 = max(-((128 - (min(ay, by) - R)) // 256), 0), min((max(ay, by) + R - 128) // 256, height - 1)
    c0, c1 = max(-((128 - (min(ax, bx) - R)) // 256), -1), min((max(ax, bx) + R - 128) // 256, width)
    if r0 > r1 or c0 > c1:
        return None
    # the largest intermediates: (u x d)^2 and R^2 D
    u = max(abs(256 * c + 128 - ax) for c in (c0, c1)) + max(abs(256 * r + 128 - ay) for r in (r0, r1))
    d = abs(bx - ax) + abs(by - ay)
    small = (u + d) ** 2 * max(d, 1) ** 2 < 1 << 62 and R * R * max(d * d, 1) < 1 << 62
    kind = np.int64 if small else object
    py = (256 * np.arange(r0, r1 + 1, dtype=np.int64) + 128).astype(kind)[:, None]
    px = (256 * np.arange(c0, c1 + 1, dtype=np.int64) + 128).astype(kind)[None, :]
    if small:
        hit = reached(px, py, np.int64(ax), np.int64(ay), np.int64(bx), np.int64(by), np.int64(R))
    else:
        hit = reached(px, py, ax, ay, bx, by, R).astype(bool)
    return hit, r0, c0


def reach_tile(verts, radius, height, width):
    """(acc uint32 [H, W], head words 0 .. 5) of the records of ONE tile."""
    verts = np.asarray(verts, dtype=VERTEX_DTYPE)
    count, R = len(verts), int(radius)
    acc = np.zeros((height, width), dtype=np.uint32)
    head = [count, 0, 0, 0, 0, 0]
    for v in verts:
        if int(v['next']) >= count:
            head[1] += 1
            continue
        w = verts[int(v['next'])]
        ax, ay, bx, by = int(v['x']), int(v['y']), int(w['x']), int(w['y'])
        if max(abs(ax), abs(ay), abs(bx), abs(by)) > MAX_COORD:
            head[1] += 1
            continue
        got = edge_pixels(ax, ay, bx, by, R, height, width)
        if got is None:
            continue
        hit, r0, c0 = got
        # columns c0 .. of the box: those inside the raster, and the two beside it
        lo, hi = max(0, -c0), min(hit.shape[1], width - c0)
        inside = hit[:, lo:hi]
        rows = inside.any(axis=1)
        if not rows.any():
            continue
        acc[r0:r0 + hit.shape[0], c0 + lo:c0 + hi] += inside.astype(np.uint32)
        head[2] += 1
        head[3] += int(rows.sum())
        if c0 == -1:
            head[4] += int((rows & hit[:, 0]).sum())
        if c0 + hit.shape[1] - 1 == width:
            head[5] += int((rows & hit[:, -1]).sum())
    return acc, head


def reach_tiles(verts, tile_first, height, width, spec, src=None):
    """{'acc': uint32 [n, H, W], 'mask': uint8 [n, H, W], 'head': uint64 [n, 8]} of the records `verts` (VERTEX_DTYPE) shared
    out by `tile_first` (int64 [n + 1]); `src` uint8 [n, H, W], or [n, stride] with stride >= H * W, or None."""
    verts = np.asarray(verts, dtype=VERTEX_DTYPE)
    tile_first = np.asarray(tile_first, dtype=np.int64)
    n = len(tile_first) - 1
    if height * width > 1 << 30:
        raise ValueError(f'{height} x {width} pixels: at most 2^30')
    acc = np.zeros((n, height, width), dtype=np.uint32)
    head = np.zeros((n, HEAD_WORDS), dtype=np.uint64)
    for t in range(n):
        first, behind = int(tile_first[t]), int(tile_first[t + 1])
        mine = verts[first:behind] if first >= 0 and behind > first else verts[:0]
        acc[t], head[t, :6] = reach_tile(mine, spec.radius, height, width)
    head[:, 6] = (acc != 0).sum(axis=(1, 2))
    if src is None:
        other = np.full((n, height, width), spec.background, dtype=np.uint8)
    else:
        other = np.asarray(src, dtype=np.uint8)
        other = other.reshape(n, other.size // max(n, 1))[:, :height * width].reshape(n, height, width)
    return {'acc': acc, 'mask': np.where(acc != 0, np.uint8(spec.burn), other), 'head': head}
