"""The outline of an id plane, include/dswx_hip.h ("outline"), stated in numpy.

`ids` is uint32 [n_tiles, H, W]: 0 is background, any other value the id of the region the pixel belongs to -- typically the
`label` plane of the label entries or the `dense` plane of the body table, but any content is legal.  A boundary edge is a
pair (pixel p with ids[p] = v != 0, direction d) whose neighbour across d is outside the tile or holds another value; its key
is 4 * idx(p) + d, with d = 0 the top edge travelled left to right, 1 the right edge downward, 2 the bottom edge right to
left and 3 the left edge upward, so that the region lies on the right of the travel.  Every edge has one successor (the rule
is in `successors` below), the successor map is a bijection, and its cycles are the rings: a ring starts at its smallest key
and the rings of a tile are ordered by their start keys.

    chain   the keys of all E edges, ring after ring, each ring from its start along the successor map, then zeros   uint32
    rings   ROW_DTYPE [n_tiles, max_rings]: id, start key, offset in chain, length, corners, 0, area2 (int64); the
            rows behind min(R, max_rings) zero
    head    E, R, min(R, max_rings), edges written, rings with area2 > 0, with area2 < 0, corners, 1 if E > max_edges   uint64

A tile with E > max_edges has head words 1 .. 6, its chain and its rings zero.  The statement holds the edges of a tile as
arrays (key, successor by the rule) and finds the cycles by following them.  It calls neither dswx_outline_host nor the
device: the tests pin the three to each other, and to scipy.ndimage and matplotlib.path.
"""
import numpy as np

ROW_WORDS, HEAD_WORDS = 8, 8
OUTPUTS = ('chain', 'rings', 'head')
ROW_DTYPE = np.dtype([('id', '<u4'), ('start', '<u4'), ('offset', '<u4'), ('length', '<u4'), ('corners', '<u4'), ('zero', '<u4'),
                      ('area2', '<i8')])
assert ROW_DTYPE.itemsize == ROW_WORDS * 4
# the travel T[d] of edge d and the step O[d] across it as (dx, dy), x right and y down
T = ((1, 0), (0, 1), (-1, 0), (0, -1))
O = ((0, -1), (1, 0), (0, 1), (-1, 0))
# the corner at which edge d of pixel (0, 0) starts
CORNER = ((0, 0), (1, 0), (1, 1), (0, 1))


class Spec:
    """dswx_outline_spec_t: max_edges and max_rings 0 .. 2^31 (the capacities of chain and rings per tile), connectivity 4
    or 8 (whether two pixels of one id that touch at a corner are joined by the ring or separated)."""

    def __init__(self, max_edges, max_rings, connectivity=4):
        self.max_edges, self.max_rings, self.connectivity = int(max_edges), int(max_rings), int(connectivity)
        if self.connectivity not in (4, 8):
            raise ValueError(f'connectivity {self.connectivity} is neither 4 nor 8')
        if not 0 <= self.max_edges <= 1 << 31:
            raise ValueError(f'max_edges {self.max_edges} outside 0 .. 2^31')
        if not 0 <= self.max_rings <= 1 << 31:
            raise ValueError(f'max_rings {self.max_rings} outside 0 .. 2^31')


def _same(grid, ys, xs, v):
    """ids at (ys, xs) == v in a raster padded with one ring of background (v is never 0)."""
    return grid[ys + 1, xs + 1] == v


def successors(ids, connectivity):
    """The boundary edges of one raster uint32 [H, W] in the order of their keys, and the key of the successor of each:
    (key int64 [E], succ int64 [E])."""
    H, W = ids.shape
    grid = np.zeros((H + 2, W + 2), dtype=np.int64)
    grid[1:-1, 1:-1] = ids
    keys, succ = [], []
    for d in range(4):
        ys, xs = np.nonzero((ids != 0) & (grid[1 + O[d][1]:H + 1 + O[d][1], 1 + O[d][0]:W + 1 + O[d][0]] != ids))
        v = grid[ys + 1, xs + 1]
        ay, ax = ys + T[d][1], xs + T[d][0]                  # ahead on the region's side (never further out than the padding)
        by, bx = ay + O[d][1], ax + O[d][0]                  # ahead on the other side
        a = _same(grid, np.clip(ay, -1, H), np.clip(ax, -1, W), v)
        b = _same(grid, np.clip(by, -1, H), np.clip(bx, -1, W), v)
        right = 4 * (ys * W + xs) + (d + 1) % 4
        straight = 4 * (ay * W + ax) + d
        left = 4 * (by * W + bx) + (d + 3) % 4
        keys.append(4 * (ys * W + xs) + d)
        succ.append(np.where(~a, right, np.where(~b, straight, left)) if connectivity == 4 else
                    np.where(b, left, np.where(a, straight, right)))
    keys, succ = np.concatenate(keys), np.concatenate(succ)
    order = np.argsort(keys, kind='stable')
    return keys[order].astype(np.int64), succ[order].astype(np.int64)


def edge_area2(keys, W):
    """x1 * y2 - x2 * y1 of every edge, corner 1 its start and corner 2 its end."""
    p, d = keys >> 2, keys & 3
    x, y = p % W, p // W
    cx, cy = np.array([c[0] for c in CORNER])[d], np.array([c[1] for c in CORNER])[d]
    tx, ty = np.array([t[0] for t in T])[d], np.array([t[1] for t in T])[d]
    x1, y1 = x + cx, y + cy
    return x1 * (y1 + ty) - (x1 + tx) * y1


def outline_tiles(ids, spec):
    """{'chain': uint32 [n, max_edges], 'rings': ROW_DTYPE [n, max_rings], 'head': uint64 [n, 8]} of an id plane uint32
    [n, H, W]."""
    ids = np.asarray(ids)
    if ids.dtype != np.uint32 or ids.ndim != 3:
        raise ValueError(f'an id plane is uint32 [n_tiles, H, W], not {ids.dtype} {ids.shape}')
    n, H, W = ids.shape
    if H * W > 1 << 30:
        raise ValueError(f'{H} x {W} pixels: at most 2^30')
    chain = np.zeros((n, spec.max_edges), dtype=np.uint32)
    rings = np.zeros((n, spec.max_rings), dtype=ROW_DTYPE)
    head = np.zeros((n, HEAD_WORDS), dtype=np.uint64)
    for t in range(n):
        keys, succ = successors(ids[t], spec.connectivity)
        E = len(keys)
        head[t, 0] = E
        if E > spec.max_edges:
            head[t, 7] = 1
            continue
        nxt = np.searchsorted(keys, succ)                    # (the successor of a boundary edge is one)
        assert np.array_equal(keys[nxt], succ) if E else True
        area2 = edge_area2(keys, W)
        corner = (succ & 3) != (keys & 3)                    # as many edges turn INTO their successor as out of their predecessor
        taken = np.zeros(E, dtype=bool)
        at = R = 0
        flat = ids[t].reshape(-1)
        for s in range(E):                                   # rising keys: an edge no ring has taken starts the next ring
            if taken[s]:
                continue
            ring, e = [], s
            while not taken[e]:
                taken[e] = True
                ring.append(e)
                e = nxt[e]
            ring = np.array(ring)
            chain[t, at:at + len(ring)] = keys[ring]
            a2 = int(area2[ring].sum())
            if R < spec.max_rings:
                rings[t, R] = (flat[keys[s] >> 2], keys[s], at, len(ring), int(corner[ring].sum()), 0, a2)
            head[t, 4] += a2 > 0
            head[t, 5] += a2 < 0
            head[t, 6] += int(corner[ring].sum())
            at += len(ring)
            R += 1
        head[t, 1:4] = R, min(R, spec.max_rings), E
    return {'chain': chain, 'rings': rings, 'head': head}


def ring_points(keys, width):
    """The vertices of one ring (its keys in chain order) as int64 [k, 2] of (x, y) pixel corners with collinear points
    dropped: the start corners of the edges whose direction differs from their predecessor's, in the ring's order."""
    keys = np.asarray(keys, dtype=np.int64)
    d = keys & 3
    turn = d != np.roll(d, 1)
    p = keys[turn] >> 2
    c = np.array(CORNER)[d[turn]]
    return np.stack([p % width + c[:, 0], p // width + c[:, 1]], axis=1)


def polygons(chain, rings, width):
    """The polygons of ONE tile: yields (id, outer, [holes]) per outer ring (area2 > 0) in ring order, from the tile's `chain`
    (uint32 [max_edges]) and `rings` (ROW_DTYPE [max_rings], or the uint32 [max_rings, 8] the entries write), each ring an
    int64 [k, 2] array of (x, y) pixel corners with collinear points dropped; outer rings run clockwise on screen, holes the
    other way.  A hole belongs to the outer ring with the same id -- each body of a label plane has exactly one; of an id
    with several outer rings the first takes the holes."""
    rings = np.asarray(rings)
    if rings.dtype != ROW_DTYPE:
        rings = np.ascontiguousarray(rings, dtype=np.uint32).view(ROW_DTYPE)[..., 0]
    rings = rings[rings['length'] > 0]
    holes = {}
    for r in rings[rings['area2'] < 0]:
        holes.setdefault(int(r['id']), []).append(ring_points(chain[r['offset']:r['offset'] + r['length']], width))
    for r in rings[rings['area2'] > 0]:
        yield int(r['id']), ring_points(chain[r['offset']:r['offset'] + r['length']], width), holes.pop(int(r['id']), [])
