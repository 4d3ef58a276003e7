"""Polygon rings burnt onto planes, include/dswx_hip.h ("burn"), stated in numpy.

Coordinates are int32 in units of 1/256 pixel, x right and y down; pixel (c, r) has its centre at (256 c + 128, 256 r + 128)
and a coordinate v is legal iff |v| <= 2^30.  `verts` is VERTEX_DTYPE [k] -- x, y, word, next -- and `tile_first` int64
[n_tiles + 1]: tile t owns the records tile_first[t] .. tile_first[t + 1] - 1 (none when that range is empty, decreasing or
begins below 0).  Record i of a tile is the directed edge from its (x, y) to the (x, y) of record `next` of the same tile; a
record whose `next` is not below the tile's count, or one of whose two endpoints has an illegal coordinate, is malformed: it
contributes nothing and is counted.  Oriented so that y0 < y1 (an edge with y0 == y1 contributes nothing), an edge crosses row
r iff y0 <= 256 r + 128 < y1 and 0 <= r < height, and there, with yc = 256 r + 128,

    col = max(0, ceil(((x1 - x0) * (yc - y0) + (x0 - 128) * (y1 - y0)) / (256 * (y1 - y0))))

is the first pixel of the row whose centre is at or to the right of the crossing.  With col < width the crossing toggles
acc[r][col] ^= word, else it is dropped; then acc[r][c] becomes the XOR of the toggles of row r at columns <= c.

    acc     uint32 [n_tiles, H, W]: for one ring with word w, w exactly where the centre is inside by the even-odd rule
    mask    uint8 [n_tiles, H, W]: spec.burn where acc != 0, else src (when given) or spec.background
    head    uint64 [n_tiles, 8]: records, malformed records, edges that cross a row of the tile, toggles applied, crossings
            dropped at col >= width, crossings whose column was negative before the clamp, pixels with acc != 0, 0

`burn_tiles` makes the toggles of all edges with int64 arithmetic (every intermediate stays below 2^63 for legal
coordinates), applies them with np.bitwise_xor.at and runs np.bitwise_xor.accumulate along the rows.  It calls neither
dswx_burn_host nor the device: the tests pin the three to each other, to a per-pixel crossing predicate in Python ints and to
matplotlib.path.  GDAL is not available to this project, so how GDAL treats a centre exactly on an edge is UNPINNED; the
definition agrees with its documented default (burnt when the centre is inside) wherever no centre lies on an edge.
"""
import numpy as np

HEAD_WORDS = 8
MAX_COORD = 1 << 30
OUTPUTS = ('acc', 'mask', 'head')
VERTEX_DTYPE = np.dtype([('x', '<i4'), ('y', '<i4'), ('word', '<u4'), ('next', '<u4')])
assert VERTEX_DTYPE.itemsize == 16


class Spec:
    """dswx_burn_spec_t: `burn` 0 .. 255 the byte of a pixel with acc != 0 in `mask`, `background` 0 .. 255 the byte of every
    other pixel when there is no `src`, and the elements between the tiles of `mask` and of `src` (0 = height * width)."""

    def __init__(self, burn=1, background=0, mask_tile_stride=0, src_tile_stride=0):
        self.burn, self.background = int(burn), int(background)
        self.mask_tile_stride, self.src_tile_stride = int(mask_tile_stride), int(src_tile_stride)
        if not 0 <= self.burn <= 255 or not 0 <= self.background <= 255:
            raise ValueError(f'burn {self.burn} and background {self.background} are bytes, 0 .. 255')
        if self.mask_tile_stride < 0 or self.src_tile_stride < 0:
            raise ValueError('negative tile stride')


def quantise(xy):
    """Pixel coordinates (floats, any shape; a pixel is one unit and (0, 0) the top left corner of the raster) -> int32 in
    units of 1/256 pixel, rounded to nearest; raises outside +-2^30."""
    q = np.rint(256.0 * np.asarray(xy, dtype=np.float64))
    if q.size and not (np.abs(q) <= MAX_COORD).all():          # (a NaN fails too)
        raise ValueError(f'coordinates outside +-{MAX_COORD // 256} pixels')
    return q.astype(np.int32)


def records(polygons, words=None):
    """The rings of ONE tile -- each an integer [k, 2] array of (x, y) in 1/256 pixel, without a repeated closing point -- as
    VERTEX_DTYPE records with a cyclic `next` per ring; ring j toggles words[j] (default 1)."""
    polygons = [np.asarray(p) for p in polygons]
    words = [1] * len(polygons) if words is None else list(words)
    if len(words) != len(polygons):
        raise ValueError(f'{len(words)} words for {len(polygons)} rings')
    out = np.zeros(sum(len(p) for p in polygons), dtype=VERTEX_DTYPE)
    at = 0
    for p, w in zip(polygons, words):
        if p.ndim != 2 or p.shape[1] != 2 or not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f'a ring is an integer [k, 2] array (see quantise), not {p.dtype} {p.shape}')
        if p.size and not (np.abs(p.astype(np.int64)) <= MAX_COORD).all():
            raise ValueError(f'coordinates outside +-2^30')
        k = len(p)
        out['x'][at:at + k], out['y'][at:at + k] = p[:, 0], p[:, 1]
        out['word'][at:at + k] = np.uint32(int(w) & 0xFFFFFFFF)
        out['next'][at:at + k] = at + (np.arange(k) + 1) % max(k, 1)
        at += k
    return out


def tiles(per_tile):
    """(verts, tile_first) of a list with the records of every tile (each as `records` returns them)."""
    per_tile = [np.asarray(v, dtype=VERTEX_DTYPE) for v in per_tile]
    first = np.zeros(len(per_tile) + 1, dtype=np.int64)
    first[1:] = np.cumsum([len(v) for v in per_tile])
    return (np.concatenate(per_tile) if per_tile else np.zeros(0, dtype=VERTEX_DTYPE)), first


def records_of_outline(chain, rings, width):
    """The records of ONE tile from what the outline entries return for it -- `chain` uint32 [max_edges] and `rings`
    (outline.ROW_DTYPE [max_rings], or the uint32 [max_rings, 8] the entries write): every ring, outer or hole, with its id as
    word; its vertices are the start corners of the edges that turn (outline.ring_points), times 256.  Burning them gives the
    id plane back.  Vectorised over all rings: a tile of class noise has hundreds of thousands."""
    from .outline import CORNER, ROW_DTYPE
    rings = np.asarray(rings)
    if rings.dtype != ROW_DTYPE:
        rings = np.ascontiguousarray(rings, dtype=np.uint32).view(ROW_DTYPE)[..., 0]
    rings = rings[rings['length'] > 0]
    lens = rings['length'].astype(np.int64)
    begin = np.cumsum(lens) - lens                           # of every ring among the edges taken together
    total = int(lens.sum())
    at = np.arange(total, dtype=np.int64)
    keys = np.asarray(chain)[np.repeat(rings['offset'].astype(np.int64) - begin, lens) + at].astype(np.int64)
    d = keys & 3
    before = at - 1
    before[begin] = begin + lens - 1                         # the predecessor of a ring's first edge is its last
    turn = d != d[before]
    ring_of = np.repeat(np.arange(len(rings)), lens)[turn]
    p, corner = keys[turn] >> 2, np.array(CORNER)[d[turn]]
    out = np.zeros(int(turn.sum()), dtype=VERTEX_DTYPE)
    out['x'], out['y'] = 256 * (p % width + corner[:, 0]), 256 * (p // width + corner[:, 1])
    out['word'] = rings['id'][ring_of]
    count = np.bincount(ring_of, minlength=len(rings))       # at least 4 each
    first = np.cumsum(count) - count
    nxt = np.arange(len(out), dtype=np.int64) + 1
    nxt[first + count - 1] = first
    out['next'] = nxt
    return out


def toggles(verts, height, width):
    """The crossings of the records of ONE tile: (rows, cols, words) of the toggles applied, and head words 0 .. 5."""
    verts = np.asarray(verts, dtype=VERTEX_DTYPE)
    count = len(verts)
    nxt = verts['next'].astype(np.int64)
    inside = nxt < count
    to = np.where(inside, nxt, 0)
    ax, ay = verts['x'].astype(np.int64), verts['y'].astype(np.int64)
    bx, by = (ax[to], ay[to]) if count else (ax, ay)
    legal = inside & (np.abs(ax) <= MAX_COORD) & (np.abs(ay) <= MAX_COORD) & (np.abs(bx) <= MAX_COORD) & (np.abs(by) <= MAX_COORD)
    down = ay < by
    x0, y0, x1, y1 = np.where(down, ax, bx), np.where(down, ay, by), np.where(down, bx, ax), np.where(down, by, ay)
    r0 = np.maximum(-((128 - y0) // 256), 0)                 # ceil((y0 - 128) / 256)
    r1 = np.minimum(-((128 - y1) // 256), height)
    rows_of = np.where(legal & (y0 < y1), np.maximum(r1 - r0, 0), 0)
    edge = np.repeat(np.arange(count), rows_of)
    r = r0[edge] + (np.arange(len(edge)) - np.repeat(np.cumsum(rows_of) - rows_of, rows_of))
    yc = 256 * r + 128
    dy = (y1 - y0)[edge]
    num = (x1 - x0)[edge] * (yc - y0[edge]) + (x0[edge] - 128) * dy
    col = -((-num) // (256 * dy)) if len(edge) else num
    clamped = col < 0
    col = np.maximum(col, 0)
    applied = col < width
    head = [count, int((~legal).sum()), int((rows_of > 0).sum()), int(applied.sum()), int((~applied).sum()), int(clamped.sum())]
    return r[applied], col[applied], verts['word'][edge][applied], head


def burn_tiles(verts, tile_first, height, width, spec, src=None):
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
        r, c, w, head_t = toggles(mine, height, width)
        np.bitwise_xor.at(acc[t], (r, c), w)
        head[t, :6] = head_t
    acc = np.bitwise_xor.accumulate(acc, axis=2)
    head[:, 6] = (acc != 0).sum(axis=(1, 2))
    if src is None:
        other = np.full((n, height, width), spec.background, dtype=np.uint8)
    else:
        other = np.asarray(src, dtype=np.uint8)
        other = other.reshape(n, other.size // max(n, 1))[:, :height * width].reshape(n, height, width)
    return {'acc': acc, 'mask': np.where(acc != 0, np.uint8(spec.burn), other), 'head': head}
