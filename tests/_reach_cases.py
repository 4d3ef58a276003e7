"""What the reach tests share (tests/test_reach.py on the host, tests/test_gpu_reach.py on the device): a third statement of the
definition in include/dswx_hip.h ("reach") as a per-pixel loop in Python ints, a fourth in floating point, and the named cases.
Every case is a dict {'name', 'H', 'W', 'R', 'verts', 'first'}: the records of all its tiles, the table that shares them out and
the radius in 1/256 pixel.  No tile has more than the 9216 pixels of 96 x 96 (the tall one is 300 x 30)."""
import numpy as np

from proteus_amd import _capi
from proteus_amd import reach as RC
from proteus_amd.burn import MAX_COORD, VERTEX_DTYPE, tiles
from proteus_amd.reach import MAX_RADIUS, Spec

PX = 256
M = MAX_COORD
BAND = 0.05 * PX                                  # the float statement abstains within this of the radius
SHARE = 0.01                                      # and may abstain on at most this share of a case's pixels


def case(name, H, W, R, per_tile, first=None):
    verts, table = tiles(per_tile)
    return {'name': name, 'H': H, 'W': W, 'R': int(R), 'verts': verts, 'first': table if first is None else np.asarray(first, dtype=np.int64)}


def raw(rows):
    """Records from (x, y, word, next) rows as they are."""
    out = np.zeros(len(rows), dtype=VERTEX_DTYPE)
    for i, (x, y, w, n) in enumerate(rows):
        out[i] = (x, y, w, n)
    return out


def segments(segs, word=7):
    """Every segment (ax, ay, bx, by) as TWO records, A -> B and B -> A: each direction is an edge of its own."""
    rows = []
    for ax, ay, bx, by in segs:
        i = len(rows)
        rows += [(int(ax), int(ay), word, i + 1), (int(bx), int(by), word ^ 0xFFFF, i)]
    return raw(rows)


def points(pts):
    """Every point as one record whose `next` is itself: an edge whose endpoints coincide."""
    return raw([(int(x), int(y), 0, i) for i, (x, y) in enumerate(pts)])


def edges_of(verts):
    """The well-formed edges (ax, ay, bx, by) of the records of ONE tile, and the count of the malformed ones."""
    n, out, bad = len(verts), [], 0
    for v in verts:
        if int(v['next']) >= n:
            bad += 1
            continue
        w = verts[int(v['next'])]
        e = (int(v['x']), int(v['y']), int(w['x']), int(w['y']))
        if max(abs(k) for k in e) > M:
            bad += 1
            continue
        out.append(e)
    return out, bad


def reached(px, py, e, R):
    """THE PREDICATE in Python ints."""
    ax, ay, bx, by = e
    dx, dy, ux, uy = bx - ax, by - ay, px - ax, py - ay
    D, t = dx * dx + dy * dy, ux * dx + uy * dy
    if D == 0 or t <= 0:
        return ux * ux + uy * uy <= R * R
    if t >= D:
        return (px - bx) ** 2 + (py - by) ** 2 <= R * R
    return (ux * dy - uy * dx) ** 2 <= R * R * D


def brute(verts, R, H, W):
    """(acc uint32 [H, W], head words 0 .. 6) of the records of ONE tile: every pixel against every edge, and the columns -1 and
    W for the two cut counts."""
    edges, bad = edges_of(verts)
    acc = np.zeros((H, W), dtype=np.uint32)
    head = [len(verts), bad, 0, 0, 0, 0, 0]
    for e in edges:
        # (the rows and columns that the edge can reach at all: a bounding box, one pixel wider than needed)
        r0, r1 = max((min(e[1], e[3]) - R) // PX - 1, 0), min((max(e[1], e[3]) + R) // PX + 1, H - 1)
        c0, c1 = max((min(e[0], e[2]) - R) // PX - 1, 0), min((max(e[0], e[2]) + R) // PX + 1, W - 1)
        any_row = False
        for r in range(r0, r1 + 1):
            py = PX * r + 128
            hit = [c for c in range(c0, c1 + 1) if reached(PX * c + 128, py, e, R)]
            if not hit:
                continue
            assert hit == list(range(hit[0], hit[-1] + 1)), 'the reached pixels of a row are one interval'
            acc[r, hit[0]:hit[-1] + 1] += 1
            any_row = True
            head[3] += 1
            head[4] += reached(-128, py, e, R)
            head[5] += reached(PX * W + 128, py, e, R)
        head[2] += any_row
    head[6] = int((acc != 0).sum())
    return acc, head


def float_distance(verts, H, W):
    """float64 [H, W]: the distance in 1/256 pixel from every centre to the nearest well-formed edge of ONE tile (inf without
    one), in floating point with the projection clamped to the segment -- no integer, no case split on t."""
    edges, _ = edges_of(verts)
    ys, xs = np.mgrid[0:H, 0:W]
    px, py = PX * xs + 128.0, PX * ys + 128.0
    best = np.full((H, W), np.inf)
    for ax, ay, bx, by in edges:
        dx, dy = float(bx - ax), float(by - ay)
        D = dx * dx + dy * dy
        s = np.clip(((px - ax) * dx + (py - ay) * dy) / D, 0.0, 1.0) if D else 0.0
        best = np.minimum(best, np.hypot(px - (ax + s * dx), py - (ay + s * dy)))
    return best


def tile_records(c, t):
    first, behind = int(c['first'][t]), int(c['first'][t + 1])
    return c['verts'][first:behind] if first >= 0 and behind > first else c['verts'][:0]


def coast(n=40, H=96, W=96, seed=12):
    """A wiggly open coastline of n vertices across a tile, as segments."""
    rng = np.random.default_rng(seed)
    x = np.linspace(-20.0, W + 20.0, n) + rng.uniform(-1.0, 1.0, n)
    y = H * 0.55 + 0.3 * H * np.sin(np.linspace(0, 5.0, n)) + rng.uniform(-2.0, 2.0, n)
    q = np.rint(PX * np.stack([x, y], axis=1)).astype(np.int64) | 1
    return segments([(q[i, 0], q[i, 1], q[i + 1, 0], q[i + 1, 1]) for i in range(n - 1)])


def width_cases():
    """Widths either side of the lanes' 4-pixel slots and of a wave's 256-pixel step, and height 1: an edge that crosses the
    whole width, a point in the last column, one beside the tile on either side.  Odd coordinates: no centre lies within BAND
    of a boundary."""
    out = []
    for H, W in ((3, 1), (3, 15), (3, 16), (3, 17), (3, 63), (3, 64), (3, 65), (3, 257), (1, 1), (1, 65), (1, 257)):
        R = 333
        a = segments([(-3 * PX + 1, 131, (W + 3) * PX + 1, 141)])
        b = points([(PX * W - 121, 95), (-41, 133), (PX * W + 77, PX * H - 101)])
        c = segments([(PX * (W // 2) + 77, -5 * PX + 1, PX * (W // 2) + 55, 9 * PX + 1)])
        out.append(case(f'width_{H}x{W}', H, W, R, [a, b, c, raw([])]))
    return out


def named_cases():
    H = W = 96
    c = PX * 40 + 128                                        # the centre of pixel (40, 40)
    out = [
        # a point whose circle passes exactly through centres: offsets (3, 4), (5, 0) at R = 5 pixels: <= decides
        case('point_circle', H, W, 5 * PX, [points([(c, c)]), points([(128, 128), (PX * 95 + 128, PX * 95 + 128)])]),
        case('directions', 24, 24, 589, [segments([s]) for s in (
            (3 * PX + 1, 12 * PX + 3, 20 * PX + 1, 12 * PX + 3), (12 * PX + 3, 3 * PX + 1, 12 * PX + 3, 20 * PX + 1),
            (4 * PX + 1, 4 * PX + 1, 19 * PX + 3, 19 * PX + 3), (4 * PX + 1, 19 * PX + 3, 19 * PX + 3, 4 * PX + 1),
            (2 * PX + 1, 9 * PX + 1, 21 * PX + 1, 13 * PX + 5), (2 * PX + 1, 13 * PX + 5, 21 * PX + 1, 9 * PX + 1),
            (9 * PX + 1, 2 * PX + 1, 13 * PX + 5, 21 * PX + 1), (13 * PX + 5, 2 * PX + 1, 9 * PX + 1, 21 * PX + 1))]),
        # edges wholly outside the tile that reach in across each side and each corner, and some that do not
        case('outside', 16, 16, 3 * PX + 17, [segments([s]) for s in (
            (-2 * PX + 1, 3 * PX + 1, -2 * PX + 5, 12 * PX + 1), (18 * PX + 1, 3 * PX + 1, 18 * PX + 5, 12 * PX + 1),
            (3 * PX + 1, -2 * PX + 1, 12 * PX + 1, -2 * PX + 5), (3 * PX + 1, 18 * PX + 1, 12 * PX + 1, 18 * PX + 5),
            (-9 * PX + 1, -PX + 1, -PX + 1, -PX - 3), (17 * PX + 1, -PX + 1, 25 * PX + 1, -7 * PX + 1),
            (-PX + 1, 17 * PX + 1, -7 * PX + 1, 25 * PX + 1), (17 * PX + 1, 17 * PX + 1, 30 * PX + 1, 17 * PX + 1),
            (-5 * PX + 1, 3 * PX + 1, -5 * PX + 1, 12 * PX + 1), (-4 * PX + 1, -4 * PX + 1, -9 * PX + 1, -9 * PX + 1))]),
        # R = 0: only the centres exactly ON an edge; slope 1/2 through centres, a row of centres, a point on a centre
        case('radius_zero', H, W, 0, [segments([(2 * PX + 128, 2 * PX + 128, 42 * PX + 128, 22 * PX + 128)]),
                                      segments([(10 * PX + 128, 50 * PX + 128, 40 * PX + 128, 50 * PX + 128)]),
                                      np.concatenate([points([(c, c), (c + 1, c)])]),
                                      segments([(30 * PX + 128, 5 * PX + 128, 30 * PX + 128, 60 * PX + 128)])]),
        # R = 2^20 (4096 pixels) with endpoints at +-2^30: u x d passes 2^63 and R^2 D reaches 2^103
        case('extreme', H, W, MAX_RADIUS, [
            segments([(-M, -MAX_RADIUS + 10 * PX + 3, M, -MAX_RADIUS + 70 * PX - 5)]),
            segments([(W * PX + MAX_RADIUS - 30 * PX + 1, -M, W * PX + MAX_RADIUS - 60 * PX + 7, M)]),
            segments([(-M, -M, -MAX_RADIUS // 2 + 1, -MAX_RADIUS // 2 - 250 * PX + 3)]),
            points([(-MAX_RADIUS + 33 * PX + 1, 40 * PX + 1), (M, M), (-M, M)]),
            segments([(-M, M, M, -M + 8 * MAX_RADIUS // 3 + 1)]),
            segments([(-M, -M, M, M)])]),
        # an edge of more rows than the four waves of a workgroup have lanes, on a tall narrow tile; short ones beside it
        case('long', 300, 30, 333, [np.concatenate([segments([(-PX + 1, -3 * PX + 1, 31 * PX + 1, 303 * PX + 1)]),
                                                    points([(3 * PX + 1, 150 * PX + 1)])]),
                                    segments([(13 * PX + 1, 1, 13 * PX + 5, 299 * PX + 1)])]),
        # thousands of edges over one pixel
        case('pile', 7, 7, 100, [segments([(3 * PX + 128 + (i % 41) - 20, 3 * PX + 128 + (i % 37) - 18,
                                            3 * PX + 128 - (i % 29) + 14, 3 * PX + 128 + (i % 31) - 15) for i in range(1500)]),
                                 points([(3 * PX + 128, 3 * PX + 128)] * 3000)]),
        # malformed records of every kind beside a good edge; a point written as `next` = itself is NOT malformed
        case('malformed', 16, 16, 2 * PX + 1, [
            np.concatenate([segments([(3 * PX + 1, 3 * PX + 1, 12 * PX + 1, 9 * PX + 1)]),
                            raw([(10, 10, 1, 9), (10, 900, 1, 0xFFFFFFFF), (M + 1, 0, 1, 0), (0, -M - 1, 1, 0), (5 * PX, 5 * PX, 1, 7),
                                 (100, M + 1, 1, 0), (-(1 << 31), 7, 1, 1), (9 * PX + 1, 13 * PX + 1, 1, 9), (20, 20, 1, 4), (10, 10, 1, 12)])]),
            raw([]), raw([(5 * PX + 1, 5 * PX + 1, 0, 1)])]),
        case('coast', H, W, 8525, [coast(), coast(seed=13)[:30]]),
    ]
    # a table that decreases, or begins below zero: the affected tiles have no records
    sq = segments([(2 * PX + 1, 2 * PX + 1, 6 * PX + 1, 5 * PX + 1), (6 * PX + 1, 5 * PX + 1, 2 * PX + 1, 5 * PX + 1)])
    out.append(case('decreasing', 9, 11, 300, [sq, sq, sq], first=[0, 8, 4, 8, 8, 12, -4, 4, 4]))
    return out + width_cases()


def tiny_tiles_case(n_tiles=65535 + 4, H=8, W=8, seed=78):
    """More tiles than a launch has rows of workgroups: a few segments or points each, some tiles empty."""
    rng = np.random.default_rng(seed)
    kinds = [segments([tuple(rng.integers(-3 * PX, 11 * PX, size=4) | 1) for _ in range(1 + j % 3)]) if j % 4 else
             points([tuple(rng.integers(-PX, 9 * PX, size=2) | 1)]) for j in range(37)]
    pick = rng.integers(0, len(kinds) + 6, size=n_tiles)     # (>= len(kinds): an empty tile)
    pick[-1] = 3                                             # the last tile has records
    lens = np.array([len(k) for k in kinds] + [0] * 6)
    first = np.zeros(n_tiles + 1, dtype=np.int64)
    first[1:] = np.cumsum(lens[pick])
    verts = np.concatenate([kinds[p] if p < len(kinds) else kinds[0][:0] for p in pick])
    return {'name': 'tiny_tiles', 'H': H, 'W': W, 'R': 411, 'verts': verts, 'first': first}


def spec_of(c, **kw):
    return Spec(c['R'], **kw)


def host(c, spec=None, **kw):
    return _capi.reach_host(c['verts'], c['first'], c['H'], c['W'], spec or spec_of(c), **kw)


def numpy_statement(c, spec=None, src=None):
    return RC.reach_tiles(c['verts'], c['first'], c['H'], c['W'], spec or spec_of(c), src)
