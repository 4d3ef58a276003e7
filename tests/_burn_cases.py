"""What the burn tests share (tests/test_burn.py on the host, tests/test_gpu_burn.py on the device): a third, brute-force
statement of the definition in include/dswx_hip.h ("burn"), random polygons, the named corner cases, the round trip through the
outline, and the shapes built around the seams of the kernels.  Every case is a dict {'name', 'H', 'W', 'verts', 'first'}: the
records of all its tiles and the table that shares them out."""
import numpy as np

from proteus_amd import _capi
from proteus_amd import burn as BN
from proteus_amd.burn import MAX_COORD, VERTEX_DTYPE, Spec, records, tiles
from tests import _outline_cases as OC

PX = 256
SHAPES = ((12, 12), (5, 9), (1, 12), (12, 1))             # of the random tiles: up to 12 x 12
CORNER_SHAPE = (9, 11)


def case(name, H, W, per_tile):
    verts, first = tiles(per_tile)
    return {'name': name, 'H': H, 'W': W, 'verts': verts, 'first': first}


def brute(verts, H, W):
    """acc uint32 [H, W] of the records of ONE tile, per pixel and per edge by the crossing predicate in Python ints:
    y0 <= yc < y1 and (x1 - x0) * (yc - y0) <= (xc - x0) * (y1 - y0)."""
    n = len(verts)
    edges = []
    for v in verts:
        if int(v['next']) >= n:
            continue
        w = verts[int(v['next'])]
        x0, y0, x1, y1 = int(v['x']), int(v['y']), int(w['x']), int(w['y'])
        if max(abs(x0), abs(y0), abs(x1), abs(y1)) > MAX_COORD or y0 == y1:
            continue
        if y0 > y1:
            x0, y0, x1, y1 = x1, y1, x0, y0
        edges.append((x0, y0, x1, y1, int(v['word'])))
    acc = np.zeros((H, W), dtype=np.uint32)
    for r in range(H):
        yc = PX * r + 128
        for c in range(W):
            xc, a = PX * c + 128, 0
            for x0, y0, x1, y1, word in edges:
                if y0 <= yc < y1 and (x1 - x0) * (yc - y0) <= (xc - x0) * (y1 - y0):
                    a ^= word
            acc[r, c] = a
    return acc


def random_tile(rng, ties, odd=False):
    """The records of one tile: 1 .. 3 polygons of 3 .. 6 vertices between -3 and +14 pixels, so that tiles of up to 12 x 12
    are left on all four sides; `ties`: every coordinate a multiple of 128 (centres lie ON vertices and edges); `odd`: every
    coordinate odd (no centre lies on an edge)."""
    rings, words = [], []
    for _ in range(int(rng.integers(1, 4))):
        k = int(rng.integers(3, 7))
        if ties:
            p = 128 * rng.integers(-6, 29, size=(k, 2))
        else:
            p = rng.integers(-3 * PX, 14 * PX + 1, size=(k, 2))
            if odd:
                p |= 1
        rings.append(p)
        words.append(int(rng.integers(1, 1 << 32)))
    return records(rings, words)


def random_cases(seed=20261020, per_shape=16):
    rng = np.random.default_rng(seed)
    return [case(f'random_{H}x{W}', H, W, [random_tile(rng, ties=bool(i % 2)) for i in range(per_shape)]) for H, W in SHAPES]


def ring(points_px, word=1):
    """One ring from pixel coordinates (floats allowed)."""
    return records([BN.quantise(points_px)], [word])


def raw(rows):
    """Records from (x, y, word, next) rows as they are."""
    out = np.zeros(len(rows), dtype=VERTEX_DTYPE)
    for i, (x, y, w, n) in enumerate(rows):
        out[i] = (x, y, w, n)
    return out


def corner_cases():
    """The named cases, one tile each, all of CORNER_SHAPE -- with empty tiles between full ones in the table."""
    H, W = CORNER_SHAPE
    M = MAX_COORD
    sq = [(2, 2), (6, 2), (6, 5), (2, 5)]
    named = [
        # an edge that ENDS exactly on a row centre, and one that begins on one: half-open both ways
        ('ends_on_centre', ring([(1, 1.5), (5, 1.5), (5, 4.5), (1, 4.5)], 3)),
        ('vertex_on_centre', ring([(3.5, 0.5), (7.5, 4.5), (3.5, 8.5), (0.5, 4.5)], 5)),
        ('left_of_tile', ring([(-9, 1), (-2, 1), (-2, 7), (-9, 7)], 7)),
        ('right_of_tile', ring([(W + 1, 1), (W + 5, 1), (W + 5, 7), (W + 1, 7)], 7)),
        ('above_tile', ring([(1, -9), (5, -9), (5, -1), (1, -1)], 7)),
        ('below_tile', ring([(1, H + 1), (5, H + 1), (5, H + 4), (1, H + 4)], 7)),
        ('covers_tile', ring([(-4, -4), (W + 4, -4), (W + 4, H + 4), (-4, H + 4)], 0x80000001)),
        ('exactly_tile', ring([(0, 0), (W, 0), (W, H), (0, H)], 9)),
        ('zero_area', ring([(1, 1), (8, 7)], 11)),
        ('empty_a', raw([])),
        ('next_is_self', raw([(300, 300, 5, 0), (900, 2000, 5, 1)])),
        # (the `next` of the raw records are written out relative to the tile: the ring takes 0 .. 3)
        ('next_out_of_range', np.concatenate([ring(sq, 13), raw([(10, 10, 1, 5), (10, 900, 1, 0xFFFFFFFF), (700, 10, 1, 6)])])),
        ('illegal_coordinate', np.concatenate([ring(sq, 13), raw([(M + 1, 0, 1, 5), (-M - 1, 2000, 1, 6), (100, M + 1, 1, 4),
                                                                    (200, -(1 << 31), 1, 1)])])),
        ('empty_b', raw([])),
        ('extreme_square', raw([(-M, -M, 17, 1), (M, -M, 17, 2), (M, M, 17, 3), (-M, M, 17, 0)])),
        ('extreme_skew', raw([(-M, -M, 19, 1), (M, M - 1, 19, 2), (-M + 7, M, 19, 0)])),
        ('extreme_sliver', raw([(-M, 127, 21, 1), (M, 129, 21, 2), (M, 128 + 8 * PX, 21, 3), (-M, 130 + 8 * PX, 21, 0)])),
        ('cancel_one_word', concat_rings(ring(sq, 6), ring([(4, 3), (9, 3), (9, 8), (4, 8)], 6))),
        ('union_two_bits', concat_rings(ring(sq, 1), ring([(4, 3), (9, 3), (9, 8), (4, 8)], 2))),
        ('zero_word', ring(sq, 0)),
    ]
    return [n for n, _ in named], case('corners', H, W, [v for _, v in named])


def concat_rings(*parts):
    """Records of several `records` results as ONE tile: the `next` of every part moved behind the parts before it."""
    out, at = [], 0
    for p in parts:
        p = p.copy()
        p['next'] = p['next'] + np.uint32(at)
        out.append(p)
        at += len(p)
    return np.concatenate(out)


def outline_records(ids, connectivity):
    """(verts, first, vertical boundary edges per tile, those of them on the right border) of an id plane uint32 [n, H, W]:
    dswx_outline_host, then every ring of every tile with its id as word."""
    n, H, W = ids.shape
    got = OC.host(ids, OC.full_spec(ids, connectivity))
    per_tile, vertical, border = [], [], []
    for t in range(n):
        E = int(got['head'][t, 0])
        keys = got['chain'][t, :E].astype(np.int64)
        vertical.append(int(((keys & 1) == 1).sum()))
        border.append(int((((keys & 3) == 1) & ((keys >> 2) % W == W - 1)).sum()))
        per_tile.append(BN.records_of_outline(got['chain'][t], got['rings'][t], W))
    verts, first = tiles(per_tile)
    return verts, first, np.array(vertical), np.array(border)


def carry_case(W, H=3, seed=5):
    """Toggles in the first and the last columns of every step of the scan, each with a word of its own, on every row (the
    rows of widths that are no multiple of 4 begin at other offsets in their 16-byte slots): a lost carry shows."""
    rng = np.random.default_rng(seed + W)
    cols = sorted({c for c in range(W) if c % _capi.BURN_SCAN_STEP in (0, 1, 2, 3, 4, 251, 252, 253, 254, 255)} | {W - 1} |
                  set(rng.integers(0, W, size=8).tolist()))
    rows = []
    for i, c in enumerate(cols):                             # a vertical edge through the centres of column c, then a stub
        rows.append((PX * c + 128, -40, int(rng.integers(1, 1 << 32)), 2 * i + 1))
        rows.append((PX * c + 128 - int(rng.integers(0, 100)), PX * H + 40, 0, 2 * i + 1))
    return case(f'carry_{W}', H, W, [raw(rows), raw(rows[:8])])


def fan_case(H=700, W=37):
    """A tall tile: two edges from (-3.3, -5) to (W + 2, H + 7) and back, and a fan of edges whose row counts sit at, one below
    and one above the rows a thread finishes alone, and at 64 times that: the wave-shared path, its first and its last step."""
    L = _capi.BURN_THREAD_ROWS
    rows = [(int(-3.3 * PX), -5 * PX, 0x10001, 1), ((W + 2) * PX, (H + 7) * PX, 0x20002, 0)]
    for k, n in enumerate((1, L - 1, L, L + 1, 63, 64, 65, 64 * L - 1, 64 * L, 64 * L + 1, H - 1, H, 2 * H)):
        y0 = 128 + PX * (k % 5) - (k % 3)                    # (begins on, or just above, a row centre)
        x0 = PX * (k * 3 % W) + 17 * k
        i = len(rows)
        rows.append((x0, y0, 1 << (k % 32), i + 1))
        rows.append((x0 + (k - 6) * 997, y0 + PX * n - 1 + (k % 2), 0x400 << (k % 20), i))    # and back: another word
    return case('fan', H, W, [raw(rows), raw(rows[:2]), raw([])])


def tiny_tiles_case(n_tiles=65535 + 4, H=4, W=5, seed=77):
    """More tiles than a launch has rows of workgroups: one or two rings each, some tiles empty."""
    rng = np.random.default_rng(seed)
    kinds = [records([rng.integers(-PX, 6 * PX, size=(int(rng.integers(3, 6)), 2)) for _ in range(1 + j % 2)],
                     [int(rng.integers(1, 1 << 32)) for _ in range(1 + j % 2)]) for j in range(37)]
    pick = rng.integers(0, len(kinds) + 6, size=n_tiles)     # (>= len(kinds): an empty tile)
    pick[-1] = 3                                             # the last tile has rings
    lens = np.array([len(k) for k in kinds] + [0] * 6)
    first = np.zeros(n_tiles + 1, dtype=np.int64)
    first[1:] = np.cumsum(lens[pick])
    verts = np.concatenate([kinds[p] if p < len(kinds) else kinds[0][:0] for p in pick])
    return {'name': 'tiny_tiles', 'H': H, 'W': W, 'verts': verts, 'first': first}


def host(c, spec=None, **kw):
    return _capi.burn_host(c['verts'], c['first'], c['H'], c['W'], spec or Spec(), **kw)


def numpy_statement(c, spec=None, src=None):
    return BN.burn_tiles(c['verts'], c['first'], c['H'], c['W'], spec or Spec(), src)
