"""TEST INFRASTRUCTURE -- named Fmask domains for the two masked dilations of mask_adjacent_to_cloud_mode 'cover'
(_add_snow_to_cloud_layer :2055-2078), shared by oracle/gen_golden.py, tests/test_cover_domain.py and
tests/test_gpu_cover_domain.py.

    snow  = dilate^10(Fmask bit 4)            inside  area = adjacent (bit 2) & (CLOUD == 0)
    clear = dilate^7(~snow & (CLOUD == 0))    inside  area & (WTR-2 in 1..4)
    snow &= ~clear

The device code works on windows of 256 rows x 128 or 256 columns whose 17-pixel halo must be exactly the 10 + 7
steps; a window's output region starts at a multiple of 222 (rows; columns of the 8-word kernel) or 94 (columns of the
4-word kernel).  `seams(H, W, nw)` lists those positions inside a raster; every builder takes (rng, H, W, seams) and
aims its structures at them.  A builder returns a scene (a list of four for `saturated`):

    fmask   uint8 [H, W]
    water   bool [H, W]: the band override -- True = the survey's water vector (WTR-2 class 1), False = its land vector
            (WTR-2 class 0); `planes()` makes the six int16 band planes from it
    ocean, shad   optional uint8 mask planes
    meta    what the builder placed (corridor cells in order, the near / far pixels of a chain), for the assertions

Fmask bytes: 4 = area (adjacent, nothing else), 20 = area + snow seed, 2 = cloud (a wall: neither area nor a clear
seed), 0 = clear and not area, 255 = fill.
"""
import numpy as np

AREA, SEED, WALL, FILL = 4, 20, 2, 255
SNOW_REACH, CLEAR_REACH = 10, 7
HALO = SNOW_REACH + CLEAR_REACH
OUT_ROWS, OUT_COLS = 222, {8: 222, 4: 94}
WATER_PX, LAND_PX = (300, 400, 300, 200, 100, 50), (500, 600, 700, 3000, 2500, 1500)
DOMAINS = ('diamonds', 'corridors', 'chain17', 'chain17_toggled', 'bytes256', 'saturated', 'holes', 'speckle')
DIRS = ((0, 1), (0, -1), (1, 0), (-1, 0))


def seams(H, W, nw=(8,)):
    """(row seams, column seams) inside an H x W raster for the kernel variants `nw` (words per window row)."""
    nw = (nw,) if isinstance(nw, int) else tuple(nw)
    cols = sorted({c for k in nw for c in range(OUT_COLS[k], W, OUT_COLS[k])})
    return list(range(OUT_ROWS, H, OUT_ROWS)), cols


def planes(scene):
    """(six int16 band planes, fmask, {mask planes}) of a scene."""
    bands = [np.where(scene['water'], w, l).astype(np.int16) for l, w in zip(LAND_PX, WATER_PX)]
    return bands, scene['fmask'], {m: scene[m] for m in ('ocean', 'shad') if scene.get(m) is not None}


def _scene(fmask, water, meta=None, **masks):
    return dict(fmask=np.ascontiguousarray(fmask, np.uint8), water=np.ascontiguousarray(water, bool), meta=meta or [],
                **masks)


def _line(y, x, d, n):
    return [(y + d[0] * i, x + d[1] * i) for i in range(n)]


def _inside(cells, H, W):
    return [(y, x) for y, x in cells if 0 <= y < H and 0 <= x < W]


class _Placer:
    """Puts one-pixel-wide paths on a raster so that no two touch (4-neighbourhood), sliding a path sideways until it
    is free."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.used = np.zeros((H + 2, W + 2), bool)          # the cells of every path and their 8-neighbours

    def place(self, cells, slide, tries=400, need=None, ok=None):
        """The path `cells` moved by k * slide for the first k >= 0 at which it is free and the cells with indices
        `need` lie inside the raster (default: all of them; the rest is cut at the raster edge).  None if there is no
        such k."""
        for k in range(tries):
            moved = [(y + k * slide[0], x + k * slide[1]) for y, x in cells]
            must = moved if need is None else [moved[i] for i in need]
            if ok is not None and not ok(moved):
                continue
            if len(_inside(must, self.H, self.W)) != len(must):
                continue
            # cut at the first cell outside the raster: a path is connected
            kept = []
            for c in moved:
                if not (0 <= c[0] < self.H and 0 <= c[1] < self.W):
                    if kept:
                        break
                    continue
                kept.append(c)
            if need is not None and not all(moved[i] in kept for i in need):
                continue
            if any(self.used[y + 1, x + 1] for y, x in kept):
                continue
            for y, x in kept:
                self.used[y:y + 3, x:x + 3] = True
            return kept, [moved.index(c) for c in kept]
        return None


def _seed_points(H, W, seam_lists):
    """Snow seeds at every offset -11 .. +11 from each row and column seam (spread along the seam, so that the
    diamonds stay apart where the raster has room), at the four corners and at the middles of the four edges."""
    rows, cols = seam_lists
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    for s in rows:
        for i, d in enumerate(range(-11, 12)):
            pts.append((s + d, (11 + 29 * i) % W))
    for s in cols:
        for i, d in enumerate(range(-11, 12)):
            pts.append(((17 + 31 * i) % H, s + d))
    return sorted({(y, x) for y, x in pts if 0 <= y < H and 0 <= x < W})


def diamonds(rng, H, W, seam_lists):
    """Area everywhere, single snow seeds around every seam: radius-10 diamonds that cross every seam from both sides
    and stop at the raster edge.  Water in a coarse checker, so that the clear dilation eats some diamonds back."""
    fm = np.full((H, W), AREA, np.uint8)
    pts = _seed_points(H, W, seam_lists)
    for y, x in pts:
        fm[y, x] = SEED
    yy, xx = np.mgrid[0:H, 0:W]
    return _scene(fm, (yy // 37 + xx // 41) % 2 == 1, [dict(seeds=pts)])


def _seam_or_middle(seam_list, n):
    return seam_list if seam_list else [n // 2]


def corridors(rng, H, W, seam_lists):
    """One-pixel-wide area corridors between cloud walls, at least 25 pixels long where the raster has the room, straight
    and with a right-angle turn, across every seam in all four directions, a snow seed on the first cell: the front moves
    one pixel per iteration for all ten iterations, and snow ends exactly 10 cells past the seed.  Land only."""
    fm = np.full((H, W), WALL, np.uint8)
    rows, cols = seam_lists
    pl, meta = _Placer(H, W), []
    jobs = []
    for d in DIRS:
        along = 0 if d[0] else 1                                     # the axis the corridor runs along
        for s in _seam_or_middle(rows if along == 0 else cols, H if along == 0 else W):
            for before in (1, 2, 5, 9, 10, 11, 12, 16, 17):          # the seed lies this many cells before the seam
                for turn in (0, 14, 7):
                    start = s - before if d[along] > 0 else s - 1 + before
                    jobs.append((d, along, start, turn, before))
    for n, (d, along, start, turn, before) in enumerate(jobs):
        side = (7 + 13 * n) % max((W if along == 0 else H) - 1, 1)
        y, x = (start, side) if along == 0 else (side, start)
        if turn:
            t = (d[1], d[0]) if n % 2 else (-d[1], -d[0])            # the right-angle turn after `turn` cells
            cells = _line(y, x, d, turn) + _line(y + d[0] * (turn - 1) + t[0], x + d[1] * (turn - 1) + t[1], t, 27 - turn)
        else:
            cells = _line(y, x, d, 27)
        got = pl.place(cells, (0, 3) if along == 0 else (3, 0), need=(0,))
        if got is None:
            continue
        kept, _ = got
        for c in kept:
            fm[c] = AREA
        fm[kept[0]] = SEED
        meta.append(dict(cells=kept, dir=d, turn=turn, before=before))
    return _scene(fm, np.zeros((H, W), bool), meta)


CHAIN_HALOS = (17, 16, 15, 14)


def seam_for_halo(s, halo, out):
    """Where the seam `s` of the real windows (halo 17, output regions of `out` rows or columns: 222 or 94) would lie
    if the windows had `halo`: output sizes are 256 - 2 halo rows and 128 / 256 - 2 halo columns, so a kernel built
    with a smaller halo is self-consistent and wrong only across ITS seams."""
    assert out in (OUT_ROWS, OUT_COLS[8], OUT_COLS[4]) and s % out == 0, (s, out)
    return (s // out) * (out + 2 * (HALO - halo))


def _out_size(s, along):
    """The output size (222 or 94) of the windows that the seam `s` belongs to: rows (along == 0) are always 222; a
    builder gets its column seams as positions only, and below 222 * 94 / 2 no position is a seam of both widths."""
    if along == 0:
        return OUT_ROWS
    assert 0 < s < OUT_COLS[8] * OUT_COLS[4] // 2, s
    return OUT_COLS[8] if s % OUT_COLS[8] == 0 else OUT_COLS[4]


def _chain(rng, H, W, seam_lists, parity):
    """The 17-pixel dependency.  A walled corridor c0 .. c30 of area-and-water cells, a snow seed on c0: alone, snow
    reaches c10, the clear seeds c11 .. eat back to c4, c0 .. c3 stay snow.  With a second seed on c21 the whole
    corridor is snow, so c4 depends on a pixel 17 away.  c4 is put on the first (last) output row / column of a window
    and on its neighbours +-1; c21 then lies on the outermost halo row / column of that window and on its neighbours.
    The same again at the seams that windows with a halo of 16, 15 and 14 would have (seam_for_halo): there c21 lies
    outside such a window, so that a halo that is too small shows at c4 -- at the real seams alone it would not, since
    the output size follows the halo.  Placement k carries the far seed when (k + parity) is even, so that `chain17` and
    `chain17_toggled` differ in the far seed of every placement."""
    fm = np.full((H, W), WALL, np.uint8)
    water = np.zeros((H, W), bool)
    rows, cols = seam_lists
    pl, meta = _Placer(H, W), []
    k = 0
    must_fit = (H, W) in [shape for shapes in KERNEL_SHAPES.values() for shape in shapes]

    def clear_of_row_seams(cells):
        """Horizontal chains keep out of the rows that the vertical ones need around the row seams: no two ever meet."""
        return all(not (s - 31 <= cells[0][0] <= s + 38) for s in rows)

    for d in DIRS:
        along = 0 if d[0] else 1
        horizontal = along == 1
        for s17 in _seam_or_middle(rows if along == 0 else cols, H if along == 0 else W):
            real = s17 in (rows if along == 0 else cols)
            for halo in CHAIN_HALOS if real else (HALO,):
                s = seam_for_halo(s17, halo, _out_size(s17, along)) if real else s17
                for shift in (0, -1, 1):
                    # running towards lower indices, c4 sits on the first output row s of a window and c21 on s - 17, the
                    # first row of a window of halo 17; running towards higher ones, c4 sits on the last output row s - 1
                    # of the window before and c21 on s + 16, that window's last row
                    near = (s if d[along] < 0 else s - 1) + shift
                    size = W if along == 0 else H
                    got = None
                    for j in range(size):                            # sideways, around the raster, to the first free place
                        side = (5 + 17 * k + 3 * j) % size
                        y, x = (near - 4 * d[0], side) if along == 0 else (side, near - 4 * d[1])
                        # (no sliding inside place: one try at this place; c0 .. c21 must lie inside the raster)
                        got = pl.place(cells=_line(y, x, d, 31), slide=(0, 0), tries=1, need=tuple(range(22)),
                                       ok=clear_of_row_seams if horizontal else None)
                        if got is not None:
                            break
                    if got is None:
                        # a raster that is too small leaves the chain out; the shapes of the kernel tests hold every one
                        assert not must_fit, (H, W, d, s, shift)
                        continue
                    kept, _ = got
                    far = (k + parity) % 2 == 0
                    for c in kept:
                        fm[c] = AREA
                        water[c] = True
                    fm[kept[0]] = SEED
                    if far:
                        fm[kept[21]] = SEED
                    meta.append(dict(cells=kept, near=kept[4], far=kept[21], far_seed=far, dir=d, shift=shift, seam=s,
                                     halo=halo, axis=along))
                    k += 1
    return _scene(fm, water, meta)


def chain17(rng, H, W, seam_lists):
    return _chain(rng, H, W, seam_lists, 0)


def chain17_toggled(rng, H, W, seam_lists):
    """`chain17` with the far seed of every placement toggled."""
    return _chain(rng, H, W, seam_lists, 1)


def _patches(rng, H, W, values, smax):
    """An H x W plane tiled with rectangles of sides 3 .. smax that take `values` in turn."""
    out = np.empty((H, W), values.dtype)
    k, y = 0, 0
    while y < H:
        h = int(rng.integers(3, smax + 1))
        x = 0
        while x < W:
            w = int(rng.integers(3, smax + 1))
            out[y:y + h, x:x + w] = values[k % len(values)]
            k += 1
            x += w
        y += h
    return out, k


def bytes256(rng, H, W, seam_lists):
    """All 256 Fmask bytes in coherent rectangular patches (sides 3 .. 20, smaller where the raster would not hold 256
    such patches), the order shuffled, every value present on rasters of 4096 pixels or more; water in patches of its
    own.  Every byte is a seed, area, a wall or fill next to every kind of neighbour."""
    smax = 20
    while smax > 3 and ((3 + smax) / 2) ** 2 * 256 * 1.5 > H * W:
        smax -= 1
    values = np.concatenate([rng.permutation(256) for _ in range(max(1, H * W // (9 * 256) + 1))]).astype(np.uint8)
    fm, n = _patches(rng, H, W, values, smax)
    water, _ = _patches(rng, H, W, np.array([1, 1, 0], np.uint8)[rng.integers(0, 3, 4096)], smax + 5)
    if H * W >= 4096:
        assert n >= 256 and len(np.unique(fm)) == 256
    return _scene(fm, water.astype(bool), [dict(smax=smax, patches=n)])


def saturated(rng, H, W, seam_lists):
    """Four scenes: all area and all snow; all area and no snow; a checkerboard of area and wall with snow seeds, where
    no dilation can travel; all fill except one row of area (fill is byte 255, which carries the snow bit: the rows
    either side seed it)."""
    yy, xx = np.mgrid[0:H, 0:W]
    all_water = np.ones((H, W), bool)
    checker = np.where((yy + xx) % 2 == 0, AREA, WALL).astype(np.uint8)
    checker[(checker == AREA) & (rng.random((H, W)) < 0.2)] = SEED
    row = np.full((H, W), FILL, np.uint8)
    row[H // 2] = AREA
    row[H // 2, [0, W - 1]] = SEED
    return [_scene(np.full((H, W), SEED, np.uint8), all_water, [dict(kind='all snow')]),
            _scene(np.full((H, W), AREA, np.uint8), all_water, [dict(kind='no snow')]),
            _scene(checker, xx % 3 != 0, [dict(kind='checkerboard')]),
            _scene(row, xx % 2 == 0, [dict(kind='one row')])]


def holes(rng, H, W, seam_lists):
    """`diamonds` over water, with fill (255) rectangles, an ocean mask and a shadow mask cutting through the diamonds:
    fill stops both dilations, ocean and shadow take the water away and with it the clear dilation."""
    base = diamonds(rng, H, W, seam_lists)
    fm = base['fmask'].copy()
    pts = base['meta'][0]['seeds']
    ocean = np.ones((H, W), np.uint8)
    shad = np.ones((H, W), np.uint8)
    for i, (y, x) in enumerate(pts):
        a, b = int(rng.integers(-6, 7)), int(rng.integers(2, 9))
        if i % 3 == 0:
            fm[max(y + a, 0):y + a + b, max(x + 2, 0):x + 2 + int(rng.integers(1, 12))] = FILL
        elif i % 3 == 1:
            ocean[max(y - b, 0):y + 1, max(x + a, 0):x + a + 5] = 0
        else:
            shad[max(y + 1, 0):y + 1 + b, max(x + a - 4, 0):x + a + 3] = 0
    for y, x in pts[1::3] + pts[2::3]:
        fm[y, x] = SEED
    return _scene(fm, np.ones((H, W), bool), [dict(seeds=pts)], ocean=ocean, shad=shad)


def speckle(rng, H, W, seam_lists):
    """Per pixel a pick from area, seed, wall, clear, fill and any byte; water at random: for rasters of a few pixels,
    where nothing larger fits."""
    picks = np.array([AREA, AREA, AREA, SEED, WALL, 0, FILL, 0], np.uint8)[rng.integers(0, 8, (H, W))]
    fm = np.where(rng.random((H, W)) < 0.15, rng.integers(0, 256, (H, W)), picks).astype(np.uint8)
    return _scene(fm, rng.random((H, W)) < 0.6)


BUILDERS = dict(speckle=speckle, diamonds=diamonds, corridors=corridors, chain17=chain17, chain17_toggled=chain17_toggled,
                bytes256=bytes256, saturated=saturated, holes=holes)


def scenes(domain, H, W, nw=(8,), seed=0):
    """The scenes (a list: four for `saturated`, else one) of `domain` on an H x W raster aimed at the seams of the
    kernel variants `nw`."""
    rng = np.random.default_rng([DOMAINS.index(domain), H, W, seed])
    out = BUILDERS[domain](rng, H, W, seams(H, W, nw))
    return out if isinstance(out, list) else [out]


def with_edge_rows(scene):
    """A copy of `scene` whose first and last rows are snow seeds and whose second and second-to-last rows are area
    over water: in a batch, whatever bleeds across a tile boundary shows in the neighbouring tile."""
    s = dict(scene, fmask=scene['fmask'].copy(), water=scene['water'].copy())
    fm, water = s['fmask'], s['water']
    fm[[0, -1], :] = SEED
    if fm.shape[0] > 2:
        fm[[1, -2], :] = AREA
        water[[1, -2], :] = True
    return s


# ---- what the tests of both kinds share: kernels, shapes, the oracle's answer, a windowed restatement -------------------
# (kernel variant of the lab switch cover_kernel -> words per window row)
KERNELS = {'8': 8, '4': 4, '8,direct': 8, '4,direct': 4}
# the smallest shapes that hold the seams of each width AND the chains aimed at the seams of halos 17 .. 14 behind the last
# seam (+ 6 for halo 14, + 17 to the far seed, + 1 for the shifted neighbour)
KERNEL_SHAPES = {8: [(250, 250), (476, 250)], 4: [(250, 140), (250, 220)]}
THIN_SHAPES = ([(1, 1), (1, 7), (1, 700), (700, 1), (300, 3), (5, 300)] + [(24, w) for w in (33, 221, 222, 223, 256, 257)] +
               [(h, 24) for h in (222, 223, 239, 240)])
# entries, strides and addresses: H * W % 8 = 0 .. 7, H * W % 32 zero and not; about 9,000 pixels, so that the finishing
# kernel has threads on its 8-byte path and threads on its byte path; then tiles of a few pixels
ENTRY_SHAPES = [(96, 100), (91, 91), (97, 98), (97, 99), (98, 98), (95, 99), (99, 98), (97, 95), (98, 100), (5, 5), (3, 10),
                (3, 3), (4, 6)]
assert [h * w % 8 for h, w in ENTRY_SHAPES[:9]] == [0, 1, 2, 3, 4, 5, 6, 7, 0] and 96 * 100 % 32 == 0 and 98 * 100 % 32
STALE_SHAPES = [(300, 300), (1, 1), (7, 9), (240, 1), (1, 240), (37, 53), (230, 100)]
SNOW, CLEAR = 2, 0                  # CLOUD of an area pixel with and without snow


def expected(scene, collapse=True, mode='cover', **kw):
    """The numpy oracle's layers and counters of a scene."""
    from oracle import dswx_oracle as o
    bands, fm, masks = planes(scene)
    with np.errstate(all='ignore'):
        return o.classify_tile(bands, fm, landcover=None, shadow=masks.get('shad'), ocean_mask=masks.get('ocean'),
                               mask_adjacent_to_cloud_mode=mode, collapse=collapse, **kw)


def windowed_cloud(scene, halo, nw):
    """CLOUD (uncollapsed) of a scene as windows of 256 rows x 32 nw columns with `halo` would compute it: each window
    sees nothing outside itself, runs the 10 + 7 steps on what it sees and keeps its output region.  With halo 17 that
    is the oracle's layer; with a smaller one it is what a kernel built with that halo gives."""
    from oracle import dswx_oracle as o
    e = expected(scene, False, 'ignore')            # ('ignore': the preliminary CLOUD of 'cover' + 2 on Fmask snow)
    fm, wtr_2 = scene['fmask'], e['WTR-2']
    snow0 = (fm & 16) == 16
    cloud = e['CLOUD'].copy()
    cloud[snow0 & (wtr_2 != 255)] -= 2
    cloud[wtr_2 == 255] = 1                         # (fill: any value but 0 -- neither area nor a clear seed)
    area = ((fm & 4) == 4) & (cloud == 0)
    water = area & (wtr_2 >= 1) & (wtr_2 <= 4)
    H, W = fm.shape
    oh, ow = 256 - 2 * halo, 32 * nw - 2 * halo
    final = np.zeros((H, W), bool)
    for y0 in range(0, H, oh):
        for x0 in range(0, W, ow):
            ys, xs = slice(max(y0 - halo, 0), min(y0 - halo + 256, H)), slice(max(x0 - halo, 0), min(x0 - halo + 32 * nw, W))
            s = o.masked_dilation_by_shifts(snow0[ys, xs], SNOW_REACH, area[ys, xs])
            c = o.masked_dilation_by_shifts(~s & (cloud[ys, xs] == 0), CLEAR_REACH, water[ys, xs])
            s &= ~c
            final[y0:y0 + oh, x0:x0 + ow] = s[y0 - ys.start:y0 - ys.start + oh, x0 - xs.start:x0 - xs.start + ow]
    out = e['CLOUD'].copy()
    out[snow0 & (wtr_2 != 255)] -= 2
    out[final & (wtr_2 != 255)] += 2
    return out
