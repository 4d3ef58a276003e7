"""Cases shared by tests/test_land_mesh_domain.py (CPU) and tests/test_gpu_land_mesh_domain.py: the land-mesh entry over its
whole value domain and over lattices of more than LM_MAX_GRID_X = 1024 rectangles, with expected values that no mesh or warp
line of the project computes.

EVERY CASE IS BUILT BACKWARDS from the rasters the definition ends in.  Full rasters w3 [n, 3 H, 3 W] and c1 [n, H, W] are
drawn by oracle/land_inputs.py; integer margins, different per side and per map and some of them 0, are cut off them, and what
is left are the source windows the entry reads.  An identity mesh (tests/_land_mesh_cases.identity_mesh) is pointed at each
window with the matching offset plus a sub-pixel offset o of 128, 0, 255, -1 or 256 in 1/256 pixel: since the tap is sx >> 8,
o moves it by floor(o / 256) = 0, 0, 0, -1 or +1 whole pixels.  So lattice pixel X reads full pixel X + floor(o / 256) where
that lies in the window and `outside` elsewhere -- an index expression written out by hand in `cut` -- and the expected LAND is
oracle.dswx_oracle.landcover_mask_from_warped of those hand-padded rasters.  Head words 1 .. 6 are counted from the same
index expression and from the oracle's LAND.

ONE DEPARTURE from the plain identity mesh.  Behind a rectangular window an HLS pixel has rows x columns inside taps, rows and
columns in 0 .. 3, which is never 5, 7 or 8.  In the cases whose WorldCover shift is 0 -- where the position of a fine pixel
IS its node, nothing is interpolated -- a seeded third of the nodes is moved to a column left or right of the window (the
INT32 ends among them): those fine pixels read `outside`, and every count 0 .. 9 of inside taps occurs.

THE SWEEP follows sweep_cases of tests/test_gpu_land_domain.py: every axis walked in its own shuffled order, 90 cases.  One
case is N_CALLS calls on the same maps with different `outside` bytes: the first call pairs a counted WorldCover code with one
of the case's forest classes, the second gives both bytes with bit 7 flipped (138 for 10: a kernel that dropped the bit would
count it), the others walk all 256 values of either byte.
THE WALK is four lattices of more than 1024 rectangles in the 'blocks' mode.
"""
import functools

import numpy as np

from oracle import dswx_oracle as O
from oracle import land_inputs as L
from proteus_amd import landmesh
from tests import _land_mesh_cases as C
from tests.test_gpu_land_domain import YEAR_OFFSETS

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
RECT_H, RECT_W, MAX_GRID_X = 8, 32, 1024                       # dswx_land_mesh.hip (tests/test_land_mesh.py pins the first two)

LATTICES = [(1, 1), (8, 32), (9, 33), (19, 70), (3, 257), (33, 41)]
WC_MODES = ['classes', 'full', 'near', 'dense', 10, 50, 80, 95, 0, 255]
FOREST_KEYS = list(L.FOREST_SETS) + [0, 31, 32, 223, 224, 255]     # the sets, and single classes at the edges of the bitset words
THR_KEYS = list(L.THRESHOLD_SETS)
SHIFT_PAIRS = [(a, b) for a in range(9) for b in range(9)]
SUBPIXEL = [128, 0, 255, -1, 256]
MARGINS = [0, 0, 1, 2, 3, 4, 5, 7, 8]
N_SWEEP = 90
N_CALLS = 5
SEED = 20260131


def forest_of(key):
    return L.FOREST_SETS[key] if isinstance(key, str) else [key]


def rectangles(shape):
    return -(-shape[0] // RECT_H) * -(-shape[1] // RECT_W)


class Case:
    """One set of maps and meshes, and the calls made on it."""

    def __init__(self, name, shape, n, modes, forest_key, thr_key, year_offset, shifts, sub, margins_wc, margins_cg, outs, seed,
                 land_pad=0):
        self.name, self.shape, self.n, self.modes = name, shape, n, modes
        self.forest_key, self.thr_key, self.year_offset, self.shifts = forest_key, thr_key, year_offset, shifts
        self.sub, self.margins_wc, self.margins_cg, self.outs, self.seed, self.land_pad = sub, margins_wc, margins_cg, outs, seed, land_pad
        self.forest, self.thresholds = forest_of(forest_key), L.THRESHOLD_SETS[thr_key]
        self.holes = shifts[0] == 0 and rectangles(shape) <= MAX_GRID_X

    def spec(self, call=0):
        """The landmesh.Spec of call number `call`."""
        H, W = self.shape
        return landmesh.Spec(self.shifts[0], self.shifts[1], self.outs[call][0], self.outs[call][1], self.thresholds, self.year_offset,
                             self.forest, land_tile_stride=H * W + self.land_pad if self.land_pad else 0)


def _margins(rng, dim, empty=False):
    """(low, high) cut off a side of `dim` pixels, at least one pixel left -- or none at all."""
    if empty:
        return dim, 0
    lo = min(MARGINS[rng.integers(len(MARGINS))], dim - 1)
    return lo, min(MARGINS[rng.integers(len(MARGINS))], dim - 1 - lo)


def sweep_cases():
    rng = np.random.default_rng(SEED)
    axes = [LATTICES, WC_MODES, FOREST_KEYS, THR_KEYS, YEAR_OFFSETS, SHIFT_PAIRS, SUBPIXEL, SUBPIXEL, SUBPIXEL, SUBPIXEL]
    orders = [np.concatenate([rng.permutation(len(a)) for _ in range(-(-N_SWEEP // len(a)))]) for a in axes]
    drawn = [tuple(a[order[i]] for a, order in zip(axes, orders)) for i in range(N_SWEEP)]
    walked = [np.concatenate([rng.permutation(256), rng.integers(0, 256, N_SWEEP * (N_CALLS - 2) - 256)]) for _ in range(2)]
    # the two empty sources: the first two cases on the 19 x 70 lattice (more than one rectangle)
    large = [i for i, d in enumerate(drawn) if d[0] == (19, 70)]
    cases = []
    for i, (shape, mode, fk, tk, year, shifts, *sub) in enumerate(drawn):
        H, W = shape
        n = 2 + i % 2
        modes = [WC_MODES[(WC_MODES.index(mode) + t) % len(WC_MODES)] for t in range(n)]
        m_wc = _margins(rng, 3 * H, i == large[0]) + _margins(rng, 3 * W)
        m_cg = _margins(rng, H) + _margins(rng, W, i == large[1])
        outs = [(int(walked[0][(N_CALLS - 2) * i + k]), int(walked[1][(N_CALLS - 2) * i + k])) for k in range(N_CALLS - 2)]
        classes = sorted({c for c in forest_of(fk) or [] if 0 <= c <= 255})
        first = (int(L.WC_CODES[i % len(L.WC_CODES)]), int(classes[rng.integers(len(classes))]) if classes else int(rng.integers(256)))
        alias = (first[0] ^ 128, first[1] ^ 128)              # what a byte that lost its bit 7 would make a counted code, a forest class
        name = f'{i}-{H}x{W}-{mode}-{fk}-{tk.replace(" ", "_")}-{year}-s{shifts[0]}{shifts[1]}'
        cases.append(Case(name, shape, n, modes, fk, tk, year, shifts, tuple(sub), m_wc, m_cg, [first, alias] + outs, 6000 + i))
    return cases


SWEEP = sweep_cases()

# (lattice, outputs wanted, twice into the same outputs): 1031 rectangles in one row, 1031 in one column, 1144 ragged in both
# directions, 2050 so that some workgroups take three
WALK_PLAN = [((8, 32987), ('land', 'head'), True), ((8245, 31), ('head',), False), ((203, 1400), ('land',), False),
             ((8, 65569), ('land', 'head'), False)]
WALK = [Case(f'{H}x{W}', (H, W), 2, ['blocks', 'blocks'], fk, tk, year, shifts, sub, m_wc, m_cg, [outs], 9000 + k, land_pad=13)
        for k, (((H, W), _, _), fk, tk, year, shifts, sub, m_wc, m_cg, outs) in enumerate(zip(
            WALK_PLAN, ('edge', 'default', 224, 'all'), ('standard', 'water heavy', 'standard', '1991'), (21, -1, 156, 99),
            ((5, 3), (0, 8), (8, 0), (6, 4)), ((0, 255, 256, -1), (-1, 128, 0, 256), (256, -1, 255, 0), (255, 0, -1, 128)),
            ((2, 1, 5, 0), (0, 7, 3, 2), (4, 0, 0, 8), (1, 3, 7, 5)), ((1, 0, 0, 3), (2, 5, 1, 0), (0, 3, 4, 1), (0, 1, 2, 0)),
            ((10, 111), (50, 0), (80, 224), (95, 200))))]
WALK_WANT = {c.name: (want, twice) for c, (_, want, twice) in zip(WALK, WALK_PLAN)}


def cut(full, margins, sub, shift, holes=None):
    """The source window of `full` [n, h, w] with `margins` (top, bottom, left, right) cut off, the identity mesh that points
    the lattice h x w at it with the sub-pixel offsets `sub` (x, y), and which full pixel each lattice pixel reads: (window,
    mesh, rows, cols, inside [h, w]) -- lattice pixel (X, Y) reads window pixel (cols[X], rows[Y]) where `inside`."""
    n, h, w = full.shape
    top, bottom, left, right = margins
    window = np.ascontiguousarray(full[:, top:h - bottom, left:w - right])
    mesh = C.identity_mesh((h, w), shift, offset=(sub[0] - 256 * left, sub[1] - 256 * top))
    rows = np.arange(h) + sub[1] // 256 - top
    cols = np.arange(w) + sub[0] // 256 - left
    inside = ((rows >= 0) & (rows < window.shape[1]))[:, None] & ((cols >= 0) & (cols < window.shape[2]))[None, :]
    if holes is not None:
        assert shift == 0 and mesh.shape == (h + 1, w + 1, 2)               # one node per lattice pixel, nothing interpolated
        far = np.array([-1, -256, INT32_MIN, 256 * window.shape[2], 256 * window.shape[2] + 255, INT32_MAX], dtype=np.int64)
        mesh[:h, :w, 0][holes] = far[np.arange(int(holes.sum())) % far.size]
        inside = inside & ~holes
    return window, mesh, rows, cols, inside


def padded(window, rows, cols, inside, outside):
    """[n, h, w]: what each lattice pixel reads -- the window's byte where `inside`, `outside` elsewhere."""
    n, wh, ww = window.shape
    if wh * ww == 0:
        return np.full((n,) + inside.shape, outside, np.uint8)
    taken = window[:, np.clip(rows, 0, wh - 1)[:, None], np.clip(cols, 0, ww - 1)[None, :]]
    return np.where(inside[None], taken, np.uint8(outside))


class Built:
    """The arrays of a Case: the full rasters, the windows `wc` / `cg` and meshes `m_wc` / `m_cg` that the entries are given, and
    the index expression the expected values come from."""

    def __init__(self, case):
        rng = np.random.default_rng(case.seed)
        H, W = case.shape
        self.case = case
        self.w3 = np.stack([L.worldcover(rng, H, W, m) for m in case.modes])
        self.c1 = np.stack([L.copernicus(rng, H, W) for _ in case.modes])
        holes = rng.random((3 * H, 3 * W)) < 0.35 if case.holes else None
        self.wc, self.m_wc, self.rows_wc, self.cols_wc, self.in_wc = cut(self.w3, case.margins_wc, case.sub[:2], case.shifts[0], holes)
        self.cg, self.m_cg, self.rows_cg, self.cols_cg, self.in_cg = cut(self.c1, case.margins_cg, case.sub[2:], case.shifts[1])
        self.taps_inside = self.in_wc.reshape(H, 3, W, 3).sum(axis=(1, 3))             # per HLS pixel, 0 .. 9
        self._expected = {}

    def warped(self, call=0):
        """(W3 [n, 3 H, 3 W], CG [n, H, W]) of the definition for the `outside` bytes of call number `call`."""
        o_wc, o_cg = self.case.outs[call]
        return padded(self.wc, self.rows_wc, self.cols_wc, self.in_wc, o_wc), padded(self.cg, self.rows_cg, self.cols_cg, self.in_cg, o_cg)

    def expected(self, call=0):
        """(land [n, H, W], head [n, 8]) of call number `call`: the oracle on the hand-padded rasters, the head counted here."""
        if call not in self._expected:
            c = self.case
            H, W = c.shape
            w3, c1 = self.warped(call)
            land = np.stack([O.landcover_mask_from_warped(w3[t], c1[t], c.forest, year=2000 + c.year_offset, thresholds=c.thresholds)
                             for t in range(c.n)])
            wc_in, cg_in = int(self.in_wc.sum()), int(self.in_cg.sum())
            head = np.array([[H * W, wc_in, 9 * H * W - wc_in, cg_in, H * W - cg_in, int((self.taps_inside == 0).sum()),
                              int((land[t] == 255).sum()), 0] for t in range(c.n)], dtype=np.uint64)
            land.setflags(write=False)
            head.setflags(write=False)
            self._expected[call] = (land, head)
        return self._expected[call]


@functools.lru_cache(maxsize=None)
def built(kind, k):
    """The arrays of SWEEP[k] ('sweep') or WALK[k] ('walk'), made once and left unchanged."""
    b = Built((SWEEP if kind == 'sweep' else WALK)[k])
    for a in (b.w3, b.c1, b.wc, b.cg, b.m_wc, b.m_cg):
        a.setflags(write=False)
    return b


def entry_cases():
    """A dozen sweep cases for the other ways in: thresholds, forest list, year offset and (first call) `outside` bytes none of
    them the default, both sources present."""
    return [k for k, c in enumerate(SWEEP)
            if c.thr_key != 'standard' and c.forest_key not in ('none', 'empty', 'default') and c.year_offset != 0 and c.outs[0][0] != 0
            and c.outs[0][1] != 0 and c.margins_wc[0] < 3 * c.shape[0] and c.margins_cg[2] < c.shape[1]][:12]
