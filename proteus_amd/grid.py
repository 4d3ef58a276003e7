"""A plane aggregated onto a coarse grid, include/dswx_hip.h ("grid"), stated in numpy.

A plane is uint8 [n_tiles, H, W].  The grid has GH = ceil(H / cell_h) rows and GW = ceil(W / cell_w) columns of cells; cell
(gy, gx) covers the rows gy * cell_h .. min(H, (gy + 1) * cell_h) - 1 and the corresponding columns, so the last row and column
of cells are ragged and n_pix is what a cell really covers.  Per tile and cell, with c(p) = cat_of_byte[byte at pixel p]:

    count[k]   the number of pixels with c(p) == k, k < n_cats                                            uint32
    share      (100 * count[0]) // n_obs, n_obs = the sum of the counts; NO_SHARE (255) where n_obs == 0   uint8
    coverage   (100 * n_obs) // n_pix                                                                      uint8
    major      the smallest k whose count is the largest; NONE (255) where n_obs == 0                      uint8

This module calls neither dswx_grid_host nor the device: the tests pin the three to each other.
"""
import numpy as np

from .stack import wtr_spec

MAX_CATS, MAX_CELL_PIXELS, NO_SHARE, NONE = 4, 1 << 24, 255, 255
OUTPUTS = ('count', 'share', 'coverage', 'major')


class Spec:
    """dswx_grid_spec_t: n_cats 1 .. 4, cell_h and cell_w >= 1, cat_of_byte uint8 [256] (a value >= n_cats: not an
    observation; the table of a stack.Spec, unchanged)."""

    def __init__(self, n_cats, cell_h, cell_w, cat_of_byte):
        self.n_cats, self.cell_h, self.cell_w = int(n_cats), int(cell_h), int(cell_w)
        self.cat_of_byte = np.ascontiguousarray(cat_of_byte, dtype=np.uint8)
        if not 1 <= self.n_cats <= MAX_CATS:
            raise ValueError(f'n_cats {self.n_cats} outside 1 .. {MAX_CATS}')
        if self.cell_h < 1 or self.cell_w < 1:
            raise ValueError(f'cell {self.cell_h} x {self.cell_w}: sizes below 1')
        if self.cat_of_byte.shape != (256,):
            raise ValueError(f'cat_of_byte has shape {self.cat_of_byte.shape}, not (256,)')


def wtr_grid_spec(cell, collapsed=True, partial_is_water=True):
    """The spec of a WTR-family layer on square cells of `cell` pixels, from stack.wtr_spec's table: category 0 = water,
    category 1 = clear and not water, every other byte is not an observation.  `share` is then the water fraction of the
    clear pixels of a cell in percent, `coverage` the clear fraction of the cell, `major` 0 (water) / 1 (not water) / 255."""
    s = wtr_spec(collapsed=collapsed, partial_is_water=partial_is_water)
    return Spec(s.n_cats, cell, cell, s.cat_of_byte)


def grid_shape(height, width, spec):
    """(GH, GW) of a height x width raster; an empty raster has no cells."""
    if height <= 0 or width <= 0:
        return (0, 0)
    return (-(-height // min(spec.cell_h, height)), -(-width // min(spec.cell_w, width)))


def grid_tiles(tiles, spec):
    """{'count': uint32 [n_cats, n, GH, GW], 'share', 'coverage', 'major': uint8 [n, GH, GW]} of a plane uint8 [n, H, W]."""
    tiles = np.asarray(tiles)
    if tiles.dtype != np.uint8 or tiles.ndim != 3:
        raise ValueError(f'a plane is uint8 [n_tiles, H, W], not {tiles.dtype} {tiles.shape}')
    n, H, W = tiles.shape
    GH, GW = grid_shape(H, W, spec)
    if GH and min(spec.cell_h, H) * min(spec.cell_w, W) > MAX_CELL_PIXELS:
        raise ValueError(f'a cell of {min(spec.cell_h, H)} x {min(spec.cell_w, W)} pixels: at most {MAX_CELL_PIXELS}')
    count = np.zeros((spec.n_cats, n, GH, GW), dtype=np.int64)
    n_pix = np.zeros((GH, GW), dtype=np.int64)
    if n and GH:
        rows = np.arange(0, H, min(spec.cell_h, H))      # the first row / column of every cell
        cols = np.arange(0, W, min(spec.cell_w, W))
        cat = spec.cat_of_byte[tiles]
        for k in range(spec.n_cats):
            by_row = np.add.reduceat((cat == k).astype(np.int64), rows, axis=1)
            count[k] = np.add.reduceat(by_row, cols, axis=2)
    if GH:
        n_pix = np.outer(np.diff(np.append(np.arange(0, H, min(spec.cell_h, H)), H)),
                         np.diff(np.append(np.arange(0, W, min(spec.cell_w, W)), W)))
    n_obs = count.sum(axis=0)
    share = np.where(n_obs > 0, (100 * count[0]) // np.maximum(n_obs, 1), NO_SHARE)
    coverage = (100 * n_obs) // np.maximum(n_pix, 1)
    # argmax returns the FIRST largest: the smallest k
    major = np.where(n_obs > 0, np.argmax(count, axis=0), NONE)
    return {'count': count.astype(np.uint32), 'share': share.astype(np.uint8), 'coverage': coverage.astype(np.uint8),
            'major': major.astype(np.uint8)}
