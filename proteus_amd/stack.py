"""The per-pixel composite of the tiles of a plane, include/dswx_hip.h ("stack"), stated in numpy.

A stack is uint8 [n_tiles, ...]; the tile index is time order.  With c(t) = cat_of_byte[stack[t][i]] for pixel i:

    count[k][i]    the number of tiles with c(t) == k, k < n_cats                                    uint16
    last[i]        the byte of the latest tile with c(t) < n_cats ("an observation"); `fill` if none  uint8
    last_index[i]  that tile's index; NONE (65535) if none                                            uint16
    share[i]       (100 * count[0][i]) // n_obs, n_obs = the sum of the counts; NO_SHARE (255) if 0   uint8

This module calls neither dswx_stack_host nor the device: the tests pin the three to each other.
"""
import numpy as np

MAX_CATS, MAX_TILES, NONE, NO_SHARE = 4, 65535, 65535, 255
OUTPUTS = ('count', 'last', 'last_index', 'share')
# the WTR family (dswx_hls.py: the saved, collapsed classes 0 not water / 1 open water / 2 partial surface water, 252 snow /
# 253 cloud / 254 ocean masked / 255 fill; uncollapsed 1 .. 4 = open water high / moderate, partial conservative / aggressive)
WTR_NOT_WATER, WTR_MASKED = 0, (252, 253, 254, 255)


class Spec:
    """dswx_stack_spec_t: n_cats 1 .. 4, fill 0 .. 255, cat_of_byte uint8 [256] (a value >= n_cats: not an observation)."""

    def __init__(self, n_cats, cat_of_byte, fill=255):
        self.n_cats, self.fill = int(n_cats), int(fill)
        self.cat_of_byte = np.ascontiguousarray(cat_of_byte, dtype=np.uint8)
        if not 1 <= self.n_cats <= MAX_CATS:
            raise ValueError(f'n_cats {self.n_cats} outside 1 .. {MAX_CATS}')
        if not 0 <= self.fill <= 255:
            raise ValueError(f'fill {self.fill} outside 0 .. 255')
        if self.cat_of_byte.shape != (256,):
            raise ValueError(f'cat_of_byte has shape {self.cat_of_byte.shape}, not (256,)')


def wtr_spec(collapsed=True, partial_is_water=True, fill=255):
    """The spec of a WTR-family layer: category 0 = water, category 1 = clear and not water, every other byte is not an
    observation.  Saved (collapsed) form: water is {1, 2}, or {1} with partial_is_water=False; not water is {0}.
    Uncollapsed form: water is {1, 2, 3, 4}, or {1, 2}.  With partial_is_water=False the partial-surface-water classes (2;
    3 and 4) are clear observations that are NOT water: they count in category 1 and can be the latest observation -- a
    pixel seen as partial water was seen.  252 .. 255 and the bytes of the other family are not observations."""
    cat = np.full(256, 255, dtype=np.uint8)
    cat[WTR_NOT_WATER] = 1
    water, partial = ([1], [2]) if collapsed else ([1, 2], [3, 4])
    cat[water] = 0
    cat[partial] = 0 if partial_is_water else 1
    return Spec(2, cat, fill)


def stack_tiles(tiles, spec):
    """{'count': uint16 [n_cats, ...], 'last': uint8 [...], 'last_index': uint16 [...], 'share': uint8 [...]} of a stack
    uint8 [n_tiles, ...]; [...] is the shape of a tile."""
    tiles = np.asarray(tiles)
    if tiles.dtype != np.uint8 or tiles.ndim < 1:
        raise ValueError(f'a stack is uint8 [n_tiles, ...], not {tiles.dtype} {tiles.shape}')
    T, shape = tiles.shape[0], tiles.shape[1:]
    if T > MAX_TILES:
        raise ValueError(f'{T} tiles: at most {MAX_TILES}')
    N = int(np.prod(shape, dtype=np.int64))
    flat = tiles.reshape(T, N)
    count = np.zeros((spec.n_cats, N), dtype=np.int64)
    index = np.full(N, -1, dtype=np.int64)
    for t0 in range(0, T, 256):                                  # (in slabs: the category array of 65535 tiles stays small)
        cat = spec.cat_of_byte[flat[t0:t0 + 256]]
        for k in range(spec.n_cats):
            count[k] += np.count_nonzero(cat == k, axis=0)
        seen = np.where(cat < spec.n_cats, np.arange(t0, t0 + len(cat))[:, None], -1).max(axis=0)
        index = np.maximum(index, seen)
    n_obs = count.sum(axis=0)
    any_obs = index >= 0
    last = np.where(any_obs, flat[np.maximum(index, 0), np.arange(N)] if T else 0, spec.fill)
    share = np.where(n_obs > 0, (100 * count[0]) // np.maximum(n_obs, 1), NO_SHARE)
    return {'count': count.astype(np.uint16).reshape((spec.n_cats,) + shape), 'last': last.astype(np.uint8).reshape(shape),
            'last_index': np.where(any_obs, index, NONE).astype(np.uint16).reshape(shape),
            'share': share.astype(np.uint8).reshape(shape)}
