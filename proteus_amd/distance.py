"""The exact Euclidean distance of every pixel to the nearest target of a plane, include/dswx_hip.h ("distance"), stated in
numpy.

A plane is uint8 [n_tiles, H, W].  Pixel q is a target iff target_of_byte[byte at q] != 0.  With idx(p) = y * W + x,
d2(p, q) = (yp - yq)^2 + (xp - xq)^2 and R = max_radius (0 = unbounded), a target q reaches p when R == 0 or
d2(p, q) <= R * R.  Rows do not wrap and tiles never see each other.  Per tile:

    dist2[p]    the minimum of d2(p, q) over the targets that reach p; 0 on a target; NONE when none does           uint32
    nearest[p]  idx(q) of the target that attains it: the smallest (d2, xq, yq); NONE where dist2 is                 uint32
    within[p]   the byte, except that a non-target p with dist2[p] != NONE becomes `mark` (only with R > 0)          uint8
    summary     40 words per tile: targets, reached non-targets, pixels not reached, the largest dist2 of a reached  uint64
                pixel, the smallest idx holding it, the sum of dist2 over reached pixels, 0, 0, then the reached
                non-targets with floor(log2(dist2)) == b

The statement is the minimum over ALL targets at once, one row of pixels at a time: the key (d2, xq, yq) of every target
against every pixel of the row, and the smallest key wins.  It is quadratic and meant for the shapes of a test.  This module
calls neither dswx_distance_host nor the device, nor scipy: the tests pin them to each other.
"""
import numpy as np

from .stack import wtr_spec

NONE = 0xFFFFFFFF
SUMMARY_WORDS = 40
OUTPUTS = ('dist2', 'nearest', 'within', 'summary')
MAX_SIDE = 46340                                         # (H - 1)^2 + (W - 1)^2 stays below NONE


class Spec:
    """dswx_distance_spec_t: max_radius in pixels (0 = unbounded), mark 0 .. 255, target_of_byte uint8 [256] (non-zero: target)."""

    def __init__(self, target_of_byte, max_radius=0, mark=0):
        self.max_radius, self.mark = int(max_radius), int(mark)
        self.target_of_byte = np.ascontiguousarray(target_of_byte, dtype=np.uint8)
        if not 0 <= self.max_radius < 1 << 32:
            raise ValueError(f'max_radius {self.max_radius} outside 0 .. 2^32 - 1')
        if not 0 <= self.mark <= 255:
            raise ValueError(f'mark {self.mark} outside 0 .. 255')
        if self.target_of_byte.shape != (256,):
            raise ValueError(f'target_of_byte has shape {self.target_of_byte.shape}, not (256,)')


WTR_BUFFER_MARK = 200                                    # a byte that no WTR-family layer uses: the ring stands out


def wtr_distance_spec(radius=0, collapsed=True, partial_is_water=True, mark=WTR_BUFFER_MARK):
    """The spec of a WTR-family layer: the targets are the bytes that stack.wtr_spec puts in category 0 (water) -- the bytes
    label.wtr_label_spec calls members -- so dist2 is the squared distance to the nearest water pixel, in pixels; with
    `radius` > 0 only water within that many pixels counts, and `mark` is the byte of the ring in the `within` plane."""
    s = wtr_spec(collapsed=collapsed, partial_is_water=partial_is_water)
    return Spec((s.cat_of_byte == 0).astype(np.uint8), radius, mark)


def distance_tiles(tiles, spec, want=OUTPUTS):
    """{'dist2': uint32 [n, H, W], 'nearest': uint32 [n, H, W], 'within': uint8 [n, H, W] (only with spec.max_radius > 0),
    'summary': uint64 [n, 40]} of a plane uint8 [n, H, W]."""
    tiles = np.asarray(tiles)
    if tiles.dtype != np.uint8 or tiles.ndim != 3:
        raise ValueError(f'a plane is uint8 [n_tiles, H, W], not {tiles.dtype} {tiles.shape}')
    n, H, W = tiles.shape
    if H > MAX_SIDE or W > MAX_SIDE or H * W > 1 << 31:
        raise ValueError(f'{H} x {W} pixels: each side at most {MAX_SIDE} and at most 2^31 pixels')
    R = spec.max_radius
    target = spec.target_of_byte[tiles] != 0
    dist2 = np.full((n, H, W), NONE, dtype=np.uint32)
    nearest = np.full((n, H, W), NONE, dtype=np.uint32)
    xs = np.arange(W, dtype=np.int64)
    for t in range(n):
        ty, tx = np.nonzero(target[t])
        if not len(ty):
            continue
        ty, tx = ty.astype(np.int64), tx.astype(np.int64)
        for y in range(H):
            d2 = (ty[None, :] - y) ** 2 + (tx[None, :] - xs[:, None]) ** 2                  # [pixel of the row, target]
            key = (d2 << 40) | (tx[None, :] << 20) | ty[None, :]                            # (d2 < 2^32, x and y < 2^20)
            k = np.argmin(key, axis=1)
            best = d2[xs, k]
            ok = (best <= R * R) if R else np.ones(W, dtype=bool)
            dist2[t, y, ok] = best[ok]
            nearest[t, y, ok] = (ty[k] * W + tx[k])[ok]
    out = {'dist2': dist2, 'nearest': nearest}
    if R:
        out['within'] = np.where(~target & (dist2 != NONE), spec.mark, tiles).astype(np.uint8)
    out['summary'] = summary_of(dist2)
    return {k: v for k, v in out.items() if k in want}


def summary_of(dist2):
    """The summary uint64 [n, 40] from the dist2 plane [n, H, W] of distance_tiles (or of the library)."""
    dist2 = np.asarray(dist2)
    n = dist2.shape[0]
    out = np.zeros((n, SUMMARY_WORDS), dtype=np.uint64)
    for t in range(n):
        d = dist2[t].reshape(-1).astype(np.int64)
        reached = d != NONE
        out[t, 0] = np.count_nonzero(d == 0)
        out[t, 1] = np.count_nonzero(reached & (d != 0))
        out[t, 2] = np.count_nonzero(~reached)
        if reached.any():
            r = np.where(reached, d, -1)
            out[t, 3] = r.max()
            out[t, 4] = np.argmax(r)                     # argmax returns the FIRST largest: the smallest index
            out[t, 5] = d[reached].sum()
        ring = d[reached & (d != 0)]
        for b in range(32):
            out[t, 8 + b] = np.count_nonzero((ring >> b) == 1)
    return out
