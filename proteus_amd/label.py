"""The connected bodies of a plane, include/dswx_hip.h ("label"), stated in numpy.

A plane is uint8 [n_tiles, H, W].  Pixel p is a member iff member_of_byte[byte at p] != 0; two members are adjacent when they
are neighbours in the 4- or the 8-neighbourhood of the same tile (rows do not wrap, tiles never connect); a body is a maximal
set of members connected through adjacency.  Per tile, with idx(p) = y * W + x:

    label[p]   0 for a non-member, else 1 + the smallest idx(q) over the body of p                          uint32
    size[p]    0 for a non-member, else the number of pixels of the body of p                                uint32
    sieved[p]  the byte, except that a member of a body of fewer than min_size pixels becomes `replace`     uint8
    summary    40 words per tile: bodies, member pixels, largest size, its label (the smallest on a tie),   uint64
               bodies of at least min_size, their pixels, 0, 0, then the bodies with floor(log2(size)) == b

The statement is repeated min-propagation over the neighbourhood to a fixed point: every member starts with its own index and
takes the smallest value among itself and its member neighbours until nothing changes.  To reach the fixed point in few
rounds a round sweeps along each direction of the neighbourhood with a running minimum that restarts at every non-member.
This module calls neither dswx_label_host nor the device: the tests pin the three to each other.
"""
import numpy as np

from .stack import WTR_NOT_WATER, wtr_spec

SUMMARY_WORDS = 40
OUTPUTS = ('label', 'size', 'sieved', 'summary')
_NONE = np.int64(1) << 40                                # above every index


class Spec:
    """dswx_label_spec_t: connectivity 4 or 8, replace 0 .. 255, min_size >= 1, member_of_byte uint8 [256] (non-zero: member)."""

    def __init__(self, connectivity, min_size, member_of_byte, replace=0):
        self.connectivity, self.min_size, self.replace = int(connectivity), int(min_size), int(replace)
        self.member_of_byte = np.ascontiguousarray(member_of_byte, dtype=np.uint8)
        if self.connectivity not in (4, 8):
            raise ValueError(f'connectivity {self.connectivity}: 4 or 8')
        if not 1 <= self.min_size < 1 << 32:
            raise ValueError(f'min_size {self.min_size} outside 1 .. 2^32 - 1')
        if not 0 <= self.replace <= 255:
            raise ValueError(f'replace {self.replace} outside 0 .. 255')
        if self.member_of_byte.shape != (256,):
            raise ValueError(f'member_of_byte has shape {self.member_of_byte.shape}, not (256,)')


def wtr_label_spec(min_size, connectivity=8, collapsed=True, partial_is_water=True, replace=WTR_NOT_WATER):
    """The spec of a WTR-family layer: the members are the bytes that stack.wtr_spec puts in category 0 (water), so a body is
    a water body; a body of fewer than `min_size` pixels becomes `replace` (not water) in the sieved plane."""
    s = wtr_spec(collapsed=collapsed, partial_is_water=partial_is_water)
    return Spec(connectivity, min_size, (s.cat_of_byte == 0).astype(np.uint8), replace)


def _sweep(v, member, axis_step):
    """One running minimum along a direction (dy, dx) and back, restarting at every non-member: v[p] = min(v[p], v[p - step])
    where both are members, carried as far as the run of members goes.  The carry is a cumulative minimum per line of the
    direction with a segment id that changes at every non-member."""
    dy, dx = axis_step
    T, H, W = v.shape
    out = v
    # lines of the direction: shear the raster so that the direction becomes axis 2
    if dy == 0:
        lines, mem = out, member
    elif dx == 0:
        lines, mem = out.transpose(0, 2, 1), member.transpose(0, 2, 1)
    else:
        # a diagonal: row y is shifted by dx * y, so that (y, x) and (y + 1, x + dx) lie in one column; then columns are lines
        shear = np.full((T, H, W + H - 1), _NONE, dtype=np.int64)
        smem = np.zeros((T, H, W + H - 1), dtype=bool)
        for y in range(H):
            o = (H - 1 - y) if dx > 0 else y
            shear[:, y, o:o + W] = out[:, y]
            smem[:, y, o:o + W] = member[:, y]
        lines, mem = shear.transpose(0, 2, 1), smem.transpose(0, 2, 1)
    lines = np.ascontiguousarray(lines)
    mem = np.ascontiguousarray(mem)
    L = lines.shape[2]
    # the minimum over each run of members of a line, by a segmented reduce: runs are numbered by the non-members before them
    seg = np.cumsum(~mem, axis=2) + (np.arange(lines.shape[0] * lines.shape[1]).reshape(lines.shape[0], lines.shape[1], 1) * (L + 1))
    flat_seg, flat_val, flat_mem = seg.reshape(-1), lines.reshape(-1), mem.reshape(-1)
    best = np.full(int(flat_seg.max()) + 1 if flat_seg.size else 1, _NONE, dtype=np.int64)
    np.minimum.at(best, flat_seg[flat_mem], flat_val[flat_mem])
    res = np.where(flat_mem, best[flat_seg], _NONE).reshape(lines.shape)
    if dy == 0:
        return res
    if dx == 0:
        return res.transpose(0, 2, 1)
    res = res.transpose(0, 2, 1)
    back = np.empty_like(out)
    for y in range(H):
        o = (H - 1 - y) if dx > 0 else y
        back[:, y] = res[:, y, o:o + W]
    return back


def label_tiles(tiles, spec):
    """{'label': uint32 [n, H, W], 'size': uint32 [n, H, W], 'sieved': uint8 [n, H, W], 'summary': uint64 [n, 40]} of a plane
    uint8 [n, H, W]."""
    tiles = np.asarray(tiles)
    if tiles.dtype != np.uint8 or tiles.ndim != 3:
        raise ValueError(f'a plane is uint8 [n_tiles, H, W], not {tiles.dtype} {tiles.shape}')
    n, H, W = tiles.shape
    if H * W > 1 << 31:
        raise ValueError(f'{H} x {W} pixels: at most 2^31, so that a label fits 32 bits')
    member = spec.member_of_byte[tiles] != 0
    v = np.where(member, np.arange(H * W, dtype=np.int64).reshape(1, H, W), _NONE)
    steps = ((0, 1), (1, 0)) + (((1, 1), (1, -1)) if spec.connectivity == 8 else ())
    if n and H and W:
        while True:                                      # a fixed point: the values only fall and are bounded below
            before = v
            for step in steps:
                v = _sweep(v, member, step)
            if np.array_equal(v, before):
                break
    label = np.where(member, v + 1, 0).astype(np.uint32)
    size = np.zeros((n, H, W), dtype=np.uint32)
    for t in range(n):
        counts = np.bincount(label[t].reshape(-1), minlength=1)
        counts[0] = 0
        size[t] = counts[label[t]]
    sieved = np.where(member & (size < spec.min_size), spec.replace, tiles).astype(np.uint8)
    return {'label': label, 'size': size, 'sieved': sieved, 'summary': summary_of(label, size, spec)}


def summary_of(label, size, spec):
    """The summary uint64 [n, 40] from the label and size planes [n, H, W] of label_tiles (or of the library)."""
    label, size = np.asarray(label), np.asarray(size)
    n = label.shape[0]
    out = np.zeros((n, SUMMARY_WORDS), dtype=np.uint64)
    for t in range(n):
        lab, sz = label[t].reshape(-1).astype(np.int64), size[t].reshape(-1).astype(np.int64)
        roots = np.flatnonzero(lab == np.arange(1, lab.size + 1))
        s = sz[roots]
        out[t, 0], out[t, 1] = len(roots), np.count_nonzero(lab)
        if len(roots):
            out[t, 2] = s.max()
            out[t, 3] = lab[roots[np.argmax(s)]]         # argmax returns the FIRST largest: the smallest label
            keep = s >= spec.min_size
            out[t, 4], out[t, 5] = np.count_nonzero(keep), s[keep].sum()
            bins = np.zeros(32, dtype=np.int64)
            for b in range(32):
                bins[b] = np.count_nonzero((s >> b) == 1)
            out[t, 8:40] = bins
    return out
