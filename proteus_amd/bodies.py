"""The body table of a label plane, include/dswx_hip.h ("body table"), stated in numpy.

`label` is uint32 [n_tiles, H, W] as the label entries leave it: 0 for a non-member, else 1 + the smallest pixel index
y * W + x of the body.  `value` is an optional uint8 plane of the same shape.  A non-zero pixel p with L = label[p] is
well-formed iff L <= idx(p) + 1 and label[L - 1] == L; every other non-zero pixel is malformed, belongs to no body and is only
counted in the head.  The roots are the pixels with label[p] == idx(p) + 1, K their number, rank(r) the roots before r.

    dense[p]  0 for label 0 or a malformed pixel, else 1 + rank(label[p] - 1): scipy.ndimage.label's own array     uint32
    rows      ROW_DTYPE [n_tiles, max_rows]: row k is the body with dense == k + 1 for k < min(K, max_rows), the
              rest zero
    head      K, min(K, max_rows), well-formed pixels, malformed pixels, the perimeters of all K bodies, 0, 0, 0     uint64

The statement sorts nothing and walks nothing: ranks are a cumulative sum over the root mask, every column of the table a
np.bincount over the dense plane (np.minimum.at / np.maximum.at for the box).  It calls neither dswx_body_table_host nor the
device: the tests pin the three to each other, and to scipy.ndimage.
"""
import numpy as np

ROW_WORDS, HEAD_WORDS, MAX_CATS = 16, 8, 4
OUTPUTS = ('dense', 'rows', 'head')
ROW_DTYPE = np.dtype([('label', '<u4'), ('area', '<u4'), ('x_min', '<u4'), ('x_max', '<u4'), ('y_min', '<u4'), ('y_max', '<u4'),
                      ('perimeter', '<u8'), ('sum_x', '<u8'), ('sum_y', '<u8'), ('count', '<u4', (MAX_CATS,))])
assert ROW_DTYPE.itemsize == ROW_WORDS * 4


class Spec:
    """dswx_body_spec_t: n_cats 0 .. 4, cat_of_byte uint8 [256] (a value >= n_cats: the byte is not counted; None with
    n_cats 0), max_rows 0 .. 2^31 (the capacity of the table per tile)."""

    def __init__(self, n_cats, cat_of_byte, max_rows):
        self.n_cats, self.max_rows = int(n_cats), int(max_rows)
        self.cat_of_byte = np.ascontiguousarray(np.full(256, 255) if cat_of_byte is None else cat_of_byte, dtype=np.uint8)
        if not 0 <= self.n_cats <= MAX_CATS:
            raise ValueError(f'n_cats {self.n_cats} outside 0 .. {MAX_CATS}')
        if not 0 <= self.max_rows <= 1 << 31:
            raise ValueError(f'max_rows {self.max_rows} outside 0 .. 2^31')
        if self.cat_of_byte.shape != (256,):
            raise ValueError(f'cat_of_byte has shape {self.cat_of_byte.shape}, not (256,)')


def wtr_body_spec(max_rows, collapsed=True):
    """The spec for a WTR-family layer as `value`: byte 1 (open water) is category 0 and byte 2 (partial surface water)
    category 1; with collapsed=False the uncollapsed layer's bytes 1 and 2 (high- and moderate-confidence open water) are
    category 0 and 3 and 4 (the partial classes) category 1.  Everything else is not counted.  A WTR plane of ANOTHER date
    with stack.wtr_spec's table (Spec(2, stack.wtr_spec().cat_of_byte, max_rows): water / clear and not water) is an equally
    valid `value`: the table then says how much of each body was water or dry on that date, and area minus the two counts
    how much of it was masked."""
    cat = np.full(256, 255, dtype=np.uint8)
    if collapsed:
        cat[1], cat[2] = 0, 1
    else:
        cat[[1, 2]], cat[[3, 4]] = 0, 1
    return Spec(2, cat, max_rows)


def body_table(label, value, spec):
    """{'dense': uint32 [n, H, W], 'rows': ROW_DTYPE [n, max_rows], 'head': uint64 [n, 8]} of a label plane uint32 [n, H, W]
    and a value plane uint8 [n, H, W] (None iff spec.n_cats == 0)."""
    label = np.asarray(label)
    if label.dtype != np.uint32 or label.ndim != 3:
        raise ValueError(f'a label plane is uint32 [n_tiles, H, W], not {label.dtype} {label.shape}')
    if (value is None) != (spec.n_cats == 0):
        raise ValueError('value is None if and only if n_cats is 0')
    if value is not None:
        value = np.asarray(value)
        if value.dtype != np.uint8 or value.shape != label.shape:
            raise ValueError(f'a value plane is uint8 {label.shape}, not {value.dtype} {value.shape}')
    n, H, W = label.shape
    N = H * W
    if N > 1 << 31:
        raise ValueError(f'{H} x {W} pixels: at most 2^31')
    dense = np.zeros((n, H, W), dtype=np.uint32)
    rows = np.zeros((n, spec.max_rows), dtype=ROW_DTYPE)
    head = np.zeros((n, HEAD_WORDS), dtype=np.uint64)
    if N == 0:
        return {'dense': dense, 'rows': rows, 'head': head}
    idx = np.arange(N, dtype=np.int64)
    ys, xs = idx // W, idx % W
    for t in range(n):
        lab = label[t].reshape(-1).astype(np.int64)
        root = lab == idx + 1
        K = int(root.sum())
        rank1 = np.cumsum(root)                              # at a root: 1 + its rank
        reach = (lab != 0) & (lab <= idx + 1)
        target = np.where(reach, lab - 1, 0)                 # (looked at only where `reach`)
        good = reach & (lab[target] == lab)
        d = np.where(good, rank1[target], 0)
        dense[t] = d.reshape(H, W)
        # the edges of every pixel: a neighbour outside the tile or with another label VALUE
        grid = np.zeros((H + 2, W + 2), dtype=np.int64)
        grid[1:-1, 1:-1] = lab.reshape(H, W)
        inner = grid[1:-1, 1:-1]
        edges = ((grid[:-2, 1:-1] != inner).astype(np.int64) + (grid[2:, 1:-1] != inner) + (grid[1:-1, :-2] != inner) +
                 (grid[1:-1, 2:] != inner)).reshape(-1)
        head[t, :5] = K, min(K, spec.max_rows), np.count_nonzero(good), np.count_nonzero((lab != 0) & ~good), edges[good].sum()
        R = min(K, spec.max_rows)
        if R == 0:
            continue
        keep = good & (d <= R)
        b, x, y = d[keep] - 1, xs[keep], ys[keep]
        r = rows[t, :R]
        r['label'] = np.flatnonzero(root)[:R] + 1
        r['area'] = np.bincount(b, minlength=R)
        r['perimeter'] = np.bincount(b, weights=edges[keep], minlength=R).astype(np.uint64)
        # (weights are float64: exact below 2^53, which a tile of 2^31 pixels with coordinates below 2^31 can pass; the
        # sums are therefore taken in two halves of the coordinate, each exact)
        for name, c in (('sum_x', x), ('sum_y', y)):
            lo = np.bincount(b, weights=c & 0xFFFF, minlength=R).astype(np.uint64)
            hi = np.bincount(b, weights=c >> 16, minlength=R).astype(np.uint64)
            r[name] = lo + (hi << np.uint64(16))
        for name, c, fn, start in (('x_min', x, np.minimum, N), ('x_max', x, np.maximum, 0), ('y_min', y, np.minimum, N),
                                   ('y_max', y, np.maximum, 0)):
            acc = np.full(R, start, dtype=np.int64)
            fn.at(acc, b, c)
            r[name] = acc
        if value is not None:
            cat = spec.cat_of_byte[value[t].reshape(-1)[keep]]
            for c in range(spec.n_cats):
                r['count'][:, c] = np.bincount(b[cat == c], minlength=R)
    return {'dense': dense, 'rows': rows, 'head': head}
