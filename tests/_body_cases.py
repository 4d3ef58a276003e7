"""What the body-table tests share (tests/test_body_table.py on the host, tests/test_gpu_body_table.py on the device): label
planes made by dswx_label_host from the patterns of tests/_label_cases.py, value planes and category tables, and the
MALFORMED label planes -- every one legal input by the definition in include/dswx_hip.h ("body table")."""
import numpy as np

from proteus_amd import _capi
from proteus_amd.bodies import Spec
from proteus_amd.label import Spec as LabelSpec
from tests import _label_cases as C

VALUE_BYTES = np.array([0, 1, 2, 3, 7, 128, 253, 254, 255], dtype=np.uint8)
PAD_VALUE = 1                                      # a COUNTED byte of every table below: padding that was read would be counted


def labels_of(members, rng, connectivity):
    """uint32 [n, H, W]: the label plane of dswx_label_host for boolean rasters [n, H, W]."""
    plane, table = C.plane_of(np.asarray(members), rng)
    return _capi.label_host(plane, LabelSpec(connectivity, 1, table), want=('label',))['label']


def pattern_labels(H, W, rng, connectivity, extra_noise=False):
    members = list(C.patterns(H, W, rng).values())
    if extra_noise:
        members.append(C.noise(H, W, 0.6, rng))
    return labels_of(np.stack(members), rng, connectivity)


def cat_table(n_cats):
    """A table that uses bytes 0, 1, 254 and 255 and has "not counted" values: entries n_cats .. 255 are not counted."""
    cat = np.full(256, 255, dtype=np.uint8)
    cat[0], cat[1], cat[254], cat[255] = 3, 0, 1, 2
    cat[2], cat[3], cat[7] = 0, n_cats, 4          # (n_cats: the first value that is not counted)
    return cat


def spec_of(n_cats, max_rows):
    return Spec(n_cats, cat_table(n_cats) if n_cats else None, max_rows)


def value_like(label, rng):
    return rng.choice(VALUE_BYTES, size=label.shape).astype(np.uint8)


def bodies_of(label):
    """K per tile of a label plane [n, H, W]."""
    n = label.shape[0]
    flat = label.reshape(n, -1)
    return (flat == np.arange(1, flat.shape[1] + 1, dtype=np.uint64)).sum(axis=1)


def malformed_tiny(H, W):
    """uint32 [H, W] for a raster too small for `malformed` (6 pixels are enough): a root with one follower, a label above
    the tile, a label above idx + 1 that names a later NON-member, a second root and a non-member."""
    N = H * W
    assert N >= 6
    a = np.zeros(N, dtype=np.uint32)
    a[:5] = (1, 1, N + 3, N, 5)
    return a.reshape(H, W)


def malformed(H, W, rng):
    """name -> uint32 [H, W]: a labelled noise raster with pixels that are malformed in one way each.  Needs bodies of more
    than one pixel and some non-members: H * W >= 64."""
    N = H * W
    base = labels_of(C.noise(H, W, 0.5, rng)[None], rng, 4)[0].reshape(-1)
    idx = np.arange(N)
    roots = np.flatnonzero(base == idx + 1)
    followers = np.flatnonzero((base != 0) & (base != idx + 1))
    outside = np.flatnonzero(base == 0)
    assert len(roots) > 4 and len(followers) > 8 and len(outside) > 8
    out = {}
    a = base.copy()                                   # a label above height * width: the bound, nothing is read
    a[rng.choice(N, 6, replace=False)] = (N + 1, N + 5, 1 << 31, (1 << 31) + 1, 0xFFFFFFFE, 0xFFFFFFFF)
    out['above_the_tile'] = a
    a = base.copy()                                   # a label above idx + 1, inside the tile: names a LATER pixel
    for p in rng.choice(N - 2, 8, replace=False):
        a[p] = p + 2 + rng.integers(0, N - p - 1)
    a[roots[1] - 1] = roots[1] + 1                    # ... which is a root, and the pixel before it the same VALUE as it
    out['above_idx'] = a
    a = base.copy()                                   # a label whose target is a member but not a root
    for p in followers[-6:]:
        q = followers[followers < p][0] if np.any(followers < p) else None
        if q is not None:
            a[p] = q + 1
    out['target_not_a_root'] = a
    a = base.copy()                                   # a label that points at a non-member
    for p in rng.choice(np.arange(outside[0] + 1, N), 8, replace=False):
        a[p] = outside[0] + 1
    out['target_not_a_member'] = a
    a = base.copy()                                   # the plane of the label entry with one root zeroed
    sizes = np.bincount(base, minlength=N + 1)
    big = roots[np.argmax(sizes[roots + 1])]
    assert sizes[big + 1] > 1
    a[big] = 0
    out['one_root_zeroed'] = a
    return {k: v.astype(np.uint32).reshape(H, W) for k, v in out.items()}
