"""What the outline tests share (tests/test_outline.py on the host, tests/test_gpu_outline.py on the device): member patterns,
the id planes made from them by dswx_label_host with both connectivities, and planes of arbitrary uint32 -- every one legal
input by the definition in include/dswx_hip.h ("outline")."""
import numpy as np

from proteus_amd import _capi
from proteus_amd.outline import Spec
from tests import _body_cases as B
from tests import _label_cases as C

SHAPES = ((1, 1), (1, 7), (7, 1), (2, 3), (33, 129), (64, 64), (65, 130))
GARBAGE_VALUES = np.array([0, 0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)


def frame(H, W):
    """Members on all four borders."""
    m = C.empty(H, W)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


def nested(H, W, depth=4):
    """Rings inside each other with a free ring between them, `depth` deep where the raster has the room."""
    m = C.empty(H, W)
    for k in range(depth):
        o = 2 * k
        if H - 2 * o < 1 or W - 2 * o < 1:
            break
        m[o:H - o, o:W - o] = frame(H - 2 * o, W - 2 * o)
    return m


def patterns(H, W, rng):
    """name -> boolean raster."""
    out = {'empty': C.empty(H, W), 'full': C.full(H, W), 'one_pixel': C.one_pixel(H, W), 'checkerboard': C.checkerboard(H, W),
           'frame': frame(H, W), 'nested': nested(H, W), 'comb': C.serpentine(H, W), 'spiral': C.spiral(H, W)}
    for d in (0.3, 0.5, 0.7):
        out[f'noise_{d}'] = C.noise(H, W, d, rng)
    return out


def garbage(H, W, rng):
    """uint32 [2, H, W]: a few values that meet each other often, among them 0 and 0xFFFFFFFF; and anything at all."""
    return np.stack([rng.choice(GARBAGE_VALUES, size=(H, W)), rng.integers(0, 1 << 32, size=(H, W), dtype=np.uint64).astype(np.uint32)])


def id_planes(H, W, rng):
    """(names, members bool [n, H, W], {4: ids, 8: ids} uint32 [n + 2, H, W]): every pattern labelled by dswx_label_host with
    either connectivity, then the two garbage planes (which have no members)."""
    pats = patterns(H, W, rng)
    members = np.stack(list(pats.values()))
    junk = garbage(H, W, rng)
    return list(pats) + ['garbage_few', 'garbage_any'], members, {c: np.concatenate([B.labels_of(members, rng, c), junk]) for c in (4, 8)}


def edges_of(ids):
    """E per tile of an id plane [n, H, W], counted by four shifted comparisons."""
    ids = np.asarray(ids).astype(np.int64)
    pad = np.pad(ids, ((0, 0), (1, 1), (1, 1)), constant_values=0)
    e = ((pad[:, :-2, 1:-1] != ids).astype(np.int64) + (pad[:, 2:, 1:-1] != ids) + (pad[:, 1:-1, :-2] != ids) + (pad[:, 1:-1, 2:] != ids))
    return (e * (ids != 0)).reshape(len(ids), -1).sum(axis=1)


def full_spec(ids, connectivity):
    """A spec whose capacities hold every tile of `ids` with a row to spare."""
    E = int(edges_of(ids).max()) if len(ids) else 0
    return Spec(E + 3, E // 4 + 1, connectivity)


def isolated(n_pixels, H, W):
    """uint32 [H, W]: `n_pixels` isolated pixels on the even coordinates, each its own id: 4 edges and one ring each."""
    ys, xs = np.nonzero(np.ones(((H + 1) // 2, (W + 1) // 2), dtype=bool))
    assert n_pixels <= len(ys)
    ids = np.zeros((H, W), dtype=np.uint32)
    ids[2 * ys[:n_pixels], 2 * xs[:n_pixels]] = 2 * ys[:n_pixels] * W + 2 * xs[:n_pixels] + 1
    return ids


def host(ids, spec, want=('chain', 'rings', 'head')):
    return _capi.outline_host(ids, spec, want)
