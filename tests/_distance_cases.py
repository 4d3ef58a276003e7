"""The target patterns that the distance tests share (tests/test_distance.py on the host, tests/test_gpu_distance.py on the
device): each is a boolean raster [H, W]; `plane_of` turns a stack of them into a uint8 plane and a target table."""
import numpy as np

DENSITIES = (0.5, 0.05, 0.002)


def empty(H, W):
    return np.zeros((H, W), dtype=bool)


def full(H, W):
    return np.ones((H, W), dtype=bool)


def one_at(H, W, y, x):
    m = empty(H, W)
    m[y, x] = True
    return m


def full_row(H, W):
    m = empty(H, W)
    m[(2 * H) // 3] = True
    return m


def full_column(H, W):
    m = empty(H, W)
    m[:, W // 3] = True
    return m


def diagonal(H, W):
    y, x = np.indices((H, W))
    return y == x


def two_equidistant(H, W):
    """Two targets in one row, an even number of columns apart where the width allows, and the same two columns in the last
    row: every pixel of the column between them, and every pixel of a row half way down, is equally far from two targets, so
    `nearest` is decided by the tie rule alone (the smaller column, then the smaller row)."""
    m = empty(H, W)
    a, b = 0, (W - 1) - (W - 1) % 2
    m[0, a] = m[0, b] = True
    m[H - 1, a] = m[H - 1, b] = True
    return m


def checkerboard(H, W):
    y, x = np.indices((H, W))
    return (y + x) % 2 == 0


def noise(H, W, density, rng):
    return rng.random((H, W)) < density


def patterns(H, W, rng):
    """name -> raster, the whole list at one shape."""
    out = {'empty': empty(H, W), 'full': full(H, W), 'top_left': one_at(H, W, 0, 0), 'top_right': one_at(H, W, 0, W - 1),
           'bottom_left': one_at(H, W, H - 1, 0), 'bottom_right': one_at(H, W, H - 1, W - 1),      # the last row and column
           'centre': one_at(H, W, H // 2, W // 2), 'full_row': full_row(H, W), 'full_column': full_column(H, W),
           'diagonal': diagonal(H, W), 'two_equidistant': two_equidistant(H, W), 'checkerboard': checkerboard(H, W)}
    for d in DENSITIES:
        out[f'noise_{d}'] = noise(H, W, d, rng)
    return out


GRID_Y = 65535                                    # the blocks of grid.y: a workgroup walks on to tile blockIdx.y + 65535


def second_pass_targets(H, W, rng):
    """bool [65535 + 4, H, W]: tiles 0 .. 3 dense (full, noise 0.9, checkerboard, a full row), tiles 65535 .. 65538 sparse
    (empty, one corner, noise 0.1, the last pixel), so that anything a workgroup leaves behind for its second tile shows;
    every other tile noise at densities 0.6, 0.2, 0.05 and 0 in turn."""
    T = GRID_Y + 4
    density = np.array((0.6, 0.2, 0.05, 0.0))[np.arange(T) % 4]
    m = rng.random((T, H, W)) < density[:, None, None]
    m[:4] = np.stack([full(H, W), noise(H, W, 0.9, rng), checkerboard(H, W), full_row(H, W)])
    m[GRID_Y:] = np.stack([empty(H, W), one_at(H, W, 0, 0), noise(H, W, 0.1, rng), one_at(H, W, H - 1, W - 1)])
    return m


TARGET_BYTES = (1, 2, 31, 32, 200)                # 200 is also the byte of every padding and guard in the device tests
OTHER_BYTES = (0, 3, 33, 252, 253, 254, 255)


def plane_of(targets, rng, only_255=False):
    """A uint8 plane of the shape of `targets` and a target table: target bytes and the other bytes are drawn from several
    values each (or, with only_255, byte 255 alone is a target), so that the table is exercised and `within` has bytes to
    copy."""
    table = np.zeros(256, dtype=np.uint8)
    if only_255:
        table[255] = 1
        yes, no = np.array([255], dtype=np.uint8), np.arange(255, dtype=np.uint8)
    else:
        yes = np.array(TARGET_BYTES, dtype=np.uint8)
        table[yes] = (1, 1, 7, 255, 128)
        no = np.array(OTHER_BYTES, dtype=np.uint8)
    targets = np.asarray(targets, dtype=bool)
    plane = np.where(targets, rng.choice(yes, size=targets.shape), rng.choice(no, size=targets.shape)).astype(np.uint8)
    return plane, table
