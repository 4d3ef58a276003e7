"""The member patterns that the label tests share (tests/test_label.py on the host, tests/test_gpu_label.py on the device):
each is a boolean raster [H, W]; `plane_of` turns a stack of them into a uint8 plane and a member table."""
import numpy as np

DENSITIES = (0.1, 0.5, 0.593, 0.9)                # 0.593: the site-percolation threshold of the square lattice, the longest bodies


def empty(H, W):
    return np.zeros((H, W), dtype=bool)


def full(H, W):
    return np.ones((H, W), dtype=bool)


def one_pixel(H, W):
    m = empty(H, W)
    m[H // 2, W // 2] = True
    return m


def checkerboard(H, W):
    """Every member its own body at connectivity 4, ONE body at connectivity 8."""
    y, x = np.indices((H, W))
    return (y + x) % 2 == 0


def diagonals(H, W, slope):
    """Lines of slope +1 or -1, three pixels apart: one body per line at 8, one per pixel at 4."""
    y, x = np.indices((H, W))
    return (x - slope * y) % 3 == 0


def spiral(H, W):
    """A one-pixel-wide spiral that fills the raster, walked from the top left corner inwards with a free ring between its
    turns: ONE body, the longest path."""
    m = empty(H, W)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    while True:
        for _ in range(2):                        # straight on, else one turn to the right; neither: the walk is over
            ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(ay, ax) and m[ay, ax]):
                y, x = ny, nx
                m[y, x] = True
                break
            dy, dx = dx, -dy
        else:
            return m


def serpentine(H, W):
    """A comb: every other row is full, joined to the next full row alternately at the right and the left end: ONE body
    whose path runs through every member."""
    m = empty(H, W)
    m[0::2] = True
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def corner_touch(H, W):
    """Two blocks that touch only at a corner: one body at 8, two at 4."""
    m = empty(H, W)
    cy, cx = max(H // 2, 1), max(W // 2, 1)
    m[:cy, :cx] = True
    m[cy:, cx:] = True
    return m


def row_wrap(H, W):
    """Members in the last column of row y and the first column of row y + 1 only, every third row: consecutive indices that
    are NOT neighbours (for W >= 3: two bodies per pair)."""
    m = empty(H, W)
    for y in range(0, H, 3):
        m[y, W - 1] = True
        if y + 1 < H:
            m[y + 1, 0] = True
    return m


def noise(H, W, density, rng):
    return rng.random((H, W)) < density


def patterns(H, W, rng):
    """name -> raster, the whole list at one shape."""
    out = {'empty': empty(H, W), 'full': full(H, W), 'one_pixel': one_pixel(H, W), 'checkerboard': checkerboard(H, W),
           'diagonal_down': diagonals(H, W, 1), 'diagonal_up': diagonals(H, W, -1), 'spiral': spiral(H, W),
           'serpentine': serpentine(H, W), 'corner_touch': corner_touch(H, W), 'row_wrap': row_wrap(H, W)}
    for d in DENSITIES:
        out[f'noise_{d}'] = noise(H, W, d, rng)
    return out


GRID_Y = 65535                                    # the blocks of grid.y: a workgroup of the tile-loop kernels walks on to tile blockIdx.y + 65535
EARLY = ('full', 'noise 0.9', 'checkerboard', 'serpentine')
LATE = ('empty', 'one_pixel', 'noise 0.1', 'row_wrap')


def second_pass_members(H, W, rng):
    """bool [65535 + 4, H, W] for the calls in which the workgroups of tiles 0 .. 3 do a second tile with the LDS, the
    barriers and the wave-wide state of the first: tiles 0 .. 3 are EARLY (dense), tiles 65535 .. 65538 LATE (sparse, so that
    anything left behind shows), every other tile noise at the densities of DENSITIES in turn."""
    T = GRID_Y + 4
    density = np.array(DENSITIES)[np.arange(T) % len(DENSITIES)]
    m = rng.random((T, H, W)) < density[:, None, None]
    m[:4] = np.stack([full(H, W), noise(H, W, 0.9, rng), checkerboard(H, W), serpentine(H, W)])
    m[GRID_Y:] = np.stack([empty(H, W), one_pixel(H, W), noise(H, W, 0.1, rng), row_wrap(H, W)])
    for i in range(4):
        assert not np.array_equal(m[GRID_Y + i], m[i]), (LATE[i], EARLY[i])
    return m


def plane_of(members, rng, only_255=False):
    """A uint8 plane of the shape of `members` and a member table: member bytes and non-member bytes are drawn from several
    values each (or, with only_255, byte 255 alone is a member), so that the table is exercised and `sieved` has bytes to
    copy."""
    table = np.zeros(256, dtype=np.uint8)
    if only_255:
        table[255] = 1
        yes, no = np.array([255], dtype=np.uint8), np.arange(255, dtype=np.uint8)
    else:
        yes = np.array([1, 2, 31, 32, 200], dtype=np.uint8)
        table[yes] = (1, 1, 7, 255, 128)
        no = np.array([0, 3, 33, 252, 253, 254, 255], dtype=np.uint8)
    members = np.asarray(members, dtype=bool)
    plane = np.where(members, rng.choice(yes, size=members.shape), rng.choice(no, size=members.shape)).astype(np.uint8)
    return plane, table
