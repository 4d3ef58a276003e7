"""The resample definition (include/dswx_hip.h "resample") on the CPU: dswx_resample_host, proteus_amd.resample.resample_tiles and a
per-pixel loop in plain Python floats (IEEE doubles: the same operation sequence by construction) are pinned to each other BIT
FOR BIT on dst, how and head -- both kinds, both methods, every mesh content of tests/test_warp.py, shifts 0, 1, 4, 8, sources
from empty to many cells; the loop's result is pinned to the EXACT rational value of the rule (fractions.Fraction) within
8 * 2^-53 * sum |w p|, and the stored element to the correct rounding of that double.  Closed forms (polynomials of degree 2,
the identity, the weights), every kind of invalid tap, scipy's bilinear, every refusal, the struct mirrors, and the geographic
mesh of proteus_amd.warp."""
import ctypes
import itertools
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from proteus_amd import _capi, resample, warp
from proteus_amd.resample import BILINEAR, CUBIC, Spec, outside_word, resample_tiles
from proteus_amd.warp import mesh_shape
from tests.test_warp import MESHES, exact_mesh, loop_positions, make_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = (0, 1, 4, 8)
SRCS = ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 3), (64, 80))
SMALL_DSTS = ((1, 1), (1, 17), (17, 1), (9, 13))
BIG_DST = (33, 47)
KINDS = (np.float32, np.int16)
OUTSIDE = {np.float32: -12345.5, np.int16: -321}
NODATA = {np.float32: -9999.0, np.int16: 7}
U = Fraction(1, 1 << 53)
WEIGHTS = resample.weights().tolist()


def random_tiles(rng, n, src, dtype, special=True):
    """[n, H, W] of the dtype: float32 over many binades with NaN, infinities, the nodata value, subnormals and FLT_MAX
    sprinkled in; int16 over its whole range with the nodata value and both ends."""
    size = n * src[0] * src[1]
    if dtype == np.float32:
        t = (rng.normal(0.0, 1.0, size) * 10.0 ** rng.integers(-3, 5, size)).astype(np.float32)
        marks = (np.nan, np.inf, -np.inf, NODATA[np.float32], 1e-45, -3e-39, np.finfo(np.float32).max, -np.finfo(np.float32).max, 0.0)
    else:
        t = rng.integers(-32768, 32768, size).astype(np.int16)
        marks = (NODATA[np.int16], 32767, -32768, -32767, 0)
    if special and size:
        for m in marks:
            t[rng.integers(0, size, max(size // 40, 1))] = m
    return t.reshape((n,) + src)


def loop_pixel(rows, fracs, H, W, sx, sy, cubic, nodata):
    """(how, result as a Python float, exact Fraction, sum |w p| as a Fraction, rlo, rhi) of one pixel: the rule as written."""
    ux, uy = sx - 128, sy - 128
    c0, r0, fx, fy = ux >> 8, uy >> 8, ux & 255, uy & 255

    def valid(c, r):
        if not (0 <= c < W and 0 <= r < H):
            return False
        v = rows[r][c]
        return math.isfinite(v) and not (nodata is not None and v == nodata)

    if cubic and all(valid(c0 - 1 + c, r0 - 1 + r) for r in range(4) for c in range(4)):
        nx, ny = WEIGHTS[fx], WEIGHTS[fy]
        p = [[float(rows[r0 - 1 + r][c0 - 1 + c]) for c in range(4)] for r in range(4)]
        h = [((float(nx[0]) * p[r][0] + float(nx[1]) * p[r][1]) + float(nx[2]) * p[r][2]) + float(nx[3]) * p[r][3] for r in range(4)]
        v = (((float(ny[0]) * h[0] + float(ny[1]) * h[1]) + float(ny[2]) * h[2]) + float(ny[3]) * h[3]) * 2.0 ** -50
        q = [[fracs[r0 - 1 + r][c0 - 1 + c] for c in range(4)] for r in range(4)]
        exact = sum(ny[r] * nx[c] * q[r][c] for r in range(4) for c in range(4)) / (1 << 50)
        mass = sum(abs(ny[r] * nx[c] * q[r][c]) for r in range(4) for c in range(4)) / (1 << 50)
        return 3, v, exact, mass, r0 - 1, r0 + 2
    S, Wt, n, exact, mass, rlo, rhi = 0.0, 0, 0, Fraction(0), Fraction(0), r0 + 1, r0
    for k, w in enumerate(((256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy)):
        c, r = c0 + (k & 1), r0 + (k >> 1)
        if valid(c, r):
            S = S + float(w) * float(rows[r][c])
            Wt += w
            n += 1
            exact += w * fracs[r][c]
            mass += abs(w * fracs[r][c])
            rlo, rhi = min(rlo, r), max(rhi, r)
    if Wt == 0:
        return 0, 0.0, Fraction(0), Fraction(0), None, None
    return (1 if n == 4 else 2), (S * 2.0 ** -16 if Wt == 65536 else S / float(Wt)), exact / Wt, mass / Wt, rlo, rhi


def element_of(v, dtype):
    """The correct rounding of the double `v` to an element, from the exact value of v -- not through numpy's conversion."""
    if dtype == np.int16:
        return max(-32768, min(32767, round(Fraction(v))))                # round(Fraction) is half to even
    with np.errstate(over='ignore'):
        f = np.float32(v)
    if np.isfinite(f):
        mine = abs(Fraction(float(f)) - Fraction(v))
        with np.errstate(over='ignore'):
            others = (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)))
        for other in others:
            if np.isfinite(other):
                far = abs(Fraction(float(other)) - Fraction(v))
                assert mine < far or (mine == far and int(f.view(np.uint32)) % 2 == 0), (v, f, other)
    else:
        assert abs(v) >= float(np.finfo(np.float32).max) * (1 + 2.0 ** -25)
    return f


def loop_resample(tile, pos, dst, cubic, nodata, fill, pin=True):
    """(dst, how, head) of ONE tile [H, W] from loop_positions, in Python floats; with `pin`, every result is held against the
    exact rational value of the rule."""
    H, W = tile.shape
    rows = tile.tolist()
    fracs = [[Fraction(v) if math.isfinite(v) else None for v in row] for row in rows] if pin else rows
    if tile.dtype == np.float32 and nodata is not None:
        nodata = float(np.float32(nodata))
    d, hw = [], []
    counts, rmin, rmax = [0, 0, 0, 0], H, 0
    for sx, sy in pos:
        how, v, exact, mass, rlo, rhi = loop_pixel(rows, fracs, H, W, sx, sy, cubic, nodata)
        counts[how] += 1
        hw.append(how)
        if how == 0:
            d.append(fill)
            continue
        if pin:
            assert abs(Fraction(v) - exact) <= 8 * U * mass, (sx, sy, how, v, float(exact))
        d.append(element_of(v, tile.dtype.type) if pin else v)
        rmin, rmax = min(rmin, rlo), max(rmax, rhi)
    n = dst[0] * dst[1]
    with np.errstate(over='ignore'):
        out = np.array(d, dtype=tile.dtype).reshape(dst)
    return out, np.array(hw, dtype=np.uint8).reshape(dst), np.array([n, counts[3], counts[1], counts[2], counts[0], rmin, rmax, 0], dtype=np.uint64)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def fill_of(dtype):
    return np.array([OUTSIDE[dtype]], dtype=dtype)[0]


@pytest.mark.parametrize('shift', SHIFTS)
@pytest.mark.parametrize('method', (BILINEAR, CUBIC))
@pytest.mark.parametrize('dtype', KINDS)
def test_host_numpy_and_python_float_loop_agree_and_the_exact_pin(dtype, method, shift):
    """Every mesh content x every source for this kind, method and shift: the three statements bit for bit, the loop's doubles
    within 8 * 2^-53 * sum |w p| of the exact rational value, the element the correct rounding of the double."""
    rng = np.random.default_rng(100 * shift + 10 * method + (dtype == np.int16))
    word = outside_word(OUTSIDE[dtype], dtype)
    seen = np.zeros(4, dtype=np.int64)
    for src in SRCS:
        for dst in SMALL_DSTS + ((BIG_DST,) if src == SRCS[-1] else ()):
            tiles = random_tiles(rng, 2, src, dtype)
            for kind in MESHES:
                mesh = make_mesh(kind, dst, shift, src, rng)
                nodata = NODATA[dtype] if len(kind) % 2 else None
                ref = resample_tiles(tiles, mesh, shift, dst, method, nodata=nodata, outside=word)
                got = _capi.resample_host(tiles, mesh, Spec(dtype, method, shift, nodata, word), dst)
                for k in resample.OUTPUTS:
                    assert same_bits(got[k], ref[k]), (kind, src, dst, k)
                pos = loop_positions(mesh, shift, dst)
                for t in range(2):
                    d, how, head = loop_resample(tiles[t], pos, dst, method == CUBIC, nodata, fill_of(dtype))
                    assert same_bits(ref['dst'][t], d) and same_bits(ref['how'][t], how) and same_bits(ref['head'][t], head), (kind, src, dst, t)
                    seen += np.bincount(how.reshape(-1), minlength=4)
    assert seen[0] and seen[1] and seen[2] and (seen[3] > 0) == (method == CUBIC), seen
    # a mesh per tile with nodes between the meshes, and a plane with elements between the tiles
    src, dst, n = SRCS[-1], (9, 13), 3
    mh, mw = mesh_shape(dst, shift)
    tiles = random_tiles(rng, n, src, dtype)
    kinds = [MESHES[(k + shift) % len(MESHES)] for k in range(n)]
    meshes = [make_mesh(k, dst, shift, src, rng) for k in kinds]
    nodes, stride = mh * mw + 5, src[0] * src[1] + 7
    per_tile = rng.integers(-(1 << 31), 1 << 31, size=(n, nodes, 2), dtype=np.int64).astype(np.int32)
    for t in range(n):
        per_tile[t, :mh * mw] = meshes[t].reshape(-1, 2)
    padded = random_tiles(rng, n, (1, stride), dtype).reshape(n, stride)
    padded[:, :src[0] * src[1]] = tiles.reshape(n, -1)
    got = _capi.resample_host(padded, per_tile, Spec(dtype, method, shift, None, word, src_tile_stride=stride, mesh_tile_stride_nodes=nodes), dst, raster=src)
    ref = resample_tiles(tiles, np.stack(meshes), shift, dst, method, outside=word)
    for k in resample.OUTPUTS:
        assert same_bits(got[k], ref[k]), ('per tile', k)


def test_the_4x4_source_has_one_base_pixel_with_a_full_cubic_window():
    tiles = np.arange(16, dtype=np.float32).reshape(1, 4, 4)
    mesh = exact_mesh((4, 4), 0, lambda X, Y: X, lambda X, Y: Y)
    got = _capi.resample_host(tiles, mesh, Spec(np.float32, CUBIC, 0), (4, 4))
    assert (got['how'][0] == 3).sum() == 1 and got['how'][0, 1, 1] == 3 and got['head'][0].tolist() == [16, 1, 8, 7, 0, 0, 3, 0]


def fine_mesh(n, start_x, start_y):
    """Shift 8, one cell: the position advances 257/256 pixel per destination pixel over n = 256 pixels along both axes, so the
    fractions visit all 256 values."""
    mesh = np.zeros((2, 2, 2), dtype=np.int32)
    for i in range(2):
        for j in range(2):
            mesh[i, j] = (start_x + 257 * 256 * j, start_y + 257 * 256 * i)
    return mesh


@pytest.mark.parametrize('method', (BILINEAR, CUBIC))
def test_polynomials_of_degree_two_are_reproduced(method):
    """p(c, r) = a + b c + d r + e c^2 + g c r + k r^2 with small integer coefficients (exact in float32) under a mesh that
    visits all 256 values of fx and of fy: CUBIC returns p at the quantised position within the bound of the exact pin;
    BILINEAR does for e = k = 0."""
    H = W = 270
    c, r = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    a, b, d, e, g, k = 3, -2, 5, (1 if method == CUBIC else 0), -1, (2 if method == CUBIC else 0)
    plane = a + b * c + d * r + e * c * c + g * c * r + k * r * r
    assert np.abs(plane).max() < 1 << 24
    tiles = plane.astype(np.float32)[None]
    mesh = fine_mesh(256, 256 * 2 + 128, 256 * 3 + 128)
    got = _capi.resample_host(tiles, mesh, Spec(np.float32, method, 8), (256, 256), want=('dst', 'how'))
    sx, sy = warp.positions(mesh, 8, (256, 256))
    assert set(((sx - 128) & 255).reshape(-1).tolist()) == set(range(256)) and set(((sy - 128) & 255).reshape(-1).tolist()) == set(range(256))
    assert np.all(got['how'] == (3 if method == CUBIC else 1))
    rows = tiles[0].tolist()
    fracs = [[Fraction(v) for v in row] for row in rows]
    for Y in range(256):                                                  # every fy; every fx over five consecutive rows
        for X in range(Y % 5, 256, 5):
            x, y = Fraction(int(sx[Y, X]) - 128, 256), Fraction(int(sy[Y, X]) - 128, 256)
            want = a + b * x + d * y + e * x * x + g * x * y + k * y * y
            _, v, exact, mass, _, _ = loop_pixel(rows, fracs, H, W, int(sx[Y, X]), int(sy[Y, X]), method == CUBIC, None)
            assert exact == want, (X, Y)                                  # the weights reproduce the polynomial EXACTLY
            assert abs(Fraction(v) - want) <= 8 * U * mass
            assert got['dst'][0, Y, X] == np.float32(v)


@pytest.mark.parametrize('dtype', KINDS)
@pytest.mark.parametrize('method', (BILINEAR, CUBIC))
def test_the_identity_mesh_returns_the_source(dtype, method):
    rng = np.random.default_rng(5)
    H, W = 23, 31
    tiles = random_tiles(rng, 2, (H, W), dtype, special=False)
    for shift in SHIFTS:
        got = _capi.resample_host(tiles, exact_mesh((H, W), shift, lambda X, Y: X, lambda X, Y: Y), Spec(dtype, method, shift), (H, W))
        assert same_bits(got['dst'], tiles)
        if method == CUBIC:
            assert np.all(got['how'][:, 1:H - 2, 1:W - 2] == 3) and np.all(got['how'][:, 0] != 3)
        assert np.all(got['how'][:, :H - 1, :W - 1] != 0)


def test_weights():
    n = resample.weights()
    assert n.shape == (256, 4) and n.dtype == np.int64
    assert np.all(n.sum(axis=1) == 1 << 25) and np.abs(n).max() <= 1 << 25
    assert n[0].tolist() == [0, 1 << 25, 0, 0]
    for f in range(1, 256):
        assert [n[f, k] for k in range(4)] == [n[256 - f, 3 - k] for k in range(4)]       # N_k(f) = N_{3-k}(256 - f)
    a = Fraction(-1, 2)
    for f in range(256):
        t = Fraction(f, 256)
        keys = lambda x: (a + 2) * abs(x) ** 3 - (a + 3) * abs(x) ** 2 + 1 if abs(x) <= 1 else a * abs(x) ** 3 - 5 * a * abs(x) ** 2 + 8 * a * abs(x) - 4 * a
        assert [Fraction(int(v), 1 << 25) for v in n[f]] == [keys(t + 1), keys(t), keys(1 - t), keys(2 - t)]
    # they reproduce 1, x and x^2 about the base pixel
    for f in range(256):
        t = Fraction(f, 256)
        for power in range(3):
            assert sum(int(n[f, k]) * Fraction(k - 1) ** power for k in range(4)) == (1 << 25) * t ** power


def centred(H, W, dx=0, dy=0):
    """Shift 0 mesh: destination pixel (X, Y) samples the source at pixel centre (X, Y) + (dx, dy) / 256."""
    X, Y = np.meshgrid(np.arange(W + 1, dtype=np.int64), np.arange(H + 1, dtype=np.int64))    # (shift 0: a node per pixel and one more)
    return np.stack([256 * X + 128 + dx, 256 * Y + 128 + dy], axis=-1).astype(np.int32)


def check_against_loop(tiles, mesh, shift, dst, method, nodata, dtype):
    word = outside_word(OUTSIDE[dtype], dtype)
    got = _capi.resample_host(tiles, mesh, Spec(dtype, method, shift, nodata, word), dst)
    ref = resample_tiles(tiles, mesh, shift, dst, method, nodata=nodata, outside=word)
    pos = loop_positions(mesh, shift, dst)
    for t in range(tiles.shape[0]):
        d, how, head = loop_resample(tiles[t], pos, dst, method == CUBIC, nodata, fill_of(dtype))
        for k, v in (('dst', d), ('how', how), ('head', head)):
            assert same_bits(got[k][t], v) and same_bits(ref[k][t], v), k
    return got


def test_every_kind_of_invalid_tap():
    base = (np.arange(8 * 9, dtype=np.float32).reshape(1, 8, 9) - 30.0) * 1.5
    for bad, nodata in ((np.nan, None), (np.inf, None), (-np.inf, None), (NODATA[np.float32], NODATA[np.float32])):
        # one invalid tap in each of the 16 window positions of the pixel whose base pixel is (3, 3)
        for r, c in itertools.product(range(4), range(4)):
            tiles = base.copy()
            tiles[0, 2 + r, 2 + c] = bad
            got = check_against_loop(tiles, centred(8, 9, 77, 130), 0, (8, 9), CUBIC, nodata, np.float32)
            inner = (r in (1, 2)) and (c in (1, 2))
            assert got['how'][0, 3, 3] == (2 if inner else 1)
            assert np.isfinite(got['dst']).all()
    # the nodata value is an ordinary value without has_nodata
    tiles = base.copy()
    tiles[0, 3, 3] = NODATA[np.float32]
    assert check_against_loop(tiles, centred(8, 9, 77, 130), 0, (8, 9), CUBIC, None, np.float32)['how'][0, 3, 3] == 3
    # all four bilinear taps invalid; the only valid tap carrying weight 0
    tiles = base.copy()
    tiles[0, 3:5, 3:5] = np.nan
    got = check_against_loop(tiles, centred(8, 9, 77, 130), 0, (8, 9), CUBIC, None, np.float32)
    assert got['how'][0, 3, 3] == 0 and got['dst'][0, 3, 3] == np.float32(OUTSIDE[np.float32])
    tiles[0, 4, 4] = 2.0                                                  # weight fx * fy = 0 at a pixel centre
    for method in (BILINEAR, CUBIC):
        got = check_against_loop(tiles, centred(8, 9), 0, (8, 9), method, None, np.float32)
        assert got['how'][0, 3, 3] == 0 and got['how'][0, 4, 4] == 1 and got['dst'][0, 4, 4] == 2.0
    # float32 subnormals are kept; FLT_MAX inputs produce no NaN and stay finite under bilinear
    tiny = np.full((1, 6, 6), 1e-45, dtype=np.float32)
    tiny[0, ::2] = 3e-45
    for method in (BILINEAR, CUBIC):
        got = check_against_loop(tiny, centred(6, 6, 100, 60), 0, (6, 6), method, None, np.float32)
        assert np.all(got['dst'][got['how'] != 0] > 0) and np.all(got['dst'] < 1e-44)
        assert same_bits(check_against_loop(tiny, centred(6, 6), 0, (6, 6), method, None, np.float32)['dst'], tiny)
    big = np.full((1, 6, 6), np.finfo(np.float32).max, dtype=np.float32)
    big[0, :, ::2] = -np.finfo(np.float32).max
    got = check_against_loop(big, centred(6, 6, 128, 0), 0, (6, 6), CUBIC, None, np.float32)
    assert not np.isnan(got['dst']).any()
    assert np.isfinite(check_against_loop(big, centred(6, 6, 128, 0), 0, (6, 6), BILINEAR, None, np.float32)['dst']).all()
    # int16: the ends of the range, cubic overshoot clamps, nodata as an integer
    ends = np.full((1, 6, 6), 32767, dtype=np.int16)
    ends[0, :, 3:] = -32768
    got = check_against_loop(ends, centred(6, 6, 200, 0), 0, (6, 6), CUBIC, None, np.int16)
    exact = resample_tiles(ends.astype(np.float32), centred(6, 6, 200, 0), 0, (6, 6), CUBIC)['dst']
    assert exact.min() < -32768 and got['dst'].min() == -32768           # the overshoot exists and is clamped
    got = check_against_loop(ends, centred(6, 6, 56, 0), 0, (6, 6), CUBIC, None, np.int16)
    exact = resample_tiles(ends.astype(np.float32), centred(6, 6, 56, 0), 0, (6, 6), CUBIC)['dst']
    assert exact.max() > 32767 and got['dst'].max() == 32767
    ends[0, 2, 2] = -32767
    got = check_against_loop(ends, centred(6, 6, 56, 9), 0, (6, 6), CUBIC, -32767, np.int16)
    assert got['how'][0, 2, 2] == 2 and got['how'][0, 3, 3] == 1 and got['how'][0, 1, 1] == 2
    # rint is half to even: 0.5 -> 0, 1.5 -> 2, -0.5 -> -0
    steps = np.array([[[0, 1, 2, 1, -1, 0]]], dtype=np.int16)
    mesh = np.zeros(mesh_shape((1, 3), 0) + (2,), dtype=np.int32)
    mesh[..., 0], mesh[..., 1] = np.array([256, 512, 1280, 0]), 128        # halfway between columns 0 | 1, 1 | 2, 4 | 5
    assert _capi.resample_host(steps, mesh, Spec(np.int16, BILINEAR, 0), (1, 3))['dst'].tolist() == [[[0, 2, 0]]]


def test_bilinear_against_scipy():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(9)
    H, W, dst, shift = 64, 80, (33, 47), 4
    tiles = random_tiles(rng, 1, (H, W), np.float32, special=False)
    mesh = make_mesh('rotation', dst, shift, (H, W), rng)
    got = _capi.resample_host(tiles, mesh, Spec(np.float32, BILINEAR, shift), dst, want=('dst', 'how'))
    sx, sy = warp.positions(mesh, shift, dst)
    full = got['how'][0] == 1
    assert full.sum() > 500
    x, y = (sx - 128) / 256.0, (sy - 128) / 256.0
    want = ndimage.map_coordinates(tiles[0].astype(np.float64), [y[full], x[full]], order=1)
    mass = ndimage.map_coordinates(np.abs(tiles[0]).astype(np.float64), [y[full], x[full]], order=1)
    assert np.all(np.abs(got['dst'][0][full].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 8 * 2.0 ** -53 * mass)


def test_every_refusal_needs_no_device_and_writes_nothing():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    H, W, DH, DW, T = 5, 6, 7, 9, 2
    src = np.zeros((T, H, W), dtype=np.float32)
    mesh = np.zeros(mesh_shape((DH, DW), 2) + (2,), dtype=np.int32)
    SENT = 0xEE
    dst = np.full(T * DH * DW * 4 + 16, SENT, dtype=np.uint8)
    how = np.full(T * DH * DW + 16, SENT, dtype=np.uint8)
    head = np.full(T * 64 + 16, SENT, dtype=np.uint8)
    out = lambda: _capi.ResampleOut.of(dst.ctypes.data, how.ctypes.data, head.ctypes.data)
    spec = lambda **kw: _capi.ResampleSpec(**{**dict(kind=0, method=2, shift=2, has_nodata=0, nodata=0, outside=1, reserved=0, reserved2=0,
                                                     src_tile_stride=0, mesh_tile_stride_nodes=0), **kw})

    def refused(rc, code, word):
        said = lib.dswx_last_error().decode()
        assert rc == code and word in said, (rc, word, said)
        assert np.all(dst == SENT) and np.all(how == SENT) and np.all(head == SENT), word

    host = lambda sp, o, n=T, h=H, w=W, m=mesh.ctypes.data, dh=DH, dw=DW, p=src.ctypes.data: lib.dswx_resample_host(
        vp(p), ctypes.byref(sp) if sp is not None else None, n, h, w, vp(m), dh, dw, ctypes.byref(o) if o is not None else None)
    dev = lambda sp, o, n=T, h=H, w=W, m=0x40000, dh=DH, dw=DW, p=0x10000, ctx=None: lib.dswx_resample_device(
        ctx, vp(p), ctypes.byref(sp) if sp is not None else None, n, h, w, vp(m), dh, dw, ctypes.byref(o) if o is not None else None, None)
    assert host(spec(), out()) == 0 and not np.all(dst == SENT)
    dst[:], how[:], head[:] = SENT, SENT, SENT
    for entry in (host, dev):
        refused(entry(None, out()), _capi.ERR_ARG, 'spec is NULL')
        refused(entry(spec(), None), _capi.ERR_ARG, 'out is NULL')
        for kind in (-1, 2, 4):
            refused(entry(spec(kind=kind), out()), _capi.ERR_ARG, 'kind')
        for method in (0, 3, -1):
            refused(entry(spec(method=method), out()), _capi.ERR_ARG, 'method')
        for s in (-1, 9):
            refused(entry(spec(shift=s), out()), _capi.ERR_ARG, 'shift')
        refused(entry(spec(reserved=1), out()), _capi.ERR_ARG, 'reserved')
        refused(entry(spec(reserved2=1), out()), _capi.ERR_ARG, 'reserved')
        for kw in (dict(n=-1), dict(h=-1), dict(w=-1), dict(dh=-1), dict(dw=-1)):
            refused(entry(spec(), out(), **kw), _capi.ERR_ARG, 'negative size')
        refused(entry(spec(src_tile_stride=-1), out()), _capi.ERR_ARG, 'negative stride')
        refused(entry(spec(mesh_tile_stride_nodes=-1), out()), _capi.ERR_ARG, 'negative stride')
        refused(entry(spec(src_tile_stride=H * W - 1), out()), _capi.ERR_ARG, 'src_tile_stride smaller')
        refused(entry(spec(mesh_tile_stride_nodes=mesh.size // 2 - 1), out()), _capi.ERR_ARG, 'mesh_tile_stride_nodes')
        refused(entry(spec(), out(), h=(1 << 15) + 1, w=1 << 15), _capi.ERR_ARG, 'above 2^30')
        refused(entry(spec(), out(), dh=1 << 15, dw=(1 << 15) + 1), _capi.ERR_ARG, 'destination')
        refused(entry(spec(), out(), n=(1 << 32) + 1), _capi.ERR_ARG, 'tiles')
        refused(entry(spec(src_tile_stride=1 << 40), out(), n=1 << 7), _capi.ERR_ARG, 'too large')
        refused(entry(spec(), out(), m=0), _capi.ERR_ARG, 'mesh is NULL')
        refused(entry(spec(), out(), p=0), _capi.ERR_ARG, 'plane is NULL')
        refused(entry(spec(), _capi.ResampleOut.of(None, how.ctypes.data, None), p=0), _capi.ERR_ARG, 'plane is NULL')   # `how` reads the plane
    # the device entry alone: alignment, then the context -- after every argument
    refused(dev(spec(), out(), m=0x40002), _capi.ERR_ALIGN, 'mesh')
    refused(dev(spec(), _capi.ResampleOut.of(dst.ctypes.data, how.ctypes.data, head.ctypes.data + 4)), _capi.ERR_ALIGN, 'head')
    refused(dev(spec(), out(), p=0x10002), _capi.ERR_ALIGN, 'plane')
    refused(dev(spec(kind=1), out(), p=0x10001), _capi.ERR_ALIGN, 'plane')
    refused(dev(spec(), _capi.ResampleOut.of(dst.ctypes.data + 2, how.ctypes.data, head.ctypes.data)), _capi.ERR_ALIGN, 'dst')
    assert dev(spec(kind=1), _capi.ResampleOut.of(dst.ctypes.data + 2, how.ctypes.data + 1, head.ctypes.data), p=0x10002) == _capi.ERR_ARG   # aligned for int16
    refused(dev(spec(), out()), _capi.ERR_ARG, 'ctx is NULL')
    # the host entry takes buffers at any address, and a NULL mesh or plane when there is nothing to write
    odd = np.zeros(T * DH * DW * 4 + 1, dtype=np.uint8)
    assert host(spec(), _capi.ResampleOut.of(odd.ctypes.data + 1, None, None)) == 0
    assert host(spec(), out(), m=0, dh=0) == 0 and host(spec(), out(), m=0, n=0) == 0 and host(spec(), _capi.ResampleOut.of(), m=0) == 0
    assert np.all(dst == SENT) and np.all(how == SENT) and np.all(head == SENT)
    assert host(spec(), out(), p=0, h=0) == 0                                # an empty raster: every pixel outside
    assert how[:T * DH * DW].max() == 0 and head.view(np.uint64)[:8].tolist() == [DH * DW, 0, 0, 0, DH * DW, 0, 0, 0]
    for bad in (lambda: Spec(np.uint8, CUBIC, 0), lambda: Spec(np.float32, 'nearest', 0), lambda: Spec(np.float32, CUBIC, 9),
                lambda: Spec(np.int16, CUBIC, 0, nodata=1.5)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        resample_tiles(np.zeros((1, 2, 2), dtype=np.uint8), mesh, 2, (DH, DW), CUBIC)


def test_host_binding_refuses_a_mesh_with_too_few_nodes():
    """As tests/test_warp.py has it for the warp: the binding knows the mesh array's size and refuses one with fewer nodes than
    the destination needs, before dswx_resample_host would read past its end."""
    src = np.zeros((2, 3, 4), dtype=np.float32)
    mh, mw = mesh_shape((5, 9), 2)
    mesh = np.zeros((2, mh * mw + 1, 2), dtype=np.int32)
    per_tile = Spec(np.float32, CUBIC, 2, mesh_tile_stride_nodes=mh * mw + 1)
    assert _capi.resample_host(src, mesh[0, :mh * mw], Spec(np.float32, CUBIC, 2), (5, 9))['dst'].shape == (2, 5, 9)      # exactly enough
    assert _capi.resample_host(src, mesh.reshape(-1, 2)[:-1], per_tile, (5, 9))['dst'].shape == (2, 5, 9)             # (the last tile has no padding)
    with pytest.raises(ValueError, match='too small'):
        _capi.resample_host(src, mesh[0, :mh * mw - 1], Spec(np.float32, CUBIC, 2), (5, 9))
    with pytest.raises(ValueError, match='too small'):
        _capi.resample_host(src, mesh.reshape(-1, 2)[:-2], per_tile, (5, 9))
    assert _capi.resample_host(src, mesh[0, :1], Spec(np.float32, CUBIC, 2), (0, 9))['head'].tolist() == [[0] * 8] * 2  # nothing to read


def test_header_says_has_resample_and_the_struct_mirrors_match(tmp_path):
    import shutil
    import subprocess
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_RESAMPLE 1' in text and '#define DSWX_ABI_VERSION 7' in text and _capi.HAS_RESAMPLE == 1
    section = text.split('---- resample')[1]
    assert 'STILL REFUSED' in section and 'UNPINNED' in section and 'NO dswx_batch_resample' in section
    for name in ('dswx_resample_device', 'dswx_resample_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    assert not hasattr(_capi.load_library(), 'dswx_batch_resample')
    assert ctypes.sizeof(_capi.ResampleSpec) == 48 and ctypes.sizeof(_capi.ResampleOut) == 24
    if shutil.which('gcc') is None:
        return
    fields = {'dswx_resample_spec_t': _capi.ResampleSpec, 'dswx_resample_out_t': _capi.ResampleOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for st, cls in fields.items():
        for n, _ in cls._fields_:
            lines.append(f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));')
        lines.append(f'  printf("{st}.sizeof %zu\\n", sizeof({st}));')
    lines += ['  printf("consts %d %d %d %d %d\\n", DSWX_RESAMPLE_HEAD_WORDS, DSWX_RESAMPLE_F32, DSWX_RESAMPLE_I16, DSWX_RESAMPLE_BILINEAR, '
              'DSWX_RESAMPLE_CUBIC);', '  return 0;', '}']
    (tmp_path / 'off.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'off.c'), '-o', str(tmp_path / 'off')], check=True)
    got = dict(l.split(' ', 1) for l in subprocess.run([str(tmp_path / 'off')], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in fields.items():
        assert int(got[f'{st}.sizeof']) == ctypes.sizeof(cls)
        for n, _ in cls._fields_:
            assert int(got[f'{st}.{n}']) == getattr(cls, n).offset, (st, n)
    assert got['consts'] == (f'{_capi.RESAMPLE_HEAD_WORDS} {_capi.RESAMPLE_F32} {_capi.RESAMPLE_I16} {_capi.RESAMPLE_BILINEAR} '
                             f'{_capi.RESAMPLE_CUBIC}')
    assert (resample.KIND_F32, resample.KIND_I16, resample.BILINEAR, resample.CUBIC) == (
        _capi.RESAMPLE_F32, _capi.RESAMPLE_I16, _capi.RESAMPLE_BILINEAR, _capi.RESAMPLE_CUBIC)
    rule = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_resample_rule.h')).read()
    for name, value in (('RECT_H', _capi.RESAMPLE_RECT_H), ('RECT_W', _capi.RESAMPLE_RECT_W), ('LDS_ELEMS', _capi.RESAMPLE_LDS_ELEMS)):
        assert f'#define DSWX_RESAMPLE_{name} {value}\n' in rule


# ---- the geographic mesh --------------------------------------------------------------------------------------------------

ARC = 1.0 / 3600.0


def dem_grids(lat, zone=33, size=3760, pixel=30.0):
    """(src_gt of a 1-arc-second raster in degrees, dst_gt of a `size` x `size` grid of 30 m pixels centred on the central
    meridian of the zone at latitude `lat` -- south of the equator in EPSG 327zz --, the EPSG code)."""
    lon0 = -183.0 + 6.0 * zone
    fn = 10000000.0 if lat < 0 else 0.0
    _, north = warp.tm_forward(lon0, lat, lon0)
    x0, y0 = 500000.0 - size // 2 * pixel, round(float(north) / pixel) * pixel + size // 2 * pixel
    lon, la = warp.tm_inverse(x0 - 500000.0, y0, lon0)
    return ((math.floor(float(lon)) - 1.0, ARC, 0.0, math.ceil(float(la)) + 1.0, 0.0, -ARC), (x0, pixel, 0.0, y0 + fn, 0.0, -pixel),
            (32700 if lat < 0 else 32600) + zone)


def test_geographic_mesh_against_the_forward_projection():
    """Every node, taken back through tm_forward of its own longitude and latitude, lands on the centre of its destination
    pixel: round trip below 1e-6 destination pixel (the node's quantisation to 1/256 source pixel allowed for)."""
    for lat in (5.0, 45.0, 70.0, -33.0):
        src_gt, dst_gt, epsg = dem_grids(lat, size=512)
        for shift in (4, 6):
            mesh, deviation = warp.geographic_mesh(src_gt, dst_gt, epsg, (512, 512), shift)
            mh, mw = mesh_shape((512, 512), shift)
            assert mesh.shape == (mh, mw, 2) and mesh.dtype == np.int32 and 0.0 <= deviation < 8.0
            # unquantised: the exact mapping of the nodes through the forward projection
            Y, X = warp._node_pixels((512, 512), shift)
            col, row, _ = warp._geographic_exact(src_gt, dst_gt, epsg, Y, X)
            lon, la = src_gt[0] + col * src_gt[1], src_gt[3] + row * src_gt[5]
            e, n = warp.tm_forward(lon, la, 15.0)
            fn = 10000000.0 if lat < 0 else 0.0
            px, py = (e + 500000.0 - dst_gt[0]) / dst_gt[1] - 0.5, (n + fn - dst_gt[3]) / dst_gt[5] - 0.5
            assert np.abs(px - X).max() < 1e-6 and np.abs(py - Y).max() < 1e-6
            assert np.abs(mesh[..., 0] - 256.0 * col).max() <= 0.5 and np.abs(mesh[..., 1] - 256.0 * row).max() <= 0.5
            # the southern hemisphere looks at southern latitudes
            assert (la.max() < 0) == (lat < 0)


# The issue prints a table of deviations (1-arc-second source onto a 30 m grid, shifts 4, 5, 6, 7) but not the grid it was
# measured on, and no grid tried here gives its figures to the printed digits (each figure is the largest over the cells of
# |curvature + rounding of four nodes|, which moves in the second decimal with the place inside the zone): 5 degrees 0.49 0.48
# 0.47 0.60, 45 degrees 0.53 0.62 1.01 2.78, 70 degrees 0.57 0.80 2.05 6.78.  Pinned instead: THIS grid's own figures (3760 x
# 3760 pixels of 30 m in zone 33, centred on the central meridian at the latitude), to the two printed decimals.
DEVIATIONS = {5.0: (0.48, 0.47, 0.51, 0.63), 45.0: (0.50, 0.60, 1.05, 2.80), 70.0: (0.60, 0.88, 2.08, 7.02)}


@pytest.mark.parametrize('lat', sorted(DEVIATIONS))
def test_geographic_mesh_deviation_table(lat):
    """The deviations of this grid to two decimals (0.006: half a unit of the second decimal and the last bits of another
    libm), and what the product path's choice of the shift rests on: at 45 and 70 degrees N shift 6 deviates by more than 1.0
    and shift 5 does not; at 5 degrees shift 6 does not."""
    src_gt, dst_gt, epsg = dem_grids(lat)
    got = [warp.geographic_mesh(src_gt, dst_gt, epsg, (3760, 3760), shift)[1] for shift in (4, 5, 6, 7)]
    print(lat, ' '.join(f'{v:.4f}' for v in got))
    for mine, pinned in zip(got, DEVIATIONS[lat]):
        assert abs(mine - pinned) <= 0.006, (lat, got)
    assert (got[2] > 1.0) == (lat >= 45.0) and got[1] <= 1.0 and got[0] <= 1.0


def test_mesh_between_routes_geographic_sources():
    """mesh_between hands a source in EPSG:4326 whose geotransform is in degrees to geographic_mesh; everything else as before:
    equal codes are affine, two UTM zones go through utm_mesh, anything else -- a geotransform in metres that merely carries
    the code 4326 included -- is refused with the message it always had."""
    src_gt, dst_gt, epsg = dem_grids(45.0, size=256)
    mesh, deviation = warp.mesh_between(src_gt, 4326, dst_gt, epsg, (256, 256), 5)
    ref, dev = warp.geographic_mesh(src_gt, dst_gt, epsg, (256, 256), 5)
    assert np.array_equal(mesh, ref) and deviation == dev and warp.in_degrees(src_gt) and not warp.in_degrees(dst_gt)
    assert warp.mesh_between(dst_gt, epsg, dst_gt, epsg, (8, 8), 2)[1] == 0.0
    assert np.array_equal(warp.mesh_between(dst_gt, 32632, dst_gt, epsg, (8, 8), 2)[0], warp.utm_mesh(dst_gt, 32632, dst_gt, epsg, (8, 8), 2)[0])
    for s, d, gt in ((4326, 3857, src_gt), (3857, epsg, src_gt), (epsg, 4326, dst_gt), (None, epsg, src_gt), (4326, None, src_gt), (4326, epsg, dst_gt)):
        with pytest.raises(ValueError, match='not WGS 84 / UTM'):
            warp.mesh_between(gt, s, dst_gt, d, (8, 8), 2)
    with pytest.raises(ValueError, match='rotated'):
        warp.geographic_mesh((0.0, ARC, 1e-9, 46.0, 0.0, -ARC), dst_gt, epsg, (8, 8), 2)


def test_dem_resample_plan_accepts_and_refuses():
    """The product path's plan: EPSG:4326 always; a UTM zone or the product's own SRS only when asked; the shift is 6 unless
    the mesh deviates by more than 1/256 source pixel."""
    from types import SimpleNamespace
    from proteus_amd import dswx_hls as D, geotiff
    gt = (600000.0, 30.0, 0.0, 4000020.0, 0.0, -30.0)
    tags = geotiff.geo_tags_from_geotransform(gt, epsg=32615)
    dem = lambda g, epsg, h=600, w=600: SimpleNamespace(geotransform=g, geo_tags=geotiff.geo_tags_from_geotransform(g, epsg), height=h, width=w)
    window, mesh, shift, deviation, dst_shape = D.dem_resample_plan(dem((-92.0, ARC, 0.0, 36.25, 0.0, -ARC), 4326), gt, tags, 128, 128)
    assert dst_shape == (228, 228) and shift in D.DEM_MESH_SHIFTS and deviation <= 1.0 and mesh.shape == warp.mesh_shape(dst_shape, shift) + (2,)
    assert 0 <= window[0] and window[0] + window[2] <= 600 and window[2] > 200 and int(mesh[..., 0].min()) >= 3 * 256
    shifted = dem((gt[0] - 1500.0 - 300.0 + 7.0, 30.0, 0.0, gt[3] + 1500.0 + 300.0, 0.0, -30.0), 32615, 248, 248)
    other_zone = dem((600000.0 - 6e5, 30.0, 0.0, 4000020.0, 0.0, -30.0), 32616)
    for info in (shifted, other_zone, dem((-92.0, ARC, 0.0, 36.25, 0.0, -ARC), 3857), dem(gt, 4326)):
        with pytest.raises(NotImplementedError, match='not on the HLS grid'):
            D.dem_resample_plan(info, gt, tags, 128, 128)
    window, mesh, shift, deviation, _ = D.dem_resample_plan(shifted, gt, tags, 128, 128, projected=True)
    assert shift == 6 and deviation == 0.0 and window == (7, 7, 241, 241)       # 10 pixels of margin, 3 of them needed
    assert mesh[0, 0].tolist() == [256 * 3 + 128 - round(256 * 7 / 30), 256 * 3 + 128]       # relative to the window
    assert D.dem_resample_plan(other_zone, gt, tags, 128, 128, projected=True)[2] in D.DEM_MESH_SHIFTS
    with pytest.raises(NotImplementedError, match='not on the HLS grid'):
        D.dem_resample_plan(dem((-92.0, ARC, 0.0, 36.25, 0.0, -ARC), 3857), gt, tags, 128, 128, projected=True)


def test_the_antimeridian_is_refused():
    # zone 60 reaches 180 degrees east at 500 km + some 230 km of easting at 45 degrees north; zone 1 the same to the west
    _, north = warp.tm_forward(177.0, 45.0, 177.0)
    src_gt = (170.0, ARC, 0.0, 47.0, 0.0, -ARC)
    inside = (600000.0, 30.0, 0.0, float(north), 0.0, -30.0)
    across = (730000.0, 30.0, 0.0, float(north), 0.0, -30.0)
    warp.geographic_mesh(src_gt, inside, 32660, (512, 512), 6)
    with pytest.raises(ValueError, match='antimeridian'):
        warp.geographic_mesh(src_gt, across, 32660, (512, 512), 6)
    with pytest.raises(ValueError, match='antimeridian'):
        warp.geographic_mesh((-180.0, ARC, 0.0, 47.0, 0.0, -ARC), (270000.0 - 512 * 30.0, 30.0, 0.0, float(north), 0.0, -30.0), 32601, (512, 512), 6)
