"""The warp definition (include/dswx_hip.h "warp") on the CPU: dswx_warp_host, proteus_amd.warp.warp_tiles and a per-pixel loop in
Python ints are pinned to each other byte for byte on dst, src_index and head -- shifts 0, 1, 4, 8; destinations of one pixel, one
row, one column, and sizes that are no multiple of the step or of 16; sources from empty to many cells; 1-, 2- and 4-byte
elements; shared and per-tile meshes, with strides; identity, whole-pixel shifts, offsets either side of a pixel boundary, a
small rotation and int32 garbage.  Closed forms (identity, shifts, quarter turns, flips, transpose, decimation, the gather
through src_index); every refusal, each before anything is written; and the host side of the projection: the transverse
Mercator of proteus_amd.warp pinned, without PROJ, to its own inverse, to the meridian arc by quadrature, to conformality and
to the Redfearn / Snyder series; affine_mesh and utm_mesh against closed forms and a brute-force evaluation."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest

from proteus_amd import _capi, warp
from proteus_amd.warp import INT32_MAX, INT32_MIN, OUTSIDE, Spec, mesh_shape, warp_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = (0, 1, 4, 8)
DSTS = ((1, 1), (1, 17), (17, 1), (33, 47), (70, 300))
SRCS = ((0, 0), (1, 1), (5, 3), (64, 80))
DTYPES = {1: np.uint8, 2: np.int16, 4: np.uint32}
MESHES = ('identity', 'shift', 'half', 'below', 'edge', 'under', 'rotation', 'garbage')
OUT_WORD = 0xA1B2C3FE


def make_mesh(kind, dst, shift, src, rng):
    """int32 [mesh_h, mesh_w, 2] of one of MESHES for a destination `dst` and a source `src`."""
    mh, mw = mesh_shape(dst, shift)
    step = 1 << shift
    jj, ii = np.meshgrid(np.arange(mw, dtype=np.int64) * step, np.arange(mh, dtype=np.int64) * step)
    x, y = 256 * jj + 128, 256 * ii + 128                    # the centres of the pixels the nodes describe: the identity
    if kind == 'shift':
        x, y = x + 256 * 3, y - 256 * 2
    elif kind == 'half':                                     # a centre exactly ON a pixel boundary: floor puts it in the next pixel
        x, y = x + 128, y + 128
    elif kind == 'below':                                    # 1/256 in front of that boundary
        x, y = x + 127, y + 127
    elif kind == 'edge':                                     # exactly on the boundary behind
        x, y = x - 128, y - 128
    elif kind == 'under':                                    # 1/256 behind it: the previous pixel
        x, y = x - 129, y - 129
    elif kind == 'rotation':                                 # three degrees about the middle of the source
        a = math.radians(3.0)
        cx, cy = 128.0 * src[1], 128.0 * src[0]
        dx, dy = x - 128.0 * dst[1], y - 128.0 * dst[0]
        x = np.rint(cx + math.cos(a) * dx - math.sin(a) * dy).astype(np.int64)
        y = np.rint(cy + math.sin(a) * dx + math.cos(a) * dy).astype(np.int64)
    elif kind == 'garbage':
        g = rng.integers(INT32_MIN, INT32_MAX + 1, size=(mh, mw, 2), dtype=np.int64)
        g[rng.random((mh, mw, 2)) < 0.2] = INT32_MIN
        g[rng.random((mh, mw, 2)) < 0.2] = INT32_MAX
        g[:2, :2] = INT32_MAX                                # all four nodes of a cell at either end of the range
        g[-2:, -2:] = INT32_MIN
        if mh > 2 and mw > 2:
            g[1:3, 1:3, 0], g[1:3, 1:3, 1] = INT32_MIN, INT32_MAX
        return g.astype(np.int32)
    return np.stack([x, y], axis=-1).astype(np.int32)


def loop_positions(mesh, shift, dst):
    """[(sx, sy)] per destination pixel, row-major, in Python ints: the definition as written."""
    m = mesh.tolist()
    step = 1 << shift
    out = []
    for Y in range(dst[0]):
        i, fy = Y >> shift, Y & (step - 1)
        for X in range(dst[1]):
            j, fx = X >> shift, X & (step - 1)
            pos = []
            for k in range(2):
                num = (step - fy) * ((step - fx) * m[i][j][k] + fx * m[i][j + 1][k]) + fy * ((step - fx) * m[i + 1][j][k] + fx * m[i + 1][j + 1][k])
                assert abs(num) < 1 << 48
                pos.append((num + (1 << (2 * shift - 1))) >> (2 * shift) if shift else num)
            out.append(tuple(pos))
    return out


def loop_warp(tile, pos, dst, outside):
    """(dst, src_index, head) of ONE tile [H, W] from loop_positions, in Python ints."""
    H, W = tile.shape
    flat = tile.reshape(-1).tolist()
    d, idx = [], []
    inside, rmin, rmax, cmin, cmax = 0, H, 0, W, 0
    for sx, sy in pos:
        c, r = sx >> 8, sy >> 8
        if 0 <= c < W and 0 <= r < H:
            d.append(flat[r * W + c])
            idx.append(r * W + c)
            inside += 1
            rmin, rmax, cmin, cmax = min(rmin, r), max(rmax, r), min(cmin, c), max(cmax, c)
        else:
            d.append(outside)
            idx.append(OUTSIDE)
    n = dst[0] * dst[1]
    return (np.array(d, dtype=tile.dtype).reshape(dst), np.array(idx, dtype=np.uint32).reshape(dst),
            np.array([n, inside, n - inside, rmin, rmax, cmin, cmax, 0], dtype=np.uint64))


def outside_of(dtype):
    """The element that the low bytes of OUT_WORD are."""
    return np.array([OUT_WORD & ((1 << (8 * np.dtype(dtype).itemsize)) - 1)], dtype=f'<u{np.dtype(dtype).itemsize}').view(dtype)[0]


def random_tiles(rng, n, src, eb):
    return rng.integers(0, 1 << (8 * eb), size=(n,) + src, dtype=np.uint64).astype(f'<u{eb}').view(DTYPES[eb]).reshape((n,) + src)


@pytest.mark.parametrize('shift', SHIFTS)
@pytest.mark.parametrize('dst', DSTS)
def test_host_numpy_and_python_loop_agree(shift, dst):
    """For this shift and destination: every mesh content x every source x every element size, with a shared mesh and with
    per-tile meshes, the plane and the meshes packed and strided."""
    rng = np.random.default_rng(1000 * shift + dst[0] * 31 + dst[1])
    mh, mw = mesh_shape(dst, shift)
    for src in SRCS:
        meshes = {k: make_mesh(k, dst, shift, src, rng) for k in MESHES}
        loops = {k: loop_positions(m, shift, dst) for k, m in meshes.items()}
        for eb in (1, 2, 4):
            n = 3
            tiles = random_tiles(rng, n, src, eb)
            fill = outside_of(tiles.dtype)
            for kind in MESHES:
                # one mesh for all tiles, a packed plane
                got = _capi.warp_host(tiles, meshes[kind], Spec(eb, shift, OUT_WORD), dst)
                ref = warp_tiles(tiles, meshes[kind], shift, dst, OUT_WORD)
                for t in range(n):
                    d, idx, head = loop_warp(tiles[t], loops[kind], dst, fill)
                    assert np.array_equal(ref['dst'][t], d) and np.array_equal(ref['src_index'][t], idx) and np.array_equal(ref['head'][t], head), (kind, src, eb, t)
                for k in warp.OUTPUTS:
                    assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (kind, src, eb, k)
                inside = got['src_index'] != OUTSIDE
                for t in range(n):
                    assert np.array_equal(got['dst'][t][inside[t]], tiles[t].reshape(-1)[got['src_index'][t][inside[t]]])
                    assert np.all(got['dst'][t][~inside[t]] == fill)
            # a mesh per tile with nodes between the meshes, and a plane with elements between the tiles
            order = [MESHES[(k + shift) % len(MESHES)] for k in range(n)]
            nodes = mh * mw + 5
            per_tile = rng.integers(INT32_MIN, INT32_MAX + 1, size=(n, nodes, 2), dtype=np.int64).astype(np.int32)
            for t, kind in enumerate(order):
                per_tile[t, :mh * mw] = meshes[kind].reshape(-1, 2)
            stride = src[0] * src[1] + 7
            padded = random_tiles(rng, n, (1, stride), eb).reshape(n, stride)
            padded[:, :src[0] * src[1]] = tiles.reshape(n, -1)
            got = _capi.warp_host(padded, per_tile, Spec(eb, shift, OUT_WORD, src_tile_stride=stride, mesh_tile_stride_nodes=nodes), dst, raster=src)
            ref = warp_tiles(tiles, np.stack([meshes[k] for k in order]), shift, dst, OUT_WORD)
            for k in warp.OUTPUTS:
                assert np.array_equal(got[k], ref[k]), ('per tile', src, eb, k)
            for t, kind in enumerate(order):
                assert np.array_equal(got['dst'][t], loop_warp(tiles[t], loops[kind], dst, fill)[0]), ('per tile', kind)
        if dst == (70, 300) and shift == 4:
            # the meshes do what their names say on the largest source
            h = warp_tiles(random_tiles(rng, 1, SRCS[-1], 1), meshes['rotation'], shift, dst)['head'][0]
            assert 0 < h[1] < h[0] and h[3] < h[4] and h[5] < h[6]
            g = warp_tiles(random_tiles(rng, 1, SRCS[-1], 1), meshes['garbage'], shift, dst)['head'][0]
            assert g[2] > 0


def test_pixel_boundaries_floor_and_rounding():
    """A centre exactly on a pixel boundary belongs to the pixel behind it (floor), 1/256 in front of it to the pixel in front;
    and the rounding of the interpolation is to nearest, half UP, also for negative numerators."""
    src = np.arange(6 * 7, dtype=np.uint8).reshape(1, 6, 7)
    for kind, (dr, dc) in (('identity', (0, 0)), ('half', (1, 1)), ('below', (0, 0)), ('edge', (0, 0)), ('under', (-1, -1))):
        got = _capi.warp_host(src, make_mesh(kind, (6, 7), 0, (6, 7), None), Spec(1, 0, 255), (6, 7))['dst'][0]
        want = np.full((6, 7), 255, dtype=np.uint8)
        ys, xs = slice(max(-dr, 0), 6 - max(dr, 0)), slice(max(-dc, 0), 7 - max(dc, 0))
        want[ys, xs] = src[0][max(dr, 0):6 + min(dr, 0), max(dc, 0):7 + min(dc, 0)]
        assert np.array_equal(got, want), kind
    # shift 1, one cell: nodes 0 and 1 along x -> the middle pixel is 0.5 -> rounds up to 1; -1 and 0 -> -0.5 -> rounds up to 0
    for x0, x1, mid in ((0, 1, 1), (-1, 0, 0), (-3, -2, -2), (255, 256, 256), (-257, -256, -256)):
        mesh = np.zeros((2, 2, 2), dtype=np.int32)
        mesh[:, 0, 0], mesh[:, 1, 0] = x0, x1
        sx, sy = warp.positions(mesh, 1, (1, 2))
        assert sx.tolist() == [[x0, mid]] and sy.tolist() == [[0, 0]]
        got = _capi.warp_host(np.array([[[7, 9]]], dtype=np.uint8), mesh, Spec(1, 1, 0), (1, 2))['src_index'][0, 0]
        assert got.tolist() == [x if 0 <= x < 2 else OUTSIDE for x in (x0 >> 8, mid >> 8)]


def exact_mesh(dst, shift, fx, fy):
    """The mesh whose node for destination pixel (X, Y) is the CENTRE of source pixel (fx(X, Y), fy(X, Y)), for integer-affine fx, fy."""
    mh, mw = mesh_shape(dst, shift)
    step = 1 << shift
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) * step, np.arange(mh, dtype=np.int64) * step)
    return np.stack([256 * fx(X, Y) + 128, 256 * fy(X, Y) + 128], axis=-1).astype(np.int32)


@pytest.mark.parametrize('shift', SHIFTS)
@pytest.mark.parametrize('eb', (1, 2, 4))
def test_closed_forms(shift, eb):
    rng = np.random.default_rng(77 + shift + 10 * eb)
    H, W = 37, 53
    src = random_tiles(rng, 2, (H, W), eb)
    fill = outside_of(src.dtype)
    run = lambda mesh, dst: _capi.warp_host(src, mesh, Spec(eb, shift, OUT_WORD), dst)
    # the identity
    got = run(exact_mesh((H, W), shift, lambda X, Y: X, lambda X, Y: Y), (H, W))
    assert np.array_equal(got['dst'], src) and np.array_equal(got['src_index'][0].reshape(-1), np.arange(H * W))
    assert got['head'].tolist() == [[H * W, H * W, 0, 0, H - 1, 0, W - 1, 0]] * 2
    # a shift by (a, b) pixels: the slice, `outside` elsewhere
    for a, b in ((5, 0), (0, -4), (-7, 9), (W, 0), (-60, -60)):
        got = run(exact_mesh((H, W), shift, lambda X, Y: X + a, lambda X, Y: Y + b), (H, W))
        want = np.full_like(src, fill)
        ys, xs = slice(max(-b, 0), max(H - max(b, 0), 0)), slice(max(-a, 0), max(W - max(a, 0), 0))
        part = src[:, max(b, 0):max(H + min(b, 0), 0), max(a, 0):max(W + min(a, 0), 0)]
        if part.size:
            want[:, ys, xs] = part
        assert np.array_equal(got['dst'], want), (a, b)
        n_in = part[0].size
        assert got['head'][0, :3].tolist() == [H * W, n_in, H * W - n_in]
        if n_in:
            assert got['head'][0, 3:7].tolist() == [max(b, 0), H - 1 + min(b, 0), max(a, 0), W - 1 + min(a, 0)]
        else:
            assert got['head'][0, 3:].tolist() == [H, 0, W, 0, 0]
    # quarter turns, flips and the transpose
    assert np.array_equal(run(exact_mesh((W, H), shift, lambda X, Y: W - 1 - Y, lambda X, Y: X), (W, H))['dst'], np.rot90(src, 1, axes=(1, 2)))
    assert np.array_equal(run(exact_mesh((H, W), shift, lambda X, Y: W - 1 - X, lambda X, Y: H - 1 - Y), (H, W))['dst'], np.rot90(src, 2, axes=(1, 2)))
    assert np.array_equal(run(exact_mesh((W, H), shift, lambda X, Y: Y, lambda X, Y: H - 1 - X), (W, H))['dst'], np.rot90(src, 3, axes=(1, 2)))
    assert np.array_equal(run(exact_mesh((H, W), shift, lambda X, Y: W - 1 - X, lambda X, Y: Y), (H, W))['dst'], src[:, :, ::-1])
    assert np.array_equal(run(exact_mesh((H, W), shift, lambda X, Y: X, lambda X, Y: H - 1 - Y), (H, W))['dst'], src[:, ::-1, :])
    assert np.array_equal(run(exact_mesh((W, H), shift, lambda X, Y: Y, lambda X, Y: X), (W, H))['dst'], src.transpose(0, 2, 1))
    # twice the pixel size: the centre of destination pixel X lies on the boundary between source pixels 2X and 2X + 1, which
    # by the floor belongs to 2X + 1
    mh, mw = mesh_shape((H // 2, W // 2), shift)
    step = 1 << shift
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) * step, np.arange(mh, dtype=np.int64) * step)
    coarse = np.stack([512 * X + 256, 512 * Y + 256], axis=-1).astype(np.int32)
    got = run(coarse, (H // 2, W // 2))
    assert np.array_equal(got['dst'], src[:, 1::2, 1::2][:, :H // 2, :W // 2])
    got = run(coarse - 1, (H // 2, W // 2))                   # 1/256 in front of the boundary: 2X
    assert np.array_equal(got['dst'], src[:, 0::2, 0::2][:, :H // 2, :W // 2])


def test_wanted_outputs_and_empty_inputs():
    src = np.arange(12, dtype=np.uint8).reshape(1, 3, 4)
    mesh = exact_mesh((3, 4), 2, lambda X, Y: X, lambda X, Y: Y)
    full = _capi.warp_host(src, mesh, Spec(1, 2, 9), (3, 4))
    for r in range(1, 4):
        for want in itertools.combinations(warp.OUTPUTS, r):
            got = _capi.warp_host(src, mesh, Spec(1, 2, 9), (3, 4), want=want)
            assert list(got) == list(want) and all(np.array_equal(got[k], full[k]) for k in want)
    # no tiles, an empty destination: nothing; an empty source: everything outside
    assert _capi.warp_host(src[:0], mesh, Spec(1, 2, 9), (3, 4))['dst'].shape == (0, 3, 4)
    assert _capi.warp_host(src, np.zeros((1, 2, 2), dtype=np.int32), Spec(1, 2, 9), (0, 4))['head'].tolist() == [[0] * 8]
    got = _capi.warp_host(np.zeros((2, 0, 5), dtype=np.uint8), mesh, Spec(1, 2, 9), (3, 4))
    assert np.all(got['dst'] == 9) and np.all(got['src_index'] == OUTSIDE) and got['head'].tolist() == [[12, 0, 12, 0, 0, 5, 0, 0]] * 2


def test_every_refusal_needs_no_device_and_writes_nothing():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    H, W, DH, DW, T = 5, 6, 7, 9, 2
    src = np.zeros((T, H, W), dtype=np.uint32)
    mesh = np.zeros(mesh_shape((DH, DW), 2) + (2,), dtype=np.int32)
    SENT = 0xEE
    dst = np.full(T * DH * DW * 4 + 16, SENT, dtype=np.uint8)
    index = np.full(T * DH * DW * 4 + 16, SENT, dtype=np.uint8)
    head = np.full(T * 64 + 16, SENT, dtype=np.uint8)
    out = lambda: _capi.WarpOut.of(dst.ctypes.data, index.ctypes.data, head.ctypes.data)
    spec = lambda **kw: _capi.WarpSpec(**{**dict(elem_bytes=4, shift=2, outside=1, reserved=0, src_tile_stride=0, mesh_tile_stride_nodes=0), **kw})

    def refused(rc, code, word):
        said = lib.dswx_last_error().decode()
        assert rc == code and word in said, (rc, word, said)
        assert np.all(dst == SENT) and np.all(index == SENT) and np.all(head == SENT), word

    host = lambda sp, o, n=T, h=H, w=W, m=mesh.ctypes.data, dh=DH, dw=DW, p=src.ctypes.data: lib.dswx_warp_host(
        vp(p), ctypes.byref(sp) if sp is not None else None, n, h, w, vp(m), dh, dw, ctypes.byref(o) if o is not None else None)
    dev = lambda sp, o, n=T, h=H, w=W, m=0x40000, dh=DH, dw=DW, p=0x10000, ctx=None: lib.dswx_warp_device(
        ctx, vp(p), ctypes.byref(sp) if sp is not None else None, n, h, w, vp(m), dh, dw, ctypes.byref(o) if o is not None else None, None)
    assert host(spec(), out()) == 0 and not np.all(dst == SENT)
    dst[:], index[:], head[:] = SENT, SENT, SENT
    for entry in (host, dev):
        refused(entry(None, out()), _capi.ERR_ARG, 'spec is NULL')
        refused(entry(spec(), None), _capi.ERR_ARG, 'out is NULL')
        for eb in (0, 3, 8, -1):
            refused(entry(spec(elem_bytes=eb), out()), _capi.ERR_ARG, 'elem_bytes')
        for s in (-1, 9):
            refused(entry(spec(shift=s), out()), _capi.ERR_ARG, 'shift')
        refused(entry(spec(reserved=1), out()), _capi.ERR_ARG, 'reserved')
        for kw in (dict(n=-1), dict(h=-1), dict(w=-1), dict(dh=-1), dict(dw=-1)):
            refused(entry(spec(), out(), **kw), _capi.ERR_ARG, 'negative size')
        refused(entry(spec(src_tile_stride=-1), out()), _capi.ERR_ARG, 'negative stride')
        refused(entry(spec(mesh_tile_stride_nodes=-1), out()), _capi.ERR_ARG, 'negative stride')
        refused(entry(spec(src_tile_stride=H * W - 1), out()), _capi.ERR_ARG, 'src_tile_stride smaller')
        refused(entry(spec(mesh_tile_stride_nodes=mesh.size // 2 - 1), out()), _capi.ERR_ARG, 'mesh_tile_stride_nodes')
        refused(entry(spec(), out(), h=(1 << 15) + 1, w=1 << 15), _capi.ERR_ARG, 'above 2^30')
        refused(entry(spec(), out(), h=(1 << 30) + 1, w=0), _capi.ERR_ARG, 'above 2^30')
        refused(entry(spec(), out(), dh=1 << 15, dw=(1 << 15) + 1), _capi.ERR_ARG, 'destination')
        refused(entry(spec(), out(), dh=0, dw=(1 << 30) + 1), _capi.ERR_ARG, 'destination')
        refused(entry(spec(), out(), n=(1 << 32) + 1), _capi.ERR_ARG, 'tiles')
        refused(entry(spec(src_tile_stride=1 << 40), out(), n=1 << 7), _capi.ERR_ARG, 'too large')
        refused(entry(spec(), out(), m=0), _capi.ERR_ARG, 'mesh is NULL')
        refused(entry(spec(), out(), p=0), _capi.ERR_ARG, 'plane is NULL')
    # the device entry alone: alignment, then the context -- after every argument
    refused(dev(spec(), out(), m=0x40002), _capi.ERR_ALIGN, 'mesh')
    refused(dev(spec(), _capi.WarpOut.of(dst.ctypes.data, index.ctypes.data + 2, head.ctypes.data)), _capi.ERR_ALIGN, 'src_index')
    refused(dev(spec(), _capi.WarpOut.of(dst.ctypes.data, index.ctypes.data, head.ctypes.data + 4)), _capi.ERR_ALIGN, 'head')
    refused(dev(spec(), out(), p=0x10002), _capi.ERR_ALIGN, 'plane')
    refused(dev(spec(elem_bytes=2), out(), p=0x10001), _capi.ERR_ALIGN, 'plane')
    refused(dev(spec(), _capi.WarpOut.of(dst.ctypes.data + 2, index.ctypes.data, head.ctypes.data)), _capi.ERR_ALIGN, 'dst')
    refused(dev(spec(), out()), _capi.ERR_ARG, 'ctx is NULL')
    refused(lib.dswx_batch_warp(None, 14, ctypes.byref(spec(elem_bytes=1)), 0, 1, vp(0x40000), DH, DW, ctypes.byref(out()), None),
            _capi.ERR_ARG, 'batch is NULL')
    # the host entry takes buffers at any address, and a NULL mesh or plane when there is nothing to write
    odd = np.zeros(T * DH * DW * 4 + 1, dtype=np.uint8)
    assert host(spec(), _capi.WarpOut.of(odd.ctypes.data + 1, None, None)) == 0
    assert host(spec(), out(), m=0, dh=0) == 0 and host(spec(), out(), m=0, n=0) == 0 and host(spec(), _capi.WarpOut.of(), m=0) == 0
    assert host(spec(), _capi.WarpOut.of(None, index.ctypes.data, None), p=0) == 0      # src_index does not read the plane
    dst[:], index[:], head[:] = SENT, SENT, SENT
    with pytest.raises(ValueError):
        Spec(3, 0)
    with pytest.raises(ValueError):
        Spec(1, 9)


def test_host_binding_refuses_a_mesh_with_too_few_nodes():
    """dswx_warp_host trusts the caller's mesh to have mesh_h * mesh_w nodes per tile; the binding knows the array's size and
    refuses a smaller one before the call would read past its end."""
    src = np.zeros((2, 3, 4), dtype=np.uint8)
    mh, mw = mesh_shape((5, 9), 2)
    mesh = np.zeros((2, mh * mw + 1, 2), dtype=np.int32)
    per_tile = Spec(1, 2, 9, mesh_tile_stride_nodes=mh * mw + 1)
    assert _capi.warp_host(src, mesh[0, :mh * mw], Spec(1, 2, 9), (5, 9))['dst'].shape == (2, 5, 9)         # exactly enough
    assert _capi.warp_host(src, mesh.reshape(-1, 2)[:-1], per_tile, (5, 9))['dst'].shape == (2, 5, 9)       # (the last tile has no padding)
    with pytest.raises(ValueError, match='too small'):
        _capi.warp_host(src, mesh[0, :mh * mw - 1], Spec(1, 2, 9), (5, 9))
    with pytest.raises(ValueError, match='too small'):
        _capi.warp_host(src, mesh.reshape(-1, 2)[:-2], per_tile, (5, 9))
    assert _capi.warp_host(src, mesh[0, :1], Spec(1, 2, 9), (0, 9))['head'].tolist() == [[0] * 8] * 2      # nothing to read


def test_mesh_rule_and_host_entries_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/mesh_host_san.cpp with proteus_amd/csrc/dswx_warp.hip and dswx_resample.hip compiled into it, host code
    under ASan + UBSan: the warp kernel's per-cell linear form (dswx_mesh_rule.h, executed on the host) against the definition
    for every fx and fy of a cell at every shift with nodes up to INT32_MIN and INT32_MAX, the definition against 128-bit
    integers, and both host entries on heap blocks of exactly the bytes they may touch at odd addresses, every result against
    a plain loop.  A child process; nothing is loaded into this interpreter."""
    import json
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'mesh_host_san')
    csrc = os.path.join(ROOT, 'proteus_amd', 'csrc')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', csrc,
           os.path.join(ROOT, 'tests', 'native', 'mesh_host_san.cpp'), os.path.join(csrc, 'dswx_warp.hip'), os.path.join(csrc, 'dswx_resample.hip'),
           '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0 and 'libclang_rt.asan' in res.stderr:     # (only the runtime: an error in the sources must fail)
        pytest.skip(f'sanitizer runtime missing: {res.stderr[-300:]}')
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr and 'LeakSanitizer' not in res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out['failures'] == 0 and out['cases'] >= 100


def test_header_says_has_warp_and_the_struct_mirrors_match(tmp_path):
    import shutil
    import subprocess
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_WARP 1' in text and '#define DSWX_ABI_VERSION 7' in text and _capi.HAS_WARP == 1
    assert 'STILL REFUSED' in text.split('---- warp')[1] and 'UNPINNED' in text.split('---- warp')[1]
    for name in ('dswx_warp_device', 'dswx_batch_warp', 'dswx_warp_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    assert ctypes.sizeof(_capi.WarpSpec) == 32 and ctypes.sizeof(_capi.WarpOut) == 24
    if shutil.which('gcc') is None:
        return
    fields = {'dswx_warp_spec_t': _capi.WarpSpec, 'dswx_warp_out_t': _capi.WarpOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for st, cls in fields.items():
        for n, _ in cls._fields_:
            lines.append(f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));')
        lines.append(f'  printf("{st}.sizeof %zu\\n", sizeof({st}));')
    lines += ['  printf("words %d shift %d outside %u\\n", DSWX_WARP_HEAD_WORDS, DSWX_WARP_MAX_SHIFT, DSWX_WARP_OUTSIDE);', '  return 0;', '}']
    (tmp_path / 'off.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'off.c'), '-o', str(tmp_path / 'off')], check=True)
    got = dict(l.split(' ', 1) for l in subprocess.run([str(tmp_path / 'off')], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in fields.items():
        assert int(got[f'{st}.sizeof']) == ctypes.sizeof(cls)
        for n, _ in cls._fields_:
            assert int(got[f'{st}.{n}']) == getattr(cls, n).offset, (st, n)
    assert got['words'] == f'{_capi.WARP_HEAD_WORDS} shift {_capi.WARP_MAX_SHIFT} outside {_capi.WARP_OUTSIDE}' and _capi.WARP_HEAD_WORDS == 8


# ---- the position walk of the kernel: meshes of every slope, sign and edge ---------------------------------------------------
# The builders, the cases and their conditions live here, where the host entry is pinned on them (no GPU needed);
# tests/test_gpu_warp.py runs the same cases through dswx_warp_device against the host entry.

UNIT = 16                                                    # destination pixels per thread of dswx_warp_k (_capi.WARP_UNIT)
SLOPES = (85, 102, 256, 384, 512, 640, 768, 1021, 1023)      # 1/256 source pixel per destination pixel, all below four pixels
DECIMATIONS = (1024, 1280, 4096)                             # four pixels and more: the 64-bit form
ROTATIONS = (30, 45, 87, 177, 183)
WALK_SRCS = ((100, 257), (300, 470))
ENTER_K = (1, 15, 16, 59, 60, 61, 127, 128, 129, 130, 200)
ENTER_SLOPES = (256, 512, 1021)
FAR = 1 << 22                                                # source pixels: nodes near 2^30


def affine_mesh(dst, shift, xc, yc):
    """The mesh whose node for destination pixel (X, Y) is (ax * X + bx * Y + cx, ay * X + by * Y + cy), xc = (ax, bx, cx) and
    yc = (ay, by, cy) integers in 1/256 source pixel (per destination pixel): fractional slopes are exact, and so is every
    interpolated position, a bilinear mesh being exact on an affine function."""
    mh, mw = mesh_shape(dst, shift)
    step = 1 << shift
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) * step, np.arange(mh, dtype=np.int64) * step)
    nodes = np.stack([int(xc[0]) * X + int(xc[1]) * Y + int(xc[2]), int(yc[0]) * X + int(yc[1]) * Y + int(yc[2])], axis=-1)
    assert nodes.min() >= INT32_MIN and nodes.max() <= INT32_MAX, (xc, yc)
    return nodes.astype(np.int32)


def rotation_mesh(dst, shift, src, degrees, scale=1.0):
    """make_mesh('rotation') with the angle as a parameter: the middle of the destination on the middle of the source, turned by
    `degrees` and magnified by `scale` source pixels per destination pixel."""
    mh, mw = mesh_shape(dst, shift)
    step = 1 << shift
    jj, ii = np.meshgrid(np.arange(mw, dtype=np.int64) * step, np.arange(mh, dtype=np.int64) * step)
    a = math.radians(degrees)
    dx, dy = 256 * jj + 128 - 128.0 * dst[1], 256 * ii + 128 - 128.0 * dst[0]
    x = np.rint(128.0 * src[1] + scale * (math.cos(a) * dx - math.sin(a) * dy)).astype(np.int64)
    y = np.rint(128.0 * src[0] + scale * (math.sin(a) * dx + math.cos(a) * dy)).astype(np.int64)
    return np.stack([x, y], axis=-1).astype(np.int32)


def unit_paths(mesh, shift, dst, src):
    """bool [dst_h, ceil(dst_w / 16)]: the unit of 16 destination pixels takes the narrow (32-bit) form of dswx_warp_k -- by the
    kernel's statement of its rule: both sides of the raster below 2^23 and |bx|, |by| < 1 << (2 * shift + 10), with b recomputed
    here in int64 from the four nodes of the unit's cell as dswx_mesh_rule.h states it, gy * (v01 - v00) + hy * (v11 - v10),
    gy = step - fy, hy = fy.  Shift >= 4 only: a unit lies in one cell.  This INFERS the path; nothing the device does is
    observed, so a kernel that took the other form with the same bits would pass.  What is observed is that the units of both
    kinds give the host entry's bits."""
    assert shift >= 4
    dh, dw = dst
    m = np.asarray(mesh).astype(np.int64)
    assert m.shape == mesh_shape(dst, shift) + (2,)
    step = 1 << shift
    Y, X = np.arange(dh, dtype=np.int64)[:, None], np.arange(0, dw, UNIT, dtype=np.int64)[None, :]
    i, fy, j = Y >> shift, Y & (step - 1), X >> shift
    lim = 1 << (2 * shift + 10)
    narrow = np.full((dh, X.shape[1]), src[0] < (1 << 23) and src[1] < (1 << 23))
    for k in range(2):
        v = m[:, :, k]
        b = (step - fy) * (v[i, j + 1] - v[i, j]) + fy * (v[i + 1, j + 1] - v[i + 1, j])
        narrow &= np.abs(b) < lim
    return narrow


def whole_units(index, dst):
    """int64 [dst_h, dst_w // 16, 16]: the source indices of the whole units of one tile, and which of them lie inside."""
    u = np.asarray(index).reshape(dst)[:, :dst[1] // UNIT * UNIT].reshape(dst[0], -1, UNIT)
    return u.astype(np.int64), u != OUTSIDE


def fit_offsets(dst, xs, ys, src):
    """(cx, cy) for the linear parts xs = (ax, bx), ys = (ay, by): a coordinate whose extent over the destination is 1.25 sides
    of the raster or more is centred on it and hangs over both edges; a shorter one lies with a fifth of its extent in front of
    the first row or column, where positions are negative.  An odd number of 1/256 is added: no position is a pixel's centre."""
    out = []
    for (a, b), side, odd in ((xs, src[1], 37), (ys, src[0], 91)):
        ends = [a * X + b * Y for X in (0, dst[1] - 1) for Y in (0, dst[0] - 1)]
        lo, hi = min(ends), max(ends)
        out.append((128 * side - (lo + hi) // 2 if hi - lo >= 320 * side else -lo - (hi - lo) // 5) + odd)
    return out


def axis_slice(o, m, n, size):
    """(slice of the destination, slice of the source) along one axis for source coordinate o + m * k of destination
    coordinate k < n, m != 0: where that lies inside 0 .. size - 1; None where none does."""
    v = o + m * np.arange(n)
    ok = np.flatnonzero((v >= 0) & (v < size))
    if not len(ok):
        return None
    k0, k1 = int(ok[0]), int(ok[-1]) + 1
    assert len(ok) == k1 - k0
    stop = int(v[k1 - 1]) + (1 if m > 0 else -1)
    return slice(k0, k1), slice(int(v[k0]), stop if stop >= 0 else None, m)


def closed_form(case, tiles, fill):
    """`dst` of a case whose coefficients are whole pixels, by numpy slices: family 'x' is src[:, oy + q * Y, ox + m * X] -- a
    slice, [::-1] and [::p, ::p] in one -- and family 'y' the transpose of src[:, oy + m * X, ox + q * Y]."""
    fam, m, q, ox, oy = case['whole']
    dh, dw = case['dst']
    H, W = case['src']
    want = np.full((len(tiles), dh, dw), fill, dtype=tiles.dtype)
    if fam == 'x':
        rows, cols = axis_slice(oy, q, dh, H), axis_slice(ox, m, dw, W)
        if rows and cols:
            want[:, rows[0], cols[0]] = tiles[:, rows[1], cols[1]]
    else:
        rows, cols = axis_slice(oy, m, dw, H), axis_slice(ox, q, dh, W)
        if rows and cols:
            want[:, cols[0], rows[0]] = tiles[:, rows[1], cols[1]].transpose(0, 2, 1)
    return want


def axis_case(fam, slope, shift, src, dst_h=21):
    """One coordinate runs along the destination's rows at `slope` (family 'x': the column, 'y': the row, the column standing
    still: transposes and quarter turns), the other along its columns in whole pixels, 1.3 sides of the raster over the
    destination's height.  The destination is as wide as 1.5 sides of the raster take at this slope, between 53 and 293."""
    along, across = (src[1], src[0]) if fam == 'x' else (src[0], src[1])
    dw = min(max(-(-384 * along // abs(slope)), 48), 288) // UNIT * UNIT + 5
    dst = (dst_h, dw)
    q = 256 * -(-14 * across // (10 * dst_h))
    xs, ys = ((slope, 0), (0, q)) if fam == 'x' else ((0, q), (slope, 0))
    cx, cy = fit_offsets(dst, xs, ys, src)
    traits = ['share', 'narrow' if abs(slope) < 1024 else 'wide']
    if abs(slope) < 256:
        traits.append('repeats')
    if slope == 256:
        traits.append('runs and cuts' if fam == 'x' else 'no run')
    if slope == -256:
        traits.append('descends by 1' if fam == 'x' else 'descends by a row')
    case = dict(name=(fam, slope), shift=shift, src=src, dst=dst, mesh=affine_mesh(dst, shift, xs + (cx,), ys + (cy,)), traits=traits)
    if slope % 256 == 0:
        case['whole'] = (fam, slope // 256, q // 256, cx >> 8, cy >> 8)
    return case


def slope_cases(shift, src, slopes=SLOPES, bent=True):
    """Section (a): both families at every slope and sign; with `bent`, the shears x = X + 0.3 Y with y = Y + 0.25 X, each sign
    flipped in turn, on a destination of 9 rows that hangs over the raster's left and right edges, and the rotations, magnified
    until the destination's long side is 1.3 widths of the raster."""
    for fam in 'xy':
        for slope in slopes:
            for sign in (1, -1):
                yield axis_case(fam, sign * slope, shift, src)
    if not bent:
        return
    dst = (9, (1024 if src[1] < 300 else 2048) + 17)
    for xs, ys in (((256, 77), (64, 256)), ((-256, 77), (64, 256)), ((256, -77), (64, 256)), ((256, 77), (-64, 256)), ((256, 77), (64, -256)),
                   ((-256, -77), (-64, -256))):
        cx, cy = fit_offsets(dst, xs, ys, src)
        # the rows that the columns inside the raster take: around the raster's middle
        cy = 128 * src[0] - (ys[0] * (128 * src[1] - cx) // xs[0] + ys[1] * (dst[0] // 2)) + 91
        yield dict(name=('shear', xs, ys), shift=shift, src=src, dst=dst, mesh=affine_mesh(dst, shift, xs + (cx,), ys + (cy,)), traits=['share', 'narrow'])
    dst = (70, 300)
    for deg in ROTATIONS:
        yield dict(name=('rotation', deg), shift=shift, src=src, dst=dst, mesh=rotation_mesh(dst, shift, src, deg, 1.3 * src[1] / dst[1]),
                   traits=['share', 'narrow'])


def decimation_cases(shift, src):
    """Section (e) on an ordinary raster: slopes of 4, 5 and 16 pixels, both signs and families: every unit in the 64-bit form."""
    return slope_cases(shift, src, DECIMATIONS, bent=False)


def switch_cases(shift, src):
    """Section (b): meshes built from node DIFFERENCES along a row around lim = 4 * 256 * step, the difference at which
    b = step * (v01 - v00) reaches 1 << (2 * shift + 10): lim - 1 (narrow), lim and lim + 1 (wide; the comparison is strict), in
    x only, in y only, in both, and negated.  The twisted meshes have lim - 16 on one edge of every cell and lim + 16 on the
    other, alternating along both axes of the mesh, so b = lim +- 16 * (2 fy - step) crosses the limit at the middle row of a
    cell.  A destination has at most 70 rows: at shift 4 (70 x 300) the crossing lies between the rows of every cell; at shift 8
    its row 128 cannot, and the destination is 9 x 2065, where neighbouring cells of the row of cells lie on either side."""
    step = 1 << shift
    lim = 4 * 256 * step
    for twisted in (False, True):
        dst = (9, 2 * 1024 + 17) if twisted and shift == 8 else (70, 300)
        mh, mw = mesh_shape(dst, shift)
        i, j = np.meshgrid(np.arange(mh, dtype=np.int64), np.arange(mw - 1, dtype=np.int64), indexing='ij')
        for delta in ((16,) if twisted else (-1, 0, 1)):
            d = lim - delta * (1 - 2 * ((i + j) & 1)) if twisted else lim + delta + 0 * i      # [mh, mw - 1] differences along the rows
            for where in ('x', 'y', 'both'):
                for sign in (1, -1):
                    nodes = np.zeros((mh, mw, 2), dtype=np.int64)
                    for k, side in ((0, src[1]), (1, src[0])):
                        if where in ('xy'[k], 'both'):
                            walk = np.concatenate([np.zeros((mh, 1), dtype=np.int64), np.cumsum(sign * d, axis=1)], axis=1)
                            span = lim * (dst[1] // step + 1)
                            nodes[:, :, k] = walk + (-(span // 5) if sign > 0 else 256 * side + span // 5) + 41
                            if where == 'both' and k == 1:
                                nodes[:, :, k] += 256 * step * np.arange(mh, dtype=np.int64)[:, None]
                        else:                                                                 # a pixel per destination row, from row or column 3
                            nodes[:, :, k] = (256 * step * np.arange(mh, dtype=np.int64) + 256 * 3 + 128)[:, None]
                    assert nodes.min() >= INT32_MIN and nodes.max() <= INT32_MAX
                    traits = ['some inside', 'both sides' if twisted else ('narrow' if delta < 0 else 'wide')]
                    if twisted and shift == 4:
                        traits.append('crosses inside cells')
                    yield dict(name=('switch', 'twisted' if twisted else delta, where, sign), shift=shift, src=src, dst=dst,
                               mesh=nodes.astype(np.int32), traits=traits)


def entering_cases(src):
    """Section (c), shift 4: the first pixel of the first unit of every row lies k source pixels before the left edge and the
    row walks into the raster at the slope; the same before the top edge with the slope in y, and mirrored past the right and
    the bottom edge with the slope negated; the other coordinate is three pixels inside.  The kernel clamps the unit's first
    pixel to -128 (k >= 129).  And translations by 2^22 source pixels either way: nodes near +-2^30."""
    H, W = src
    dst, still = (5, 14 * UNIT + 5), (0, 256, 256 * 3 + 128)
    for slope in ENTER_SLOPES:
        for k in ENTER_K:
            traits = ['some inside'] + (['first unit enters'] if k <= 59 and slope == 1021 else []) + (['first unit outside'] if k >= 128 else [])
            yield dict(name=('left', slope, k), shift=4, src=src, dst=dst, traits=traits, mesh=affine_mesh(dst, 4, (slope, 0, -256 * k + 128), still))
            yield dict(name=('right', slope, k), shift=4, src=src, dst=dst, traits=traits,
                       mesh=affine_mesh(dst, 4, (-slope, 0, 256 * (W - 1 + k) + 128), still))
            yield dict(name=('top', slope, k), shift=4, src=src, dst=dst, traits=traits, mesh=affine_mesh(dst, 4, still, (slope, 0, -256 * k + 128)))
            yield dict(name=('bottom', slope, k), shift=4, src=src, dst=dst, traits=traits,
                       mesh=affine_mesh(dst, 4, still, (-slope, 0, 256 * (H - 1 + k) + 128)))
    for slope in (256, 768):
        for far in (256 * FAR, -256 * FAR):
            yield dict(name=('far x', slope, far), shift=4, src=src, dst=dst, traits=['nothing inside'], mesh=affine_mesh(dst, 4, (slope, 0, far + 128), still))
            yield dict(name=('far y', slope, far), shift=4, src=src, dst=dst, traits=['nothing inside'], mesh=affine_mesh(dst, 4, still, (slope, 0, far + 128)))


def flat_mesh(dst, shift, src_w, move):
    """Every node is the centre of the source pixel (of a raster `src_w` wide) whose flat index is that of the node's
    destination pixel plus `move`."""
    mh, mw = mesh_shape(dst, shift)
    step = 1 << shift
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) * step, np.arange(mh, dtype=np.int64) * step)
    f = Y * dst[1] + X + move
    return np.stack([256 * (f % src_w) + 128, 256 * (f // src_w) + 128], axis=-1).astype(np.int32)


FLAT_DST, FLAT_MOVES = (20, 48), (0, 7, 16)


def flat_cases():
    """Section (d).  Shift 0, a source of 24 x 40 and a destination of 20 x 48: every unit is 16 consecutive elements, one of
    every five across a row's end (two with an odd move); moved on by 7 and by 16 elements the last units run off the end of the tile.
    Shift 3 with a source 8 wide (120 x 8): every node has the same column (48 and the step are multiples of 8) and its row is
    linear in X and Y, so the interpolated positions are exact -- column `move`, row (f + 4) >> 3 of the pixel with flat index
    f -- but NOT consecutive: the positions of a mesh are continuous across its nodes, so at a shift above 0 the column cannot
    fall back by a row's width between two pixels, and a run across a row's end exists at shift 0 alone."""
    n = FLAT_DST[0] * FLAT_DST[1]
    for move in FLAT_MOVES:
        want = np.arange(n, dtype=np.int64) + move
        yield dict(name=('flat', 0, move), shift=0, src=(24, 40), dst=FLAT_DST, mesh=flat_mesh(FLAT_DST, 0, 40, move), traits=['flat'], flat=want)
        want = 8 * ((np.arange(n, dtype=np.int64) + 4) >> 3) + move
        yield dict(name=('flat', 3, move), shift=3, src=(120, 8), dst=FLAT_DST, mesh=flat_mesh(FLAT_DST, 3, 8, move), traits=['flat'], flat=want)


LONG_SIDE = 1 << 23
LONG_DST = (33, 300)


def long_side_cases(src):
    """Section (e) on the rasters of 2 x 2^23 and 2^23 x 2: the slope along the long side, the last node of a row (or the
    first, for the negative slope) 50 / 256 of a pixel in front of INT32_MAX, the end of the raster; the short side takes 8
    destination rows per pixel from one pixel outside."""
    long_x = src[1] == LONG_SIDE
    assert src in ((2, LONG_SIDE), (LONG_SIDE, 2))
    last = (mesh_shape(LONG_DST, 4)[1] - 1) * 16
    for slope in (-256, 512, 768, 1021):
        along = (slope, 0, INT32_MAX - 50 - max(slope, 0) * last)
        short = (0, 32, -256)
        yield dict(name=('long side', src, slope), shift=4, src=src, dst=LONG_DST, traits=['some inside', 'wide'],
                   mesh=affine_mesh(LONG_DST, 4, along, short) if long_x else affine_mesh(LONG_DST, 4, short, along))


def check_traits(case, ref):
    """What makes a case worth running, asserted on the reference's outputs of its first tile: conditions, not measurements."""
    head, dst, src, shift = ref['head'][0], case['dst'], case['src'], case['shift']
    name = case['name']
    idx, inside = whole_units(ref['src_index'][0], dst)
    whole = inside.all(axis=2)
    step = np.diff(idx, axis=2)
    for trait in case['traits']:
        if trait == 'share':
            assert 0.1 < int(head[1]) / int(head[0]) < 0.9, (name, head[:3])
        elif trait == 'some inside':
            assert 0 < head[1] < head[0], (name, head[:3])
        elif trait == 'nothing inside':
            assert head[1] == 0, (name, head[:3])
        elif trait in ('narrow', 'wide', 'both sides', 'crosses inside cells'):
            if shift < 4:
                continue                                                     # (the FINE instantiation has one form)
            narrow = unit_paths(case['mesh'], shift, dst, src)
            if trait == 'narrow':
                assert narrow.all(), name
            elif trait == 'wide':
                assert not narrow.any(), name
            elif trait == 'both sides':
                assert 0.25 <= narrow.mean() <= 0.75, (name, narrow.mean())
            else:
                cells = narrow[:dst[0] >> shift << shift].reshape(dst[0] >> shift, 1 << shift, -1)
                assert (cells.any(axis=1) & ~cells.all(axis=1)).all(), name
        elif trait == 'repeats':
            assert ((step == 0) & inside[:, :, 1:] & inside[:, :, :-1]).any(), name
        elif trait == 'runs and cuts':
            runs = whole & np.all(step == 1, axis=2)
            assert runs.any() and (~runs).any(), name
        elif trait == 'no run':
            assert not (whole & np.all(step == 1, axis=2)).any() and (whole & np.all(step == src[1], axis=2)).any(), name
        elif trait == 'descends by 1':
            assert (whole & np.all(step == -1, axis=2)).any(), name
        elif trait == 'descends by a row':
            assert (whole & np.all(step == -src[1], axis=2)).any(), name
        elif trait == 'first unit enters':
            assert inside[:, 0, :].any(), name
        elif trait == 'first unit outside':
            assert not inside[:, 0, :].any(), name
        elif trait == 'flat':
            want = np.where(case['flat'] < src[0] * src[1], case['flat'], OUTSIDE)
            assert np.array_equal(ref['src_index'][0].reshape(-1), want), name
            if shift == 0:                                                   # whole units across a source row's end
                assert (whole & np.all(step == 1, axis=2) & (idx[:, :, 0] // src[1] != idx[:, :, -1] // src[1])).sum() >= 10, name
        else:
            raise AssertionError(trait)


def pin_on_the_host(case, rng, planes, n=2):
    """dswx_warp_host on a case against the loop in Python ints and warp_tiles, every output and element size; its closed form;
    its conditions."""
    shift, src, dst, mesh = case['shift'], case['src'], case['dst'], case['mesh']
    pos = loop_positions(mesh, shift, dst)
    sx, sy = warp.positions(mesh, shift, dst)
    assert [p[0] for p in pos] == sx.reshape(-1).tolist() and [p[1] for p in pos] == sy.reshape(-1).tolist(), case['name']
    ebs = (1,) if src[0] * src[1] > 1 << 20 else (1, 2, 4)
    for eb in ebs:
        if (src, eb) not in planes:                                          # one plane per raster and element size
            planes[src, eb] = random_tiles(rng, 1 if len(ebs) == 1 else n, src, eb)
        tiles = planes[src, eb]
        fill = outside_of(tiles.dtype)
        got = _capi.warp_host(tiles, mesh, Spec(eb, shift, OUT_WORD), dst)
        ref = warp_tiles(tiles, mesh, shift, dst, OUT_WORD)
        for k in warp.OUTPUTS:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (case['name'], eb, k)
        if len(ebs) == 1:                                                    # (a raster of 2^24 elements is not made a list)
            c, r = np.array([p[0] >> 8 for p in pos]), np.array([p[1] >> 8 for p in pos])
            ok = (c >= 0) & (c < src[1]) & (r >= 0) & (r < src[0])
            idx = np.where(ok, r * src[1] + c, OUTSIDE)
            assert np.array_equal(got['src_index'][0].reshape(-1), idx) and got['head'][0, 1] == ok.sum()
            assert np.array_equal(got['dst'][0].reshape(-1)[ok], tiles[0].reshape(-1)[idx[ok]]) and np.all(got['dst'][0].reshape(-1)[~ok] == fill)
        else:
            t = eb % n
            d, idx, head = loop_warp(tiles[t], pos, dst, fill)
            assert np.array_equal(got['dst'][t], d) and np.array_equal(got['src_index'][t], idx) and np.array_equal(got['head'][t], head), (case['name'], eb)
        if 'whole' in case:
            assert np.array_equal(got['dst'], closed_form(case, tiles, fill)), (case['name'], eb, 'closed form')
        if 'flat' in case and case['shift'] == 0 and case['name'][2] == 0:
            assert np.array_equal(got['dst'], tiles.reshape((-1,) + dst))
    check_traits(case, got)


WALK_SECTIONS = {
    'slopes at shift 4': lambda: (c for src in WALK_SRCS for c in slope_cases(4, src)),
    'slopes at shift 6': lambda: (c for src in WALK_SRCS for c in slope_cases(6, src)),
    'slopes at shift 8': lambda: (c for src in WALK_SRCS for c in slope_cases(8, src)),
    'fine':lambda: (c for s in (0, 3) for c in slope_cases(s, WALK_SRCS[0])),
    'switch': lambda: (c for s in (4, 8) for c in switch_cases(s, WALK_SRCS[1])),
    'entering': lambda: entering_cases(WALK_SRCS[0]),
    'flat': flat_cases,
    'decimation': lambda: (c for s in (4, 8) for c in decimation_cases(s, WALK_SRCS[1])),
    'long side': lambda: (c for src in ((2, LONG_SIDE), (LONG_SIDE, 2)) for c in long_side_cases(src)),
}


@pytest.mark.parametrize('section', list(WALK_SECTIONS))
def test_the_meshes_of_the_position_walk_on_the_host(section):
    """Every mesh that tests/test_gpu_warp.py drives the kernel's position walk with, at its sizes, through dswx_warp_host: equal
    to the loop in Python ints and to warp_tiles on every output, to numpy slices where the coefficients are whole pixels, and
    with every condition that makes the case worth running on the device."""
    rng = np.random.default_rng(7000 + len(section))
    count, planes = 0, {}
    for case in WALK_SECTIONS[section]():
        pin_on_the_host(case, rng, planes)
        count += 1
    assert count >= 6, count


def test_unit_paths_and_the_builders_say_what_they_claim():
    """affine_mesh is the node formula; unit_paths follows the raster's sides, the limit of four pixels and its strictness."""
    m = affine_mesh((5, 9), 2, (3, -7, 11), (-256, 1023, -5))
    assert m.shape == (3, 4, 2) and m[2, 3].tolist() == [3 * 12 - 7 * 8 + 11, -256 * 12 + 1023 * 8 - 5]
    sx, sy = warp.positions(m, 2, (5, 9))
    assert sx[4, 7] == 3 * 7 - 7 * 4 + 11 and sy[3, 8] == -256 * 8 + 1023 * 3 - 5
    dst = (20, 40)
    for shift in (4, 8):
        lim = 4 * 256 << shift
        for d, narrow in ((lim - 1, True), (lim, False), (1 - lim, True), (-lim, False)):
            mesh = np.zeros(mesh_shape(dst, shift) + (2,), dtype=np.int64)
            mesh[:, :, 1] = d * np.arange(mesh.shape[1])
            assert unit_paths(mesh, shift, dst, (100, 100)).shape == (20, 3)
            assert unit_paths(mesh, shift, dst, (100, 100)).all() == narrow and unit_paths(mesh, shift, dst, (100, 100)).any() == narrow
            assert not unit_paths(mesh, shift, dst, (1 << 23, 2)).any() and not unit_paths(mesh, shift, dst, (2, 1 << 23)).any()
            assert unit_paths(mesh, shift, dst, ((1 << 23) - 1, 2)).all() == narrow


# ---- the projection, pinned without PROJ ---------------------------------------------------------------------------------

A, F, K0 = warp.WGS84_A, 1.0 / warp.WGS84_INV_F, warp.UTM_K0
E2 = F * (2.0 - F)
MM = 1e-3                                                    # the bar of (a) and (b): 1 mm, below 1/100 of the mesh quantum 30 m / 256


def test_tm_round_trip():
    """(a) inverse(forward) over |lat| <= 84 degrees, |lon - lon0| <= 6 degrees: below 1 mm on the ground."""
    lat, dlon = np.meshgrid(np.linspace(-84.0, 84.0, 337), np.linspace(-6.0, 6.0, 241), indexing='ij')
    worst = 0.0
    for lon0 in (-177.0, 9.0, 15.0, 177.0):
        e, n = warp.tm_forward(lon0 + dlon, lat, lon0)
        lon, la = warp.tm_inverse(e, n, lon0)
        metres = np.hypot(np.radians(lon - lon0 - dlon) * A * np.cos(np.radians(lat)), np.radians(la - lat) * A)
        worst = max(worst, float(metres.max()))
        e2, n2 = warp.tm_forward(lon, la, lon0)
        worst = max(worst, float(np.hypot(e2 - e, n2 - n).max()))
    print(f'round trip: worst {worst * 1e3:.6f} mm')
    assert worst < MM


def test_tm_central_meridian_is_k0_times_the_meridian_arc():
    """(b) on the central meridian the northing is k0 times the meridian arc, here by quadrature of the meridional radius of
    curvature M(phi) = a (1 - e^2) / (1 - e^2 sin^2 phi)^(3/2)."""
    from scipy.integrate import quad
    worst = 0.0
    for lat in (-84.0, -60.0, -33.3, -1.0, 0.0, 0.5, 12.0, 45.0, 59.9, 72.0, 84.0):
        arc, err = quad(lambda p: A * (1 - E2) / (1 - E2 * math.sin(p) ** 2) ** 1.5, 0.0, math.radians(lat), epsabs=1e-9, epsrel=1e-14)
        e, n = warp.tm_forward(21.0, lat, 21.0)
        assert abs(float(e)) < 1e-6 and err < 1e-5
        worst = max(worst, abs(float(n) - K0 * arc))
    print(f'meridian arc: worst {worst * 1e3:.6f} mm')
    assert worst < MM


def test_tm_is_conformal_and_its_scale_is_k0_on_the_central_meridian():
    """(c) the finite-difference Jacobian with respect to metres on the ellipsoid is a similarity (equal columns at a right
    angle), and on the central meridian its scale is the closed-form point scale k0."""
    h = 1e-5                                                 # degrees: about a metre
    lat, dlon = np.meshgrid(np.linspace(-80.0, 80.0, 41), np.linspace(-5.0, 5.0, 21), indexing='ij')
    phi = np.radians(lat)
    nu = A / np.sqrt(1 - E2 * np.sin(phi) ** 2)              # prime vertical radius
    rho = A * (1 - E2) / (1 - E2 * np.sin(phi) ** 2) ** 1.5  # meridional radius
    e1, n1 = warp.tm_forward(dlon + h, lat, 0.0)
    e0, n0 = warp.tm_forward(dlon - h, lat, 0.0)
    ex, nx = (e1 - e0) / (2 * np.radians(h) * nu * np.cos(phi)), (n1 - n0) / (2 * np.radians(h) * nu * np.cos(phi))
    e1, n1 = warp.tm_forward(dlon, lat + h, 0.0)
    e0, n0 = warp.tm_forward(dlon, lat - h, 0.0)
    ey, ny = (e1 - e0) / (2 * np.radians(h) * rho), (n1 - n0) / (2 * np.radians(h) * rho)
    # a similarity: (ex, nx) rotated by a quarter turn is (ey, ny)
    assert float(np.abs(ex - ny).max()) < 2e-7 and float(np.abs(nx + ey).max()) < 2e-7
    scale = np.hypot(ex, nx)
    centre = dlon == 0.0
    assert centre.any() and float(np.abs(scale[centre] - K0).max()) < 2e-7
    assert float(scale.min()) > K0 - 2e-7 and float(scale.max()) < 1.01          # it grows away from the central meridian


def redfearn(lon_deg, lat_deg, lon0_deg):
    """The forward mapping a second time, by the older series in powers of the longitude difference (Redfearn 1948 as printed
    by Snyder 1987, eqs. 8-9, 8-10, 3-21): terms to the 6th (easting: 5th) power only."""
    phi, lam = np.radians(lat_deg), np.radians(np.asarray(lon_deg) - lon0_deg)
    ep2 = E2 / (1 - E2)
    N = A / np.sqrt(1 - E2 * np.sin(phi) ** 2)
    T, C, Av = np.tan(phi) ** 2, ep2 * np.cos(phi) ** 2, lam * np.cos(phi)
    e4, e6 = E2 ** 2, E2 ** 3
    M = A * ((1 - E2 / 4 - 3 * e4 / 64 - 5 * e6 / 256) * phi - (3 * E2 / 8 + 3 * e4 / 32 + 45 * e6 / 1024) * np.sin(2 * phi)
             + (15 * e4 / 256 + 45 * e6 / 1024) * np.sin(4 * phi) - (35 * e6 / 3072) * np.sin(6 * phi))
    x = K0 * N * (Av + (1 - T + C) * Av ** 3 / 6 + (5 - 18 * T + T ** 2 + 72 * C - 58 * ep2) * Av ** 5 / 120)
    y = K0 * (M + N * np.tan(phi) * (Av ** 2 / 2 + (5 - T + 9 * C + 4 * C ** 2) * Av ** 4 / 24
                                     + (61 - 58 * T + T ** 2 + 600 * C - 330 * ep2) * Av ** 6 / 720))
    return x, y


# What the two statements disagree by over |lat| <= 84, |lon - lon0| <= 4.5 degrees, measured on the CPU (the test prints it):
# 1.572 mm, worst at latitude 0 and 4.5 degrees from the central meridian; 0.956 mm within 3 degrees.  That is the truncation of
# the Redfearn series, not of the Krueger series: its first omitted easting term is k0 N A^7 (61 - 479 T + 179 T^2 - T^3) / 5040
# with A = (lon - lon0) cos(lat), which at the equator and 4.5 degrees is 0.9996 * 6378137 * 0.0785^7 * 61 / 5040 = 1.4 mm, and
# its meridian arc is cut at e^6.  The margins are not taken from the figures above: 10 mm is a twelfth of the mesh quantum of
# 117 mm and seven times that omitted term; inside the zone proper (3 degrees) the omitted term is (3 / 4.5)^7 = 1 / 17 of it
# and the margin is 2 mm.  A wrong coefficient of order n^3 or lower in the Krueger series moves points by a n^3 = 3 cm or more
# and fails either; the n^4 .. n^6 coefficients (a n^4 = 0.05 mm) are pinned only by the round trip and the meridian arc.
REDFEARN_MARGIN_M = 0.010
REDFEARN_ZONE_MARGIN_M = 0.002


def test_tm_against_the_redfearn_series():
    """(d) over |lon - lon0| <= 4.5 degrees, what a neighbouring zone's tile needs."""
    lat, dlon = np.meshgrid(np.linspace(-84.0, 84.0, 169), np.linspace(-4.5, 4.5, 181), indexing='ij')
    e, n = warp.tm_forward(dlon, lat, 0.0)
    x, y = redfearn(dlon, lat, 0.0)
    d = np.hypot(e - x, n - y)
    k = np.unravel_index(int(d.argmax()), d.shape)
    print(f'Redfearn: worst {d[k] * 1e3:.3f} mm at lat {lat[k]} dlon {dlon[k]}; within 3 degrees {d[np.abs(dlon) <= 3.0].max() * 1e3:.3f} mm')
    assert float(d.max()) < REDFEARN_MARGIN_M
    assert float(d[np.abs(dlon) <= 3.0].max()) < REDFEARN_ZONE_MARGIN_M


def test_affine_mesh_against_the_closed_form():
    src_gt = (600000.0, 30.0, 0.0, 4100040.0, 0.0, -30.0)
    # a shifted origin (whole and fractional pixels), a coarser and a finer lattice
    for dst_gt, dst, shift in (((600000.0 + 90.0, 30.0, 0.0, 4100040.0 - 60.0, 0.0, -30.0), (40, 50), 4),
                               ((600000.0 + 7.5, 30.0, 0.0, 4100040.0 + 15.0, 0.0, -30.0), (33, 47), 3),
                               ((600000.0, 60.0, 0.0, 4100040.0, 0.0, -60.0), (20, 25), 2),
                               ((600000.0 - 10.0, 10.0, 0.0, 4100040.0, 0.0, -10.0), (90, 100), 6)):
        mesh = warp.affine_mesh(src_gt, dst_gt, dst, shift)
        mh, mw = mesh_shape(dst, shift)
        assert mesh.shape == (mh, mw, 2) and mesh.dtype == np.int32
        for i, j in ((0, 0), (mh - 1, mw - 1), (mh // 2, 1)):
            X, Y = j << shift, i << shift
            x, y = dst_gt[0] + (X + 0.5) * dst_gt[1], dst_gt[3] + (Y + 0.5) * dst_gt[5]
            assert mesh[i, j].tolist() == [round(256 * (x - src_gt[0]) / 30.0), round(256 * (y - src_gt[3]) / -30.0)]
    # whole-pixel shift: the slice; twice the pixel size: every second pixel (the centre lies on a boundary: the pixel behind it)
    src = np.arange(40 * 50, dtype=np.uint16).reshape(1, 40, 50)
    mesh = warp.affine_mesh(src_gt, (600000.0 + 90.0, 30.0, 0.0, 4100040.0 - 60.0, 0.0, -30.0), (40, 50), 4)
    got = warp_tiles(src, mesh, 4, (40, 50), 9)['dst'][0]
    assert np.array_equal(got[:38, :47], src[0, 2:, 3:]) and np.all(got[38:] == 9) and np.all(got[:, 47:] == 9)
    mesh = warp.affine_mesh(src_gt, (600000.0, 60.0, 0.0, 4100040.0, 0.0, -60.0), (20, 25), 2)
    assert np.array_equal(warp_tiles(src, mesh, 2, (20, 25), 9)['dst'][0], src[0, 1::2, 1::2])
    with pytest.raises(ValueError, match='rotated'):
        warp.affine_mesh((0.0, 30.0, 0.1, 0.0, 0.0, -30.0), src_gt, (4, 4), 1)
    with pytest.raises(ValueError, match='rotated'):
        warp.affine_mesh(src_gt, (0.0, 30.0, 0.0, 0.0, 0.2, -30.0), (4, 4), 1)


def test_utm_mesh():
    """Equal zones give affine_mesh; two zones: the nodes and the reported deviation against a brute-force evaluation through
    tm_inverse / tm_forward; what is not WGS 84 / UTM is refused with a message; positions beyond int32 are clamped."""
    src_gt = (199980.0, 30.0, 0.0, 5000040.0, 0.0, -30.0)            # a tile on the west side of zone 33, about 45 degrees N
    dst_gt = (699960.0, 30.0, 0.0, 5000040.0, 0.0, -30.0)            # a tile on the east side of zone 32
    dst = (300, 470)
    for shift in (4, 6):
        mesh, dev = warp.utm_mesh(src_gt, 32633, src_gt, 32633, dst, shift)
        assert np.array_equal(mesh, warp.affine_mesh(src_gt, src_gt, dst, shift)) and dev <= 0.5
        mesh, dev = warp.utm_mesh(src_gt, 32633, dst_gt, 32632, dst, shift)
        mh, mw = mesh_shape(dst, shift)
        step = 1 << shift

        def exact(X, Y):                                            # destination pixel index (floats allowed) -> 1/256 source pixel
            x, y = dst_gt[0] + (X + 0.5) * 30.0, dst_gt[3] - (Y + 0.5) * 30.0
            lon, lat = warp.tm_inverse(x - 500000.0, y, 9.0)
            e, n = warp.tm_forward(lon, lat, 15.0)
            return 256 * (e + 500000.0 - src_gt[0]) / 30.0, 256 * (n - src_gt[3]) / -30.0
        J, I = np.meshgrid(np.arange(mw) * float(step), np.arange(mh) * float(step))
        ex, ey = exact(J, I)
        assert np.array_equal(mesh[..., 0], np.rint(ex).astype(np.int32)) and np.array_equal(mesh[..., 1], np.rint(ey).astype(np.int32))
        cx, cy = exact(J[:-1, :-1] + step / 2, I[:-1, :-1] + step / 2)
        m = mesh.astype(np.float64)
        mid = (m[:-1, :-1] + m[:-1, 1:] + m[1:, :-1] + m[1:, 1:]) / 4
        brute = float(np.maximum(np.abs(mid[..., 0] - cx), np.abs(mid[..., 1] - cy)).max())
        assert dev == pytest.approx(brute, abs=1e-6) and dev < 2.0          # the mapping is smooth: far below a pixel at these steps
        # the tiles do overlap: zone 33's west edge lies in zone 32's east edge, rotated by a few degrees
        head = warp_tiles(np.zeros((1, 3660, 3660), dtype=np.uint8), mesh, shift, dst)['head'][0]
        assert head[1] > 0
        rot = math.degrees(math.atan2(float(mesh[0, -1, 1] - mesh[0, 0, 1]), float(mesh[0, -1, 0] - mesh[0, 0, 0])))
        assert 1.0 < abs(rot) < 6.0
    # the south: false northing 10,000,000
    mesh, _ = warp.utm_mesh((199980.0, 30.0, 0.0, 6000040.0, 0.0, -30.0), 32733, (699960.0, 30.0, 0.0, 6000040.0, 0.0, -30.0), 32732, (64, 64), 5)
    assert abs(int(mesh[0, 0, 1])) < 256 * 400                       # the same northing band, a few hundred pixels at most
    for bad in (4326, 32600, 32661, 32700, 3857, None, 26915):
        with pytest.raises(ValueError, match='WGS 84 / UTM'):
            warp.utm_mesh(src_gt, bad, dst_gt, 32632, (8, 8), 2)
    with pytest.raises(ValueError, match='rotated'):
        warp.utm_mesh((0.0, 30.0, 1.0, 0.0, 0.0, -30.0), 32633, dst_gt, 32632, (8, 8), 2)
    mesh, _ = warp.utm_mesh((199980.0, 1e-4, 0.0, 5000040.0, 0.0, -1e-4), 32633, dst_gt, 32632, (8, 8), 2)
    assert set(np.unique(mesh).tolist()) <= {INT32_MIN, INT32_MAX}
    assert warp.mesh_between(src_gt, 32633, dst_gt, 32632, dst, 6)[0].shape == mesh_shape(dst, 6) + (2,)
    assert warp.mesh_between(src_gt, None, dst_gt, None, dst, 6)[1] == 0.0
    with pytest.raises(ValueError, match='WGS 84 / UTM'):
        warp.mesh_between(src_gt, 4326, dst_gt, 32632, dst, 6)


def test_epsg_of_reads_the_geokeys():
    from proteus_amd import geotiff
    assert warp.epsg_of(geotiff.geo_tags_from_geotransform((0.0, 30.0, 0.0, 0.0, 0.0, -30.0), epsg=32633)) == 32633
    assert warp.epsg_of({}) is None
