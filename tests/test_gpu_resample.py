"""The resample entry on the GPU: dswx_resample_device against the library's scalar statement (dswx_resample_host;
tests/test_resample.py pins that to numpy, to a loop in Python floats and to exact rationals), EVERY byte of dst, how and head --
both kinds, both methods, shifts 0, 1, 4, 8, the mesh contents and destinations of tests/test_warp.py and one destination of
more than three rectangles of the kernel either way; both tap paths (the source window staged in LDS, taps gathered from global
memory), INFERRED, not observed: the kernel reports nothing about the path a rectangle took (the head's eight words are all
defined), so the test applies the kernel's rule on the host with the rectangle and window sizes the kernel-info string names; raster edges, a source row's end and nodata
pixels inside rectangles and on their borders; float32 subnormals; every subset of outputs, a second call, odd element
addresses, strides, a mesh per tile; a caller's stream; 65535 + 4 tiles; DevicePlane.resample; and the product run with a DEM
in EPSG:4326 against resample_tiles plus the shadow oracle."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py)
    import torch
except ImportError:
    torch = None

from oracle import dswx_oracle as o
from proteus_amd import _capi, dswx_hls as D, geotiff, pipeline, resample, warp
from proteus_amd.resample import BILINEAR, CUBIC, Spec, outside_word, resample_tiles
from proteus_amd.warp import mesh_shape
from tests.test_resample import KINDS, NODATA, OUTSIDE, random_tiles
from tests.test_warp import DSTS, MESHES, SHIFTS, exact_mesh, make_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_synthetic_hls as synth_hls   # noqa: E402

SENT, PAD, GUARD = 0xEE, 0xA5, 256
KEYS = ('dst', 'how', 'head')
RH, RW = _capi.RESAMPLE_RECT_H, _capi.RESAMPLE_RECT_W
RAGGED = (3 * RH + 3, 3 * RW + 5)                 # more than three rectangles either way, ragged in both


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Bufs:
    """Device buffers that a sequence of runs shares: grown on demand, freed at the end."""

    def __init__(self, ctx):
        self.ctx, self.b = ctx, {}

    def get(self, name, n):
        if name not in self.b or self.b[name].nbytes < n:
            if name in self.b:
                self.b[name].free()
            self.b[name] = self.ctx.malloc(max(2 * n, 4096))
        return self.b[name]

    def free(self):
        for b in self.b.values():
            b.free()


def run_device(ctx, bufs, tiles, mesh, spec, dst, want=KEYS, raster=None, off=1, stream=None, twice=False, what=''):
    """One call of dswx_resample_device against dswx_resample_host.  The plane lies `off` ELEMENTS past a 256-byte boundary
    behind a guard, every byte that is not tile data PAD; dst lies `off` elements, how one byte and head one head word past a
    256-byte boundary, every byte of the output buffer SENT beforehand and every byte outside the wanted outputs SENT afterwards."""
    eb = spec.dtype.itemsize
    tiles = np.ascontiguousarray(tiles)
    n = tiles.shape[0]
    H, W = tiles.shape[1:] if raster is None else raster
    dh, dw = dst
    ref = _capi.resample_host(tiles, mesh, spec, dst, raster=raster)
    raw = tiles.view(np.uint8).reshape(-1)
    start = GUARD + off * eb
    shost = np.full(start + raw.size + GUARD, PAD, dtype=np.uint8)
    shost[start:start + raw.size] = raw
    sbuf = bufs.get('src', shost.size)
    sbuf.upload(shost)
    mhost = np.ascontiguousarray(mesh, dtype=np.int32).view(np.uint8).reshape(-1)
    mbuf = bufs.get('mesh', mhost.size + 4)
    if mhost.size:
        mbuf.upload(mhost, offset=4)                                     # 4-byte aligned and no more
    px = n * dh * dw
    where, cursor = {}, 0
    for key, size, shiftby in (('dst', px * eb, off * eb), ('how', px, 1), ('head', n * 64, 8)):
        begin = -(-cursor // 256) * 256 + shiftby
        where[key] = (begin, size)
        cursor = begin + size + 64
    obuf = bufs.get('out', cursor)
    obuf.upload(np.full(cursor, SENT, dtype=np.uint8))
    out = _capi.ResampleOut.of(**{k: obuf.ptr + where[k][0] for k in want})
    for _ in range(2 if twice else 1):
        ctx.resample_device(sbuf.ptr + start, spec, n, H, W, mbuf.ptr + 4, dh, dw, out, stream=stream)
    ctx.synchronize(stream) if stream else ctx.synchronize()
    got = obuf.download(np.uint8, cursor)
    written = np.zeros(cursor, dtype=bool)
    for key in want:
        begin, size = where[key]
        a, b = got[begin:begin + size], ref[key].view(np.uint8).reshape(-1)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError((what, key, 'first differing bytes', bad[:8], a[bad[:8]], b[bad[:8]], len(bad)))
        written[begin:begin + size] = True
    assert np.all(got[~written] == SENT), (what, 'bytes outside the wanted outputs were written', np.flatnonzero((got != SENT) & ~written)[:8])
    assert np.array_equal(sbuf.download(np.uint8, shost.size), shost), (what, 'the plane was written')
    return ref


def staged_rectangles(info, mesh, shift, dst, src, cubic):
    """bool per rectangle of the launch: its source window is staged in LDS -- by the kernel's statement of the rule (the
    bounding box of the windows that meet the raster, clipped, against the window size) with the rectangle and the window
    size that the kernel-info string of the launch names.  This INFERS the path; nothing the device does is observed, so a
    kernel that took the other path with the same bits would pass.  What is observed is that both kinds of rectangle give the
    host entry's bits."""
    m = re.search(r'dswx_resample_k .* rect=(\d+)x(\d+) lds_elems=(\d+) ', info)
    assert m, info
    rh, rw, cap = (int(v) for v in m.groups())
    assert (rh, rw, cap) == (RH, RW, _capi.RESAMPLE_LDS_ELEMS)
    H, W = src
    sx, sy = warp.positions(mesh, shift, dst)
    c0, r0 = (sx - 128) >> 8, (sy - 128) >> 8
    lo, hi = (1, 2) if cubic else (0, 1)
    near = (c0 + hi >= 0) & (c0 - lo < W) & (r0 + hi >= 0) & (r0 - lo < H)
    out = []
    for y in range(0, dst[0], rh):
        for x in range(0, dst[1], rw):
            k = near[y:y + rh, x:x + rw]
            if not k.any():
                out.append(True)
                continue
            c, r = c0[y:y + rh, x:x + rw][k], r0[y:y + rh, x:x + rw][k]
            bw = min(int(c.max()) + hi, W - 1) - max(int(c.min()) - lo, 0) + 1
            bh = min(int(r.max()) + hi, H - 1) - max(int(r.min()) - lo, 0) + 1
            out.append(bw * bh <= cap)
    return np.array(out)


def word_of(dtype):
    return outside_word(OUTSIDE[dtype], dtype)


@pytest.mark.parametrize('shift', SHIFTS)
@pytest.mark.parametrize('method', (BILINEAR, CUBIC))
@pytest.mark.parametrize('dtype', KINDS)
def test_device_entry_against_the_host_entry(ctx, dtype, method, shift):
    """Kind x method x shift: every mesh content on every destination from a 64 x 80 source (NaN, infinities, nodata,
    subnormals and the ends of the range sprinkled in), with and without a nodata value, then a mesh per tile with strides."""
    rng = np.random.default_rng(7000 + 100 * shift + 10 * method + (dtype == np.int16))
    bufs = Bufs(ctx)
    src = (64, 80)
    try:
        for dst in DSTS + (RAGGED,):
            n = 2
            tiles = random_tiles(rng, n, src, dtype)
            meshes = {k: make_mesh(k, dst, shift, src, rng) for k in MESHES}
            for kind in MESHES:
                nodata = NODATA[dtype] if len(kind) % 2 else None
                run_device(ctx, bufs, tiles, meshes[kind], Spec(dtype, method, shift, nodata, word_of(dtype)), dst,
                           off=1 + 2 * (len(kind) % 2), what=(dst, kind))
                if kind in ('identity', 'rotation'):
                    assert staged_rectangles(ctx.last_kernel_info(), meshes[kind], shift, dst, src, method == CUBIC).all(), (dst, kind)
            mh, mw = mesh_shape(dst, shift)
            nodes, stride = mh * mw + 5, src[0] * src[1] + 7
            per_tile = rng.integers(-(1 << 31), 1 << 31, size=(n, nodes, 2), dtype=np.int64).astype(np.int32)
            for t in range(n):
                per_tile[t, :mh * mw] = meshes[MESHES[(t + shift + method) % len(MESHES)]].reshape(-1, 2)
            padded = random_tiles(rng, n, (1, stride), dtype).reshape(n, stride)
            padded[:, :src[0] * src[1]] = tiles.reshape(n, -1)
            run_device(ctx, bufs, padded, per_tile, Spec(dtype, method, shift, None, word_of(dtype), src_tile_stride=stride, mesh_tile_stride_nodes=nodes),
                       dst, raster=src, what=(dst, 'per tile'))
        info = ctx.last_kernel_info()
        assert 'dswx_resample_k' in info and f'kind={"f32" if dtype == np.float32 else "i16"}' in info, info
        assert f'method={"cubic" if method == CUBIC else "bilinear"}' in info and f'shift={shift}' in info, info
    finally:
        bufs.free()


def decimating_mesh(dst, shift, factor):
    """`factor` source pixels per destination pixel along both axes."""
    return exact_mesh(dst, shift, lambda X, Y: factor * X + 1, lambda X, Y: factor * Y + 2)


def scattered_mesh(dst, shift, src, rng):
    """Garbage that hits: every node somewhere in (or just outside) the raster, so the windows of a rectangle span all of it."""
    mh, mw = mesh_shape(dst, shift)
    return np.stack([rng.integers(-600, 256 * src[1] + 600, size=(mh, mw)), rng.integers(-600, 256 * src[0] + 600, size=(mh, mw))],
                    axis=-1).astype(np.int32)


@pytest.mark.parametrize('method', (BILINEAR, CUBIC))
@pytest.mark.parametrize('dtype', KINDS)
def test_both_tap_paths_are_taken_and_agree(ctx, dtype, method):
    """A 300 x 470 source: the identity and a rotation by three degrees stage every rectangle's window in LDS; a mesh of 8
    source pixels per destination pixel and garbage that lands inside the raster gather from global memory; int32 garbage
    mostly misses the raster.  Which path a rectangle took follows from the sizes the kernel-info string names."""
    rng = np.random.default_rng(7100 + 10 * method + (dtype == np.int16))
    bufs = Bufs(ctx)
    src, dst = (300, 470), (5 * RH + 1, 4 * RW + 9)
    try:
        tiles = random_tiles(rng, 2, src, dtype)
        for shift in (4, 1):
            for kind, mesh, lds in (('identity', make_mesh('identity', dst, shift, src, rng), 'all'), ('rotation', make_mesh('rotation', dst, shift, src, rng), 'all'),
                                    ('decimate', decimating_mesh((src[0] // 8, src[1] // 8), shift, 8), 'none'), ('scattered', scattered_mesh(dst, shift, src, rng), 'few'),
                                    ('garbage', make_mesh('garbage', dst, shift, src, rng), None)):
                d = (src[0] // 8, src[1] // 8) if kind == 'decimate' else dst
                ref = run_device(ctx, bufs, tiles, mesh, Spec(dtype, method, shift, NODATA[dtype], word_of(dtype)), d, what=(kind, shift))
                staged = staged_rectangles(ctx.last_kernel_info(), mesh, shift, d, src, method == CUBIC)
                if lds == 'all':
                    assert staged.all() and ref['head'][0, 4] < ref['head'][0, 0], kind
                elif lds == 'none':
                    assert not staged.any() and ref['head'][0, 4] < ref['head'][0, 0], (kind, staged)
                elif lds == 'few':
                    assert (~staged).mean() > 0.5 and ref['head'][0, 4] < ref['head'][0, 0], (kind, staged)
        # a window of exactly the LDS size and one element more: 128 x 32 and 129 x 32 source pixels under one rectangle
        for cols in (_capi.RESAMPLE_LDS_ELEMS // 32, _capi.RESAMPLE_LDS_ELEMS // 32 + 1):
            lo, hi = (1, 2) if method == CUBIC else (0, 1)
            mesh = np.zeros((2, 2, 2), dtype=np.int32)                    # shift 8, one cell: the corners of the rectangle's box
            span_c, span_r = cols - 1 - lo - hi, 32 - 1 - lo - hi
            for i, j in itertools.product(range(2), range(2)):
                mesh[i, j] = (256 * (lo + 5) + 128 + 64 + j * span_c * 256 * 256 // (RW - 1), 256 * (lo + 3) + 128 + 64 + i * span_r * 256 * 256 // (RH - 1))
            run_device(ctx, bufs, tiles, mesh, Spec(dtype, method, 8, None, word_of(dtype)), (RH, RW), what=('window', cols))
            staged = staged_rectangles(ctx.last_kernel_info(), mesh, 8, (RH, RW), src, method == CUBIC)
            assert staged.tolist() == [cols * 32 <= _capi.RESAMPLE_LDS_ELEMS], (cols, staged)
    finally:
        bufs.free()


@pytest.mark.parametrize('method', (BILINEAR, CUBIC))
@pytest.mark.parametrize('dtype', KINDS)
def test_seams_of_rectangles_rows_nodata_and_the_four_edges(ctx, dtype, method):
    """Whole-pixel and fractional shifts of a 100 x 257 source put each of the raster's four edges, the end of a source row
    and nodata pixels inside a rectangle and exactly on its border (multiples of 8 rows and 32 columns), and push the
    destination over each edge."""
    rng = np.random.default_rng(7200 + 10 * method + (dtype == np.int16))
    bufs = Bufs(ctx)
    src = (100, 257)
    dst = (src[0] + 2 * RH + 3, src[1] + 2 * RW + 5)
    try:
        tiles = random_tiles(rng, 2, src, dtype, special=False)
        tiles[:, ::RH, ::RW] = NODATA[dtype]                              # on the corners of rectangles under the identity
        tiles[:, 5::13, 7::29] = NODATA[dtype]                            # and inside them
        for a, b in ((0, 0), (-RW, -RH), (-RW + 1, -RH + 1), (-RW - 1, -RH - 1), (-5, -3), (src[1] - RW, src[0] - RH), (src[1] - 2 * RW - 7, src[0] - 3 * RH - 2)):
            for fx, fy in ((0, 0), (77, 130), (255, 1)):
                mesh = exact_mesh(dst, 4, lambda X, Y: X + a, lambda X, Y: Y + b) + np.array([fx, fy], dtype=np.int32)
                ref = run_device(ctx, bufs, tiles, mesh, Spec(dtype, method, 4, NODATA[dtype], word_of(dtype)), dst, what=(a, b, fx, fy))
                assert 0 < ref['head'][0, 4] < ref['head'][0, 0] and ref['head'][0, 3] > 0
                assert staged_rectangles(ctx.last_kernel_info(), mesh, 4, dst, src, method == CUBIC).all()
        # destination sizes around the rectangle
        small = random_tiles(rng, 2, (37, 53), dtype)
        for dh, dw in itertools.product((1, RH - 1, RH, RH + 1), (1, RW - 1, RW, RW + 1, 2 * RW + 1)):
            mesh = exact_mesh((dh, dw), 5, lambda X, Y: X - 3, lambda X, Y: Y - 1) + np.array([40, 200], dtype=np.int32)
            run_device(ctx, bufs, small, mesh, Spec(dtype, method, 5, None, word_of(dtype)), (dh, dw), what=('sizes', dh, dw))
    finally:
        bufs.free()


def test_more_rectangles_than_workgroups(ctx):
    """A destination of 34 x 33 rectangles, more than the 1024 workgroups of a row of the grid: every workgroup walks several
    rectangles, reusing its LDS window, and adds its sums to the head once."""
    rng = np.random.default_rng(7250)
    bufs = Bufs(ctx)
    src, dst = (100, 257), (33 * RH + 3, 32 * RW + 5)
    try:
        for dtype, method in ((np.float32, CUBIC), (np.int16, BILINEAR)):
            tiles = random_tiles(rng, 2, src, dtype)
            for mesh in (make_mesh('rotation', dst, 5, src, rng), decimating_mesh(dst, 5, 1) + np.array([70, 200], dtype=np.int32), scattered_mesh(dst, 5, src, rng)):
                ref = run_device(ctx, bufs, tiles, mesh, Spec(dtype, method, 5, NODATA[dtype], word_of(dtype)), dst, twice=True, what=('walk', dtype))
                assert 'grid=(1024,2,1)' in ctx.last_kernel_info() and 0 < ref['head'][0, 4] < ref['head'][0, 0]
    finally:
        bufs.free()


def test_float32_subnormals_are_kept_on_the_device(ctx):
    tiny = np.full((1, 40, 70), 1e-45, dtype=np.float32)
    tiny[0, ::2] = 3e-45
    tiny[0, :, ::3] = -4e-39
    bufs = Bufs(ctx)
    try:
        for method in (BILINEAR, CUBIC):
            mesh = exact_mesh((40, 70), 3, lambda X, Y: X, lambda X, Y: Y)
            ref = run_device(ctx, bufs, tiny, mesh, Spec(np.float32, method, 3), (40, 70), what='identity')
            assert np.array_equal(ref['dst'].view(np.uint32), tiny.view(np.uint32))
            ref = run_device(ctx, bufs, tiny, mesh + np.array([100, 60], dtype=np.int32), Spec(np.float32, method, 3), (40, 70), what='between')
            used = ref['dst'][ref['how'] != 0]
            assert np.all(np.abs(used) < 1e-38) and (used != 0).mean() > 0.9
    finally:
        bufs.free()


def test_every_subset_of_outputs_a_second_call_and_addresses(ctx):
    rng = np.random.default_rng(7300)
    bufs = Bufs(ctx)
    try:
        for dtype in KINDS:
            src = (100, 257)
            tiles = random_tiles(rng, 3, src, dtype)
            mesh = make_mesh('rotation', (90, 300), 4, src, rng)
            for r in range(1, 4):
                for want in itertools.combinations(KEYS, r):
                    for off in (0, 1, 3):
                        run_device(ctx, bufs, tiles, mesh, Spec(dtype, CUBIC, 4, NODATA[dtype], word_of(dtype)), (90, 300), want=want, off=off, twice=True,
                                   what=(dtype, want, off))
        # every output NULL, no tiles, an empty destination: no work, nothing written, no error
        buf = ctx.malloc(4096)
        buf.upload(np.full(4096, SENT, dtype=np.uint8))
        out = _capi.ResampleOut.of(buf.ptr, buf.ptr + 1024, buf.ptr + 2048)
        spec = Spec(np.float32, CUBIC, 2, outside=outside_word(7.0, np.float32))
        ctx.resample_device(buf.ptr + 3072, spec, 2, 5, 6, buf.ptr + 3584, 5, 6, _capi.ResampleOut.of())
        ctx.resample_device(buf.ptr + 3072, spec, 0, 5, 6, buf.ptr + 3584, 5, 6, out)
        ctx.resample_device(buf.ptr + 3072, spec, 2, 5, 6, buf.ptr + 3584, 0, 6, out)
        ctx.resample_device(buf.ptr + 3072, spec, 2, 5, 6, buf.ptr + 3584, 5, 0, out)
        ctx.synchronize()
        assert np.all(buf.download(np.uint8, 4096) == SENT)
        # an empty source raster: every pixel outside, and the plane may be NULL
        ctx.resample_device(0, spec, 2, 0, 6, buf.ptr + 3584, 5, 6, out)
        ctx.synchronize()
        assert np.all(buf.download(np.float32, 60) == 7.0) and np.all(buf.download(np.uint8, 60, offset=1024) == 0)
        assert buf.download(np.uint64, 16, offset=2048).reshape(2, 8).tolist() == [[30, 0, 0, 0, 30, 0, 0, 0]] * 2
        with pytest.raises(_capi.DswxError, match='mesh') as e:
            ctx.resample_device(buf.ptr + 3072, spec, 2, 5, 6, buf.ptr + 3586, 5, 6, out)
        assert e.value.code == _capi.ERR_ALIGN
        buf.free()
    finally:
        bufs.free()


def test_on_a_callers_stream_behind_the_copy_that_writes_the_plane(ctx):
    """The entry on a caller's stream is ordered behind that stream's earlier work: the plane is overwritten by a copy queued
    on the stream, the resample is queued behind it and sees the new plane."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(7400)
    T, H, W, dst, shift = 4, 100, 257, (120, 300), 4
    old = rng.normal(0, 100, size=(T, H, W)).astype(np.float32)
    new = rng.normal(5000, 100, size=(T, H, W)).astype(np.float32)
    mesh_host = make_mesh('rotation', dst, shift, (H, W), rng)
    plane = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    mesh = torch.from_numpy(mesh_host.copy()).to('cuda:0')
    out_d = torch.full((T * dst[0] * dst[1],), -1.0, dtype=torch.float32, device='cuda:0')
    head = torch.full((T * 8,), -1, dtype=torch.int64, device='cuda:0')
    torch.cuda.synchronize()
    spec = Spec(np.float32, CUBIC, shift, outside=outside_word(9.0, np.float32))
    want = _capi.resample_host(new, mesh_host, spec, dst)
    assert not np.array_equal(want['dst'], _capi.resample_host(old, mesh_host, spec, dst)['dst'])
    s = torch.cuda.Stream(device=0)
    with torch.cuda.stream(s):
        plane.copy_(src, non_blocking=True)
    ctx.resample_device(plane.data_ptr(), spec, T, H, W, mesh.data_ptr(), dst[0], dst[1], _capi.ResampleOut.of(out_d.data_ptr(), None, head.data_ptr()),
                        stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(out_d.cpu().numpy().view(np.uint32), want['dst'].reshape(-1).view(np.uint32))
    assert np.array_equal(head.cpu().numpy().view(np.uint64).reshape(T, 8), want['head'])


def test_past_the_tiles_of_one_launch(ctx):
    """65535 + 4 tiles of a 4 x 5 source onto 3 x 5: the workgroups of a row of the grid walk the tiles."""
    rng = np.random.default_rng(7500)
    T = 65535 + 4
    tiles = rng.integers(-3000, 3000, size=(T, 4, 5)).astype(np.int16)
    mesh = exact_mesh((3, 5), 2, lambda X, Y: X, lambda X, Y: Y) + np.array([90, 40], dtype=np.int32)
    bufs = Bufs(ctx)
    try:
        ref = run_device(ctx, bufs, tiles, mesh, Spec(np.int16, BILINEAR, 2, 7, word_of(np.int16)), (3, 5), what='tile walk')
        assert 'grid=(1,65535,1)' in ctx.last_kernel_info() and len(np.unique(ref['dst'][-4:])) > 4
    finally:
        bufs.free()


def test_device_plane_resample(ctx):
    rng = np.random.default_rng(7600)
    engine = pipeline.engine_of(D.get_context(0))
    tiles = random_tiles(rng, 2, (100, 257), np.float32)
    mesh = make_mesh('rotation', (90, 300), 5, (100, 257), rng)
    plane = engine.upload(tiles)
    res = plane.resample(mesh, (90, 300), 5, 'cubic', nodata=NODATA[np.float32], outside=word_of(np.float32), want=KEYS)
    ref = resample_tiles(tiles, mesh, 5, (90, 300), CUBIC, nodata=NODATA[np.float32], outside=word_of(np.float32))
    for k in KEYS:
        got = res[k].numpy()
        assert got.shape == ref[k].shape and np.array_equal(got.view(np.uint8), ref[k].view(np.uint8)), k
        res[k].release()
    one = engine.upload(tiles[0])
    got = one.resample(mesh, (90, 300), 5, 'bilinear')['dst']
    assert got.shape == (90, 300) and np.array_equal(got.numpy().view(np.uint32), resample_tiles(tiles[:1], mesh, 5, (90, 300), BILINEAR)['dst'][0].view(np.uint32))
    with pytest.raises(ValueError):
        engine.upload(np.zeros((4, 4), dtype=np.uint8)).resample(mesh, (90, 300), 5)


# ---- the product run ------------------------------------------------------------------------------------------------------

ARC = 1.0 / 3600.0


def write_geographic_dem(path, epsg=4326, nodata=None):
    """A smooth synthetic DEM of one arc second in degrees that covers the 128 x 128 synthetic product (UTM 15 N, 600000 E,
    4000020 N) with its margin, and the array."""
    lon, lat = warp.tm_inverse(np.array([600000.0 - 1500.0, 600000.0 + 128 * 30.0 + 1500.0]) - 500000.0,
                               np.array([4000020.0 + 1500.0, 4000020.0 - 128 * 30.0 - 1500.0]), -93.0)
    x0, y0 = math_floor(lon.min() - 0.01, ARC), math_floor(lat.max() + 0.012, ARC)
    W, H = int((lon.max() + 0.012 - x0) / ARC) + 1, int((y0 - lat.min() + 0.012) / ARC) + 1
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    dem = (300.0 + 120.0 * np.sin(c / 17.0) * np.cos(r / 23.0) + 0.4 * c - 0.3 * r + 40.0 * np.sin((c + 2 * r) / 7.0)).astype(np.float32)
    geotiff.write_geotiff(path, dem, geo_tags=geotiff.geo_tags_from_geotransform((x0, ARC, 0.0, y0, 0.0, -ARC), epsg), nodata=nodata)
    return dem


def math_floor(v, unit):
    return float(np.floor(v / unit) * unit)


def check_product_dem(tmp_path, files, dem_file, name, **kw):
    """One product run with `dem_file`: SHAD and DEM equal resample_tiles (the numpy statement, through the same plan) plus the
    shadow oracle on the host, bit for bit."""
    shad_file, dem_out = str(tmp_path / f'shad_{name}.tif'), str(tmp_path / f'dem_out_{name}.tif')
    D.generate_dswx_layers(files, dem_file=dem_file, output_shadow_layer=shad_file, output_dem_layer=dem_out, scratch_dir=str(tmp_path), **kw)
    info = geotiff.open_geotiff(dem_file).info
    band, band_info = geotiff.read_geotiff(files[0])
    window, mesh, shift, deviation, dst_shape = D.dem_resample_plan(info, band_info.geotransform, band_info.geo_tags, 128, 128,
                                                                    projected=kw.get('resample_projected_dem', False))
    assert dst_shape == (228, 228) and shift in D.DEM_MESH_SHIFTS and deviation <= 1.0 and window[2] > 200 and window[3] > 200
    src, _ = geotiff.read_geotiff(dem_file, window=window)
    want = resample_tiles(src[None].astype(np.float32), mesh, shift, dst_shape, CUBIC)
    assert np.all(want['how'] == 3)                                       # the window covers every cubic tap
    dem = want['dst'][0]
    shad = o.compute_opera_shadow_layer(dem, 143.2, 90 - 34.5, -5, 40, legacy_promotion=True)[50:-50, 50:-50]
    got_dem, dem_info = geotiff.read_geotiff(dem_out)
    assert got_dem.dtype == np.float32 and np.array_equal(got_dem.view(np.uint32), dem[50:-50, 50:-50].view(np.uint32)), name
    assert np.array_equal(geotiff.read_geotiff(shad_file)[0], shad.astype(np.uint8)), name
    assert 0 < shad.astype(np.uint8).sum() < shad.size                   # both values occur, or the comparison is vacuous


def smooth_dem(H, W):
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    return (300.0 + 120.0 * np.sin(c / 17.0) * np.cos(r / 23.0) + 0.4 * c - 0.3 * r + 40.0 * np.sin((c + 2 * r) / 7.0)).astype(np.float32)


def test_product_run_with_projected_dems_when_asked(tmp_path):
    """A DEM off the grid in the product's own SRS (7 m beside the lattice) and one in the neighbouring UTM zone: refused as
    ever without resample_projected_dem=True, resampled like the geographic one with it."""
    _, files, _, _ = synth_hls.make(str(tmp_path), size=128)
    beside = str(tmp_path / 'dem_beside.tif')
    gt = (600000.0 - 1500.0 - 480.0 + 7.0, 30.0, 0.0, 4000020.0 + 1500.0 + 480.0 - 11.0, 0.0, -30.0)
    geotiff.write_geotiff(beside, smooth_dem(260, 260), geo_tags=geotiff.geo_tags_from_geotransform(gt, 32615))
    x, y = warp.utm_to_utm(600000.0 + 64 * 30.0, 4000020.0 - 64 * 30.0, 32615, 32616)
    gt16 = (float(np.round(x / 30.0)) * 30.0 - 200 * 30.0, 30.0, 0.0, float(np.round(y / 30.0)) * 30.0 + 200 * 30.0, 0.0, -30.0)
    zone16 = str(tmp_path / 'dem_zone16.tif')
    geotiff.write_geotiff(zone16, smooth_dem(400, 400), geo_tags=geotiff.geo_tags_from_geotransform(gt16, 32616))
    for name, path in (('beside', beside), ('zone16', zone16)):
        with pytest.raises(NotImplementedError, match='not on the HLS grid'):
            D.generate_dswx_layers(files, dem_file=path, scratch_dir=str(tmp_path))
        check_product_dem(tmp_path, files, path, name, resample_projected_dem=True)


def test_resample_example_runs(tmp_path):
    """examples/batch_resample.c: its own checks (exit status 0: every bit of the resampled float32 plane against a loop in C
    and against dswx_resample_host)."""
    import shutil
    import subprocess
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_resample')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_resample.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}', '-lm',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '211', '190'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'float32 resample: device, loop and host entry agree in every bit' in r.stdout
    cubic = [int(l.split(': ')[1].split(' cubic')[0]) for l in r.stdout.splitlines() if l.startswith('tile ')]
    assert len(cubic) == 2 and min(cubic) > 1000                          # the loop did take the cubic rule


def test_product_run_with_a_dem_in_epsg_4326(tmp_path):
    """SHAD and DEM of generate_dswx_layers from a DEM in EPSG:4326 equal resample_tiles (the numpy statement, through the same
    plan) plus the shadow oracle on the host, bit for bit; the same file under an EPSG that is not supported still raises; a
    DEM on the grid gives the bytes it gave before."""
    _, files, _, _ = synth_hls.make(str(tmp_path), size=128, ancillary=True, dem_margin=50)
    grid_dem = str(tmp_path / 'ancillary' / 'dem.tif')
    dem_file = str(tmp_path / 'dem_4326.tif')
    write_geographic_dem(dem_file)
    check_product_dem(tmp_path, files, dem_file, 'geographic')
    # the same file under an EPSG this drop-in does not reproject
    bad = str(tmp_path / 'dem_3857.tif')
    write_geographic_dem(bad, epsg=3857)
    with pytest.raises(NotImplementedError, match='not on the HLS grid'):
        D.generate_dswx_layers(files, dem_file=bad, scratch_dir=str(tmp_path))
    # a DEM on the grid: the bytes of the file itself, as before
    on_grid = str(tmp_path / 'dem_on_grid.tif')
    D.generate_dswx_layers(files, dem_file=grid_dem, output_dem_layer=on_grid, scratch_dir=str(tmp_path))
    full, _ = geotiff.read_geotiff(grid_dem)
    assert np.array_equal(geotiff.read_geotiff(on_grid)[0].view(np.uint32), full[50:-50, 50:-50].view(np.uint32))


def test_the_warp_tool_interpolates_when_asked(tmp_path, capsys):
    """bin/dswx_warp.py --resample cubic lays the DEM in EPSG:4326 over the lattice of a product band: resample_tiles of the
    whole file through geographic_mesh, a COG with the lattice of --like.  Without the flag the same input is refused as before."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('dswx_warp_py', os.path.join(ROOT, 'bin', 'dswx_warp.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, files, _, _ = synth_hls.make(str(tmp_path), size=128)
    dem_file, out = str(tmp_path / 'dem_4326.tif'), str(tmp_path / 'out.tif')
    dem = write_geographic_dem(dem_file)
    assert tool.main([dem_file, '--like', files[0], '--resample', 'cubic', '--shift', '5', '--outside', '-7', '-o', out]) == 0
    arr, info = geotiff.read_geotiff(out)
    like = geotiff.open_geotiff(files[0]).info
    src_info = geotiff.open_geotiff(dem_file).info
    mesh, _ = warp.geographic_mesh(src_info.geotransform, like.geotransform, 32615, (128, 128), 5)
    want = resample_tiles(dem[None], mesh, 5, (128, 128), CUBIC, outside=outside_word(-7, np.float32))
    assert arr.dtype == np.float32 and np.array_equal(arr.view(np.uint32), want['dst'][0].view(np.uint32)) and np.all(want['how'] == 3)
    assert tuple(info.geotransform) == tuple(like.geotransform) and info.metadata['WARP_RESAMPLE'] == 'cubic'
    assert '"cubic": 16384' in capsys.readouterr().out
    assert tool.main([dem_file, '--like', files[0], '-o', str(tmp_path / 'no.tif')]) == 1
    assert 'WGS 84 / UTM' in capsys.readouterr().out and not os.path.exists(str(tmp_path / 'no.tif'))
