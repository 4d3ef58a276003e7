"""The warp entries on the GPU: dswx_warp_device and dswx_batch_warp byte for byte against the library's scalar statement
(dswx_warp_host; tests/test_warp.py pins that to numpy and to a loop in Python ints) on dst, src_index and head -- the meshes
and shapes of the CPU tests; rasters of 100 x 257 and 300 x 470, where runs of consecutive source pixels and single elements
meet inside rows; runs of 16 that start inside the raster and leave it over each of its four edges; plane and dst at odd
multiples of elem_bytes, with every byte outside the outputs checked; every subset of outputs; a caller's stream; a second call
on the same outputs; the batch form on a uint8, an int16 and the DIAG plane with tile ranges; 65535 + 4 tiles; the label plane
warped there and back; DevicePlane.warp; bin/dswx_warp.py and bin/dswx_mosaic.py --reproject; the C example."""
import importlib.util
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py)
    import torch
except ImportError:
    torch = None

from proteus_amd import _capi, geotiff, warp
from proteus_amd.warp import OUTSIDE, Spec, mesh_shape, warp_tiles
from proteus_amd.synth import SEED
from tests.test_warp import DSTS, MESHES, OUT_WORD, SHIFTS, SRCS, exact_mesh, make_mesh, random_tiles
from tests.test_warp import (DTYPES, ENTER_K, ENTER_SLOPES, FLAT_DST, LONG_SIDE, WALK_SRCS, affine_mesh, check_traits, decimation_cases,
                             entering_cases, fit_offsets, flat_cases, long_side_cases, outside_of, slope_cases, switch_cases, whole_units)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, PAD, GUARD = 0xEE, 0xA5, 256
KEYS = ('dst', 'src_index', 'head')


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
    """One call of dswx_warp_device against dswx_warp_host.  The plane lies `off` ELEMENTS past a 256-byte boundary behind a
    guard, every byte that is not tile data PAD; dst lies `off` elements, src_index one word and head one head word past a
    256-byte boundary, every byte of the output buffer SENT beforehand and every byte outside the wanted outputs SENT afterwards."""
    eb = spec.elem_bytes
    tiles = np.ascontiguousarray(tiles)
    n = tiles.shape[0]
    H, W = tiles.shape[1:] if raster is None else raster
    dh, dw = dst
    ref = _capi.warp_host(tiles, mesh, spec, dst, raster=raster)
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
    for key, size, shiftby in (('dst', px * eb, off * eb), ('src_index', px * 4, 4), ('head', n * 64, 8)):
        begin = -(-cursor // 256) * 256 + shiftby
        where[key] = (begin, size)
        cursor = begin + size + 64
    obuf = bufs.get('out', cursor)
    obuf.upload(np.full(cursor, SENT, dtype=np.uint8))
    out = _capi.WarpOut.of(**{k: obuf.ptr + where[k][0] for k in want})
    for _ in range(2 if twice else 1):
        ctx.warp_device(sbuf.ptr + start, spec, n, H, W, mbuf.ptr + 4, dh, dw, out, stream=stream)
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


@pytest.mark.parametrize('shift', SHIFTS)
@pytest.mark.parametrize('eb', (1, 2, 4))
def test_device_entry_against_the_host_entry(ctx, shift, eb):
    """The destinations, sources and mesh contents of tests/test_warp.py for this shift and element size, with a shared mesh
    and with per-tile meshes and strides; the plane and dst at an odd multiple of elem_bytes."""
    rng = np.random.default_rng(4000 + 10 * shift + eb)
    bufs = Bufs(ctx)
    try:
        for dst, src in itertools.product(DSTS, SRCS):
            n = 3
            tiles = random_tiles(rng, n, src, eb)
            meshes = {k: make_mesh(k, dst, shift, src, rng) for k in MESHES}
            for kind in MESHES:
                run_device(ctx, bufs, tiles, meshes[kind], Spec(eb, shift, OUT_WORD), dst, off=1 + 2 * (len(kind) % 2), what=(dst, src, kind))
            mh, mw = mesh_shape(dst, shift)
            nodes, stride = mh * mw + 5, src[0] * src[1] + 7
            per_tile = rng.integers(-(1 << 31), 1 << 31, size=(n, nodes, 2), dtype=np.int64).astype(np.int32)
            for t in range(n):
                per_tile[t, :mh * mw] = meshes[MESHES[(t + shift + eb) % len(MESHES)]].reshape(-1, 2)
            padded = random_tiles(rng, n, (1, stride), eb).reshape(n, stride)
            padded[:, :src[0] * src[1]] = tiles.reshape(n, -1)
            run_device(ctx, bufs, padded, per_tile, Spec(eb, shift, OUT_WORD, src_tile_stride=stride, mesh_tile_stride_nodes=nodes), dst,
                       raster=src, what=(dst, src, 'per tile'))
    finally:
        bufs.free()


@pytest.mark.parametrize('eb', (1, 2, 4))
def test_runs_and_single_elements_meet_inside_rows_and_at_every_edge(ctx, eb):
    """Rasters of 100 x 257 and 300 x 470 under a rotation of a few degrees (a destination row follows a source row for some
    tens of pixels: units that are one load and units that are 16 meet in every row), under the identity and whole-pixel shifts
    that push runs of 16 over each of the four edges of the raster by 1 .. 16 pixels, and under garbage; destination widths
    either side of a unit and of a workgroup's rectangle."""
    rng = np.random.default_rng(4100 + eb)
    bufs = Bufs(ctx)
    R, C, U = _capi.WARP_RECT_H, _capi.WARP_RECT_W, _capi.WARP_UNIT
    try:
        for src in ((100, 257), (300, 470)):
            tiles = random_tiles(rng, 2, src, eb)
            for shift in (4, 6, 2):
                spec = Spec(eb, shift, OUT_WORD)
                ref = run_device(ctx, bufs, tiles, make_mesh('rotation', src, shift, src, rng), spec, src, what=(src, shift, 'rotation'))
                idx = ref['src_index'][0][:, :src[1] // U * U].reshape(src[0], -1, U).astype(np.int64)
                runs = np.all(np.diff(idx, axis=2) == 1, axis=2) & np.all(idx != OUTSIDE, axis=2)
                assert runs.any() and (~runs).any() and (runs.any(axis=1) & (~runs).any(axis=1)).any()   # both kinds of unit in one row
                run_device(ctx, bufs, tiles, make_mesh('garbage', src, shift, src, rng), spec, src, what=(src, shift, 'garbage'))
            for a, b in [(k, 0) for k in (1, 5, 15, 16, 17)] + [(-k, 0) for k in (1, 5, 15, 16, 17)] + [(0, 1), (0, -1), (3, -2), (-9, 7),
                                                                                                          (src[1] - 5, 0), (5 - src[1], 0)]:
                mesh = exact_mesh(src, 4, lambda X, Y: X + a, lambda X, Y: Y + b)
                ref = run_device(ctx, bufs, tiles, mesh, Spec(eb, 4, OUT_WORD), src, what=(src, 'shift', a, b))
                assert 0 < ref['head'][0, 1] < ref['head'][0, 0]
        # destination widths and heights around the units and the rectangles of the launch, a source smaller than a unit's run
        tiles = random_tiles(rng, 2, (37, 53), eb)
        for dw in (1, U - 1, U, U + 1, C - 1, C, C + 1, 2 * C + 17):
            for dh in (1, R, R + 1, 2 * R + 1):
                mesh = exact_mesh((dh, dw), 5, lambda X, Y: X - 3, lambda X, Y: Y - 1)
                run_device(ctx, bufs, tiles, mesh, Spec(eb, 5, OUT_WORD), (dh, dw), what=('sizes', dh, dw))
        # the identity: every unit is one load and one store
        tiles = random_tiles(rng, 2, (64, 4 * U), eb)
        ref = run_device(ctx, bufs, tiles, exact_mesh((64, 4 * U), 6, lambda X, Y: X, lambda X, Y: Y), Spec(eb, 6, 0), (64, 4 * U), what='identity')
        assert np.array_equal(ref['dst'], tiles)
        info = ctx.last_kernel_info()
        assert 'dswx_warp_k' in info and f'elem_bytes={eb}' in info and 'fine=0' in info, info
    finally:
        bufs.free()


def test_every_subset_of_outputs_a_second_call_and_addresses(ctx):
    rng = np.random.default_rng(4200)
    bufs = Bufs(ctx)
    try:
        for eb in (1, 2, 4):
            src = (100, 257)
            tiles = random_tiles(rng, 3, src, eb)
            mesh = make_mesh('rotation', (90, 300), 4, src, rng)
            for r in range(1, 4):
                for want in itertools.combinations(KEYS, r):
                    for off in (0, 1, 3):
                        run_device(ctx, bufs, tiles, mesh, Spec(eb, 4, OUT_WORD), (90, 300), want=want, off=off, twice=True, what=(eb, want, off))
        # every output NULL, no tiles, an empty destination: no work, nothing written, no error
        tiles = random_tiles(rng, 2, (5, 6), 1)
        mesh = make_mesh('identity', (5, 6), 2, (5, 6), rng)
        buf = ctx.malloc(4096)
        buf.upload(np.full(4096, SENT, dtype=np.uint8))
        out = _capi.WarpOut.of(buf.ptr, buf.ptr + 1024, buf.ptr + 2048)
        ctx.warp_device(buf.ptr + 3072, Spec(1, 2), 2, 5, 6, buf.ptr + 3584, 5, 6, _capi.WarpOut.of())
        ctx.warp_device(buf.ptr + 3072, Spec(1, 2), 0, 5, 6, buf.ptr + 3584, 5, 6, out)
        ctx.warp_device(buf.ptr + 3072, Spec(1, 2), 2, 5, 6, buf.ptr + 3584, 0, 6, out)
        ctx.warp_device(buf.ptr + 3072, Spec(1, 2), 2, 5, 6, buf.ptr + 3584, 5, 0, out)
        ctx.synchronize()
        assert np.all(buf.download(np.uint8, 4096) == SENT)
        # an empty source raster: every pixel outside, and the plane may be NULL
        ctx.warp_device(0, Spec(1, 2, 7), 2, 0, 6, buf.ptr + 3584, 5, 6, out)
        ctx.synchronize()
        assert np.all(buf.download(np.uint8, 60) == 7) and np.all(buf.download(np.uint32, 60, offset=1024) == OUTSIDE)
        assert buf.download(np.uint64, 16, offset=2048).reshape(2, 8).tolist() == [[30, 0, 30, 0, 0, 6, 0, 0]] * 2
        # refusals that need a context come after those of the arguments, and a refused call launches nothing
        with pytest.raises(_capi.DswxError, match='mesh') as e:
            ctx.warp_device(buf.ptr + 3072, Spec(1, 2), 2, 5, 6, buf.ptr + 3586, 5, 6, out)
        assert e.value.code == _capi.ERR_ALIGN
        buf.free()
    finally:
        bufs.free()


def test_a_raster_side_of_2_to_the_23_leaves_the_32_bit_arithmetic(ctx):
    """Below 2^23 pixels a side the kernel forms r * width + c from 24-bit factors and walks a unit in 32 bits; a raster of
    2 x 2^23 and one of 2^23 x 2 take the 64-bit form of every position instead: the far end of the raster, runs and cut units."""
    rng = np.random.default_rng(4250)
    bufs = Bufs(ctx)
    side = 1 << 23
    try:
        for src, moves in (((2, side), ((0, 0), (side - 400, 0), (side - 310, 1), (-7, -1))), ((side, 2), ((0, side - 60), (-1, side - 52), (0, 0)))):
            tiles = random_tiles(rng, 1, src, 1)
            for a, b in moves:
                mesh = exact_mesh((33, 300), 4, lambda X, Y: X + a, lambda X, Y: Y + b)
                ref = run_device(ctx, bufs, tiles, mesh, Spec(1, 4, OUT_WORD), (33, 300), what=(src, a, b))
                assert ref['head'][0, 1] > 0, (src, a, b)
            ref = run_device(ctx, bufs, tiles, make_mesh('rotation', (33, 300), 4, (4, 600), rng), Spec(1, 4, OUT_WORD), (33, 300), what=(src, 'rotation'))
    finally:
        bufs.free()


# ---- the position walk: every slope, sign and edge (the cases and their conditions: tests/test_warp.py, pinned there on the host) --

def run_cases(ctx, cases, eb, seed):
    """Every case through run_device on two tiles -- every byte of dst, src_index and head against dswx_warp_host -- and the
    conditions that make the case worth running, on the reference that the device has just been held to."""
    rng = np.random.default_rng(seed)
    bufs, planes, count = Bufs(ctx), {}, 0
    try:
        for case in cases:
            key = case['src']
            if key not in planes:
                planes[key] = random_tiles(rng, 1 if key[0] * key[1] > 1 << 20 else 2, key, eb)
            ref = run_device(ctx, bufs, planes[key], case['mesh'], Spec(eb, case['shift'], OUT_WORD), case['dst'], off=1 + 2 * (count % 2),
                             what=(case['name'], case['shift'], case['src']))
            check_traits(case, ref)
            count += 1
    finally:
        bufs.free()
    return count


@pytest.mark.parametrize('shift', (4, 6, 8))
@pytest.mark.parametrize('eb', (1, 2, 4))
def test_slopes_and_signs_on_the_32_bit_path(ctx, shift, eb):
    """Section (a) of tests/test_warp.py slope_cases on rasters of 100 x 257 and 300 x 470: the column, then the row, running
    along a destination row at +-85 .. +-1023 / 256 pixels per pixel (repeated pixels, flips, units inside that are no runs,
    transposes and quarter turns), shears that change the source row inside a unit, rotations by 30 .. 183 degrees; every
    destination hangs over two opposite edges of the raster, so fractions and pixels go negative under the rounding shift.
    unit_paths infers the 32-bit form for every unit of every case."""
    assert run_cases(ctx, (c for src in WALK_SRCS for c in slope_cases(shift, src)), eb, 4800 + 10 * shift + eb) == 94
    assert 'fine=0' in ctx.last_kernel_info()


@pytest.mark.parametrize('eb', (1, 2, 4))
def test_the_switch_between_the_forms_at_four_pixels(ctx, eb):
    """Section (b): node differences one below, on and one above four source pixels per destination pixel, in x, in y, in both,
    negated; and cells whose two edges lie either side of it, so that units of both forms are neighbours in one launch."""
    assert run_cases(ctx, (c for s in (4, 8) for c in switch_cases(s, WALK_SRCS[1])), eb, 4810 + eb) == 48


@pytest.mark.parametrize('eb', (1, 2, 4))
def test_entering_the_raster_from_outside_and_the_clamp(ctx, eb):
    """Section (c): units whose first pixel lies 1 .. 200 pixels outside each of the four edges and that walk towards the raster
    at 1, 2 and 3.99 pixels per pixel -- either side of the 60 pixels a unit can cover and of the -128 that the kernel clamps
    its first pixel to -- and units 2^22 pixels away."""
    assert run_cases(ctx, entering_cases(WALK_SRCS[0]), eb, 4820 + eb) == 4 * len(ENTER_K) * len(ENTER_SLOPES) + 8


@pytest.mark.parametrize('eb', (1, 2, 4))
def test_a_run_across_a_rows_end_and_off_the_end_of_the_tile(ctx, eb):
    """Section (d): at shift 0 every node is the centre of the source pixel with the same flat index, so every unit is 16
    consecutive elements and one load, also where it runs from a row's end into the next row's start; moved on by 7 and by 16
    elements the last units run off the end of the tile and are the `outside` word, not the first elements of the next tile
    (tile 0) nor the bytes behind the plane (tile 1).  At shift 3 the same nodes on a source 8 wide: exact positions, no run
    (tests/test_warp.py flat_cases says why)."""
    rng = np.random.default_rng(4830 + eb)
    bufs = Bufs(ctx)
    fill = outside_of(DTYPES[eb])
    n = FLAT_DST[0] * FLAT_DST[1]
    try:
        for case in flat_cases():
            tiles = random_tiles(rng, 2, case['src'], eb)
            tiles[tiles == fill] ^= 1                                         # no element is the `outside` word
            ref = run_device(ctx, bufs, tiles, case['mesh'], Spec(eb, case['shift'], OUT_WORD), case['dst'], off=3, what=case['name'])
            check_traits(case, ref)
            move = case['name'][2]
            flat, dst, idx = tiles.reshape(2, -1), ref['dst'].reshape(2, -1), ref['src_index'].reshape(2, -1)
            if case['shift'] == 0:
                assert np.array_equal(dst[:, :n - move], flat[:, move:]) and np.array_equal(idx[:, :n - move], np.tile(np.arange(move, n), (2, 1)))
                assert np.all(dst[:, n - move:] == fill) and np.all(idx[:, n - move:] == OUTSIDE), case['name']
            else:
                assert np.array_equal(dst[idx != OUTSIDE], flat[:, case['flat'][case['flat'] < n]].reshape(-1)) and np.all(dst[idx == OUTSIDE] == fill)
            assert 'fine=1' in ctx.last_kernel_info()
    finally:
        bufs.free()


def test_the_64_bit_form_at_the_far_end_of_a_long_raster(ctx):
    """Section (e) on the rasters of 2 x 2^23 and 2^23 x 2: the walk along the long side at -1, 2, 3 and 3.99 pixels per pixel
    up to the last node that int32 can hold, the short side entered and left."""
    assert run_cases(ctx, (c for src in ((2, LONG_SIDE), (LONG_SIDE, 2)) for c in long_side_cases(src)), 1, 4840) == 8


@pytest.mark.parametrize('eb', (1, 2, 4))
def test_decimation_by_4_5_and_16_takes_the_64_bit_form(ctx, eb):
    """Section (e) on a raster of 300 x 470: +-4, +-5 and +-16 pixels per pixel along a row, in the column and in the row."""
    assert run_cases(ctx, (c for s in (4, 8) for c in decimation_cases(s, WALK_SRCS[1])), eb, 4850 + eb) == 24


@pytest.mark.parametrize('eb', (1, 4))
def test_slopes_and_signs_where_every_pixel_has_its_own_cell(ctx, eb):
    """Section (f): the cases of (a) at shifts 0 and 3 (the FINE instantiation) on the raster of 100 x 257."""
    assert run_cases(ctx, (c for s in (0, 3) for c in slope_cases(s, WALK_SRCS[0])), eb, 4860 + eb) == 94
    assert 'fine=1' in ctx.last_kernel_info()


def test_a_flip_and_a_decimation_behind_the_batch_and_the_plane(ctx):
    """Section (g): a mesh of slope -1 and one of slope 2 through dswx_batch_warp on the WTR and the NIR plane against
    dswx_warp_host, and through DevicePlane.warp against warp_tiles."""
    from proteus_amd.pipeline import TileEngine
    n_tiles, h, w, dst, shift = 3, 61, 67, (70, 90), 4
    meshes = {}
    for name, xs, ys in (('flip', (-256, 0), (0, 256)), ('half', (512, 0), (0, 512))):
        cx, cy = fit_offsets(dst, xs, ys, (h, w))
        meshes[name] = affine_mesh(dst, shift, xs + (cx,), ys + (cy,))
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w)
    mbuf = ctx.malloc(meshes['flip'].nbytes)
    eng = TileEngine(ctx)
    try:
        batch.synth(SEED, tile0=47)
        batch.classify(_capi.default_params())
        for plane, dtype in (('wtr', np.uint8), ('nir', np.int16)):
            tiles = np.stack([batch.read_tile(plane, t) for t in range(n_tiles)]).reshape(n_tiles, h, w)
            assert tiles.dtype == dtype and len(np.unique(tiles)) > 1
            resident = eng.upload(tiles)
            for name, mesh in meshes.items():
                spec = Spec(tiles.dtype.itemsize, shift, OUT_WORD)
                want = _capi.warp_host(tiles, mesh, spec, dst)
                assert 0.1 < int(want['head'][0, 1]) / int(want['head'][0, 0]) < 0.9
                if name == 'flip':
                    idx, inside = whole_units(want['src_index'][0], dst)
                    assert (inside.all(axis=2) & np.all(np.diff(idx, axis=2) == -1, axis=2)).any()
                mbuf.upload(mesh.view(np.uint8).reshape(-1))
                res = batch.warp(plane, mbuf.ptr, dst, spec)
                info = ctx.last_kernel_info()
                ctx.synchronize()
                got = download(res, dtype, n_tiles, dst)
                assert info.count('dswx_warp_k') == 1 and f'elem_bytes={spec.elem_bytes}' in info, info
                for k in KEYS:
                    assert np.array_equal(got[k], want[k].reshape(-1)), (plane, name, k)
                res = resident.warp(mesh, dst, shift, outside=OUT_WORD, want=KEYS)
                ref = warp_tiles(tiles, mesh, shift, dst, OUT_WORD)
                for k in KEYS:
                    assert np.array_equal(res[k].numpy(), ref[k]) and np.array_equal(ref[k], want[k]), (plane, name, k)
    finally:
        eng.close()
        mbuf.free()
        batch.free()


def test_on_a_callers_stream_behind_the_copy_that_writes_the_plane(ctx):
    """The entry on a caller's stream is ordered behind that stream's earlier work and does not touch the context's stream: the
    plane is overwritten by a copy queued on the stream, the warp is queued behind it and sees the new plane."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(4300)
    T, H, W, dst, shift = 4, 100, 257, (120, 300), 4
    old = rng.integers(0, 100, size=(T, H, W), dtype=np.uint8)
    new = rng.integers(100, 256, size=(T, H, W), dtype=np.uint8)
    mesh_host = make_mesh('rotation', dst, shift, (H, W), rng)
    plane = torch.from_numpy(old.copy()).to('cuda:0')
    src = torch.from_numpy(new.copy()).to('cuda:0')
    mesh = torch.from_numpy(mesh_host.copy()).to('cuda:0')
    out_d = torch.full((T * dst[0] * dst[1],), SENT, dtype=torch.uint8, device='cuda:0')
    head = torch.full((T * 8,), -1, dtype=torch.int64, device='cuda:0')
    torch.cuda.synchronize()
    spec = Spec(1, shift, 9)
    want = _capi.warp_host(new, mesh_host, spec, dst)
    assert not np.array_equal(want['dst'], _capi.warp_host(old, mesh_host, spec, dst)['dst'])
    s = torch.cuda.Stream(device=0)
    with torch.cuda.stream(s):
        plane.copy_(src, non_blocking=True)
    ctx.warp_device(plane.data_ptr(), spec, T, H, W, mesh.data_ptr(), dst[0], dst[1], _capi.WarpOut.of(out_d.data_ptr(), None, head.data_ptr()),
                    stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    assert np.array_equal(out_d.cpu().numpy(), want['dst'].reshape(-1))
    assert np.array_equal(head.cpu().numpy().view(np.uint64).reshape(T, 8), want['head'])


def download(res, elem, n, dst):
    shapes = {'dst': (elem, n * dst[0] * dst[1]), 'src_index': (np.uint32, n * dst[0] * dst[1]), 'head': (np.uint64, n * 8)}
    got = {k: b.download(*shapes[k]) for k, b in res.items()}
    for b in res.values():
        b.free()
    return got


@pytest.mark.parametrize('form', ['packed', 'padded'])
def test_batch_warp_on_a_uint8_an_int16_and_the_diag_plane(ctx, form):
    n_tiles, h, w = 6, 61, 67
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, tile_align=1 if form == 'packed' else 256)
    rng = np.random.default_rng(4400)
    dst, shift = (70, 90), 4
    mh, mw = mesh_shape(dst, shift)
    meshes = np.stack([make_mesh(k, dst, shift, (h, w), rng) for k in ('rotation', 'shift', 'identity', 'garbage', 'half', 'rotation')])
    mbuf = ctx.malloc(meshes.nbytes)
    mbuf.upload(meshes.view(np.uint8).reshape(-1))
    try:
        batch.synth(SEED, tile0=31)
        batch.classify(_capi.default_params())
        for name, dtype in (('wtr', np.uint8), ('nir', np.int16), ('diag', np.uint16), ('fmask', np.uint8)):
            eb = np.dtype(dtype).itemsize
            tiles = np.stack([batch.read_tile(name, t) for t in range(n_tiles)]).reshape(n_tiles, h, w)
            assert tiles.dtype == dtype and len(np.unique(tiles)) > 1
            # one mesh for all tiles, then one per tile; every tile, then the forms of a range: mesh 0 belongs to tile0
            for stride_nodes in (0, mh * mw):
                spec = Spec(eb, shift, OUT_WORD, mesh_tile_stride_nodes=stride_nodes)
                for tile0, count in ((0, None), (2, 3), (1, n_tiles - 1), (n_tiles - 1, None), (1, _capi.BATCH_ALL_TILES), (n_tiles, None), (0, 0)):
                    res = batch.warp(name, mbuf.ptr, dst, spec, tile0=tile0, n_tiles=count)
                    info = ctx.last_kernel_info()
                    ctx.synchronize()
                    sub = tiles[tile0:] if count in (None, _capi.BATCH_ALL_TILES) else tiles[tile0:tile0 + count]
                    want = _capi.warp_host(sub, meshes[:len(sub)] if stride_nodes else meshes[0], spec, dst)
                    got = download(res, dtype, len(sub), dst)
                    assert list(got) == list(KEYS)
                    for k in KEYS:
                        assert np.array_equal(got[k], want[k].reshape(-1)), (name, stride_nodes, tile0, count, k)
                    if len(sub):
                        assert info.count('dswx_warp_k') == 1 and f'elem_bytes={eb}' in info, info
                        assert 0 < want['head'][0, 1]
        # an element size that is not the plane's, a stride, the counters, a plane this batch does not have, ranges outside the batch
        with pytest.raises(_capi.DswxError, match=r'band\[') as e:
            batch.warp('blue', mbuf.ptr, dst, Spec(1, shift))
        assert e.value.code == _capi.ERR_ARG and '2 bytes' in str(e.value)
        with pytest.raises(_capi.DswxError, match='diag') as e:
            batch.warp('diag', mbuf.ptr, dst, Spec(4, shift))
        assert e.value.code == _capi.ERR_ARG
        with pytest.raises(_capi.DswxError, match='src_tile_stride') as e:
            batch.warp('wtr', mbuf.ptr, dst, Spec(1, shift, src_tile_stride=h * w + 1))
        assert e.value.code == _capi.ERR_ARG
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.warp('counters', mbuf.ptr, dst, Spec(1, shift))
        assert e.value.code == _capi.ERR_ARG
        with pytest.raises(_capi.DswxError, match='land') as e:
            batch.warp('land', mbuf.ptr, dst, Spec(1, shift))
        assert e.value.code == _capi.ERR_ARG and 'no plane' in str(e.value)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside the batch'):
                batch.warp('wtr', mbuf.ptr, dst, Spec(1, shift), tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(_capi.DswxError, match='mesh') as e:
            batch.warp('wtr', mbuf.ptr + 2, dst, Spec(1, shift))
        assert e.value.code == _capi.ERR_ALIGN
    finally:
        mbuf.free()
        batch.free()


def test_past_the_tiles_of_one_launch(ctx):
    """65535 + 4 tiles of 3 x 5 warped to 4 x 6 with a mesh per tile: every tile compared, on every output."""
    rng = np.random.default_rng(4500)
    T, src, dst, shift = 65535 + 4, (3, 5), (4, 6), 4
    tiles = rng.integers(0, 1 << 16, size=(T,) + src, dtype=np.uint16)
    mh, mw = mesh_shape(dst, shift)
    mesh = rng.integers(-256 * 20, 256 * 24, size=(T, mh, mw, 2)).astype(np.int32)         # a few pixels around the raster, inside and outside
    mesh[-3:] = make_mesh('identity', dst, shift, src, rng)
    bufs = Bufs(ctx)
    try:
        ref = run_device(ctx, bufs, tiles, mesh, Spec(2, shift, OUT_WORD, mesh_tile_stride_nodes=mh * mw), dst, what='65539 tiles')
        assert 'grid=(1,65535,1)' in ctx.last_kernel_info()
        inside = ref['head'][:, 1]
        assert inside[-1] == 15 and inside[:-3].min() < inside[:-3].max() and (inside[65535:] > 0).any()
    finally:
        bufs.free()


def test_label_plane_there_and_back(ctx):
    """A uint32 label plane warped by a whole-pixel shift (a, b) and then by (-a, -b): the interior is restored, the rim is
    `outside`; and src_index of the first warp gathers any further plane to the same positions."""
    from proteus_amd.label import wtr_label_spec
    from proteus_amd.pipeline import TileEngine
    rng = np.random.default_rng(4600)
    H, W, a, b, shift = 90, 140, 7, -5, 5
    wtr = rng.choice(np.array([0, 1, 2, 253], dtype=np.uint8), size=(2, H, W), p=[.5, .3, .1, .1])
    eng = TileEngine(ctx)
    try:
        p = eng.upload(wtr)
        lab = p.label(wtr_label_spec(1), want=('label',))['label']
        labels = lab.numpy().copy()
        assert labels.dtype == np.uint32 and labels.shape == (2, H, W) and len(np.unique(labels)) > 10
        there = lab.warp(exact_mesh((H, W), shift, lambda X, Y: X + a, lambda X, Y: Y + b), (H, W), shift, outside=OUTSIDE, want=('dst', 'src_index'))
        back = there['dst'].warp(exact_mesh((H, W), shift, lambda X, Y: X - a, lambda X, Y: Y - b), (H, W), shift, outside=OUTSIDE)
        got = back['dst'].numpy()
        inner = np.zeros((H, W), dtype=bool)
        inner[max(-b, 0):H - max(b, 0), max(-a, 0):W - max(a, 0)] = True                   # survives the first warp ...
        inner2 = np.zeros((H, W), dtype=bool)
        inner2[max(b, 0):H - max(-b, 0), max(a, 0):W - max(-a, 0)] = True                  # ... and is reachable by the second
        assert np.array_equal(got[:, inner2], labels[:, inner2]) and np.all(got[:, ~inner2] == OUTSIDE)
        # the same positions for another plane: a plain gather through src_index
        idx = there['src_index'].numpy()
        moved = p.warp(exact_mesh((H, W), shift, lambda X, Y: X + a, lambda X, Y: Y + b), (H, W), shift, outside=255)['dst'].numpy()
        for t in range(2):
            ok = idx[t] != OUTSIDE
            assert np.array_equal(ok, inner) and np.array_equal(moved[t][ok], wtr[t].reshape(-1)[idx[t][ok]]) and np.all(moved[t][~ok] == 255)
        # DevicePlane.warp against the numpy statement, one raster and a mesh per raster
        one = eng.upload(wtr[0])
        mesh = make_mesh('rotation', (80, 100), 4, (H, W), rng)
        res = one.warp(mesh, (80, 100), 4, outside=9, want=KEYS)
        want = warp_tiles(wtr[:1], mesh, 4, (80, 100), 9)
        assert res['dst'].shape == (80, 100) and res['head'].shape == (1, 8)
        for k in KEYS:
            assert np.array_equal(res[k].numpy().reshape(want[k].shape), want[k]), k
        both = np.stack([mesh, make_mesh('shift', (80, 100), 4, (H, W), rng)])
        res2 = p.warp(both, (80, 100), 4, outside=9, want=KEYS)
        want = warp_tiles(wtr, both, 4, (80, 100), 9)
        for k in KEYS:
            assert np.array_equal(res2[k].numpy(), want[k]), k
        with pytest.raises(ValueError):
            p.warp(mesh[:-1], (80, 100), 4)
        with pytest.raises(ValueError):
            p.warp(mesh, (80, -1), 4)
    finally:
        eng.close()


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name.replace('.', '_'), os.path.join(ROOT, 'bin', name))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def two_products(tmp_path):
    """Two small synthetic WTR products whose footprints overlap on the ground: one on the east side of UTM zone 32, one on
    the west side of zone 33, at about 45 degrees N."""
    rng = np.random.default_rng(4700)
    H, W = 120, 150
    gt32 = (699960.0, 30.0, 0.0, 5000040.0, 0.0, -30.0)
    lon, lat = warp.tm_inverse(gt32[0] + 2400.0 - 500000.0, gt32[3] - 600.0, 9.0)
    e, n = warp.tm_forward(lon, lat, 15.0)
    gt33 = (float(np.floor((e + 500000.0 - 900.0) / 30.0) * 30.0), 30.0, 0.0, float(np.ceil((n + 900.0) / 30.0) * 30.0), 0.0, -30.0)
    layers = rng.choice(np.array([0, 1, 2, 252, 253, 254], dtype=np.uint8), size=(2, H, W), p=[.35, .3, .1, .05, .15, .05])
    files = [str(tmp_path / 'zone32_WTR.tif'), str(tmp_path / 'zone33_WTR.tif')]
    for f, layer, gt, epsg in zip(files, layers, (gt32, gt33), (32632, 32633)):
        geotiff.write_geotiff(f, layer, geo_tags=geotiff.geo_tags_from_geotransform(gt, epsg=epsg), metadata={'SPACECRAFT_NAME': 'test'}, nodata=255)
    return files, layers, (gt32, gt33)


def test_the_warp_tool(tmp_path, capsys):
    """bin/dswx_warp.py: the zone 33 product onto the lattice of the zone 32 product, and a same-zone product onto a shifted,
    coarser lattice: the output is warp_tiles of the mesh that proteus_amd.warp makes, a valid COG with the GeoKeys and the
    geotransform of --like."""
    tool = load_tool('dswx_warp.py')
    files, layers, gts = two_products(tmp_path)
    out = str(tmp_path / 'out.tif')
    assert tool.main([files[1], '--like', files[0], '--shift', '4', '--outside', '255', '-o', out]) == 0
    arr, info = geotiff.read_geotiff(out)
    mesh, dev = warp.utm_mesh(gts[1], 32633, gts[0], 32632, layers[0].shape, 4)
    want = warp_tiles(layers[1:2], mesh, 4, layers[0].shape, 255)
    assert np.array_equal(arr, want['dst'][0]) and 0 < want['head'][0, 1] < want['head'][0, 0] and dev < 8
    assert geotiff.validate_cog(out) == [] and tuple(info.geotransform) == gts[0] and info.nodata == 255
    assert list(info.geo_tags[geotiff.TAG_GEOKEYS][1])[-1] == 32632 and info.metadata['SPACECRAFT_NAME'] == 'test'
    said = capsys.readouterr().out
    assert 'file saved' in said and 'inside' in said
    # the same SRS: another origin and pixel size
    like = str(tmp_path / 'coarse.tif')
    gt = (gts[0][0] + 45.0, 60.0, 0.0, gts[0][3] - 90.0, 0.0, -60.0)
    geotiff.write_geotiff(like, np.zeros((50, 60), dtype=np.uint8), geo_tags=geotiff.geo_tags_from_geotransform(gt, epsg=32632), nodata=255)
    assert tool.main([files[0], '--like', like, '-o', out]) == 0
    arr, info = geotiff.read_geotiff(out)
    want = warp_tiles(layers[:1], warp.affine_mesh(gts[0], gt, (50, 60), 6), 6, (50, 60), 255)['dst'][0]
    assert np.array_equal(arr, want) and tuple(info.geotransform) == gt
    # what is not WGS 84 / UTM is refused
    other = str(tmp_path / 'geographic.tif')
    geotiff.write_geotiff(other, layers[0], geo_tags=geotiff.geo_tags_from_geotransform((9.0, 1e-3, 0.0, 45.0, 0.0, -1e-3), epsg=4326), nodata=255)
    capsys.readouterr()
    assert tool.main([other, '--like', files[0], '-o', str(tmp_path / 'no.tif')]) == 1
    assert 'WGS 84 / UTM' in capsys.readouterr().out and not os.path.exists(str(tmp_path / 'no.tif'))


def test_the_mosaic_tool_reprojects_only_when_asked(tmp_path, capsys):
    """bin/dswx_mosaic.py --reproject: the zone 33 product is warped on the device onto the lattice of the zone 32 product and
    placed; the output is warp_tiles + mosaic_tiles on the host.  Without the flag the refusal is word for word the old one."""
    from proteus_amd.mosaic import mosaic_tiles, wtr_mosaic_spec
    tool = load_tool('dswx_mosaic.py')
    files, layers, gts = two_products(tmp_path)
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], files[1]]) == 1
    text = capsys.readouterr().out
    a = geotiff.read_geotiff(files[0])[1].geo_tags[geotiff.TAG_GEOKEYS]
    b = geotiff.read_geotiff(files[1])[1].geo_tags[geotiff.TAG_GEOKEYS]
    assert text.strip() == (f'[FAIL] Comparing projection\n       * input 1 GeoTIFF tag {geotiff.TAG_GEOKEYS} with content "{a}" differs from input '
                            f'2 GeoTIFF tag {geotiff.TAG_GEOKEYS} with content "{b}".')
    assert not os.path.exists(str(tmp_path / 'no_LAST.tif'))
    prefix = str(tmp_path / 'out')
    assert tool.main(['--reproject', '-o', prefix, files[0], files[1]]) == 0
    H, W = layers[0].shape
    # the window of input 2 on the lattice of input 1: H x W around the centre of its footprint, at a whole pixel
    cx, cy = warp.utm_to_utm(gts[1][0] + W / 2 * 30.0, gts[1][3] - H / 2 * 30.0, 32633, 32632)
    col0, row0 = int(round((float(cx) - gts[0][0]) / 30.0 - W / 2)), int(round((float(cy) - gts[0][3]) / -30.0 - H / 2))
    window = (gts[0][0] + col0 * 30.0, 30.0, 0.0, gts[0][3] - row0 * 30.0, 0.0, -30.0)
    assert window == tool.reproject_window(gts[1], 32633, gts[0], 32632, H, W) and (row0, col0) != (0, 0)
    mesh, _ = warp.utm_mesh(gts[1], 32633, window, 32632, (H, W), tool.REPROJECT_SHIFT)
    moved = warp_tiles(layers[1:2], mesh, tool.REPROJECT_SHIFT, (H, W), 255)['dst'][0]
    from proteus_amd.mosaic import layout
    ch, cw, place, gt = layout([gts[0], window], H, W)
    assert place.tolist() == [[max(-row0, 0), max(-col0, 0)], [max(row0, 0), max(col0, 0)]]
    want = mosaic_tiles(np.stack([layers[0], moved]), place, (ch, cw), wtr_mosaic_spec())
    for suffix, ref in (('LAST', want['last']), ('SHARE', want['share']), ('COUNT_WATER', want['count'][0]), ('LAST_INDEX', want['last_index'])):
        arr, info = geotiff.read_geotiff(f'{prefix}_{suffix}.tif')
        assert np.array_equal(arr, ref), suffix
        assert tuple(info.geotransform) == gt and list(info.geo_tags[geotiff.TAG_GEOKEYS][1])[-1] == 32632
        assert info.metadata['MOSAIC_REPROJECTED_INPUTS'] == '2'
    assert (want['last_index'] == 1).any() and (want['last_index'] == 0).any() and (want['count'].sum(axis=0) == 2).any()
    # an input off the lattice of input 1 by half a pixel: refused without the flag in the old words, resampled with it
    half = str(tmp_path / 'half.tif')
    gt_half = (gts[0][0] + 15.0 + 600.0,) + gts[0][1:]
    geotiff.write_geotiff(half, layers[1], geo_tags=geotiff.geo_tags_from_geotransform(gt_half, epsg=32632), nodata=255)
    capsys.readouterr()
    assert tool.main(['-o', str(tmp_path / 'no'), files[0], half]) == 1
    text = capsys.readouterr().out
    assert '[FAIL] Comparing geotransform' in text and 'input 2 origin' in text and 'lattice' in text
    assert tool.main(['--reproject', '-o', prefix, files[0], half]) == 0
    window = tool.reproject_window(gt_half, None, gts[0], None, H, W)
    assert window[0] in (gts[0][0] + 600.0, gts[0][0] + 630.0) and window[3] == gts[0][3]
    moved = warp_tiles(layers[1:2], warp.affine_mesh(gt_half, window, (H, W), tool.REPROJECT_SHIFT), tool.REPROJECT_SHIFT, (H, W), 255)['dst'][0]
    ch, cw, place, gt = layout([gts[0], window], H, W)
    want = mosaic_tiles(np.stack([layers[0], moved]), place, (ch, cw), wtr_mosaic_spec())
    assert np.array_equal(geotiff.read_geotiff(f'{prefix}_LAST.tif')[0], want['last'])


def test_warp_example_runs(tmp_path):
    """examples/batch_warp.c: its own checks (exit status 0: every pixel of the warped WTR plane against a loop over the
    downloaded layer and against dswx_warp_host)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_warp')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_warp.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}', '-lm',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '301', '27'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr warp: device, loop and host entry agree in every pixel' in r.stdout
