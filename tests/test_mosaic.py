"""The mosaic of include/dswx_hip.h ("mosaic") without a GPU: the library's scalar statement (dswx_mosaic_host), the numpy
statement (proteus_amd/mosaic.py) and two further statements written here -- a per-pixel Python loop, and "paste every tile
into a stack of canvases, then stack" -- agree on every output; the identity placement is dswx_stack_host in every byte;
placements over every edge of the canvas, outside it, larger than it, coinciding, INT32_MIN / INT32_MAX; empty inputs; every
refusal that needs no device, and a refused call writes nothing; layout(); the header and the struct mirror."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.mosaic import MAX_SIDE, Spec, layout, mosaic_tiles, wtr_mosaic_spec
from proteus_amd.stack import NONE, NO_SHARE, stack_tiles, wtr_spec
from proteus_amd import stack as stack_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT8, SENT16 = 0xEE, 0xEEEE
KEYS = ('count', 'last', 'last_index', 'share')
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
NOT_OBS = 0xA5                                     # a byte that the specs below never count


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4])


def random_spec(rng, n_cats):
    """Categories 0 .. 5 at random (4 and 5 are never observations); NOT_OBS is never one."""
    cat = rng.integers(0, 6, size=256).astype(np.uint8)
    cat[NOT_OBS] = 255
    return Spec(n_cats, cat, int(rng.integers(0, 256)), int(rng.integers(0, 256)))


# ---- the definition, written out again: one canvas pixel at a time -------------------------------------------------------
def scalar_mosaic(tiles, place, canvas_shape, spec):
    T, H, W = tiles.shape
    CH, CW = canvas_shape
    cat = [int(c) for c in spec.cat_of_byte]
    rows = tiles.tolist()
    res = {'count': np.zeros((spec.n_cats, CH, CW), dtype=np.uint16), 'last': np.zeros((CH, CW), dtype=np.uint8),
           'last_index': np.zeros((CH, CW), dtype=np.uint16), 'share': np.zeros((CH, CW), dtype=np.uint8)}
    for Y in range(CH):
        for X in range(CW):
            count, last, index, covered = [0] * spec.n_cats, spec.fill, 65535, False
            for t in range(T):
                r, c = Y - int(place[t][0]), X - int(place[t][1])
                if 0 <= r < H and 0 <= c < W:
                    covered = True
                    b = rows[t][r][c]
                    if cat[b] < spec.n_cats:
                        count[cat[b]] += 1
                        last, index = b, t
            n_obs = sum(count)
            res['count'][:, Y, X] = count
            res['last'][Y, X] = last if covered else spec.outside
            res['last_index'][Y, X] = index
            res['share'][Y, X] = (100 * count[0]) // n_obs if n_obs else 255
    return res


# ---- and once more: every tile pasted into a canvas of its own, the canvases stacked ------------------------------------
def pasted_stack(tiles, place, canvas_shape, spec):
    assert spec.cat_of_byte[NOT_OBS] >= spec.n_cats
    T, H, W = tiles.shape
    CH, CW = canvas_shape
    canvases = np.full((T, CH, CW), NOT_OBS, dtype=np.uint8)
    covered = np.zeros((CH, CW), dtype=bool)
    for t in range(T):
        for r in range(H):
            Y = r + int(place[t][0])
            if not 0 <= Y < CH:
                continue
            for c in range(W):
                X = c + int(place[t][1])
                if 0 <= X < CW:
                    canvases[t, Y, X] = tiles[t, r, c]
                    covered[Y, X] = True
    res = stack_tiles(canvases, spec)
    res['last'] = np.where(covered, res['last'], spec.outside).astype(np.uint8)
    return res


def all_agree(tiles, place, canvas_shape, spec, what, loop=True):
    tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
    want = mosaic_tiles(tiles, place, canvas_shape, spec)
    same(_capi.mosaic_host(tiles, place, canvas_shape, spec), want, (what, 'host entry'))
    if loop:
        same(scalar_mosaic(tiles, place, canvas_shape, spec), want, (what, 'per-pixel loop'))
        same(pasted_stack(tiles, place, canvas_shape, spec), want, (what, 'pasted stack'))
    return want


def test_four_statements_agree_on_random_placements():
    rng = np.random.default_rng(9500)
    for case, (T, H, W, CH, CW) in enumerate(((1, 3, 4, 5, 7), (4, 5, 6, 9, 11), (7, 8, 13, 24, 40), (12, 24, 40, 10, 17),
                                              (9, 1, 1, 6, 6), (5, 30, 50, 24, 40), (3, 2, 40, 24, 3))):
        for n_cats in (1, 2, 3, 4):
            spec = random_spec(rng, n_cats)
            tiles = rng.integers(0, 256, size=(T, H, W), dtype=np.uint8)
            tiles[rng.random(tiles.shape) < 0.2] = NOT_OBS
            place = np.stack([rng.integers(-H - 1, CH + 2, size=T), rng.integers(-W - 1, CW + 2, size=T)], axis=1)
            all_agree(tiles, place, (CH, CW), spec, (case, n_cats))


@pytest.mark.parametrize('n_cats', [1, 2, 3, 4])
def test_identity_placement_is_the_stack_in_every_byte(n_cats):
    """All placements (0, 0), canvas = tile: dswx_stack_host on the same bytes, n_tiles x n_elems of test_stack.py."""
    rng = np.random.default_rng(9600 + n_cats)
    for T in (0, 1, 2, 255, 256, 257):
        for n in (0, 1, 15, 16, 17):
            spec = random_spec(rng, n_cats)
            tiles = rng.integers(0, 256, size=(T, n), dtype=np.uint8)
            want = _capi.stack_host(tiles, stack_mod.Spec(spec.n_cats, spec.cat_of_byte, spec.fill))
            for shape in ((1, n), (n, 1)):
                got = _capi.mosaic_host(tiles.reshape((T,) + shape), np.zeros((T, 2), dtype=np.int32), shape, spec)
                if T == 0 and n:
                    assert np.all(got['last'] == spec.outside)
                    got['last'][:] = spec.fill                            # no tile: nothing covers, the one difference
                same({k: v.reshape((n_cats, n) if k == 'count' else (n,)) for k, v in got.items()}, want, (T, n, shape))


def test_placements_over_and_outside_every_edge():
    rng = np.random.default_rng(9700)
    H, W, CH, CW = 6, 9, 12, 20
    spec = random_spec(rng, 3)
    tile = lambda T=1, h=H, w=W: rng.integers(0, 256, size=(T, h, w), dtype=np.uint8)
    # each of the four canvas edges overhung, and every corner
    for r0 in (-3, 2, CH - 2):
        for c0 in (-4, 5, CW - 3):
            want = all_agree(tile(), [(r0, c0)], (CH, CW), spec, ('overhang', r0, c0))
            assert (want['last'] == spec.outside).sum() >= CH * CW - H * W
    # wholly outside on each side, by one pixel and by far
    for r0, c0 in ((-H, 3), (CH, 3), (2, -W), (2, CW), (-H - 50, 0), (CH + 50, 0), (0, -W - 50), (0, CW + 50), (-H, -W), (CH, CW)):
        want = all_agree(tile(), [(r0, c0)], (CH, CW), spec, ('outside', r0, c0))
        assert np.all(want['last'] == spec.outside) and np.all(want['last_index'] == NONE) and np.all(want['share'] == NO_SHARE)
        assert not want['count'].any()
    # one row / one column still on the canvas
    for r0, c0 in ((-H + 1, 3), (CH - 1, 3), (2, -W + 1), (2, CW - 1)):
        want = all_agree(tile(), [(r0, c0)], (CH, CW), spec, ('one line', r0, c0))
        assert (want['last_index'] != NONE).sum() <= max(H, W)
    # a tile larger than the canvas, over every edge at once
    big = tile(2, 30, 50)
    want = all_agree(big, [(-7, -9), (-18, -30)], (CH, CW), spec, 'larger than the canvas')
    assert not np.any(want['count'].sum(axis=0) > 2)
    # two tiles at one place: the later one wins where it observed
    two = tile(2)
    two[1, :, :4] = NOT_OBS
    want = all_agree(two, [(3, 4), (3, 4)], (CH, CW), spec, 'two tiles at one place')
    assert np.array_equal(want['last'][3:3 + H, 4:8], np.where(spec.cat_of_byte[two[0, :, :4]] < spec.n_cats, two[0, :, :4], spec.fill))
    # one pixel of overlap (a corner), one column of overlap
    want = all_agree(tile(2), [(0, 0), (H - 1, W - 1)], (CH, CW), spec, 'one pixel of overlap')
    every = Spec(1, np.zeros(256, dtype=np.uint8), 0, 0)
    both = mosaic_tiles(tile(2), [(0, 0), (H - 1, W - 1)], (CH, CW), every)['count'][0]
    assert (both == 2).sum() == 1 and both[H - 1, W - 1] == 2
    # the ends of int32: ordinary values, evaluated in 64 bits
    for r0 in (I32_MIN, I32_MAX, I32_MAX - H + 1, 0):
        for c0 in (I32_MIN, I32_MAX, 0):
            if (r0, c0) == (0, 0):
                continue
            pair = tile(2)
            all_agree(pair, [(r0, c0), (1, 1)], (CH, CW), spec, ('int32 ends', r0, c0), loop=False)
            got = _capi.mosaic_host(pair, [(r0, c0), (1, 1)], (CH, CW), every)        # the far tile covers nothing of the canvas
            alone = np.zeros((CH, CW), dtype=np.uint16)
            alone[1:1 + H, 1:1 + W] = 1
            assert np.array_equal(got['count'][0], alone) and np.array_equal(got['last_index'], np.where(alone, 1, NONE))


def test_empty_inputs():
    rng = np.random.default_rng(9800)
    spec = random_spec(rng, 2)
    # no tile: the outside values
    got = _capi.mosaic_host(np.zeros((0, 4, 5), dtype=np.uint8), np.zeros((0, 2)), (3, 7), spec)
    same(got, mosaic_tiles(np.zeros((0, 4, 5), dtype=np.uint8), np.zeros((0, 2)), (3, 7), spec), 'no tile')
    assert np.all(got['last'] == spec.outside) and np.all(got['last_index'] == NONE) and np.all(got['share'] == NO_SHARE) and not got['count'].any()
    # an empty canvas writes nothing
    tiles = rng.integers(0, 256, size=(2, 4, 5), dtype=np.uint8)
    for shape in ((0, 6), (6, 0), (0, 0)):
        got = _capi.mosaic_host(tiles, [(0, 0), (1, 1)], shape, spec)
        assert got['last'].shape == shape and got['count'].shape == (2,) + shape
        same(got, mosaic_tiles(tiles, [(0, 0), (1, 1)], shape, spec), shape)
    # an empty tile raster covers nothing
    for shape in ((0, 5), (4, 0)):
        empty = np.zeros((3,) + shape, dtype=np.uint8)
        got = _capi.mosaic_host(empty, [(0, 0)] * 3, (3, 4), spec)
        same(got, mosaic_tiles(empty, [(0, 0)] * 3, (3, 4), spec), shape)
        assert np.all(got['last'] == spec.outside)
    # a padded plane: the padding (an observation, were it read) is never read
    cat = spec.cat_of_byte.copy()
    cat[0x5A] = 0
    padded_spec = Spec(2, cat, spec.fill, spec.outside)
    plane = np.full((2, 4 * 5 + 7), 0x5A, dtype=np.uint8)
    plane[:, :20] = np.where(tiles.reshape(2, 20) == 0x5A, 1, tiles.reshape(2, 20))
    got = _capi.mosaic_host(plane, [(1, 2), (-1, 3)], (6, 9), padded_spec, raster=(4, 5))
    same(got, mosaic_tiles(plane[:, :20].reshape(2, 4, 5), [(1, 2), (-1, 3)], (6, 9), padded_spec), 'padded plane')


def test_subsets_of_outputs_and_odd_addresses_on_the_host():
    rng = np.random.default_rng(9900)
    lib = _capi.load_library()
    spec = random_spec(rng, 3)
    T, H, W, CH, CW = 4, 5, 7, 9, 13
    raw = np.zeros(T * H * W + 64, dtype=np.uint8)
    praw = np.zeros(T * 8 + 64, dtype=np.uint8)
    tiles = rng.integers(0, 256, size=(T, H, W), dtype=np.uint8)
    place = np.stack([rng.integers(-3, CH, size=T), rng.integers(-3, CW, size=T)], axis=1).astype(np.int32)
    want = mosaic_tiles(tiles, place, (CH, CW), spec)
    n = CH * CW
    for off in (0, 1, 3):
        raw[off:off + tiles.size] = tiles.reshape(-1)
        praw[off:off + T * 8] = place.view(np.uint8).reshape(-1)
        for wanted in [(k,) for k in KEYS] + [KEYS]:
            bufs = {k: np.full((3 if k == 'count' else 1) * n * 2 + 64, SENT8, dtype=np.uint8) for k in KEYS}
            eb = {'count': 2, 'last': 1, 'last_index': 2, 'share': 1}
            out = _capi.StackOut.of(count=[bufs['count'].ctypes.data + off + 2 * n * k for k in range(3)] if 'count' in wanted else (),
                                    **{k: bufs[k].ctypes.data + off for k in KEYS[1:] if k in wanted})
            rc = lib.dswx_mosaic_host(raw.ctypes.data + off, ctypes.byref(_capi.MosaicSpec.of(spec)), T, H, W, 0, praw.ctypes.data + off,
                                      CH, CW, ctypes.byref(out))
            assert rc == 0, lib.dswx_last_error()
            for k in KEYS:
                used = (3 if k == 'count' else 1) * n * eb[k] if k in wanted else 0
                b = bufs[k]
                assert np.all(b[:off] == SENT8) and np.all(b[off + used:] == SENT8), (k, wanted, off)
                if k in wanted:
                    got = b[off:off + used].copy().view(np.uint16 if eb[k] == 2 else np.uint8).reshape(want[k].shape)
                    assert np.array_equal(got, want[k]), (k, wanted, off)
    same(_capi.mosaic_host(tiles, place, (CH, CW), spec, want=('share',)), {'share': want['share']}, 'the wrapper, share alone')


def test_refusals_that_need_no_device():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    good = Spec(2, [1, 0] + [255] * 254, 255, 7)
    H, W, CH, CW = 2, 4, 3, 5
    n = CH * CW
    tiles = np.zeros((3, H, W), dtype=np.uint8)
    place = np.zeros((3, 2), dtype=np.int32)
    planes = {k: np.full(2 * n if k == 'count' else n, SENT16 if k in ('count', 'last_index') else SENT8,
                         dtype=np.uint16 if k in ('count', 'last_index') else np.uint8) for k in KEYS}

    def outs(**kw):
        o = _capi.StackOut.of(count=[planes['count'].ctypes.data, planes['count'].ctypes.data + 2 * n],
                              last=planes['last'].ctypes.data, last_index=planes['last_index'].ctypes.data,
                              share=planes['share'].ctypes.data)
        for k, v in kw.items():
            if k.startswith('count'):
                o.count[int(k[5:])] = v
            else:
                setattr(o, k, v)
        return o

    def spec_c(**kw):
        s = _capi.MosaicSpec.of(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def host(plane=tiles.ctypes.data, spec=None, n_tiles=3, height=H, width=W, stride=0, place_=place.ctypes.data, canvas_h=CH,
             canvas_w=CW, out=None, null_spec=False, null_out=False):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out
        return lib.dswx_mosaic_host(vp(plane) if plane else None, None if null_spec else ctypes.byref(spec), n_tiles, height, width,
                                    stride, vp(place_) if place_ else None, canvas_h, canvas_w, None if null_out else ctypes.byref(out))

    def dev(plane=0x10000, spec=None, n_tiles=3, height=H, width=W, stride=0, place_=0x20000, canvas_h=CH, canvas_w=CW, out=None,
            null_spec=False, null_out=False):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out                   # host addresses, never dereferenced: every call fails first
        return lib.dswx_mosaic_device(None, vp(plane) if plane else None, None if null_spec else ctypes.byref(spec), n_tiles, height,
                                      width, stride, vp(place_) if place_ else None, canvas_h, canvas_w,
                                      None if null_out else ctypes.byref(out), None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        # those of dswx_stack_device
        refused(call(null_spec=True), _capi.ERR_ARG, b'spec is NULL')
        refused(call(null_out=True), _capi.ERR_ARG, b'out is NULL')
        for n_cats in (-1, 0, 5, 100):
            refused(call(spec=spec_c(n_cats=n_cats)), _capi.ERR_ARG, b'n_cats')
        for fill in (-1, 256, 1 << 20):
            refused(call(spec=spec_c(fill=fill)), _capi.ERR_ARG, b'fill')
        for kw in ({'n_tiles': -1}, {'height': -1}, {'width': -1}, {'stride': -5}):
            refused(call(**kw), _capi.ERR_ARG, b'negative')
        refused(call(stride=H * W - 1), _capi.ERR_ARG, b'stride')
        for T in (65536, 1 << 20, 1 << 40):
            refused(call(n_tiles=T), _capi.ERR_ARG, b'n_tiles')
            assert b'65535' in lib.dswx_last_error()
        refused(call(height=(1 << 30) + 1), _capi.ERR_ARG, b'too large')
        refused(call(height=1 << 30, width=1 << 30, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(height=1 << 20, width=1 << 20, n_tiles=65535), _capi.ERR_ARG, b'too large')
        refused(call(plane=0), _capi.ERR_ARG, b'plane is NULL')
        for k in (2, 3):                                       # n_cats is 2
            refused(call(out=outs(**{f'count{k}': planes['count'].ctypes.data})), _capi.ERR_ARG, f'count[{k}]'.encode())
        refused(call(out=_capi.StackOut()), _capi.ERR_ARG, b'every output is NULL')
        # and the mosaic's own
        for outside in (-1, 256, 1 << 20):
            refused(call(spec=spec_c(outside=outside)), _capi.ERR_ARG, b'outside')
        for reserved in (1, -1):
            refused(call(spec=spec_c(reserved=reserved)), _capi.ERR_ARG, b'reserved')
        for kw in ({'canvas_h': -1}, {'canvas_w': -1}, {'canvas_h': -(1 << 40)}):
            refused(call(**kw), _capi.ERR_ARG, b'negative canvas')
        for kw in ({'canvas_h': (1 << 30) + 1}, {'canvas_w': (1 << 30) + 1}, {'canvas_h': 1 << 30, 'canvas_w': 1 << 30}, {'canvas_w': 1 << 62}):
            refused(call(**kw), _capi.ERR_ARG, b'too large')
            assert b'canvas' in lib.dswx_last_error()
        refused(call(place_=0), _capi.ERR_ARG, b'place is NULL')
    # the device entry: alignment of the uint16 outputs and of the table; then, with everything in order, the context
    for k, name in ((0, b'count[0]'), (1, b'count[1]')):
        refused(dev(out=outs(**{f'count{k}': planes['count'].ctypes.data + 1})), _capi.ERR_ALIGN, name)
    refused(dev(out=outs(last_index=planes['last_index'].ctypes.data + 1)), _capi.ERR_ALIGN, b'last_index')
    for off in (1, 2, 3):
        refused(dev(place_=0x20000 + off), _capi.ERR_ALIGN, b'place')
    refused(dev(), _capi.ERR_ARG, b'ctx')
    refused(dev(plane=0x10001, place_=0x20004), _capi.ERR_ARG, b'ctx')                   # the plane takes any address
    refused(dev(plane=0, place_=0, n_tiles=0), _capi.ERR_ARG, b'ctx')                    # nothing to read: neither is needed
    refused(dev(plane=0, height=0), _capi.ERR_ARG, b'ctx')
    refused(dev(canvas_h=0), _capi.ERR_ARG, b'ctx')
    refused(dev(canvas_h=1 << 30, canvas_w=1 << 16), _capi.ERR_ARG, b'ctx')
    refused(dev(stride=H * W + 1, n_tiles=65535), _capi.ERR_ARG, b'ctx')
    refused(lib.dswx_batch_mosaic(None, 14, ctypes.byref(spec_c()), 0, 1, vp(0x20000), CH, CW, ctypes.byref(outs()), None),
            _capi.ERR_ARG, b'batch is NULL')
    # a refused call wrote nothing
    for k in KEYS:
        assert np.all(planes[k] == (SENT16 if k in ('count', 'last_index') else SENT8)), k
    # and the same arguments, accepted: legal corners of the host entry
    assert host() == 0
    assert np.all(planes['last'].reshape(CH, CW)[:H, :W] == 0) and np.all(planes['last'].reshape(CH, CW)[H:] == 7)
    assert np.all(planes['count'][n:].reshape(CH, CW)[:H, :W] == 3)
    assert host(plane=0, place_=0, n_tiles=0) == 0 and np.all(planes['last'] == 7) and np.all(planes['last_index'] == NONE)
    planes['last'][:] = SENT8
    assert host(canvas_h=0) == 0 and host(canvas_w=0) == 0 and np.all(planes['last'] == SENT8)      # an empty canvas writes nothing
    assert host(plane=0, width=0) == 0 and np.all(planes['last'] == 7)                               # an empty raster covers nothing
    # the Python side refuses what the library would
    for bad in (lambda: Spec(0, np.zeros(256)), lambda: Spec(2, np.zeros(256), outside=256), lambda: Spec(2, np.zeros(256), outside=-1),
                lambda: Spec(2, np.zeros(256), fill=256), lambda: mosaic_tiles(np.zeros((2, 2), dtype=np.uint8), [(0, 0)] * 2, (2, 2), good),
                lambda: _capi.mosaic_host(np.zeros((2, 2, 2), dtype=np.uint16), [(0, 0)] * 2, (2, 2), good),
                lambda: _capi.mosaic_host(tiles, place, (2, 2), good, want=('median',))):
        with pytest.raises(ValueError):
            bad()


def test_layout_of_a_2_x_2_block_of_mgrs_like_tiles_and_its_refusals():
    """Tiles of 3660 x 3660 pixels of 30 m whose origins lie 3334 pixels apart (326 pixels of overlap), given in any order."""
    x0, y0, d = 499980.0, 4100040.0, 30.0
    step = 3334 * d
    gts = [(x0 + step, d, 0.0, y0, 0.0, -d), (x0, d, 0.0, y0, 0.0, -d), (x0 + step, d, 0.0, y0 - step, 0.0, -d), (x0, d, 0.0, y0 - step, 0.0, -d)]
    ch, cw, place, gt = layout(gts, 3660, 3660)
    assert (ch, cw) == (6994, 6994) and gt == (x0, d, 0.0, y0, 0.0, -d)
    assert place.dtype == np.int32 and place.tolist() == [[0, 3334], [0, 0], [3334, 3334], [3334, 0]]
    assert layout(gts[:1], 100, 130)[:2] == (100, 130) and layout(gts[:1], 100, 130)[2].tolist() == [[0, 0]]
    ch, cw, place, gt = layout([gts[3], gts[0]], 10, 20)                  # the first input need not be the top left one
    assert (ch, cw) == (3344, 3354) and place.tolist() == [[3334, 0], [0, 3334]] and gt == (x0, d, 0.0, y0, 0.0, -d)
    assert layout([gts[1], (x0 + 1e-7 * d, d, 0.0, y0, 0.0, -d)], 5, 5)[2].tolist() == [[0, 0], [0, 0]]      # within 1e-6 pixel
    with pytest.raises(ValueError, match='input 2 .*rotated'):
        layout([gts[0], (x0, d, 0.5, y0, 0.0, -d)], 10, 10)
    with pytest.raises(ValueError, match='input 1 .*rotated'):
        layout([(x0, d, 0.0, y0, 0.1, -d)], 10, 10)
    with pytest.raises(ValueError, match='input 3 pixel size'):
        layout([gts[0], gts[1], (x0, 10.0, 0.0, y0, 0.0, -10.0)], 10, 10)
    with pytest.raises(ValueError, match='input 2 pixel size'):
        layout([gts[0], (x0, d, 0.0, y0, 0.0, d)], 10, 10)
    with pytest.raises(ValueError, match='input 2 origin .*lattice'):
        layout([gts[0], (x0 + 15.0, d, 0.0, y0, 0.0, -d)], 10, 10)
    with pytest.raises(ValueError, match='input 2 origin .*lattice'):
        layout([gts[0], (x0, d, 0.0, y0 - 1e-4, 0.0, -d)], 10, 10)
    with pytest.raises(ValueError, match='beyond the limits .*input 2'):
        layout([gts[1], (x0 + d * (MAX_SIDE + 5), d, 0.0, y0, 0.0, -d)], 10, 10)
    with pytest.raises(ValueError, match='beyond the limits'):
        layout([gts[1], (x0 + d * (1 << 20), d, 0.0, y0 - d * (1 << 20), 0.0, -d)], 10, 10)
    with pytest.raises(ValueError):
        layout([], 10, 10)


def test_wtr_spec_and_one_seam_pixel_by_hand():
    s = wtr_mosaic_spec(outside=254)
    assert (s.n_cats, s.fill, s.outside) == (2, 255, 254) and s.cat_of_byte.tolist() == wtr_spec().cat_of_byte.tolist()
    # two 1 x 3 tiles overlapping in one pixel: water | cloud over not-water | water
    tiles = np.array([[[1, 1, 253]], [[0, 1, 1]]], dtype=np.uint8)
    got = mosaic_tiles(tiles, [(0, 0), (0, 2)], (1, 6), s)
    assert got['last'].tolist() == [[1, 1, 0, 1, 1, 254]] and got['last_index'].tolist() == [[0, 0, 1, 1, 1, 65535]]
    assert got['count'][0].tolist() == [[1, 1, 0, 1, 1, 0]] and got['count'][1].tolist() == [[0, 0, 1, 0, 0, 0]]
    assert got['share'].tolist() == [[100, 100, 0, 100, 100, 255]]
    same(_capi.mosaic_host(tiles, [(0, 0), (0, 2)], (1, 6), s), got, 'by hand')


def test_header_says_has_mosaic_and_the_struct_mirror_matches(tmp_path):
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_MOSAIC 1' in text and '#define DSWX_ABI_VERSION 7' in text and _capi.HAS_MOSAIC == 1
    assert text.index('---- burn:') < text.index('---- mosaic:') < text.index('---- device plumbing')
    for name in ('dswx_mosaic_device', 'dswx_batch_mosaic', 'dswx_mosaic_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    assert ctypes.sizeof(_capi.MosaicSpec) == 272
    s = _capi.MosaicSpec.of(Spec(3, np.arange(256) % 7, 9, 11))
    assert (s.n_cats, s.fill, s.outside, s.reserved) == (3, 9, 11, 0) and list(s.cat_of_byte) == [b % 7 for b in range(256)]
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for n, _ in _capi.MosaicSpec._fields_:
        lines.append(f'  printf("{n} %zu\\n", offsetof(dswx_mosaic_spec_t, {n}));')
    lines += ['  printf("sizeof %zu\\n", sizeof(dswx_mosaic_spec_t));', '  return 0;', '}']
    src = tmp_path / 'off.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'off'
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got['sizeof']) == 272
    for n, _ in _capi.MosaicSpec._fields_:
        assert int(got[n]) == getattr(_capi.MosaicSpec, n).offset, n
