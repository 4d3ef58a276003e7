"""The burn entries on the host (include/dswx_hip.h "burn"): dswx_burn_host and proteus_amd.burn.burn_tiles pinned to each other
byte for byte (acc, mask, head), to a per-pixel crossing predicate in Python ints, to matplotlib.path on pixel centres, and to
the outline entries by the round trip id plane -> rings -> id plane.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.burn import HEAD_WORDS, MAX_COORD, VERTEX_DTYPE, Spec, burn_tiles, quantise, records, records_of_outline, tiles
from tests import _burn_cases as K
from tests import _outline_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('acc', 'mask', 'head')
SENT8 = 0xA5


def both(c, spec=None, src=None):
    """The host entry's outputs, after they were found equal to the numpy statement's in every byte."""
    spec = spec or Spec(burn=200, background=3)
    got, want = K.host(c, spec, src=src), K.numpy_statement(c, spec, src)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (c['name'], k)
    return got


def tile_records(c, t):
    return c['verts'][c['first'][t]:c['first'][t + 1]]


def test_three_statements_agree_on_random_polygons():
    """Polygons of 3 .. 6 vertices from -3 to +14 pixels in tiles up to 12 x 12: clipped on all four sides; every other tile has
    all coordinates on multiples of 128, so that centres lie ON vertices and edges."""
    tiles_seen = ties = 0
    for c in K.random_cases():
        got = both(c)
        for t in range(len(c['first']) - 1):
            assert np.array_equal(got['acc'][t], K.brute(tile_records(c, t), c['H'], c['W'])), (c['name'], t)
            tiles_seen += 1
            ties += bool((tile_records(c, t)['x'] % 128 == 0).all())
        assert (got['mask'] == np.where(got['acc'] != 0, 200, 3)).all()
    assert tiles_seen == 64 and ties >= 32
    assert sum(int(K.host(c)['head'][:, 4].sum() > 0) + int(K.host(c)['head'][:, 5].sum() > 0) for c in K.random_cases()) == 8   # both sides


@pytest.mark.parametrize('H,W', OC.SHAPES)
def test_round_trip_through_the_outline_gives_the_id_plane_back(H, W):
    """Every pattern labelled with either connectivity, and the two garbage planes: dswx_outline_host -> records_of_outline ->
    burn gives acc == the id plane exactly, mask == burn exactly where the id is non-zero, head word 6 the non-zero pixels.
    Every vertical boundary edge is one crossing: applied (word 3), or dropped (word 4) when it lies on the right border of the
    tile, where the first pixel at or right of it is column `width`; none is clamped."""
    rng = np.random.default_rng(100 * H + W)
    names, _, planes = OC.id_planes(H, W, rng)
    for conn in (4, 8):
        ids = planes[conn]
        verts, first, vertical, border = K.outline_records(ids, conn)
        c = {'name': f'round_trip_{conn}', 'H': H, 'W': W, 'verts': verts, 'first': first}
        got = both(c, Spec(burn=77, background=5))
        assert np.array_equal(got['acc'], ids), [names[t] for t in range(len(ids)) if not np.array_equal(got['acc'][t], ids[t])]
        assert np.array_equal(got['mask'], np.where(ids != 0, 77, 5))
        assert np.array_equal(got['head'][:, 6], (ids != 0).sum(axis=(1, 2)))
        assert np.array_equal(got['head'][:, 3] + got['head'][:, 4], vertical) and np.array_equal(got['head'][:, 4], border)
        assert not got['head'][:, 1].any() and not got['head'][:, 5].any() and not got['head'][:, 7].any()


def test_even_odd_rule_of_matplotlib_on_pixel_centres():
    """Polygons whose coordinates are all odd: no centre (a multiple of 128) lies on an edge, so inside is inside."""
    mpath = pytest.importorskip('matplotlib.path')
    rng = np.random.default_rng(4)
    H, W = 12, 12
    ys, xs = np.mgrid[0:H, 0:W]
    centres = np.stack([256.0 * xs.ravel() + 128, 256.0 * ys.ravel() + 128], axis=1)
    for trial in range(40):
        k = int(rng.integers(3, 7))
        p = rng.integers(-3 * 256, 14 * 256, size=(k, 2)) | 1
        got = both(K.case('odd', H, W, [records([p], [1])]))
        # (Path.contains_points counts crossings of a ray: even-odd, self-intersecting rings included)
        inside = mpath.Path(np.concatenate([p, p[:1]]).astype(np.float64), closed=True).contains_points(centres).reshape(H, W)
        assert np.array_equal(got['acc'][0] != 0, inside), (trial, p.tolist())


def test_named_corner_cases():
    names, c = K.corner_cases()
    H, W = c['H'], c['W']
    got = both(c)
    acc, head = got['acc'], got['head']
    for t, name in enumerate(names):                         # the extreme coordinates among them: the overflow bound
        assert np.array_equal(acc[t], K.brute(tile_records(c, t), H, W)), name
    at = {n: t for t, n in enumerate(names)}
    want = np.zeros((H, W), dtype=np.uint32)
    want[1:4, 1:5] = 3                                       # y from 1.5 to 4.5: the centre of row 1 lies ON the top edge and is in
    assert np.array_equal(acc[at['ends_on_centre']], want)   # (y0 <= yc), that of row 4 ON the bottom edge and is out (yc < y1)
    for name in ('left_of_tile', 'right_of_tile', 'above_tile', 'below_tile', 'zero_area', 'empty_a', 'empty_b', 'next_is_self', 'zero_word'):
        assert not acc[at[name]].any(), name
    assert head[at['left_of_tile']].tolist() == [4, 0, 2, 12, 0, 12, 0, 0]          # every crossing clamped to column 0: they cancel
    assert head[at['right_of_tile']].tolist() == [4, 0, 2, 0, 12, 0, 0, 0]          # every crossing dropped
    assert head[at['above_tile']].tolist() == head[at['below_tile']].tolist() == [4, 0, 0, 0, 0, 0, 0, 0]
    for name in ('covers_tile', 'exactly_tile', 'extreme_square'):
        assert (acc[at[name]] == tile_records(c, at[name])['word'][0]).all(), name
    assert head[at['exactly_tile']].tolist() == [4, 0, 2, H, H, 0, H * W, 0]
    assert head[at['zero_area']].tolist()[:3] == [2, 0, 2] and head[at['next_is_self']].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert head[at['next_out_of_range']][1] == 1 and head[at['illegal_coordinate']][1] == 4
    assert np.array_equal(acc[at['illegal_coordinate']] != 0, acc[at['zero_word']] != acc[at['illegal_coordinate']])
    a, b = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    a[2:5, 2:6], b[3:8, 4:9] = True, True
    assert np.array_equal(acc[at['cancel_one_word']], np.where(a ^ b, 6, 0))         # one word: the overlap cancels
    assert np.array_equal(acc[at['union_two_bits']], a * 1 + b * 2) and np.array_equal(acc[at['union_two_bits']] != 0, a | b)
    assert head[at['zero_word']].tolist() == [4, 0, 2, 6, 0, 0, 0, 0]               # toggles of a zero word are toggles
    assert (head[:, 7] == 0).all() and (head[:, 0] == np.diff(c['first'])).all()


def test_src_in_place_and_tile_strides():
    rng = np.random.default_rng(11)
    c = K.random_cases(seed=3, per_shape=5)[1]               # 5 x 9
    n, H, W = 5, c['H'], c['W']
    src = rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    got = both(c, Spec(burn=9, background=1), src=src)
    assert np.array_equal(got['mask'], np.where(got['acc'] != 0, 9, src)) and (got['acc'] != 0).any() and (got['acc'] == 0).any()
    # in place: src IS the mask
    m = src.copy()
    res = _capi.burn_host(c['verts'], c['first'], H, W, Spec(burn=9), src=m, mask=m)
    assert res['mask'] is m and np.array_equal(m, got['mask'])
    # two calls in place OR together: the second tile's rings burnt over the first's result
    d = dict(c, verts=c['verts'][c['first'][1]:c['first'][2]], first=np.array([0, c['first'][2] - c['first'][1]]))
    one = src[:1].copy()
    _capi.burn_host(tile_records(c, 0), np.array([0, c['first'][1]]), H, W, Spec(burn=9), src=one, mask=one)
    _capi.burn_host(d['verts'], d['first'], H, W, Spec(burn=9), src=one, mask=one)
    assert np.array_equal(one[0], np.where((got['acc'][0] != 0) | (got['acc'][1] != 0), 9, src[0]))
    # strides above height * width, different for mask and src: the bytes between the rasters stay as they are
    ms, ss = H * W + 7, H * W + 3
    wide_src = rng.integers(0, 256, size=(n, ss), dtype=np.uint8)
    wide = np.full((n, ms), SENT8, dtype=np.uint8)
    res = _capi.burn_host(c['verts'], c['first'], H, W, Spec(9, 1, ms, ss), src=wide_src, mask=wide)
    want = burn_tiles(c['verts'], c['first'], H, W, Spec(9, 1, ms, ss), src=wide_src)
    assert np.array_equal(wide[:, :H * W].reshape(n, H, W), want['mask']) and (wide[:, H * W:] == SENT8).all()
    assert np.array_equal(want['mask'], np.where(got['acc'] != 0, 9, wide_src[:, :H * W].reshape(n, H, W)))
    for k in ('acc', 'head'):
        assert np.array_equal(res[k], got[k])
    # in place with a stride
    wide2 = np.full((n, ms), SENT8, dtype=np.uint8)
    wide2[:, :H * W] = src.reshape(n, -1)
    _capi.burn_host(c['verts'], c['first'], H, W, Spec(9, 1, ms, ms), src=wide2, mask=wide2)
    assert np.array_equal(wide2[:, :H * W].reshape(n, H, W), got['mask']) and (wide2[:, H * W:] == SENT8).all()
    # every subset of the outputs; acc always
    for keys in (('acc',), ('head',), ('mask',), ('mask', 'head')):
        res = _capi.burn_host(c['verts'], c['first'], H, W, Spec(9, 1), want=keys)
        assert set(res) == set(keys) | {'acc'}
        for k in res:
            assert np.array_equal(res[k], np.where(got['acc'] != 0, 9, 1) if k == 'mask' else got[k]), (keys, k)


def run_host_at(c, spec, off, src=None):
    """dswx_burn_host with every buffer `off` bytes behind an 8-byte boundary."""
    lib = _capi.load_library()
    n, H, W = len(c['first']) - 1, c['H'], c['W']

    def shifted(arr):
        raw = np.zeros(arr.nbytes + 24, dtype=np.uint8)
        at = (-raw.ctypes.data) % 8 + off
        raw[at:at + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8).ravel()
        return raw, raw.ctypes.data + at, at
    keep = [shifted(c['verts'] if len(c['verts']) else np.zeros(1, dtype=VERTEX_DTYPE)), shifted(c['first'])]
    outs = {k: shifted(np.zeros(s, dtype=_capi.BURN_DTYPES[k])) for k, s in (('acc', (n, H, W)), ('mask', (n, H, W)), ('head', (n, HEAD_WORDS)))}
    s = shifted(src) if src is not None else None
    out = _capi.BurnOut.of(**{k: v[1] for k, v in outs.items()})
    rc = lib.dswx_burn_host(ctypes.c_void_p(keep[0][1]), ctypes.c_void_p(keep[1][1]), ctypes.byref(_capi.BurnSpec.of(spec)), n, H, W,
                            ctypes.c_void_p(s[1]) if s else None, ctypes.byref(out))
    res = {}
    for k, shape in (('acc', (n, H, W)), ('mask', (n, H, W)), ('head', (n, HEAD_WORDS))):
        raw, _, at = outs[k]
        nbytes = int(np.prod(shape)) * np.dtype(_capi.BURN_DTYPES[k]).itemsize
        res[k] = raw[at:at + nbytes].copy().view(_capi.BURN_DTYPES[k]).reshape(shape)
    return rc, res


def test_odd_addresses_empty_tiles_and_tables_that_decrease():
    names, c = K.corner_cases()
    want = both(c)
    src = np.random.default_rng(2).integers(0, 256, size=want['mask'].shape, dtype=np.uint8)
    for off in (1, 2, 3, 5):
        rc, got = run_host_at(c, Spec(200, 3), off, src=src if off & 1 else None)
        assert rc == 0, _capi.load_library().dswx_last_error()
        assert np.array_equal(got['acc'], want['acc']) and np.array_equal(got['head'], want['head'])
        assert np.array_equal(got['mask'], np.where(want['acc'] != 0, 200, src if off & 1 else 3))
    # empty tiles between full ones are part of the corner cases; no tiles, no rows and no columns:
    for n, H, W in ((0, 5, 7), (2, 0, 5), (2, 5, 0)):
        e = {'name': 'empty', 'H': H, 'W': W, 'verts': c['verts'][:8], 'first': np.array([0, 4, 8][:n + 1])}
        got = both(e)
        assert got['acc'].shape == (n, H, W) and got['head'][:, 0].tolist() == [4] * n and not got['head'][:, 3].any()
    # a table that decreases, or begins below zero: the affected tiles have no records
    sq = K.ring([(2, 2), (6, 2), (6, 5), (2, 5)], 13)
    verts = np.concatenate([sq, sq, sq])
    d = {'name': 'decreasing', 'H': 9, 'W': 11, 'verts': verts, 'first': np.array([0, 8, 4, 8, 8, 12, -4, 4, 4])}
    got = both(d)
    assert got['head'][:, 0].tolist() == [8, 0, 4, 0, 4, 0, 0, 0]
    assert not got['acc'][0].any() and (got['acc'][2] != 0).sum() == 12 and not got['acc'][6].any()    # (tile 0: the square twice)


def test_quantise_records_and_tiles():
    assert quantise([[0.5, 1.0], [-3.3, 2.001953125]]).tolist() == [[128, 256], [-845, 512]] and quantise([]).dtype == np.int32
    assert quantise([float(1 << 22)]).tolist() == [MAX_COORD]
    for bad in ([float(1 << 22) + 0.01], [-float(1 << 22) - 1], [np.nan], [np.inf]):
        with pytest.raises(ValueError):
            quantise(bad)
    r = records([np.array([[0, 0], [256, 0], [0, 256]]), np.array([[1, 2], [3, 4], [5, 6], [7, 8]])], [5, 0xFFFFFFFF])
    assert r.dtype == VERTEX_DTYPE and r['next'].tolist() == [1, 2, 0, 4, 5, 6, 3] and r['word'].tolist() == [5] * 3 + [0xFFFFFFFF] * 4
    assert records([np.array([[0, 0], [256, 0]])])['word'].tolist() == [1, 1] and len(records([])) == 0
    v, f = tiles([r, r[:0], r[:3]])
    assert f.tolist() == [0, 7, 7, 10] and f.dtype == np.int64 and len(v) == 10
    for bad in (lambda: records([np.zeros((3, 2))]), lambda: records([np.zeros((3, 3), dtype=np.int32)]),
                lambda: records([np.array([[MAX_COORD + 1, 0]])]), lambda: records([np.zeros((3, 2), dtype=np.int32)], [1, 2]),
                lambda: Spec(burn=256), lambda: Spec(background=-1), lambda: Spec(mask_tile_stride=-1),
                lambda: _capi.burn_host(r.view(np.uint32), f, 4, 4, Spec()), lambda: _capi.burn_host(r, f, 4, 4, Spec(), want=('area',)),
                lambda: _capi.burn_host(r, f, 4, 4, Spec(), src=np.zeros(5, dtype=np.uint8)),
                lambda: _capi.burn_host(r, f, 4, 4, Spec(), mask=np.zeros(5, dtype=np.uint8))):
        with pytest.raises(ValueError):
            bad()
    # records_of_outline: the four-pixel lake and the speck of tests/test_outline.py come back as their ids
    ids = np.array([[[1, 1, 0, 4], [1, 1, 0, 0], [0, 0, 0, 0]]], dtype=np.uint32)
    o = OC.host(ids, OC.full_spec(ids, 4))
    rec = records_of_outline(o['chain'][0], o['rings'][0], 4)
    assert rec['x'].tolist() == [0, 512, 512, 0, 768, 1024, 1024, 768] and rec['word'].tolist() == [1] * 4 + [4] * 4
    assert np.array_equal(burn_tiles(rec, [0, 8], 3, 4, Spec())['acc'], ids)


def test_refusals_with_the_outputs_untouched():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    H, W, n = 4, 6, 3
    sq = K.ring([(1, 1), (4, 1), (4, 3), (1, 3)], 5)
    verts, first = tiles([sq] * n)
    vbuf = np.zeros(verts.nbytes + 16, dtype=np.uint8)
    vat = vbuf.ctypes.data + (-vbuf.ctypes.data) % 16
    ctypes.memmove(vat, verts.ctypes.data, verts.nbytes)
    count = {'acc': n * H * W * 4, 'mask': n * H * W, 'head': n * HEAD_WORDS * 8}
    planes = {k: np.full(count[k] + 16, SENT8, dtype=np.uint8) for k in KEYS}
    at = {k: planes[k].ctypes.data + (-planes[k].ctypes.data) % 8 for k in KEYS}
    src = np.zeros(n * H * W, dtype=np.uint8)

    def outs(**kw):
        o = _capi.BurnOut.of(**at)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def spec_c(**kw):
        s = _capi.BurnSpec.of(Spec(9, 1))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def host(verts=vat, first=first.ctypes.data, spec=None, n_tiles=n, height=H, width=W, src=None, out=None, null_spec=False, null_out=False):
        return lib.dswx_burn_host(vp(verts), vp(first), None if null_spec else ctypes.byref(spec or spec_c()), n_tiles, height, width,
                                  vp(src), None if null_out else ctypes.byref(out or outs()))

    def dev(verts=0x10000, first=0x20000, spec=None, n_tiles=n, height=H, width=W, src=None, out=None, null_spec=False, null_out=False, ctx=None):
        # host addresses, never dereferenced: every call fails first
        return lib.dswx_burn_device(ctx, vp(verts), vp(first), None if null_spec else ctypes.byref(spec or spec_c()), n_tiles, height, width,
                                    vp(src), None if null_out else ctypes.byref(out or outs()), None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        refused(call(null_spec=True), _capi.ERR_ARG, b'spec is NULL')
        refused(call(null_out=True), _capi.ERR_ARG, b'out is NULL')
        for v in (-1, 256, 1 << 20):
            refused(call(spec=spec_c(burn=v)), _capi.ERR_ARG, b'burn')
            refused(call(spec=spec_c(background=v)), _capi.ERR_ARG, b'background')
        for kw in ({'n_tiles': -1}, {'height': -1}, {'width': -1}, {'spec': spec_c(mask_tile_stride=-1)}, {'spec': spec_c(src_tile_stride=-1)}):
            refused(call(**kw), _capi.ERR_ARG, b'negative')
        refused(call(height=1 << 15, width=(1 << 15) + 1, n_tiles=1), _capi.ERR_ARG, b'2^30')
        refused(call(height=(1 << 30) + 1, width=1, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(height=1 << 40, width=1 << 40, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(spec=spec_c(mask_tile_stride=H * W - 1)), _capi.ERR_ARG, b'mask_tile_stride')
        refused(call(spec=spec_c(src_tile_stride=1)), _capi.ERR_ARG, b'src_tile_stride')
        refused(call(n_tiles=(1 << 32) + 1, height=0), _capi.ERR_ARG, b'2^32 tiles')
        refused(call(verts=None), _capi.ERR_ARG, b'verts is NULL')
        refused(call(first=None), _capi.ERR_ARG, b'tile_first is NULL')
        refused(call(out=outs(acc=None)), _capi.ERR_ARG, b'acc is NULL')
        refused(call(src=src.ctypes.data, out=outs(mask=None)), _capi.ERR_ARG, b'src without mask')
    # the device entry: alignment; then, with everything in order, the context -- checked last
    for off in (1, 2, 4, 8, 15):
        refused(dev(verts=0x10000 + off), _capi.ERR_ALIGN, b'verts')
    for off in (1, 2, 3):
        refused(dev(out=outs(acc=at['acc'] + off)), _capi.ERR_ALIGN, b'acc')
    for off in (1, 2, 4, 7):
        refused(dev(first=0x20000 + off), _capi.ERR_ALIGN, b'tile_first')
        refused(dev(out=outs(head=at['head'] + off)), _capi.ERR_ALIGN, b'head')
    refused(dev(), _capi.ERR_ARG, b'ctx')
    refused(dev(out=outs(acc=at['acc'] + 4, mask=at['mask'] + 3), src=src.ctypes.data + 1), _capi.ERR_ARG, b'ctx')   # mask and src: any address
    refused(dev(out=outs(mask=None, head=None)), _capi.ERR_ARG, b'ctx')                  # acc alone
    refused(dev(height=1 << 15, width=1 << 15, n_tiles=1), _capi.ERR_ARG, b'ctx')        # 2^30 pixels are legal
    refused(dev(verts=None, first=None, n_tiles=0, out=outs(acc=None)), _capi.ERR_ARG, b'ctx')     # nothing to read or write
    refused(dev(out=outs(acc=None), width=0), _capi.ERR_ARG, b'ctx')                     # an empty raster needs no acc
    refused(lib.dswx_batch_burn(None, 9, vp(0x10000), vp(0x20000), ctypes.byref(spec_c()), vp(at['acc']), vp(at['head']), 0, 1, None),
            _capi.ERR_ARG, b'batch is NULL')
    for k in KEYS:                                                                       # a refused call wrote nothing
        assert np.all(planes[k] == SENT8), k
    assert host(verts=None, first=None, n_tiles=0) == 0                                  # no tiles: legal, writes nothing
    for k in KEYS:
        assert np.all(planes[k] == SENT8), k
    # and the same arguments, accepted
    assert host() == 0
    off = {k: at[k] - planes[k].ctypes.data for k in KEYS}
    mask = planes['mask'][off['mask']:][:count['mask']].reshape(n, H, W)
    want = np.ones((H, W), dtype=np.uint8)
    want[1:3, 1:4] = 9
    assert (mask == want).all()
    assert planes['head'][off['head']:][:count['head']].view(np.uint64).reshape(n, -1).tolist() == [[4, 0, 2, 4, 0, 0, 6, 0]] * n
    for k in KEYS:
        assert (planes[k][:off[k]] == SENT8).all() and (planes[k][off[k] + count[k]:] == SENT8).all(), k


def test_header_says_has_burn_and_abi_7():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_BURN 1' in text and '#define DSWX_BURN_HEAD_WORDS 8' in text and '#define DSWX_BURN_MAX_COORD (1 << 30)' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert (_capi.HAS_BURN, _capi.BURN_HEAD_WORDS, HEAD_WORDS, _capi.BURN_MAX_COORD, MAX_COORD) == (1, 8, 8, 1 << 30, 1 << 30)
    assert text.index('---- outline:') < text.index('---- burn:') < text.index('---- device plumbing')
    for name in ('dswx_burn_device', 'dswx_batch_burn', 'dswx_burn_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    section = ' '.join(text[text.index('---- burn:'):text.index('---- device plumbing')].replace(' * ', ' ').split())
    assert 'deterministic and independent of the launch geometry' in section and 'order in which atomics' in section
    assert 'ANY CONTENT OF A RECORD IS LEGAL' in section and 'NOT CHECKED' in section and 'No workgroup ever waits for another' in section
    assert 'THE FIRST dswx_batch_* ENTRY THAT WRITES A PLANE OF THE BATCH' in section and 'UNPINNED' in section and 'STILL REFUSED' in section
    assert 'read ON THE DEVICE ONLY' in section and 'a decreasing table' in section and 'a second call on the same outputs gives the same bytes' in section
    rule = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_burn_rule.h')).read()
    assert f'#define DSWX_BURN_THREAD_ROWS {_capi.BURN_THREAD_ROWS}\n' in rule and f'#define DSWX_BURN_SCAN_STEP {_capi.BURN_SCAN_STEP}\n' in rule


def test_struct_mirrors_match_offsetof_as_gcc_sees_the_header(tmp_path):
    assert ctypes.sizeof(_capi.BurnSpec) == 24 and ctypes.sizeof(_capi.BurnOut) == 24 and VERTEX_DTYPE.itemsize == 16
    assert [VERTEX_DTYPE.fields[k][1] for k in VERTEX_DTYPE.names] == [0, 4, 8, 12]
    mirrors = {'dswx_burn_spec_t': _capi.BurnSpec, 'dswx_burn_out_t': _capi.BurnOut}
    assert all(_capi.ANALYTIC_STRUCTS[k] is v for k, v in mirrors.items())
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for st, cls in mirrors.items():
        for n, _ in cls._fields_:
            lines.append(f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));')
        lines.append(f'  printf("{st}.sizeof %zu\\n", sizeof({st}));')
    for n in VERTEX_DTYPE.names:
        lines.append(f'  printf("vertex.{n} %zu\\n", offsetof(dswx_burn_vertex_t, {n}));')
    lines += ['  printf("vertex.sizeof %zu\\n", sizeof(dswx_burn_vertex_t));', '  return 0;', '}']
    src = tmp_path / 'off.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'off'
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in mirrors.items():
        assert int(got[f'{st}.sizeof']) == ctypes.sizeof(cls), st
        for n, _ in cls._fields_:
            assert int(got[f'{st}.{n}']) == getattr(cls, n).offset, (st, n)
    assert int(got['vertex.sizeof']) == 16 and [int(got[f'vertex.{n}']) for n in VERTEX_DTYPE.names] == [0, 4, 8, 12]
    o = _capi.BurnOut.of(acc=16, head=64)
    assert (o.acc, o.mask, o.head) == (16, None, 64)
    s = _capi.BurnSpec.of(Spec(40, 9, 800, 900))
    assert (s.burn, s.background, s.mask_tile_stride, s.src_tile_stride) == (40, 9, 800, 900)


def test_host_entry_and_rule_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/burn_host_san.cpp with proteus_amd/csrc/dswx_burn.hip compiled into it, host code under ASan + UBSan: odd
    addresses, heap blocks of exactly the bytes the entry may touch, coordinates up to and past +-2^30 (a signed overflow in
    the crossing would be a finding), every pixel against a 128-bit crossing predicate.  A child process; nothing is loaded
    into this interpreter."""
    import json
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'burn_host_san')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'proteus_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'native', 'burn_host_san.cpp'), os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_burn.hip'), '-o', exe]
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


def test_burn_example_compiles_against_the_header_and_leaves_quietly_without_a_device(tmp_path):
    """examples/batch_burn.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device the
    program says so and exits 0."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_burn')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_burn.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and 'no device' in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_burn_tool_round_trips_with_the_outline_tool_on_the_host_statement():
    """bin/dswx_burn.py's geometry without a device: GeoJSON rings in map coordinates through the inverse geotransform to
    pixel coordinates, polygons and holes to records with one bit per polygon."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('dswx_burn_tool', os.path.join(ROOT, 'bin', 'dswx_burn.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    gt = (500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0)
    feats = {'type': 'FeatureCollection', 'features': [
        {'type': 'Feature', 'properties': {}, 'geometry': {'type': 'Polygon', 'coordinates': [
            [[500030.0, 4099970.0], [500150.0, 4099970.0], [500150.0, 4099880.0], [500030.0, 4099880.0], [500030.0, 4099970.0]],
            [[500060.0, 4099940.0], [500060.0, 4099910.0], [500090.0, 4099910.0], [500090.0, 4099940.0], [500060.0, 4099940.0]]]}},
        {'type': 'Feature', 'properties': {}, 'geometry': {'type': 'MultiPolygon', 'coordinates': [
            [[[500120.0, 4099910.0], [500210.0, 4099910.0], [500210.0, 4099850.0], [500120.0, 4099850.0], [500120.0, 4099910.0]]]]}}]}
    polys = tool.polygons_of(feats)
    assert [len(p) for p in polys] == [2, 1]
    verts = tool.records_of(polys, gt)
    assert sorted(set(verts['word'].tolist())) == [1, 2] and len(verts) == 12
    got = _capi.burn_host(verts, np.array([0, len(verts)]), 6, 8, Spec())
    want = np.zeros((6, 8), dtype=np.uint32)
    want[1:4, 1:5] = 1
    want[2, 2] = 0
    want[3:5, 4:7] |= 2
    assert np.array_equal(got['acc'][0], want)
