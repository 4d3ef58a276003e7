"""The outline of include/dswx_hip.h ("outline") without a GPU: the library's scalar walk (dswx_outline_host) and the numpy
statement (proteus_amd/outline.py) byte for byte on every case of tests/_outline_cases.py, and both pinned to statements that
share nothing with them -- the body table's areas and perimeters, scipy.ndimage.label for the outer rings and for the holes
(the enclosed components of a body's complement under the complementary structure), matplotlib's even-odd rule over a body's
rings against the body's mask; the successor map a bijection on arbitrary uint32 planes; capacities; the header; the struct
mirrors; refusals, with the outputs untouched; polygons(); the host entry under ASan + UBSan in a stand-alone program; the C
example."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.bodies import Spec as BodySpec, body_table, wtr_body_spec
from proteus_amd.outline import HEAD_WORDS, ROW_DTYPE, ROW_WORDS, Spec, edge_area2, outline_tiles, polygons, ring_points, successors
from tests import _body_cases as B
from tests import _label_cases as C
from tests import _outline_cases as OC

try:
    from scipy import ndimage
except ImportError:                                # (only the comparisons with scipy are skipped then)
    ndimage = None
try:
    from matplotlib.path import Path
except ImportError:                                # (only the even-odd comparison is skipped then)
    Path = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT8 = 0xEE
KEYS = ('chain', 'rings', 'head')
EB = {'chain': 4, 'rings': 4, 'head': 8}
CROSS, SQUARE = None, np.ones((3, 3))             # scipy's structures of connectivity 4 and 8


def records(rings):
    """uint32 [n, max_rings, 8] -> ROW_DTYPE [n, max_rings]."""
    return rings.view(ROW_DTYPE)[..., 0]


def two_statements(ids, spec, what):
    """Host entry == numpy statement, every byte; returns the host entry's outputs with the rings as records."""
    host = _capi.outline_host(ids, spec)
    stated = outline_tiles(ids, spec)
    assert np.array_equal(host['head'], stated['head']), (what, host['head'], stated['head'])
    assert np.array_equal(host['chain'], stated['chain']), what
    rings = records(host['rings']) if 'rings' in host else np.zeros((len(ids), 0), dtype=ROW_DTYPE)
    assert np.array_equal(rings, stated['rings']), what
    return {'chain': host['chain'], 'rings': rings, 'head': host['head']}


def enclosed_components(mask, connectivity):
    """The components of the complement of a boolean raster that do not reach the border of the raster padded by one pixel,
    under the structure complementary to `connectivity`: the holes of the body."""
    free = np.pad(~mask, 1, constant_values=True)
    lab, k = ndimage.label(free, structure=SQUARE if connectivity == 4 else CROSS)
    return k - 1                                       # (the padding joins everything that reaches the border into one)


@pytest.mark.parametrize('H,W', OC.SHAPES)
def test_host_entry_and_numpy_statement_agree_and_are_pinned_to_other_statements(H, W):
    """Every pattern at this shape labelled with 4 and with 8 and outlined with both connectivities, and two planes of
    arbitrary uint32.  Where the ids are a label plane outlined with its own connectivity: per id the area2 of its rings sum to
    twice its area and E is the sum of the perimeters of proteus_amd.bodies.body_table; the rings of positive area are the K
    of scipy.ndimage.label, one per body, started at 4 * (label - 1); the holes of a body are the enclosed components of its
    complement; the even-odd rule over its rings gives back its pixels."""
    rng = np.random.default_rng(9000 + 131 * H + W)
    names, members, planes = OC.id_planes(H, W, rng)
    centres = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), axis=-1).reshape(-1, 2)
    for label_conn in (4, 8):
        ids = planes[label_conn]
        for conn in (4, 8):
            got = two_statements(ids, OC.full_spec(ids, conn), (H, W, label_conn, conn))
            head, rings = got['head'], got['rings']
            assert np.array_equal(head[:, 0], OC.edges_of(ids)) and np.all(head[:, 7] == 0) and np.array_equal(head[:, 3], head[:, 0])
            table = body_table(ids[:len(members)], None, BodySpec(0, None, H * W))
            for t in range(len(ids)):
                R = int(head[t, 1])
                r = rings[t, :R]
                assert np.all(rings[t, R:].view(np.uint32) == 0) and head[t, 2] == R
                assert r['length'].sum() == head[t, 0] and np.array_equal(r['offset'], np.cumsum(r['length']) - r['length'])
                assert np.all(np.diff(r['start'].astype(np.int64)) > 0) and np.all(r['area2'] != 0) and np.all(r['corners'] >= 4)
                assert head[t, 4] == np.count_nonzero(r['area2'] > 0) and head[t, 5] == np.count_nonzero(r['area2'] < 0) and head[t, 6] == r['corners'].sum()
                flat = ids[t].reshape(-1)
                assert np.array_equal(r['id'], flat[r['start'] >> 2]) and np.array_equal(got['chain'][t][r['offset']], r['start'])
                for v in np.unique(r['id']):               # whatever the ids are: the rings of a value enclose its pixels
                    assert r['area2'][r['id'] == v].sum() == 2 * np.count_nonzero(flat == v), (names[t], v)
                if t >= len(members) or label_conn != conn:
                    continue
                assert head[t, 0] == table['head'][t, 4], (names[t], 'the perimeters of the body table')
                if ndimage is None:
                    continue
                lab, K = ndimage.label(members[t], structure=SQUARE if conn == 8 else CROSS)
                outer = r[r['area2'] > 0]
                assert len(outer) == K and np.array_equal(outer['start'], 4 * (np.unique(outer['id']).astype(np.int64) - 1)), names[t]
                for k in range(1, K + 1 if K <= 40 else 1):    # (per body only where there are few: the noise has its own test)
                    mask = lab == k
                    label_id = int(ids[t][mask][0])
                    mine = r[r['id'] == label_id]
                    assert np.count_nonzero(mine['area2'] < 0) == enclosed_components(mask, conn), (names[t], k)
                    if Path is not None:
                        inside = np.zeros(H * W, dtype=bool)
                        for q in mine:
                            pts = ring_points(got['chain'][t][q['offset']:q['offset'] + q['length']], W)
                            assert len(pts) == q['corners']
                            inside ^= Path(pts).contains_points(centres)
                        assert np.array_equal(inside.reshape(H, W), mask), (names[t], k, 'even-odd')


def test_holes_and_even_odd_per_body_on_noise():
    """Noise at 0.5 and 0.62 on 24 x 31, both connectivities: for EVERY body the holes are the enclosed components of its
    complement under the complementary structure, and the even-odd rule over its rings gives back exactly its pixels."""
    if ndimage is None or Path is None:
        pytest.skip('needs scipy and matplotlib')
    rng = np.random.default_rng(9010)
    H, W = 24, 31
    members = np.stack([C.noise(H, W, 0.5, rng), C.noise(H, W, 0.62, rng)])
    centres = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), axis=-1).reshape(-1, 2)
    holes_seen = 0
    for conn in (4, 8):
        ids = B.labels_of(members, rng, conn)
        got = two_statements(ids, OC.full_spec(ids, conn), conn)
        for t in range(2):
            lab, K = ndimage.label(members[t], structure=SQUARE if conn == 8 else CROSS)
            r = got['rings'][t, :int(got['head'][t, 1])]
            assert got['head'][t, 4] == K
            for k in range(1, K + 1):
                mask = lab == k
                mine = r[r['id'] == int(ids[t][mask][0])]
                holes = np.count_nonzero(mine['area2'] < 0)
                assert holes == enclosed_components(mask, conn) and np.count_nonzero(mine['area2'] > 0) == 1
                holes_seen += holes
                inside = np.zeros(H * W, dtype=bool)
                for q in mine:
                    inside ^= Path(ring_points(got['chain'][t][q['offset']:q['offset'] + q['length']], W)).contains_points(centres)
                assert np.array_equal(inside.reshape(H, W), mask), (conn, t, k)
    assert holes_seen > 5


@pytest.mark.parametrize('conn', [4, 8])
def test_the_successor_map_is_a_bijection_on_arbitrary_planes(conn):
    """Random uint32 planes -- few values that meet often, among them 0xFFFFFFFF, and anything at all -- at several shapes:
    every successor is a boundary edge, no edge is the successor of two, the chain of the host entry is a permutation of the
    keys, and following the chain inside a ring IS the successor map."""
    rng = np.random.default_rng(9020 + conn)
    for H, W in ((1, 1), (1, 9), (9, 1), (2, 2), (13, 13), (7, 40)):
        for plane in np.concatenate([OC.garbage(H, W, rng) for _ in range(6)]):
            keys, succ = successors(plane, conn)
            assert np.all(np.isin(succ, keys)) and len(np.unique(succ)) == len(keys), (H, W)
            E = len(keys)
            got = two_statements(plane[None], Spec(E, E // 4 + 1, conn), (H, W))
            chain, r = got['chain'][0], got['rings'][0, :int(got['head'][0, 1])]
            assert np.array_equal(np.sort(chain), keys)
            nxt = dict(zip(keys.tolist(), succ.tolist()))
            for q in r:
                ring = chain[q['offset']:q['offset'] + q['length']].tolist()
                assert ring[0] == min(ring) == q['start'] and all(nxt[a] == b for a, b in zip(ring, ring[1:] + ring[:1]))
    assert 0xFFFFFFFF in OC.GARBAGE_VALUES
    full = np.full((1, 3, 5), 0xFFFFFFFF, dtype=np.uint32)
    got = two_statements(full, Spec(16, 1, conn), 'all 0xFFFFFFFF')
    assert got['rings'][0, 0].tolist() == (0xFFFFFFFF, 0, 0, 16, 4, 0, 30) and got['head'][0].tolist() == [16, 1, 1, 16, 1, 0, 4, 0]


def test_capacities_either_side_of_e_and_r():
    """max_edges E - 1 for the middle tile only: that tile is zero with head word 7 set and its neighbours are unaffected;
    max_rings in {0, 1, R - 1, R, R + 1}: the first rows are those of the full table, the rest zero, the chain complete;
    every subset of the outputs the entry accepts."""
    rng = np.random.default_rng(9030)
    H, W = 20, 33
    ids = B.labels_of(np.stack([C.noise(H, W, 0.3, rng), C.noise(H, W, 0.55, rng), C.noise(H, W, 0.2, rng)]), rng, 8)
    E = OC.edges_of(ids)
    assert E[1] > E[0] and E[1] > E[2]
    full = two_statements(ids, Spec(int(E[1]), int(E[1]) // 4, 8), 'full')
    R = full['head'][:, 1]
    short = two_statements(ids, Spec(int(E[1]) - 1, int(E[1]) // 4, 8), 'E - 1')
    assert short['head'][1].tolist() == [E[1], 0, 0, 0, 0, 0, 0, 1] and not short['chain'][1].any() and not short['rings'][1].view(np.uint32).any()
    for t in (0, 2):
        assert np.array_equal(short['head'][t], full['head'][t]) and np.array_equal(short['chain'][t], full['chain'][t][:-1])
        assert np.array_equal(short['rings'][t], full['rings'][t])
    for max_rings in (0, 1, int(R.min()) - 1, int(R.min()), int(R.max()) + 1):
        got = two_statements(ids, Spec(int(E[1]), max_rings, 8), max_rings)
        assert np.array_equal(got['chain'], full['chain']) and got['head'][:, 2].tolist() == [min(int(r), max_rings) for r in R]
        assert np.array_equal(got['head'][:, [0, 1, 3, 4, 5, 6, 7]], full['head'][:, [0, 1, 3, 4, 5, 6, 7]])
        for t in range(3):
            keep = min(int(R[t]), max_rings)
            assert np.array_equal(got['rings'][t, :keep], full['rings'][t, :keep]) and np.all(got['rings'][t, keep:].view(np.uint32) == 0)
    counted = _capi.outline_host(ids, Spec(0, 0, 8), want=('head',))
    assert list(counted) == ['head'] and counted['head'].tolist() == [[int(e), 0, 0, 0, 0, 0, 0, 1] for e in E]
    assert list(_capi.outline_host(ids, Spec(int(E[1]), 0, 8), want=('chain',))) == ['chain']
    assert np.array_equal(_capi.outline_host(ids, Spec(int(E[1]), 0, 8), want=('head',))['head'][:, [0, 1, 3, 4, 5, 6, 7]], full['head'][:, [0, 1, 3, 4, 5, 6, 7]])


def run_host(ids, spec, off=0, want=KEYS):
    """dswx_outline_host with the id plane and every output `off` bytes past an aligned address and every output byte a
    sentinel beforehand.  Returns (rc, {output: array}); nothing outside the wanted outputs may have changed."""
    lib = _capi.load_library()
    T, H, W = ids.shape
    iraw = np.zeros(4 * ids.size + 64, dtype=np.uint8)
    ibase = (-iraw.ctypes.data) % 16 + off
    iraw[ibase:ibase + 4 * ids.size] = ids.reshape(-1).view(np.uint8)
    count = {'chain': T * spec.max_edges, 'rings': T * spec.max_rings * ROW_WORDS, 'head': T * HEAD_WORDS}
    bufs, out = {}, _capi.OutlineOut()
    for k in KEYS:
        b = np.full(count[k] * EB[k] + 64, SENT8, dtype=np.uint8)
        start = (-b.ctypes.data) % 16 + off
        bufs[k] = (b, start)
        if k in want:
            setattr(out, k, b.ctypes.data + start)
    rc = lib.dswx_outline_host(iraw.ctypes.data + ibase, ctypes.byref(_capi.OutlineSpec.of(spec)), T, H, W, ctypes.byref(out))
    res = {}
    for k, (b, start) in bufs.items():
        used = count[k] * EB[k] if k in want else 0
        assert np.all(b[:start] == SENT8) and np.all(b[start + used:] == SENT8), k
        if k in want:
            res[k] = b[start:start + used].copy().view(_capi.OUTLINE_DTYPES[k]).reshape(_capi._outline_shape(k, T, spec))
    return rc, res


def test_odd_addresses_and_every_subset_of_the_outputs():
    rng = np.random.default_rng(9040)
    cases = 0
    for (T, H, W) in ((0, 5, 7), (1, 1, 1), (3, 17, 33), (2, 32, 16), (2, 0, 5)):
        ids = B.labels_of(rng.random((T, H, W)) < 0.55, rng, (4, 8)[T % 2]) if T and H else np.zeros((T, H, W), dtype=np.uint32)
        E = int(OC.edges_of(ids).max()) if T and H else 0
        for keys in (('head',), ('chain',), ('chain', 'head'), ('chain', 'rings'), KEYS):
            spec = Spec(E + 2, E // 4 + 1 if 'rings' in keys else 0, (8, 4)[cases % 2])
            want = outline_tiles(ids, spec)
            rc, got = run_host(ids, spec, off=(0, 1, 2, 3, 5)[cases % 5], want=keys)
            assert rc == 0, _capi.load_library().dswx_last_error()
            for k in keys:
                assert np.array_equal(records(got[k]) if k == 'rings' else got[k], want[k]), (T, H, W, keys, k)
            cases += 1


def test_refusals_with_the_outputs_untouched():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    good = Spec(100, 25, 8)
    H, W = 4, 6
    ids = np.ones((3, H, W), dtype=np.uint32)
    count = {'chain': 3 * 100, 'rings': 3 * 25 * ROW_WORDS, 'head': 3 * HEAD_WORDS}
    planes = {k: np.full(count[k] * EB[k] + 16, SENT8, dtype=np.uint8) for k in KEYS}
    at = {k: planes[k].ctypes.data + (-planes[k].ctypes.data) % 8 for k in KEYS}
    need = _capi.outline_work_bytes(good, 3, H, W)
    assert need >= 16 and _capi.outline_work_bytes(good, 0, H, W) == 16
    assert _capi.outline_work_bytes(Spec(1 << 31, 0, 4), 3, H, W) == _capi.outline_work_bytes(Spec(4 * H * W, 0, 4), 3, H, W)   # the capacity that counts

    def outs(**kw):
        o = _capi.OutlineOut.of(**at)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def spec_c(**kw):
        s = _capi.OutlineSpec.of(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def host(ids=ids.ctypes.data, spec=None, n_tiles=3, height=H, width=W, out=None, null_spec=False, null_out=False):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out
        return lib.dswx_outline_host(vp(ids), None if null_spec else ctypes.byref(spec), n_tiles, height, width, None if null_out else ctypes.byref(out))

    def dev(ids=0x10000, spec=None, n_tiles=3, height=H, width=W, out=None, null_spec=False, null_out=False, work=0x40000, work_bytes=need, ctx=None):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out                   # host addresses, never dereferenced: every call fails first
        return lib.dswx_outline_device(ctx, vp(ids), None if null_spec else ctypes.byref(spec), n_tiles, height, width,
                                       None if null_out else ctypes.byref(out), vp(work), work_bytes, None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        refused(call(null_spec=True), _capi.ERR_ARG, b'spec is NULL')
        refused(call(null_out=True), _capi.ERR_ARG, b'out is NULL')
        for c in (0, 6, -4, 1 << 20):
            refused(call(spec=spec_c(connectivity=c)), _capi.ERR_ARG, b'connectivity')
        refused(call(spec=spec_c(reserved=1)), _capi.ERR_ARG, b'reserved')
        for kw in ({'n_tiles': -1}, {'height': -1}, {'width': -1}, {'spec': spec_c(max_edges=-1)}, {'spec': spec_c(max_rings=-1)}):
            refused(call(**kw), _capi.ERR_ARG, b'negative')
        refused(call(height=1 << 15, width=(1 << 15) + 1, n_tiles=1), _capi.ERR_ARG, b'2^30')
        refused(call(height=(1 << 30) + 1, width=1, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(height=1 << 40, width=1 << 40, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(spec=spec_c(max_edges=(1 << 31) + 1)), _capi.ERR_ARG, b'max_edges')
        refused(call(spec=spec_c(max_rings=(1 << 31) + 1)), _capi.ERR_ARG, b'max_rings')
        refused(call(ids=None), _capi.ERR_ARG, b'ids is NULL')
        refused(call(out=outs(rings=None)), _capi.ERR_ARG, b'rings is NULL')
        refused(call(out=outs(chain=None)), _capi.ERR_ARG, b'chain is NULL')
    # the device entry: the working memory, alignment; then, with everything in order, the context -- checked last
    refused(dev(work=None), _capi.ERR_ARG, b'work_device is NULL')
    refused(dev(work_bytes=need - 1), _capi.ERR_ARG, b'work_bytes')
    refused(dev(work_bytes=0), _capi.ERR_ARG, b'work_bytes')
    for off in (1, 2, 3):
        refused(dev(ids=0x10000 + off), _capi.ERR_ALIGN, b'ids')
        refused(dev(out=outs(chain=at['chain'] + off)), _capi.ERR_ALIGN, b'chain')
        refused(dev(out=outs(rings=at['rings'] + off)), _capi.ERR_ALIGN, b'rings')
    for off in (1, 2, 4, 7):
        refused(dev(out=outs(head=at['head'] + off)), _capi.ERR_ALIGN, b'head')
        refused(dev(work=0x40000 + off), _capi.ERR_ALIGN, b'work_device')
    refused(dev(), _capi.ERR_ARG, b'ctx')
    refused(dev(out=outs(rings=at['rings'] + 4, chain=at['chain'] + 4)), _capi.ERR_ARG, b'ctx')       # 4 bytes are enough for both
    refused(dev(height=1 << 15, width=1 << 15, n_tiles=1, work_bytes=1 << 40), _capi.ERR_ARG, b'ctx')   # 2^30 pixels are legal
    refused(dev(spec=spec_c(max_edges=1 << 31, max_rings=1 << 31), work_bytes=1 << 40), _capi.ERR_ARG, b'ctx')
    refused(dev(ids=None, n_tiles=0), _capi.ERR_ARG, b'ctx')                             # nothing to read: no ids needed
    refused(dev(out=outs(chain=None, rings=None), spec=spec_c(max_rings=0)), _capi.ERR_ARG, b'ctx')   # the counting call
    refused(dev(out=outs(rings=None, head=None), spec=spec_c(max_rings=0)), _capi.ERR_ARG, b'ctx')    # the chain alone
    for k in KEYS:                                                                       # a refused call wrote nothing
        assert np.all(planes[k] == SENT8), k
    assert host(ids=None, n_tiles=0) == 0                                                # no tiles: legal, writes nothing
    for k in KEYS:
        assert np.all(planes[k] == SENT8), k
    # and the same arguments, accepted: one region per tile
    assert host() == 0
    off = {k: at[k] - planes[k].ctypes.data for k in KEYS}
    rings = planes['rings'][off['rings']:][:4 * count['rings']].view(np.uint32).reshape(3, 25, ROW_WORDS).view(ROW_DTYPE)[..., 0]
    assert rings[:, 0].tolist() == [(1, 0, 0, 2 * (H + W), 4, 0, 2 * H * W)] * 3 and not rings[:, 1:].view(np.uint32).any()
    assert planes['head'][off['head']:][:8 * count['head']].view(np.uint64).reshape(3, -1).tolist() == [[2 * (H + W), 1, 1, 2 * (H + W), 1, 0, 4, 0]] * 3
    assert host(out=outs(chain=at['chain'] + 1, rings=at['rings'] + 3, head=at['head'] + 5)) == 0     # any address
    # the Python side refuses what the library would
    for bad in (lambda: Spec(10, 1, 6), lambda: Spec(-1, 1, 4), lambda: Spec(1, -1, 4), lambda: Spec((1 << 31) + 1, 1, 4),
                lambda: outline_tiles(ids.astype(np.int32), good), lambda: outline_tiles(ids[0], good),
                lambda: _capi.outline_host(ids.astype(np.uint16), good), lambda: _capi.outline_host(ids, good, want=('area',)),
                lambda: _capi.outline_host(ids, good, want=()), lambda: _capi.outline_host(ids, good, want=('chain', 'head')),
                lambda: _capi.outline_host(ids, good, want=('rings', 'head'))):
        with pytest.raises(ValueError):
            bad()


def test_header_says_has_outline_and_abi_7():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_OUTLINE 1' in text and '#define DSWX_OUTLINE_ROW_WORDS 8' in text and '#define DSWX_OUTLINE_HEAD_WORDS 8' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert (_capi.HAS_OUTLINE, _capi.OUTLINE_ROW_WORDS, _capi.OUTLINE_HEAD_WORDS, ROW_WORDS, HEAD_WORDS) == (1, 8, 8, 8, 8)
    assert text.index('---- distance:') < text.index('---- outline:') < text.index('---- device plumbing')
    for name in ('dswx_outline_work_bytes', 'dswx_outline_device', 'dswx_outline_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    assert 'dswx_batch_outline' not in _capi.EXPORTED_SYMBOLS and not hasattr(_capi.load_library(), 'dswx_batch_outline')
    section = ' '.join(text[text.index('---- outline:'):text.index('---- device plumbing')].replace(' * ', ' ').split())
    assert 'deterministic and independent of the launch geometry' in section and 'order in which atomics' in section
    assert 'MUST NOT OVERLAP' in section and 'NOT CHECKED' in section and 'ANY CONTENT IS LEGAL' in section
    assert 'No workgroup ever waits for another' in section and 'NO dswx_batch_* FORM' in section and '9 + N kernel launches' in section
    assert 'THE FIRST ENTRY THAT NEEDS WORKING MEMORY OF THE CALLER' in section and 'truncated, never wrong' in section
    assert 'dswx_*outline*' in text[text.index('---- device plumbing'):]
    rule = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_outline_rule.h')).read()
    assert f'DSWX_OUTLINE_CHUNK = {_capi.BODY_CHUNK};' in rule and f'DSWX_OUTLINE_SCAN_STEP = {_capi.BODY_SCAN_STEP};' in rule


def test_struct_mirrors_match_offsetof_as_gcc_sees_the_header(tmp_path):
    assert ctypes.sizeof(_capi.OutlineSpec) == 24 and ctypes.sizeof(_capi.OutlineOut) == 24 and ROW_DTYPE.itemsize == 32
    assert [ROW_DTYPE.fields[k][1] for k in ROW_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24]
    mirrors = _capi.ANALYTIC_STRUCTS
    assert mirrors['dswx_outline_spec_t'] is _capi.OutlineSpec and mirrors['dswx_outline_out_t'] is _capi.OutlineOut
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for st in ('dswx_outline_spec_t', 'dswx_outline_out_t'):
        for n, _ in mirrors[st]._fields_:
            lines.append(f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));')
        lines.append(f'  printf("{st}.sizeof %zu\\n", sizeof({st}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'off.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'off'
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st in ('dswx_outline_spec_t', 'dswx_outline_out_t'):
        assert int(got[f'{st}.sizeof']) == ctypes.sizeof(mirrors[st]), st
        for n, _ in mirrors[st]._fields_:
            assert int(got[f'{st}.{n}']) == getattr(mirrors[st], n).offset, (st, n)
    o = _capi.OutlineOut.of(chain=16, head=64)
    assert (o.chain, o.rings, o.head) == (16, None, 64)
    s = _capi.OutlineSpec.of(Spec(40, 9, 8))
    assert (s.max_edges, s.max_rings, s.connectivity, s.reserved) == (40, 9, 8, 0)


def test_polygons_of_the_four_pixel_lake():
    """The tile of test_wtr_body_spec_counts_open_and_partial_water (tests/test_body_table.py): a lake of four pixels and a
    speck, labelled with connectivity 4.  The lake is a 2 x 2 square, the speck one pixel: four vertices each, clockwise on
    screen from the top left corner, no holes; a ring with a hole gives it to the polygon of the same id."""
    from proteus_amd.label import label_tiles, wtr_label_spec
    tile = np.array([[[1, 1, 253, 2], [2, 1, 0, 0], [255, 0, 0, 252]]], dtype=np.uint8)
    label = label_tiles(tile, wtr_label_spec(1, connectivity=4))['label']
    table = body_table(label, tile, wtr_body_spec(9))
    got = two_statements(label, Spec(16, 4, 4), 'lake')
    assert got['head'][0].tolist() == [12, 2, 2, 12, 2, 0, 8, 0] and got['head'][0, 0] == table['head'][0, 4]
    assert got['rings'][0, :2].tolist() == [(1, 0, 0, 8, 4, 0, 8), (4, 12, 8, 4, 4, 0, 2)]
    assert got['chain'][0].tolist() == [0, 4, 5, 21, 22, 18, 19, 3, 12, 13, 14, 15, 0, 0, 0, 0]
    polys = list(polygons(got['chain'][0], got['rings'][0], 4))
    assert [(i, o.tolist(), h) for i, o, h in polys] == [(1, [[0, 0], [2, 0], [2, 2], [0, 2]], []), (4, [[3, 0], [4, 0], [4, 1], [3, 1]], [])]
    assert list(polygons(got['chain'][0], _capi.outline_host(label, Spec(16, 4, 4))['rings'][0], 4))[0][1].tolist() == polys[0][1].tolist()
    # a frame: the outer ring clockwise, its hole the other way, and the hole goes to the polygon of the frame's id
    ids = np.full((1, 3, 3), 7, dtype=np.uint32)
    ids[0, 1, 1] = 0
    got = two_statements(ids, Spec(16, 2, 8), 'frame')
    (i, outer, holes), = list(polygons(got['chain'][0], got['rings'][0], 3))
    assert i == 7 and outer.tolist() == [[0, 0], [3, 0], [3, 3], [0, 3]] and [h.tolist() for h in holes] == [[[2, 1], [1, 1], [1, 2], [2, 2]]]
    # (the hole starts at its smallest key, 6: the bottom edge of pixel (1, 0), travelled from corner (2, 1) to corner (1, 1))
    assert got['rings'][0]['start'].tolist() == [0, 6]
    assert got['rings'][0]['area2'].tolist() == [18, -2] and edge_area2(np.array([0, 1, 2, 3]), 1).tolist() == [0, 1, 1, 0]


def test_host_entry_and_rule_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/outline_host_san.cpp with proteus_amd/csrc/dswx_outline.hip compiled into it, host code under ASan + UBSan:
    odd addresses, guard bytes around every output, heap blocks of exactly the bytes the entry may touch.  A child process;
    nothing is loaded into this interpreter."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'outline_host_san')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'proteus_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'native', 'outline_host_san.cpp'), os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_outline.hip'), '-o', exe]
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


def test_outline_example_compiles_against_the_header(tmp_path):
    """examples/batch_outline.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device the
    program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_outline')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_outline.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
