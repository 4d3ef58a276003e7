"""The body table of include/dswx_hip.h ("body table") without a GPU: three statements pinned to each other -- the library's
scalar entry (dswx_body_table_host), the numpy statement (proteus_amd/bodies.py) and scipy.ndimage (label, find_objects, sum)
-- on every pattern of tests/_label_cases.py labelled by dswx_label_host, both connectivities; the perimeter against a count
made another way; capacities either side of K; malformed planes; every n_cats, strides, odd addresses; every refusal, with
the outputs untouched; the header; the struct mirrors; the WTR spec; the host entry under ASan + UBSan in a stand-alone
program; the C example."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.bodies import HEAD_WORDS, ROW_DTYPE, ROW_WORDS, Spec, body_table, wtr_body_spec
from tests import _body_cases as B
from tests import _label_cases as C

try:
    from scipy import ndimage
except ImportError:                                # (only the comparison with scipy is skipped then)
    ndimage = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT8 = 0xEE
KEYS = ('dense', 'rows', 'head')
EB = {'dense': 4, 'rows': 4, 'head': 8}


def records(rows):
    """uint32 [n, max_rows, 16] -> ROW_DTYPE [n, max_rows]."""
    return rows.view(ROW_DTYPE)[..., 0]


def perimeter_by_shifts(label):
    """Per pixel of one raster: the number of its four neighbours that are outside or hold another label value -- four
    shifted comparisons of the plane padded with a value no pixel holds."""
    lab = label.astype(np.int64)
    pad = np.pad(lab, 1, constant_values=-1)
    return ((pad[:-2, 1:-1] != lab).astype(np.int64) + (pad[2:, 1:-1] != lab) + (pad[1:-1, :-2] != lab) + (pad[1:-1, 2:] != lab))


def three_statements(label, value, spec, members=None, connectivity=None, what=None):
    """Host entry == numpy statement; for a well-formed plane also == scipy (dense, box, area, sums, counts)."""
    host = _capi.body_table_host(label, value, spec)
    stated = body_table(label, value, spec)
    assert np.array_equal(host['dense'], stated['dense']), what
    assert np.array_equal(host['head'], stated['head']), (what, host['head'], stated['head'])
    rows = records(host['rows']) if 'rows' in host else np.zeros((len(label), 0), dtype=ROW_DTYPE)
    assert np.array_equal(rows, stated['rows']), what
    n, H, W = label.shape
    ys, xs = np.indices((H, W))
    for t in range(n):
        dense, K, R = host['dense'][t], int(host['head'][t, 0]), int(host['head'][t, 1])
        assert R == min(K, spec.max_rows) and np.all(host['head'][t, 5:] == 0)
        edges = perimeter_by_shifts(label[t])
        assert host['head'][t, 4] == edges[dense != 0].sum(), (what, t, 'perimeter of all bodies')
        r = rows[t]
        assert np.all(r[R:].view(np.uint32) == 0), (what, t, 'the rows behind the last body are zero')
        index = np.arange(1, R + 1)
        if R:
            assert np.array_equal(r['perimeter'][:R], np.bincount(dense.reshape(-1), weights=edges.reshape(-1), minlength=K + 1)[1:R + 1].astype(np.uint64)), (what, t)
            assert np.array_equal(r['area'][:R], np.bincount(dense.reshape(-1), minlength=K + 1)[1:R + 1]), (what, t, 'bincount')
            assert np.array_equal(r['label'][:R] - 1, np.flatnonzero(label[t].reshape(-1) == np.arange(1, H * W + 1))[:R])
        if members is None or ndimage is None:
            continue
        lab, k = ndimage.label(members[t], structure=np.ones((3, 3)) if connectivity == 8 else None)
        assert k == K and np.array_equal(lab, dense), (what, t, 'scipy.ndimage.label')
        assert host['head'][t, 2] == np.count_nonzero(members[t]) and host['head'][t, 3] == 0
        if not R:
            continue
        boxes = ndimage.find_objects(lab)[:R]
        assert [(b[1].start, b[1].stop - 1, b[0].start, b[0].stop - 1) for b in boxes] == \
            [tuple(int(v) for v in (q['x_min'], q['x_max'], q['y_min'], q['y_max'])) for q in r[:R]], (what, t, 'find_objects')
        assert np.array_equal(r['sum_x'][:R], np.asarray(ndimage.sum(xs, lab, index)).astype(np.uint64)), (what, t, 'sum_x')
        assert np.array_equal(r['sum_y'][:R], np.asarray(ndimage.sum(ys, lab, index)).astype(np.uint64)), (what, t, 'sum_y')
        for c in range(4):
            want = np.asarray(ndimage.sum(spec.cat_of_byte[value[t]] == c, lab, index)) if value is not None and c < spec.n_cats else np.zeros(R)
            assert np.array_equal(r['count'][:R, c], want.astype(np.uint32)), (what, t, 'count', c)
    return host


@pytest.mark.parametrize('W', [1, 16, 17, 129, 257])
def test_host_entry_numpy_statement_and_scipy_agree_on_every_pattern(W):
    """Heights {1, 2, 33, 65} at this width, both connectivities, every pattern of tests/_label_cases.py labelled by
    dswx_label_host: dense is scipy.ndimage.label's own array; the box is find_objects; area is bincount; sum_x, sum_y and the
    category counts are ndimage.sum over index grids and over cat == c; the perimeter is counted by four shifted comparisons."""
    rng = np.random.default_rng(9800 + W)
    for H in (1, 2, 33, 65):
        pats = C.patterns(H, W, rng)
        members = np.stack(list(pats.values()))
        for conn in (4, 8):
            label = B.labels_of(members, rng, conn)
            K = int(B.bodies_of(label).max())
            value = B.value_like(label, rng)
            host = three_statements(label, value, B.spec_of(4, K), members, conn, (H, W, conn))
            names = list(pats)
            t = names.index('full')
            full = records(host['rows'])[t, 0]
            assert (full['label'], full['area'], full['x_min'], full['x_max'], full['y_min'], full['y_max']) == (1, H * W, 0, W - 1, 0, H - 1)
            assert full['perimeter'] == 2 * (H + W) and full['sum_x'] == H * W * (W - 1) // 2 and full['sum_y'] == W * H * (H - 1) // 2
            assert host['head'][names.index('empty')].tolist() == [0] * HEAD_WORDS
            if conn == 8 and min(H, W) >= 2:
                board = records(host['rows'])[names.index('checkerboard'), 0]
                assert board['perimeter'] == 4 * board['area'] == 4 * ((H * W + 1) // 2)


def test_capacity_either_side_of_k():
    """max_rows in {0, 1, K - 1, K, K + 1}: the first max_rows rows are those of the full table, the rest zero; dense and head
    words 0 and 2 .. 4 do not change."""
    rng = np.random.default_rng(9810)
    label = B.labels_of(np.stack([C.noise(33, 129, d, rng) for d in (0.3, 0.593)]), rng, 4)
    value = B.value_like(label, rng)
    Ks = B.bodies_of(label)
    K = int(Ks.min())
    assert K > 3
    full = three_statements(label, value, B.spec_of(3, int(Ks.max())), what='full')
    for max_rows in (0, 1, K - 1, K, K + 1):
        got = three_statements(label, value, B.spec_of(3, max_rows), what=max_rows)
        assert np.array_equal(got['dense'], full['dense'])
        assert np.array_equal(got['head'][:, [0, 2, 3, 4]], full['head'][:, [0, 2, 3, 4]]) and got['head'][:, 1].tolist() == [min(int(k), max_rows) for k in Ks]
        if max_rows:
            for t in range(2):
                keep = min(int(Ks[t]), max_rows)
                assert np.array_equal(got['rows'][t, :keep], full['rows'][t, :keep]) and np.all(got['rows'][t, keep:] == 0)
        else:
            assert 'rows' not in got


@pytest.mark.parametrize('H,W', [(33, 129), (12, 20), (1, 300)])
def test_malformed_planes(H, W):
    """A label above height * width, above idx + 1, with a target that is no root, pointing at a non-member, and the plane
    of the label entry with one root zeroed: head words 2 and 3 and the well-formed bodies are those of the numpy statement,
    and a malformed pixel has dense 0."""
    rng = np.random.default_rng(9820 + H)
    cases = B.malformed(H, W, rng)
    label = np.stack(list(cases.values()))
    value = B.value_like(label, rng)
    host = three_statements(label, value, B.spec_of(4, int(B.bodies_of(label).max()) + 1), what='malformed')
    assert np.all(host['head'][:, 3] > 0)
    flat, idx = label.reshape(len(label), -1).astype(np.int64), np.arange(H * W)
    for t, name in enumerate(cases):
        lab = flat[t]
        ok = np.array([l != 0 and l <= p + 1 and lab[l - 1] == l for p, l in zip(idx, lab)])
        assert np.array_equal(host['dense'][t].reshape(-1) != 0, ok), name
        assert host['head'][t, 2] == ok.sum() and host['head'][t, 3] == np.count_nonzero(lab) - ok.sum(), name
    t = list(cases).index('above_idx')                   # the pixel before a root with the root's VALUE is not of its body
    lab = flat[t]
    p = np.flatnonzero((lab[:-1] == lab[1:]) & (lab[1:] == idx[1:] + 1))
    assert len(p) and np.all(host['dense'][t].reshape(-1)[p] == 0) and np.all(host['dense'][t].reshape(-1)[p + 1] != 0)


def run_host(label, value, spec, stride=None, off=0, want=KEYS):
    """dswx_body_table_host with the label plane, the value plane [T][stride] and every output `off` bytes past an aligned
    address, every other byte of the value buffer a COUNTED byte and every output byte a sentinel beforehand.  Returns (rc,
    {output: array}); nothing outside the wanted outputs may have changed."""
    lib = _capi.load_library()
    T, H, W = label.shape
    n = H * W
    stride = n if stride is None else stride
    lraw = np.zeros(4 * T * n + 64, dtype=np.uint8)
    lbase = (-lraw.ctypes.data) % 16 + off
    lraw[lbase:lbase + 4 * T * n] = label.reshape(-1).view(np.uint8)
    vraw = np.full(max(T * stride, 1) + 64, B.PAD_VALUE, dtype=np.uint8)
    vbase = (-vraw.ctypes.data) % 16 + off
    if value is not None:
        for t in range(T):
            vraw[vbase + t * stride:vbase + t * stride + n] = value[t].reshape(-1)
    count = {'dense': T * n, 'rows': T * spec.max_rows * ROW_WORDS, 'head': T * HEAD_WORDS}
    bufs, out = {}, _capi.BodyOut()
    for k in KEYS:
        b = np.full(count[k] * EB[k] + 64, SENT8, dtype=np.uint8)
        start = (-b.ctypes.data) % 16 + off
        bufs[k] = (b, start)
        if k in want:
            setattr(out, k, b.ctypes.data + start)
    rc = lib.dswx_body_table_host(lraw.ctypes.data + lbase, vraw.ctypes.data + vbase if value is not None else None,
                                  ctypes.byref(_capi.BodySpec.of(spec)), T, H, W, 0 if stride == n else stride, ctypes.byref(out))
    res = {}
    for k, (b, start) in bufs.items():
        used = count[k] * EB[k] if k in want else 0
        assert np.all(b[:start] == SENT8) and np.all(b[start + used:] == SENT8), k
        if k in want:
            res[k] = b[start:start + used].copy().view(_capi.BODY_DTYPES[k]).reshape(_capi._body_shape(k, T, H, W, spec))
    return rc, res


def test_every_n_cats_strides_odd_addresses_and_every_subset_of_the_outputs():
    """n_cats 0 with no value plane and 1 .. 4 with a table that uses bytes 0, 1, 254 and 255 and has values that are not
    counted; the stride equal to the raster and above it, the padding full of a counted byte; every buffer at odd addresses;
    dense alone, dense + head, dense + rows, all three."""
    rng = np.random.default_rng(9830)
    cases = 0
    for (T, H, W) in ((0, 5, 7), (1, 1, 1), (3, 17, 33), (2, 32, 16), (4, 9, 130)):
        label = B.labels_of(rng.random((T, H, W)) < 0.55, rng, (4, 8)[T % 2]) if T else np.zeros((0, H, W), dtype=np.uint32)
        value = B.value_like(label, rng)
        K = int(B.bodies_of(label).max()) if T else 0
        for n_cats in range(5):
            val = value if n_cats else None
            table = B.cat_table(n_cats)
            assert n_cats == 0 or (set(table[[0, 1, 254, 255]].tolist()) == {0, 1, 2, 3} and table[3] == n_cats)
            for stride in (H * W, H * W + 3):
                for keys in (('dense',), ('dense', 'head'), ('dense', 'rows'), KEYS):
                    spec = B.spec_of(n_cats, K + 1 if 'rows' in keys else 0)
                    want = body_table(label, val, spec)
                    rc, got = run_host(label, val, spec, stride, off=(0, 1, 2, 3, 5)[cases % 5], want=keys)
                    assert rc == 0, _capi.load_library().dswx_last_error()
                    for k in keys:
                        g = records(got[k]) if k == 'rows' else got[k]
                        assert np.array_equal(g, want[k]), (T, H, W, n_cats, stride, keys, k)
                    cases += 1
            if n_cats and K > 1:
                counted = records(_capi.body_table_host(label, value, B.spec_of(n_cats, K))['rows'])['count']
                assert np.all(counted[..., n_cats:] == 0) and counted[..., :n_cats].sum() > 0
    padded = np.full((4, 9 * 130 + 3), B.PAD_VALUE, dtype=np.uint8)
    padded[:, :9 * 130] = value.reshape(4, -1)
    spec = B.spec_of(4, K)
    assert np.array_equal(records(_capi.body_table_host(label, padded, spec, raster=(9, 130))['rows']), body_table(label, value, spec)['rows'])
    assert list(_capi.body_table_host(label, value, spec, want=('rows',))) == ['dense', 'rows']


def test_refusals_with_the_outputs_untouched():
    lib = _capi.load_library()
    vp = ctypes.c_void_p
    good = B.spec_of(2, 5)
    H, W = 4, 6
    label = np.ones((3, H, W), dtype=np.uint32)
    value = np.ones((3, H, W), dtype=np.uint8)
    count = {'dense': 3 * H * W, 'rows': 3 * 5 * ROW_WORDS, 'head': 3 * HEAD_WORDS}
    planes = {k: np.full(count[k] * EB[k] + 16, SENT8, dtype=np.uint8) for k in KEYS}
    at = {k: planes[k].ctypes.data + (-planes[k].ctypes.data) % 8 for k in KEYS}

    def outs(**kw):
        o = _capi.BodyOut.of(**at)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def spec_c(**kw):
        s = _capi.BodySpec.of(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def host(label=label.ctypes.data, value=value.ctypes.data, spec=None, n_tiles=3, height=H, width=W, stride=0, out=None,
             null_spec=False, null_out=False):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out
        return lib.dswx_body_table_host(vp(label), vp(value), None if null_spec else ctypes.byref(spec), n_tiles, height, width, stride,
                                        None if null_out else ctypes.byref(out))

    def dev(label=0x10000, value=0x20000, spec=None, n_tiles=3, height=H, width=W, stride=0, out=None, null_spec=False,
            null_out=False, ctx=None):
        spec = spec_c() if spec is None else spec
        out = outs() if out is None else out                   # host addresses, never dereferenced: every call fails first
        return lib.dswx_body_table_device(ctx, vp(label), vp(value), None if null_spec else ctypes.byref(spec), n_tiles, height, width,
                                          stride, None if null_out else ctypes.byref(out), None)

    def refused(rc, code, text):
        assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())

    for call in (host, dev):
        refused(call(null_spec=True), _capi.ERR_ARG, b'spec is NULL')
        refused(call(null_out=True), _capi.ERR_ARG, b'out is NULL')
        for c in (-1, 5, 255, 1 << 20):
            refused(call(spec=spec_c(n_cats=c)), _capi.ERR_ARG, b'n_cats')
        refused(call(spec=spec_c(n_cats=0)), _capi.ERR_ARG, b'a value plane with n_cats 0')
        refused(call(value=None), _capi.ERR_ARG, b'value is NULL')
        for kw in ({'n_tiles': -1}, {'height': -1}, {'width': -1}, {'stride': -5}, {'spec': spec_c(max_rows=-1)}):
            refused(call(**kw), _capi.ERR_ARG, b'negative')
        refused(call(stride=H * W - 1), _capi.ERR_ARG, b'stride')
        refused(call(height=(1 << 31) + 1, width=1, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(height=1 << 16, width=(1 << 15) + 1, n_tiles=1), _capi.ERR_ARG, b'2^31')
        refused(call(height=1 << 40, width=1 << 40, n_tiles=1), _capi.ERR_ARG, b'too large')
        refused(call(spec=spec_c(max_rows=(1 << 31) + 1)), _capi.ERR_ARG, b'max_rows')
        refused(call(out=outs(dense=None)), _capi.ERR_ARG, b'dense is NULL')
        refused(call(out=outs(dense=None, rows=None, head=None)), _capi.ERR_ARG, b'dense is NULL')
        refused(call(label=None), _capi.ERR_ARG, b'label is NULL')
        refused(call(out=outs(rows=None)), _capi.ERR_ARG, b'rows is NULL')
    # the device entry: alignment; then, with everything in order, the context -- checked last
    for off in (1, 2, 3):
        refused(dev(label=0x10000 + off), _capi.ERR_ALIGN, b'label')
        refused(dev(out=outs(dense=at['dense'] + off)), _capi.ERR_ALIGN, b'dense')
    for off in (1, 2, 4, 7):
        refused(dev(out=outs(rows=at['rows'] + off)), _capi.ERR_ALIGN, b'rows')
        refused(dev(out=outs(head=at['head'] + off)), _capi.ERR_ALIGN, b'head')
    refused(dev(value=0x20001), _capi.ERR_ARG, b'ctx')                                   # the value plane takes any address
    refused(dev(), _capi.ERR_ARG, b'ctx')
    refused(dev(height=1 << 16, width=1 << 15, n_tiles=1), _capi.ERR_ARG, b'ctx')          # 2^31 pixels are legal
    refused(dev(spec=spec_c(max_rows=1 << 31)), _capi.ERR_ARG, b'ctx')                     # and 2^31 rows
    refused(dev(label=None, n_tiles=0), _capi.ERR_ARG, b'ctx')                           # nothing to read: no label needed
    refused(dev(out=outs(rows=None, head=None), spec=spec_c(max_rows=0)), _capi.ERR_ARG, b'ctx')   # dense alone
    refused(dev(value=None, spec=spec_c(n_cats=0)), _capi.ERR_ARG, b'ctx')
    refused(lib.dswx_batch_body_table(None, 14, ctypes.byref(spec_c()), 0, 1, vp(0x10000), ctypes.byref(outs()), None), _capi.ERR_ARG, b'batch is NULL')
    for k in KEYS:                                                                       # a refused call wrote nothing
        assert np.all(planes[k] == SENT8), k
    # n_tiles == 0 or an empty raster is legal and writes nothing
    assert host(label=None, n_tiles=0) == 0 and host(label=None, height=0) == 0 and host(label=None, width=0) == 0
    for k in KEYS:
        assert np.all(planes[k] == SENT8), k
    # and the same arguments, accepted: every pixel names pixel 0, one body per tile
    assert host() == 0
    off = {k: at[k] - planes[k].ctypes.data for k in KEYS}
    assert np.all(planes['dense'][off['dense']:][:4 * 3 * H * W].view(np.uint32) == 1)
    rows = planes['rows'][off['rows']:][:4 * count['rows']].view(np.uint32).reshape(3, 5, ROW_WORDS).view(ROW_DTYPE)[..., 0]
    assert rows['area'].tolist() == [[H * W, 0, 0, 0, 0]] * 3 and rows['count'][:, 0].tolist() == [[H * W, 0, 0, 0]] * 3
    assert planes['head'][off['head']:][:8 * count['head']].view(np.uint64).reshape(3, -1).tolist() == [[1, 1, H * W, 0, 2 * (H + W), 0, 0, 0]] * 3
    assert host(out=outs(dense=at['dense'] + 1, rows=at['rows'] + 3, head=at['head'] + 5), label=label.ctypes.data) == 0    # any address
    # the Python side refuses what the library would
    for bad in (lambda: Spec(5, B.cat_table(4), 1), lambda: Spec(-1, None, 1), lambda: Spec(1, B.cat_table(1), -1),
                lambda: Spec(1, B.cat_table(1), (1 << 31) + 1), lambda: Spec(1, B.cat_table(1)[:255], 1),
                lambda: body_table(label.astype(np.int32), value, good), lambda: body_table(label[0], value[0], good),
                lambda: body_table(label, None, good), lambda: body_table(label, value, Spec(0, None, 1)),
                lambda: body_table(label, value[:, :2], good), lambda: _capi.body_table_host(label.astype(np.uint16), value, good),
                lambda: _capi.body_table_host(label, value, good, want=('area',)), lambda: _capi.body_table_host(label, value, good, want=()),
                lambda: _capi.body_table_host(label, value, good, want=('dense',))):
        with pytest.raises(ValueError):
            bad()


def test_header_says_has_body_table_and_abi_7():
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    assert '#define DSWX_HAS_BODY_TABLE 1' in text and '#define DSWX_BODY_ROW_WORDS 16' in text and '#define DSWX_BODY_HEAD_WORDS 8' in text
    assert '#define DSWX_ABI_VERSION 7' in text and _capi.DSWX_ABI_VERSION == 7 and _capi.load_library().dswx_abi_version() == 7
    assert (_capi.HAS_BODY_TABLE, _capi.BODY_ROW_WORDS, _capi.BODY_HEAD_WORDS, ROW_WORDS, HEAD_WORDS) == (1, 16, 8, 16, 8)
    assert text.index('---- label:') < text.index('---- body table:') < text.index('---- device plumbing')
    for name in ('dswx_body_table_device', 'dswx_batch_body_table', 'dswx_body_table_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    section = ' '.join(text[text.index('---- body table:'):text.index('---- device plumbing')].replace(' * ', ' ').split())
    assert 'deterministic and independent of the launch geometry' in section and 'order in which atomics' in section
    assert 'MUST NOT OVERLAP' in section and 'NOT CHECKED' in section and 'WELL-FORMED' in section and 'MALFORMED' in section
    assert 'scipy.ndimage.label' in section and 'No workgroup ever waits for another' in section and 'checked before the dependent load' in section
    assert 'dswx_*body_table*' in text[text.index('---- device plumbing'):]
    rule = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_body_rule.h')).read()
    assert f'DSWX_BODY_CHUNK = {_capi.BODY_CHUNK};' in rule and f'DSWX_BODY_SCAN_STEP = {_capi.BODY_SCAN_STEP};' in rule
    assert f'DSWX_BODY_RECT_H = {_capi.BODY_RECT_H};' in rule and f'DSWX_BODY_RECT_W = {_capi.BODY_RECT_W};' in rule


def test_struct_mirrors_match_offsetof_as_gcc_sees_the_header(tmp_path):
    assert ctypes.sizeof(_capi.BodySpec) == 272 and ctypes.sizeof(_capi.BodyOut) == 24 and ROW_DTYPE.itemsize == 64
    assert [ROW_DTYPE.fields[k][1] for k in ROW_DTYPE.names] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48]
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    mirrors = _capi.ANALYTIC_STRUCTS
    assert mirrors['dswx_body_spec_t'] is _capi.BodySpec and mirrors['dswx_body_out_t'] is _capi.BodyOut
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dswx_hip.h"', 'int main(void) {']
    for st, cls in mirrors.items():
        for n, _ in cls._fields_:
            lines.append(f'  printf("{st}.{n} %zu\\n", offsetof({st}, {n}));')
        lines.append(f'  printf("{st}.sizeof %zu\\n", sizeof({st}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'off.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'off'
    subprocess.run(['gcc', '-std=c11', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in mirrors.items():
        assert int(got[f'{st}.sizeof']) == ctypes.sizeof(cls), st
        for n, _ in cls._fields_:
            assert int(got[f'{st}.{n}']) == getattr(cls, n).offset, (st, n)
    o = _capi.BodyOut.of(dense=16, head=64)
    assert (o.dense, o.rows, o.head) == (16, None, 64)
    s = _capi.BodySpec.of(Spec(3, np.arange(256) % 7, 17))
    assert (s.n_cats, s.max_rows) == (3, 17) and list(s.cat_of_byte) == [b % 7 for b in range(256)]


def test_wtr_body_spec_counts_open_and_partial_water():
    s = wtr_body_spec(9)
    assert (s.n_cats, s.max_rows) == (2, 9) and np.flatnonzero(s.cat_of_byte < 2).tolist() == [1, 2] and s.cat_of_byte[1] == 0 and s.cat_of_byte[2] == 1
    u = wtr_body_spec(9, collapsed=False)
    assert u.cat_of_byte[1:5].tolist() == [0, 0, 1, 1] and np.count_nonzero(u.cat_of_byte < 2) == 4
    assert 'ANOTHER date' in wtr_body_spec.__doc__ and 'stack.wtr_spec' in wtr_body_spec.__doc__
    # a lake of four pixels (three open, one partial), a speck of partial water, cloud between them
    from proteus_amd.label import label_tiles, wtr_label_spec
    tile = np.array([[[1, 1, 253, 2], [2, 1, 0, 0], [255, 0, 0, 252]]], dtype=np.uint8)
    label = label_tiles(tile, wtr_label_spec(1, connectivity=4))['label']
    got = body_table(label, tile, s)
    assert got['head'][0, :5].tolist() == [2, 2, 5, 0, 8 + 4] and got['dense'][0].tolist() == [[1, 1, 0, 2], [1, 1, 0, 0], [0, 0, 0, 0]]
    lake, speck = got['rows'][0, 0], got['rows'][0, 1]
    assert (lake['label'], lake['area'], lake['perimeter'], lake['sum_x'], lake['sum_y']) == (1, 4, 8, 2, 2) and lake['count'].tolist() == [3, 1, 0, 0]
    assert (speck['label'], speck['area'], speck['x_min'], speck['x_max'], speck['y_max']) == (4, 1, 3, 3, 0) and speck['count'].tolist() == [0, 1, 0, 0]
    assert np.all(got['rows'][0, 2:].view(np.uint32) == 0)


def test_host_entry_and_rule_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/body_table_host_san.cpp with proteus_amd/csrc/dswx_body_table.hip compiled into it, host code under ASan +
    UBSan: odd addresses, guard bytes around every output, heap blocks of exactly the bytes the entry may touch.  A child
    process; nothing is loaded into this interpreter."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'body_table_host_san')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'proteus_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'native', 'body_table_host_san.cpp'), os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_body_table.hip'), '-o', exe]
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


def test_body_example_compiles_against_the_header(tmp_path):
    """examples/batch_bodies.c is C (gcc -std=c11 -Wall -Wextra -Werror) and links against the library; without a device the
    program stops at dswx_ctx_create."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_bodies')
    lib_dir = os.path.dirname(_capi.library_path())
    _capi.load_library()
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_bodies.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    if _capi.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and 'dswx_ctx_create' in r.stderr and 'no CPU fallback' in r.stderr
