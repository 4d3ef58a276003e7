"""The body-table entries on the GPU: dswx_body_table_device and dswx_batch_body_table bit for bit against the library's scalar
statement (dswx_body_table_host, which tests/test_body_table.py pins to the numpy statement and to scipy) -- heights and widths
either side of a 16-element load and of a row, every pattern of tests/_label_cases.py at each, both connectivities, label and
dense at 0, 4 and 12 bytes and the value plane at 0, 1 and 3 bytes past a 16-byte boundary, padded strides, every subset of the
outputs and capacities either side of K, with every byte outside the outputs checked; element counts around the scan chunk and
more chunks than one step of the scan; a body per pixel and one body per tile; malformed planes; more tiles than grid.y has blocks; a caller's stream with the
outputs reused; the head against the label summary and the histogram; every form of batch; the DevicePlane chain;
bin/dswx_bodies.py --table; the C example."""
import csv
import ctypes
import importlib.util
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py)
    import torch
except ImportError:
    torch = None

from proteus_amd import _capi, geotiff
from proteus_amd.bodies import ROW_DTYPE, Spec, body_table, wtr_body_spec
from proteus_amd.checksum import checksum
from proteus_amd.label import Spec as LabelSpec, wtr_label_spec
from proteus_amd.synth import SEED
from tests import _body_cases as B
from tests import _label_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, STEP = _capi.BODY_CHUNK, _capi.BODY_SCAN_STEP
RW, HW = _capi.BODY_ROW_WORDS, _capi.BODY_HEAD_WORDS
SENT = 0xEE                                       # every byte of an output buffer beforehand
GUARD = 512
KEYS = ('dense', 'rows', 'head')
SUBSETS = (('dense',), ('dense', 'head'), KEYS)
EB = {'dense': 4, 'rows': 4, 'head': 8}
OFF = {'dense': 4, 'rows': 8, 'head': 8}          # past a 16-byte boundary (dense: also `off` below)


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Run:
    """One call of dswx_body_table_device.  The label plane lies guard | `loff` bytes past a 256-byte boundary | guard in
    `lbuf`; the value plane likewise `voff` bytes past in `vbuf` with `stride`, every byte that is not tile data a COUNTED
    byte; the wanted outputs lie in `obuf`, dense `loff` and rows and head 8 bytes past a 16-byte boundary, every byte SENT
    beforehand."""

    def __init__(self, ctx, label, value, spec, stride=None, loff=0, voff=0, want=KEYS, bufs=None):
        self.ctx, self.label, self.value, self.spec = ctx, label, value, spec
        self.want = tuple(k for k in want if k != 'rows' or spec.max_rows > 0)
        self.T, self.H, self.W = label.shape
        n = self.H * self.W
        self.stride = n if stride is None else stride
        self.lstart = GUARD + loff
        self.lhost = np.full(self.lstart + 4 * self.T * n + GUARD, SENT, dtype=np.uint8)
        self.lhost[self.lstart:self.lstart + 4 * self.T * n] = label.reshape(-1).view(np.uint8)
        span = (self.T - 1) * self.stride + n if self.T else 0
        self.vstart = GUARD + voff
        self.vhost = np.full(self.vstart + span + GUARD, B.PAD_VALUE, dtype=np.uint8)
        if value is not None:
            for t in range(self.T):
                self.vhost[self.vstart + t * self.stride:self.vstart + t * self.stride + n] = value[t].reshape(-1)
        self.count = {'dense': self.T * n, 'rows': self.T * spec.max_rows * RW, 'head': self.T * HW}
        self.where, cursor = {}, 0
        for k in KEYS:
            begin = -(-cursor // 16) * 16 + (loff if k == 'dense' else OFF[k])
            self.where[k] = begin
            cursor = begin + self.count[k] * EB[k] + 16
        self.osize = cursor + 16
        self.own = bufs is None
        self.lbuf, self.vbuf, self.obuf = bufs if bufs else (ctx.malloc(self.lhost.size), ctx.malloc(self.vhost.size), ctx.malloc(self.osize))
        assert self.lbuf.nbytes >= self.lhost.size and self.vbuf.nbytes >= self.vhost.size and self.obuf.nbytes >= self.osize
        assert self.lbuf.ptr % 256 == 0 and self.vbuf.ptr % 256 == 0 and self.obuf.ptr % 16 == 0
        self.lbuf.upload(self.lhost)
        self.vbuf.upload(self.vhost)
        self.poison()
        self.out = _capi.BodyOut.of(**{k: self.obuf.ptr + self.where[k] for k in self.want})

    def poison(self):
        self.obuf.upload(np.full(self.osize, SENT, dtype=np.uint8))

    def run(self, stream=None):
        self.ctx.body_table_device(self.lbuf.ptr + self.lstart, self.vbuf.ptr + self.vstart if self.value is not None else None,
                                   self.spec, self.T, self.H, self.W, self.out,
                                   value_stride=0 if self.stride == self.H * self.W else self.stride, stream=stream)

    def host(self):
        return _capi.body_table_host(self.label, self.value, self.spec)

    def get(self, k):
        return self.obuf.download(_capi.BODY_DTYPES[k], self.count[k], self.where[k])

    def check(self, what, ref=None):
        """The wanted outputs are the host entry's, every other byte of the output buffer is still SENT, and the inputs are
        what was uploaded."""
        ref = self.host() if ref is None else ref
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for k in self.want:
            begin, nb = self.where[k], self.count[k] * EB[k]
            got = raw[begin:begin + nb].copy().view(_capi.BODY_DTYPES[k])
            want = ref[k].reshape(-1)
            assert np.array_equal(got, want), (what, k, np.flatnonzero(got != want)[:6], got[got != want][:6], want[got != want][:6])
            written[begin:begin + nb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted outputs were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.array_equal(self.lbuf.download(np.uint8, self.lhost.size), self.lhost), (what, 'the label plane was written')
        assert np.array_equal(self.vbuf.download(np.uint8, self.vhost.size), self.vhost), (what, 'the value plane was written')
        return ref

    def free(self):
        for b in (self.lbuf, self.vbuf, self.obuf):
            b.free()


def once(ctx, label, value, spec, what, **kw):
    r = Run(ctx, label, value, spec, **kw)
    r.run()
    ctx.synchronize()
    ref = r.check(what)
    r.free()
    return ref


HEIGHTS = (1, 2, 31, 32, 33, 65)
WIDTHS = (1, 15, 16, 17, 127, 128, 129, 257)
assert (_capi.BODY_RECT_H, _capi.BODY_RECT_W) == (32, 128)     # (the shapes straddle the rectangle of a workgroup: 31 .. 33, 65; 127 .. 129, 257)


@pytest.mark.parametrize('W', WIDTHS)
def test_device_entry_against_the_host_entry_every_pattern_height_address_and_subset(ctx, W):
    """This width x heights {1, 2, 31, 32, 33, 65} x both connectivities; the 15 tiles of a call are the patterns of
    tests/_label_cases.py and one more of noise, labelled by dswx_label_host; label and dense 0, 4 and 12 bytes past a 16-byte
    boundary, the value plane 0, 1 and 3 bytes past with a stride 5 above the raster and padding and guards full of a counted
    byte; dense alone, dense + head, all three; max_rows cycles through 0, 1, K and K + 3; n_cats through 0 .. 4."""
    rng = np.random.default_rng(9900 + W)
    T, big = 15, max(HEIGHTS) * W
    kmax = (big + 1) // 2 + 3
    bufs = (ctx.malloc(2 * GUARD + 16 + 4 * T * big), ctx.malloc(2 * GUARD + 8 + T * (big + 5)),
            ctx.malloc(T * (4 * big + 64 * kmax + 64) + 256))
    cases = 0
    for H in HEIGHTS:
        for conn in (4, 8):
            label = B.pattern_labels(H, W, rng, conn, extra_noise=True)
            assert label.shape == (T, H, W)
            value = B.value_like(label, rng)
            K = int(B.bodies_of(label).max())
            for loff, voff in ((0, 0), (4, 1), (12, 3)):
                n_cats = cases % 5
                spec = B.spec_of(n_cats, (0, 1, K, K + 3)[cases % 4])
                val = value if n_cats else None
                ref = _capi.body_table_host(label, val, spec)
                for want in SUBSETS:
                    if 'rows' not in want and spec.max_rows:
                        continue                                     # (rows NULL requires max_rows 0: refused, tested below)
                    r = Run(ctx, label, val, spec, stride=H * W + (0 if voff == 0 else 5), loff=loff, voff=voff, want=want, bufs=bufs)
                    r.run()
                    ctx.synchronize()
                    r.check((H, W, conn, loff, voff, want, n_cats, spec.max_rows), ref=ref)
                cases += 1
            # the subsets without rows at max_rows 0, and everything at K
            for want in SUBSETS:
                spec = B.spec_of(2, K if 'rows' in want else 0)
                r = Run(ctx, label, value, spec, loff=4, voff=1, stride=H * W + 5, want=want, bufs=bufs)
                r.run()
                ctx.synchronize()
                r.check((H, W, conn, want, 'subset'))
            info = ctx.last_kernel_info()
            assert 'dswx_body_count_k' in info and 'dswx_body_scan_k' in info and f'chunk={CHUNK}' in info and f'step={STEP}' in info, info
    for b in bufs:
        b.free()


@pytest.mark.parametrize('n', [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 3 * CHUNK - 16])
def test_element_counts_around_the_scan_chunk(ctx, n):
    """One-tile calls of n elements as one row, as rows of 7 (n not a multiple of the width is avoided by trimming) and as
    one column: one below the chunk, equal to it, one above, not a multiple of 16."""
    rng = np.random.default_rng(9950 + n)
    for H, W in ((1, n), (n // 7, 7), (n, 1)):
        for conn, density in ((4, 0.5), (8, 0.3)):
            label = B.labels_of(C.noise(H, W, density, rng)[None], rng, conn)
            K = int(B.bodies_of(label)[0])
            once(ctx, label, B.value_like(label, rng), B.spec_of(3, K + 1), (H, W, conn), loff=4, voff=3, stride=H * W + 5)


@pytest.fixture(scope='module')
def deep():
    """The 1024 x 1040 spiral and serpentine (two tiles, 260 chunks each: more than one step of the scan), noise on top of a
    checkerboard so that every chunk has roots, and their labels at connectivity 4."""
    rng = np.random.default_rng(9960)
    H, W = 1024, 1040
    assert H * W > STEP * CHUNK
    members = np.stack([C.spiral(H, W), C.serpentine(H, W), C.checkerboard(H, W) & C.noise(H, W, 0.7, rng)])
    label = B.labels_of(members, rng, 4)
    return label, B.value_like(label, rng)


def test_more_chunks_than_one_step_of_the_scan(ctx, deep):
    label, value = deep
    K = B.bodies_of(label)
    assert K[0] == 1 and K[1] == 1 and K[2] > 300000
    ref = once(ctx, label, value, B.spec_of(4, int(K[2])), 'deep', loff=12, voff=1)
    # ranks cross every chunk seam: the last root of the third tile has rank K - 1
    assert ref['dense'][2].max() == K[2] and ref['head'][2, 0] == K[2] and np.all(ref['rows'][2, :, 1] == 1)


def test_every_pixel_its_own_body_and_one_body_per_tile(ctx):
    """The checkerboard at connectivity 4 (K = n / 2) and diagonals three apart at 4: ranks cross every chunk and every wave.
    A full tile and the checkerboard at 8: ONE row takes every atomic, and the perimeter of the checkerboard is 4 x area."""
    rng = np.random.default_rng(9970)
    H, W = 96, 131
    members = np.stack([C.checkerboard(H, W), C.diagonals(H, W, 1), C.diagonals(H, W, -1)])
    label = B.labels_of(members, rng, 4)
    K = B.bodies_of(label)
    assert K[0] == (H * W + 1) // 2 and K[1] == np.count_nonzero(members[1])
    ref = once(ctx, label, B.value_like(label, rng), B.spec_of(4, int(K.max())), 'own body', loff=4, voff=1, stride=H * W + 5)
    assert np.all(ref['rows'][0, :K[0], 1] == 1) and ref['head'][0, 4] == 4 * K[0]
    label = B.labels_of(np.stack([C.full(H, W), C.checkerboard(H, W)]), rng, 8)
    assert B.bodies_of(label).tolist() == [1, 1]
    ref = once(ctx, label, B.value_like(label, rng), B.spec_of(4, 2), 'one body', loff=12, voff=3)
    rows = ref['rows'].view(ROW_DTYPE)[..., 0]
    assert rows['area'][:, 0].tolist() == [H * W, (H * W + 1) // 2] and rows['perimeter'][0, 0] == 2 * (H + W)
    assert rows['perimeter'][1, 0] == 4 * rows['area'][1, 0] and np.all(ref['rows'][:, 1] == 0)


def test_malformed_planes_return_and_agree_with_the_host_entry(ctx):
    """Every malformed plane is legal input: a label above the tile or above idx + 1 is refused by the bound BEFORE the
    dependent load, a target that is no root or no member by the value loaded."""
    rng = np.random.default_rng(9980)
    for H, W in ((70, 131), (1, 4100)):
        cases = B.malformed(H, W, rng)
        label = np.stack(list(cases.values()))
        K = int(B.bodies_of(label).max())
        ref = once(ctx, label, B.value_like(label, rng), B.spec_of(4, K + 1), 'malformed', loff=4, voff=1, stride=H * W + 5)
        assert np.all(ref['head'][:, 3] > 0)
        stated = body_table(label, None, Spec(0, None, 0))
        assert np.array_equal(ref['head'][:, 2:4], stated['head'][:, 2:4]) and np.array_equal(ref['dense'], stated['dense'])
    garbage = rng.integers(0, 1 << 32, size=(2, 40, 200), dtype=np.uint64).astype(np.uint32)
    garbage[1] %= 8001
    once(ctx, garbage, None, B.spec_of(0, 50), 'garbage')


@pytest.mark.parametrize('H,W', [(2, 3), (_capi.BODY_RECT_H + 1, 2), (2, _capi.BODY_RECT_W + 1)],
                         ids=['one_rectangle', 'two_rectangles_down', 'two_rectangles_across'])
def test_a_workgroup_tabulates_a_second_tile_past_the_blocks_of_grid_y(ctx, H, W):
    """65535 + 4 tiles: grid.y is 65535 (and grid.x of the scan launch), and the workgroups of tiles 0 .. 3 walk on to tiles
    65535 .. 65538 with the `wtot` / `chunk_base` of the count and rank kernels and the `key` / `acc` / `part` of
    dswx_body_fill_k as the first tile left them.  The label planes are dswx_label_host's (connectivity 8) of
    tests/_label_cases.py's second-pass rasters: the first four tiles dense, the last four sparse, the rest noise; tile 65536
    holds a MALFORMED plane instead (the host entry is the reference for it as for the rest).  A random value plane with 4
    categories, its stride 3 above the raster and padding full of a counted byte; capacity 3, so that some tiles are
    truncated and some are not -- at 2 x 3 no tile has more than two bodies, so that shape runs again at capacity 1.  All
    three outputs of EVERY tile against the host entry, every byte outside the outputs checked."""
    rng = np.random.default_rng(9996 + H + W)
    label = B.labels_of(C.second_pass_members(H, W, rng), rng, 8)
    T = len(label)
    assert T == 65535 + 4
    label[65536] = B.malformed(H, W, rng)['above_idx'] if H * W >= 64 else B.malformed_tiny(H, W)
    for i in range(4):
        assert not np.array_equal(label[65535 + i], label[i]), i
    value = B.value_like(label, rng)
    r = None
    for max_rows in (3, 1) if H * W < 8 else (3,):
        spec = B.spec_of(4, max_rows)
        ref = _capi.body_table_host(label, value, spec)
        r = Run(ctx, label, value, spec, stride=H * W + 3, loff=4, voff=1, bufs=(r.lbuf, r.vbuf, r.obuf) if r else None)
        r.run()
        ctx.synchronize()
        info = ctx.last_kernel_info()
        assert info.count(',65535,1)') == 2 and 'dswx_body_scan_k grid=(65535,1,1)' in info, info
        r.check((H, W, max_rows), ref=ref)
    late = ref['head'][65535:]
    assert late[1, 3] > 0                                                  # (the malformed tile has malformed pixels)
    truncated = late[:, 0] > late[:, 1]
    assert truncated.any() and not truncated.all(), late[:, :2]
    whole = ref['head'][:, 0] > ref['head'][:, 1]
    assert 0 < np.count_nonzero(whole) < T
    r.free()


def test_on_a_callers_stream_twice_with_the_same_outputs(ctx):
    """On a caller's stream, and a second and third call that reuse the outputs of the first as they are (dense full of the
    first call's ranks, the rows of its sums): nothing depends on what the outputs held beyond the entry's own memsets."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(9990)
    H, W = 65, 257
    first = B.labels_of(np.stack([C.full(H, W), C.noise(H, W, 0.593, rng), C.checkerboard(H, W)]), rng, 4)
    second = B.labels_of(np.stack([C.noise(H, W, 0.5, rng), C.serpentine(H, W), C.empty(H, W)]), rng, 4)
    v1, v2 = B.value_like(first, rng), B.value_like(second, rng)
    spec = B.spec_of(3, H * W // 2 + 2)
    s = torch.cuda.Stream(device=0)
    r = Run(ctx, first, v1, spec, stride=H * W + 5, loff=4, voff=3)
    r.run(stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    r.check('first')
    r.label, r.value = second, v2                                    # the same buffers, other planes, the outputs NOT poisoned again
    r.lhost[r.lstart:r.lstart + 4 * second.size] = second.reshape(-1).view(np.uint8)
    for t in range(3):
        r.vhost[r.vstart + t * r.stride:r.vstart + t * r.stride + H * W] = v2[t].reshape(-1)
    r.lbuf.upload(r.lhost)
    r.vbuf.upload(r.vhost)
    r.run(stream=s.cuda_stream)
    r.run(stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    r.check('second')
    r.free()


def test_the_result_of_tile_0_does_not_depend_on_the_number_of_tiles(ctx):
    """There is no switch for the launch geometry, so: the bytes of tile 0 are the same whether the call has 1 tile or 7,
    run three times each, by checksums."""
    rng = np.random.default_rng(9991)
    H, W = 101, 391
    label = B.labels_of(np.stack([C.noise(H, W, d, rng) for d in (0.593, 0.1, 0.5, 0.593, 0.9, 0.6, 0.55)]), rng, 8)
    value = B.value_like(label, rng)
    spec = B.spec_of(4, int(B.bodies_of(label)[0]))
    seen = set()
    for T in (1, 7, 1, 7, 7, 1):
        r = Run(ctx, label[:T], value[:T], spec)
        r.run()
        ctx.synchronize()
        per = {'dense': H * W, 'rows': spec.max_rows * RW, 'head': HW}
        seen.add(tuple(checksum(r.get(k)[:per[k]].copy().view(np.uint8)) for k in KEYS))
        r.free()
    assert len(seen) == 1
    ref = _capi.body_table_host(label[:1], value[:1], spec)
    assert seen == {tuple(checksum(ref[k].reshape(-1).view(np.uint8)) for k in KEYS)}


def test_head_and_counts_against_the_label_summary_and_the_histogram(ctx):
    """Consistency without an oracle: the label entry's summary words 0 and 1 are head words 0 and 2; the areas of a full
    table sum to head word 2; the category counts of all rows sum to the histogram (dswx_histogram_device) of the value plane
    restricted to members -- of a plane in which every non-member's byte was replaced by one that is not counted."""
    rng = np.random.default_rng(9992)
    H, W, T = 67, 261, 4
    plane, table = C.plane_of(np.stack([C.noise(H, W, d, rng) for d in C.DENSITIES]), rng)
    lab = ctx.malloc(4 * T * H * W)
    size = ctx.malloc(4 * T * H * W)
    summ = ctx.malloc(8 * T * _capi.LABEL_SUMMARY_WORDS)
    src = ctx.malloc(T * H * W)
    src.upload(plane.reshape(-1))
    ctx.label_device(src.ptr, LabelSpec(8, 1, table), T, H, W, _capi.LabelOut.of(label=lab.ptr, size=size.ptr, summary=summ.ptr))
    ctx.synchronize()
    label = lab.download(np.uint32, T * H * W).reshape(T, H, W)
    summary = summ.download(np.uint64, T * _capi.LABEL_SUMMARY_WORDS).reshape(T, -1)
    K = int(summary[:, 0].max())
    spec = B.spec_of(4, K)
    value = np.where(label != 0, B.value_like(label, rng), 3).astype(np.uint8)      # byte 3 is not counted at n_cats 4
    assert spec.cat_of_byte[3] >= 4
    r = Run(ctx, label, value, spec)
    r.run()
    hist = ctx.malloc(T * 256 * 8)
    ctx.histogram_device(r.vbuf.ptr + r.vstart, _capi.HIST_U8, T, H * W, hist.ptr)
    ctx.synchronize()
    ref = r.check('consistency')
    bins = hist.download(np.uint64, T * 256).reshape(T, 256)
    head, rows = r.get('head').reshape(T, HW), r.get('rows').reshape(T, K, RW).view(ROW_DTYPE)[..., 0]
    for t in range(T):
        assert head[t, 0] == summary[t, 0] and head[t, 2] == summary[t, 1] and head[t, 3] == 0 and head[t, 1] == head[t, 0]
        assert rows['area'][t].sum() == head[t, 2] and rows['perimeter'][t].sum() == head[t, 4]
        for c in range(4):
            assert rows['count'][t, :, c].sum() == bins[t, spec.cat_of_byte == c].sum(), (t, c)
    assert ref['head'][:, 5:].sum() == 0
    for b in (lab, size, summ, src, hist):
        b.free()
    r.free()


def test_refusals_write_nothing(ctx):
    rng = np.random.default_rng(9993)
    label = B.labels_of(rng.random((2, 20, 30)) < 0.5, rng, 8)
    spec = B.spec_of(2, 40)
    r = Run(ctx, label, B.value_like(label, rng), spec)
    lib, h = ctx.lib, ctx.handle
    lp, vp_ = r.lbuf.ptr + r.lstart, r.vbuf.ptr + r.vstart

    def cs(**kw):
        c = _capi.BodySpec.of(spec)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def outs(**kw):
        o = _capi.BodyOut.of(**{k: r.obuf.ptr + r.where[k] for k in KEYS})
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(label=lp, value=vp_, cspec=cs(), n=2, H=20, W=30, stride=0, out=r.out, handle=h):
        return lib.dswx_body_table_device(handle, ctypes.c_void_p(label), ctypes.c_void_p(value),
                                          ctypes.byref(cspec) if cspec is not None else None, n, H, W, stride,
                                          ctypes.byref(out) if out is not None else None, None)

    A, L = _capi.ERR_ARG, _capi.ERR_ALIGN
    for rc, kw in ((A, {'cspec': None}), (A, {'out': None}), (A, {'cspec': cs(n_cats=5)}), (A, {'cspec': cs(n_cats=-1)}),
                   (A, {'cspec': cs(n_cats=0)}), (A, {'value': None}), (A, {'n': -1}), (A, {'H': -1}), (A, {'W': -1}),
                   (A, {'stride': -1}), (A, {'stride': 599}), (A, {'cspec': cs(max_rows=-1)}), (A, {'cspec': cs(max_rows=(1 << 31) + 1)}),
                   (A, {'H': 1 << 16, 'W': (1 << 15) + 1}), (A, {'label': None}), (A, {'out': outs(dense=None)}),
                   (A, {'out': outs(rows=None)}), (L, {'label': lp + 2}), (L, {'out': outs(dense=r.out.dense + 1)}),
                   (L, {'out': outs(rows=r.out.rows + 4)}), (L, {'out': outs(head=r.out.head + 4)}), (A, {'handle': None})):
        assert call(**kw) == rc, (kw, lib.dswx_last_error())
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    assert call(cspec=cs(n_cats=7), handle=None) == A and 'n_cats' in lib.dswx_last_error().decode()     # arguments before the context
    for kw in ({'n': 0}, {'H': 0}, {'W': 0}):                      # an empty raster and no tiles are legal and write nothing
        assert call(**kw) == 0, kw
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    r.run()
    ctx.synchronize()
    r.check('after the refusals')
    r.free()


FORMS = {'packed': {}, 'slide_placed': {'sliding_outputs': True}, 'contiguous': {'tile_align': 1}}


@pytest.mark.parametrize('form', list(FORMS))
def test_batch_body_table_on_the_wtr_plane_of_a_classified_batch(ctx, form):
    """The WTR plane of a classified packed, placed and contiguous batch of 4 tiles of 73 x 165, labelled by dswx_batch_label:
    every tile, tile ranges with tile0 > 0, DSWX_BATCH_ALL_TILES; the results checked by CHECKSUMS made on the device against
    the checksums of the host statement; no value plane; a band, DIAG, the counters, a missing plane and ranges outside the
    batch refused."""
    n_tiles, h, w = 4, 73, 165
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, **FORMS[form])
    sums = ctx.malloc(8 * n_tiles)
    try:
        batch.synth(SEED, tile0=31)
        p = _capi.default_params()
        if form == 'slide_placed':
            batch.place_slide(p, slack_bytes=24 << 20, step_bytes=2 << 20, spread_gaps=2, refine_passes=1, launches=2, keep_free_bytes=0)
        batch.classify(p)
        wtr = np.stack([batch.read_tile('wtr', t) for t in range(n_tiles)])
        lspec = wtr_label_spec(1)
        label = _capi.label_host(wtr, lspec, want=('label',))['label']
        K = int(B.bodies_of(label).max())
        assert K > 1
        for spec, name in ((wtr_body_spec(K), 'wtr'), (wtr_body_spec(3), 'wtr'), (Spec(0, None, K), None)):
            ref = body_table(label, wtr if name else None, spec)
            ref['rows'] = ref['rows'].view(np.uint32).reshape(n_tiles, spec.max_rows, RW)
            for tile0, count in ((0, None), (1, n_tiles - 1), (2, 1), (1, _capi.BATCH_ALL_TILES), (n_tiles, None), (0, 0)):
                lab = batch.label('wtr', lspec, tile0=tile0, n_tiles=count, want=('label',))['label']
                res = batch.body_table(name, spec, lab, tile0=tile0, n_tiles=count)
                assert list(res) == list(KEYS)
                last = tile0 + (n_tiles - tile0 if count in (None, _capi.BATCH_ALL_TILES) else count)
                nt = last - tile0
                for k in KEYS:
                    per = {'dense': h * w, 'rows': spec.max_rows * RW, 'head': HW}[k]
                    if nt:
                        ctx.checksum_device(res[k].ptr, EB[k], nt, per, sums.ptr)
                    ctx.synchronize()
                    got = sums.download(np.uint64, nt) if nt else np.zeros(0, dtype=np.uint64)
                    want = [checksum(ref[k][t].reshape(-1)) for t in range(tile0, last)]
                    assert got.tolist() == want, (form, k, tile0, count)
                for b in list(res.values()) + [lab]:
                    b.free()
        spec = wtr_body_spec(K)
        lab = batch.label('wtr', lspec, want=('label',))['label']
        for name in ('blue', 'swir2', 'diag'):
            with pytest.raises(_capi.DswxError, match=r'band\[|diag') as e:
                batch.body_table(name, spec, lab)
            assert e.value.code == _capi.ERR_ARG and 'uint8' in str(e.value)
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.body_table('counters', spec, lab)
        assert e.value.code == _capi.ERR_ARG
        for name in ('land', 'browse'):
            with pytest.raises(_capi.DswxError, match=name) as e:
                batch.body_table(name, spec, lab)
            assert e.value.code == _capi.ERR_ARG and 'no plane' in str(e.value)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside the batch'):
                batch.body_table('wtr', spec, lab, tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(_capi.DswxError, match='value is NULL'):
            batch.body_table(None, spec, lab)
        with pytest.raises(ValueError):
            batch.body_table('water', spec, lab)
        lab.free()
    finally:
        sums.free()
        batch.free()


def test_device_plane_chain_upload_label_body_table(ctx):
    """upload -> label -> body_table with no host copy in between, equal to bodies.body_table."""
    from proteus_amd.label import label_tiles
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9994)
    try:
        a = rng.choice(np.array([0, 1, 2, 252, 253, 255], dtype=np.uint8), size=(3, 52, 158), p=[0.4, 0.3, 0.1, 0.05, 0.1, 0.05])
        p = eng.upload(a)
        label = label_tiles(a, wtr_label_spec(1))['label']
        spec = wtr_body_spec(int(B.bodies_of(label).max()) + 2)
        want = body_table(label, a, spec)
        lab = p.label(wtr_label_spec(1), want=('label',))['label']
        got = lab.body_table(spec, value=p)
        assert list(got) == list(KEYS) and lab._host is None and all(got[k]._host is None for k in KEYS)
        assert np.array_equal(got['dense'].numpy(), want['dense']) and np.array_equal(got['head'].numpy(), want['head'])
        assert np.array_equal(got['rows'].numpy().view(ROW_DTYPE)[..., 0], want['rows'])
        bare = lab.body_table(Spec(0, None, 0), want=('dense', 'head'))
        assert list(bare) == ['dense', 'head'] and np.array_equal(bare['dense'].numpy(), want['dense'])
        one = eng.upload(label[0]).body_table(spec, value=eng.upload(a[0]))
        assert np.array_equal(one['rows'].numpy().view(ROW_DTYPE)[..., 0], want['rows'][:1])
        for bad in (lambda: p.body_table(spec, value=p), lambda: lab.body_table(spec), lambda: lab.body_table(Spec(0, None, 0), value=p),
                    lambda: lab.body_table(spec, value=lab), lambda: lab.body_table(spec, value=p, want=('dense',))):
            with pytest.raises(ValueError):
                bad()
    finally:
        eng.close()


@pytest.fixture(scope='module')
def product_file(tmp_path_factory):
    """The multi-band product file of the suite's own synthetic product run (tools/make_synthetic_hls.py, 301 x 301)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    from proteus_amd import dswx_hls
    tmp = tmp_path_factory.mktemp('body_product')
    _, files, _, _ = synth_hls.make(str(tmp), size=301, tile=4)
    out = str(tmp / 'product.tif')
    assert dswx_hls.generate_dswx_layers(files, out) is True
    return out


def test_the_command_line_tool_writes_the_table(product_file, tmp_path, capsys):
    """bin/dswx_bodies.py --table: one CSV line per body kept by --min-size, equal to the host statement's rows; areas in
    square metres and map coordinates from the file's geotransform; the JSON line is what it is without --table."""
    spec = importlib.util.spec_from_file_location('dswx_bodies_tool', os.path.join(ROOT, 'bin', 'dswx_bodies.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    bands, info = geotiff.read_geotiff(product_file)
    wtr = bands[0] if bands.ndim == 3 else bands
    H, W = wtr.shape
    gt = tuple(float(v) for v in info.geotransform)
    for flags, min_size, conn, cap in (([], 5, 8, None), (['--connectivity', '4'], 2, 4, 7)):
        out, table = str(tmp_path / f'sieved{min_size}.tif'), str(tmp_path / f'bodies{min_size}.csv')
        capsys.readouterr()
        assert tool.main(flags + ['--min-size', str(min_size), '-o', out, product_file]) == 0
        plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        extra = ['--max-bodies', str(cap)] if cap is not None else []
        assert tool.main(flags + extra + ['--min-size', str(min_size), '-o', out, '--table', table, product_file]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == plain
        label = _capi.label_host(wtr[None], wtr_label_spec(min_size, connectivity=conn), want=('label',))['label']
        K = int(B.bodies_of(label)[0])
        assert K == plain['bodies'] and K > 7
        rows = _capi.body_table_host(label, wtr[None], wtr_body_spec(K if cap is None else cap))['rows'].view(ROW_DTYPE)[0, :, 0]
        kept = [(k, r) for k, r in enumerate(rows) if r['area'] >= min_size]
        with open(table, newline='') as f:
            lines = list(csv.DictReader(f))
        assert len(lines) == len(kept) and (cap is not None or len(kept) == plain['bodies_kept'])
        for line, (k, r) in zip(lines, kept):
            a = int(r['area'])
            assert (int(line['rank']), int(line['label']), int(line['first_x']), int(line['first_y'])) == (k, r['label'], (r['label'] - 1) % W, (r['label'] - 1) // W)
            assert (int(line['area_px']), int(line['perimeter_edges']), int(line['open_px']), int(line['partial_px'])) == (a, r['perimeter'], r['count'][0], r['count'][1])
            assert [int(line[c]) for c in ('x_min', 'x_max', 'y_min', 'y_max')] == [r['x_min'], r['x_max'], r['y_min'], r['y_max']]
            cx, cy = int(r['sum_x']) / a, int(r['sum_y']) / a
            assert float(line['centroid_x_px']) == cx and float(line['centroid_y_px']) == cy
            assert float(line['area_m2']) == a * abs(gt[1] * gt[5]) and float(line['perimeter_m']) == int(r['perimeter']) * (abs(gt[1]) + abs(gt[5])) / 2
            assert float(line['centroid_map_x']) == gt[0] + (cx + 0.5) * gt[1] and float(line['centroid_map_y']) == gt[3] + (cy + 0.5) * gt[5]
            assert float(line['map_x_min']) == gt[0] + int(r['x_min']) * gt[1] and float(line['map_x_max']) == gt[0] + (int(r['x_max']) + 1) * gt[1]
            assert float(line['map_y_max']) == gt[3] + int(r['y_min']) * gt[5] and float(line['map_y_min']) == gt[3] + (int(r['y_max']) + 1) * gt[5]
    assert tool.main(['--min-size', '3', '--max-bodies', '-1', '--table', str(tmp_path / 'no.csv'), '-o', str(tmp_path / 'no.tif'), product_file]) == 1
    assert not os.path.exists(str(tmp_path / 'no.csv'))


def test_body_example_runs(tmp_path):
    """examples/batch_bodies.c: its own checks (exit status 0: every row of the device against its loop over the downloaded
    label and WTR planes and against dswx_body_table_host)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_bodies')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_bodies.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '3', '301'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr bodies: device, loop and host entry agree in every row' in r.stdout
    assert '3 tiles of 301 x 301 pixels' in r.stdout
