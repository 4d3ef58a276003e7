"""The label entries on the GPU: dswx_label_device and dswx_batch_label bit for bit against the library's scalar statement
(dswx_label_host, which tests/test_label.py pins to the numpy statement and to scipy) on all four outputs -- heights and widths
either side of the rectangle one workgroup labels in LDS and of a 16-byte load, every pattern of tests/_label_cases.py at
each, both connectivities, the plane at odd addresses, padded strides, every legal subset of the outputs, with every byte
outside the output planes checked; the deepest chains across seams; more tiles than grid.y has blocks; a caller's stream with the outputs reused; every form of
batch; the results as device planes; the summary against counts made another way; bin/dswx_bodies.py; the C example."""
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
from proteus_amd.checksum import checksum
from proteus_amd.label import SUMMARY_WORDS, Spec, label_tiles, summary_of, wtr_label_spec
from proteus_amd.synth import SEED
from tests import _label_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, CW = _capi.LABEL_RECT_H, _capi.LABEL_RECT_W    # the rectangle of a workgroup
PAD = 200                                         # every byte of a plane buffer that is not tile data: a MEMBER byte of C.plane_of
SENT = 0xEE                                       # every byte of an output buffer beforehand
KEYS = ('label', 'size', 'sieved', 'summary')
SUBSETS = (('label',), ('label', 'size'), KEYS)
GUARD = 512
EB = {'label': 4, 'size': 4, 'sieved': 1, 'summary': 8}


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Run:
    """One call of dswx_label_device.  The plane lies guard | `off` bytes past a 256-byte boundary | guard in `sbuf`, every byte
    that is not tile data PAD; the wanted outputs lie in `obuf`, label and size 4 bytes, sieved 1 byte and summary 8 bytes past
    a 16-byte boundary, every byte SENT beforehand."""

    def __init__(self, ctx, tiles, spec, stride=None, off=0, want=KEYS, sbuf=None, obuf=None):
        self.ctx, self.tiles, self.spec, self.want = ctx, tiles, spec, want
        self.T, self.H, self.W = tiles.shape
        n = self.H * self.W
        self.stride = n if stride is None else stride
        span = (self.T - 1) * self.stride + n if self.T else 0          # the last tile's padding need not exist
        self.start = GUARD + off
        self.shost = np.full(self.start + span + GUARD, PAD, dtype=np.uint8)
        for t in range(self.T):
            self.shost[self.start + t * self.stride:self.start + t * self.stride + n] = tiles[t].reshape(-1)
        self.sbuf = sbuf if sbuf is not None else ctx.malloc(self.shost.size)
        assert self.sbuf.nbytes >= self.shost.size and self.sbuf.ptr % 256 == 0
        self.sbuf.upload(self.shost)
        self.count = {k: self.T * (SUMMARY_WORDS if k == 'summary' else n) for k in KEYS}
        self.where, cursor = {}, 0
        for k in KEYS:
            begin = -(-cursor // 16) * 16 + EB[k]
            self.where[k] = begin
            cursor = begin + self.count[k] * EB[k] + 16
        self.osize = cursor + 16
        self.obuf = obuf if obuf is not None else ctx.malloc(self.osize)
        assert self.obuf.nbytes >= self.osize and self.obuf.ptr % 16 == 0
        self.poison()
        self.out = _capi.LabelOut.of(**{k: self.obuf.ptr + self.where[k] for k in want})

    def poison(self):
        self.obuf.upload(np.full(self.osize, SENT, dtype=np.uint8))

    def run(self, stream=None):
        self.ctx.label_device(self.sbuf.ptr + self.start, self.spec, self.T, self.H, self.W, self.out,
                              tile_stride=0 if self.stride == self.H * self.W else self.stride, stream=stream)

    def check(self, what, ref=None):
        """The wanted planes are the host entry's, every other byte of the output buffer is still SENT, and the plane buffer is
        what was uploaded."""
        ref = _capi.label_host(self.tiles, self.spec) if ref is None else ref
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for k in self.want:
            begin, nb = self.where[k], self.count[k] * EB[k]
            got = raw[begin:begin + nb].copy().view(_capi.LABEL_DTYPES[k])
            want = ref[k].reshape(-1)
            assert np.array_equal(got, want), (what, k, np.flatnonzero(got != want)[:6], got[got != want][:6], want[got != want][:6])
            written[begin:begin + nb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted planes were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.array_equal(self.sbuf.download(np.uint8, self.shost.size), self.shost), (what, 'the plane was written')
        return ref


HEIGHTS = (1, 2, R - 1, R, R + 1, 2 * R + 1)
WIDTHS = (1, 15, 16, 17, CW - 1, CW, CW + 1, 2 * CW + 1)


@pytest.mark.parametrize('W', WIDTHS)
def test_device_entry_against_the_host_entry_every_pattern_height_address_and_subset(ctx, W):
    """This width x heights {1, 2, R - 1, R, R + 1, 2R + 1} x both connectivities; the tiles of a call are the patterns of
    tests/_label_cases.py (empty, full, one pixel, checkerboard, diagonals, spiral, serpentine, corner touch, row wrap, noise at
    four densities, and one more of noise); each with the plane 0, 1 and 3 bytes past a 256-byte
    boundary, the stride equal to the raster and 5 above it with padding and guards full of a MEMBER byte, and label alone,
    label + size and all four outputs; min_size cycles through 1, 2, 5 and the largest size + 1."""
    rng = np.random.default_rng(9100 + W)
    T = 15
    big = max(HEIGHTS) * W
    sbuf = ctx.malloc(2 * GUARD + 256 + T * (big + 5))
    obuf = ctx.malloc(T * (9 * big + 8 * SUMMARY_WORDS) + 256)
    cases = 0
    for H in HEIGHTS:
        members = np.stack(list(C.patterns(H, W, rng).values()))
        plane, table = C.plane_of(members, rng)
        extra, _ = C.plane_of(C.noise(H, W, 0.6, rng)[None], rng)
        tiles = np.concatenate([plane, extra])
        assert tiles.shape == (T, H, W)
        for conn in (4, 8):
            spec = Spec(conn, (1, 2, 5, H * W + 1)[cases % 4], table, replace=(0, 77, 255)[cases % 3])
            ref = _capi.label_host(tiles, spec)
            for off in (0, 1, 3):
                for want in SUBSETS:
                    r = Run(ctx, tiles, spec, stride=H * W + (0 if off == 0 else 5), off=off, want=want, sbuf=sbuf, obuf=obuf)
                    r.run()
                    ctx.synchronize()
                    r.check((H, W, conn, off, want, spec.min_size), ref=ref)
            info = ctx.last_kernel_info()
            assert 'dswx_label_local_k' in info and f'rect={R}x{CW}' in info and f'connectivity={conn}' in info, info
            cases += 1
    sbuf.free()
    obuf.free()


def test_a_table_where_only_byte_255_is_a_member(ctx):
    rng = np.random.default_rng(9150)
    plane, table = C.plane_of(np.stack([C.noise(R + 3, CW + 9, d, rng) for d in C.DENSITIES]), rng, only_255=True)
    for conn in (4, 8):
        r = Run(ctx, plane, Spec(conn, 3, table, replace=254), stride=plane[0].size + 7, off=1)
        r.run()
        ctx.synchronize()
        ref = r.check(('only 255', conn))
        assert np.array_equal(ref['label'] != 0, plane == 255)
        r.sbuf.free()
        r.obuf.free()


@pytest.mark.parametrize('conn', [4, 8])
def test_300_x_470_with_three_tiles(ctx, conn):
    """Several rectangles in both directions with ragged last ones: noise at the percolation threshold (bodies that wander
    across many seams), a serpentine and a spiral; every address and subset; min_size the largest size and one above it."""
    rng = np.random.default_rng(9200 + conn)
    H, W = 300, 470
    members = np.stack([C.noise(H, W, 0.593, rng), C.serpentine(H, W), C.spiral(H, W)])
    tiles, table = C.plane_of(members, rng)
    ref = _capi.label_host(tiles, Spec(conn, 1, table))
    largest = int(ref['summary'][0, 2])
    assert largest > 1 and ref['summary'][1, 0] == 1 and ref['summary'][2, 0] == 1
    sbuf = ctx.malloc(2 * GUARD + 8 + 3 * (H * W + 5))
    r = None
    for min_size, off in ((largest, 0), (largest + 1, 1), (2, 3)):
        spec = Spec(conn, min_size, table, replace=9)
        ref = _capi.label_host(tiles, spec)
        for want in SUBSETS:
            r = Run(ctx, tiles, spec, stride=H * W + 5, off=off, want=want, sbuf=sbuf, obuf=r.obuf if r else None)
            r.run()
            ctx.synchronize()
            r.check((conn, min_size, off, want), ref=ref)
        if min_size > 2:                                             # at the largest size of tile 0 it stays; one above, nothing does
            assert (ref['summary'][0, 4] >= 1) == (min_size == largest) and (ref['summary'][0, 4] == 0) == (min_size == largest + 1)
    sbuf.free()
    r.obuf.free()


@pytest.fixture(scope='module')
def deep_chains():
    """The 1024 x 1024 spiral and serpentine (one call, two tiles) and the host entry's planes for both connectivities."""
    rng = np.random.default_rng(9300)
    tiles, table = C.plane_of(np.stack([C.spiral(1024, 1024), C.serpentine(1024, 1024)]), rng)
    return tiles, table, {conn: _capi.label_host(tiles, Spec(conn, 1000, table, replace=3)) for conn in (4, 8)}


@pytest.mark.parametrize('conn', [4, 8])
def test_the_deepest_chains_across_seams_1024_x_1024_spiral_and_serpentine(ctx, deep_chains, conn):
    tiles, table, refs = deep_chains
    r = Run(ctx, tiles, Spec(conn, 1000, table, replace=3), off=1)
    r.run()
    ctx.synchronize()
    ref = r.check(('deep', conn), ref=refs[conn])
    for t in range(2):                                              # ONE body from pixel 0 that holds every member
        assert ref['summary'][t, 0] == 1 and ref['summary'][t, 3] == 1 and ref['summary'][t, 2] == ref['summary'][t, 1] == np.count_nonzero(ref['label'][t])
    r.sbuf.free()
    r.obuf.free()


def test_on_a_callers_stream_twice_with_the_same_outputs(ctx):
    """On a caller's stream, and a second call on the same stream that reuses the outputs of the first as they are (full of
    the first call's labels, sizes and summary): nothing depends on what the outputs held beyond the entry's own memset."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(9400)
    H, W = 2 * R + 1, 2 * CW + 1
    first, table = C.plane_of(np.stack([C.full(H, W), C.noise(H, W, 0.593, rng), C.checkerboard(H, W)]), rng)
    second, _ = C.plane_of(np.stack([C.noise(H, W, 0.5, rng), C.serpentine(H, W), C.empty(H, W)]), rng)
    s = torch.cuda.Stream(device=0)
    for conn in (4, 8):
        spec = Spec(conn, 4, table, replace=0)
        r = Run(ctx, first, spec, stride=H * W + 5, off=3)
        r.run(stream=s.cuda_stream)
        ctx.synchronize(s.cuda_stream)
        r.check(('first', conn))
        r.tiles = second                                             # the same buffers, another plane, the outputs NOT poisoned again
        for t in range(3):
            r.shost[r.start + t * r.stride:r.start + t * r.stride + H * W] = second[t].reshape(-1)
        r.sbuf.upload(r.shost)
        r.run(stream=s.cuda_stream)
        r.run(stream=s.cuda_stream)
        ctx.synchronize(s.cuda_stream)
        r.check(('second', conn))
        r.sbuf.free()
        r.obuf.free()


def test_the_result_of_tile_0_does_not_depend_on_the_number_of_tiles(ctx):
    """There is no switch for the launch geometry, so: the planes of tile 0 are the same bytes whether the call has 1 tile or
    7 (grid.y and the number of workgroups in flight differ), run three times each."""
    rng = np.random.default_rng(9500)
    H, W = 3 * R + 5, 3 * CW + 7
    tiles, table = C.plane_of(np.stack([C.noise(H, W, 0.593, rng)] + [C.noise(H, W, d, rng) for d in (0.1, 0.5, 0.593, 0.9, 0.6, 0.55)]), rng)
    spec = Spec(8, 6, table, replace=1)
    seen = set()
    for T in (1, 7, 1, 7, 7, 1):
        r = Run(ctx, tiles[:T], spec)
        r.run()
        ctx.synchronize()
        raw = r.obuf.download(np.uint8, r.osize)
        seen.add(tuple(checksum(raw[r.where[k]:r.where[k] + (SUMMARY_WORDS if k == 'summary' else H * W) * EB[k]].copy()) for k in KEYS))
        r.sbuf.free()
        r.obuf.free()
    assert len(seen) == 1
    ref = _capi.label_host(tiles[:1], spec)
    assert seen == {tuple(checksum(ref[k].view(np.uint8).reshape(-1)) for k in KEYS)}


@pytest.mark.parametrize('H,W', [(2, 3), (R + 1, 2), (2, CW + 1)], ids=['one_rectangle', 'horizontal_seam', 'vertical_seam'])
def test_a_workgroup_labels_a_second_tile_past_the_blocks_of_grid_y(ctx, H, W):
    """65535 + 4 tiles: grid.y is 65535, and the workgroups of tiles 0 .. 3 walk on to tiles 65535 .. 65538 with the `lab` /
    `msk` of dswx_label_local_k and the `part` of dswx_label_finish_k as the first tile left them.  The first four tiles are
    dense (full, noise 0.9, checkerboard, serpentine), the last four sparse (empty, one pixel, noise 0.1, row wrap), the rest
    noise.  2 x 3: one rectangle, loaded byte by byte, no seam launch; (R + 1) x 2: a horizontal seam; 2 x (CW + 1): a
    vertical seam and a ragged last 16-byte segment.  Both connectivities, all four outputs of EVERY tile against the host
    entry, min_size 2 (sieved changes bytes), the stride 5 above the raster, the plane one byte past a 256-byte boundary,
    padding and guards full of a member byte; every byte outside the outputs checked."""
    rng = np.random.default_rng(9550 + H + W)
    members = C.second_pass_members(H, W, rng)
    T = len(members)
    assert T == 65535 + 4
    for i in range(4):
        assert not np.array_equal(members[65535 + i], members[i]), (C.LATE[i], C.EARLY[i])
    tiles, table = C.plane_of(members, rng)
    r = None
    for conn in (4, 8):
        spec = Spec(conn, 2, table, replace=77)
        ref = _capi.label_host(tiles, spec)
        assert np.count_nonzero(ref['sieved'] != tiles) > T // 8           # (single pixels are common in the noise)
        assert not ref['summary'][65535].any() and ref['summary'][0, 0] == 1 and ref['summary'][0, 2] == H * W
        r = Run(ctx, tiles, spec, stride=H * W + 5, off=1, sbuf=r.sbuf if r else None, obuf=r.obuf if r else None)
        r.run()
        ctx.synchronize()
        info = ctx.last_kernel_info()
        assert info.count(',65535,1)') == 2 and f'connectivity={conn}' in info, info
        assert ('pixels=0 ' in info) == ((H, W) == (2, 3)), info
        r.check((H, W, conn), ref=ref)
    r.sbuf.free()
    r.obuf.free()


def test_summary_words_0_and_1_counted_another_way(ctx):
    """Consistency without an oracle.  Word 1 (member pixels) is the plane's histogram -- dswx_histogram_device on the same
    bytes -- folded through the member table, and the histogram of `sieved` loses exactly the pixels of the small bodies.
    Word 0 (bodies) is the number of pixels with label == idx + 1 and word 1 also the number with label != 0: the compare
    and histogram entries have no uint32 kind, so these two are counted from the downloaded label plane."""
    rng = np.random.default_rng(9600)
    H, W, T = 2 * R + 3, 2 * CW + 5, 4
    tiles, table = C.plane_of(np.stack([C.noise(H, W, d, rng) for d in C.DENSITIES]), rng)
    spec = Spec(4, 3, table, replace=253)
    r = Run(ctx, tiles, spec)
    r.run()
    hist = ctx.malloc(2 * T * 256 * 8)
    ctx.histogram_device(r.sbuf.ptr + r.start, _capi.HIST_U8, T, H * W, hist.ptr)
    ctx.histogram_device(r.obuf.ptr + r.where['sieved'], _capi.HIST_U8, T, H * W, hist.ptr + T * 256 * 8)
    ctx.synchronize()
    bins = hist.download(np.uint64, 2 * T * 256).reshape(2, T, 256)
    summary = r.obuf.download(np.uint64, T * SUMMARY_WORDS, r.where['summary']).reshape(T, SUMMARY_WORDS)
    label = r.obuf.download(np.uint32, T * H * W, r.where['label']).reshape(T, H * W)
    size = r.obuf.download(np.uint32, T * H * W, r.where['size']).reshape(T, H * W)
    member = table != 0
    for t in range(T):
        assert summary[t, 1] == bins[0, t, member].sum() == np.count_nonzero(label[t])
        assert summary[t, 0] == np.count_nonzero(label[t] == np.arange(1, H * W + 1))
        assert summary[t, 0] == summary[t, 8:].sum() and summary[t, 6] == summary[t, 7] == 0
        assert summary[t, 1] - summary[t, 5] == bins[0, t, member].sum() - bins[1, t, member].sum()      # 253 is no member byte
        assert summary[t, 2] == size[t].max() and summary[t, 3] == label[t][np.argmax(size[t])]
    assert np.array_equal(summary, summary_of(label.reshape(T, H, W), size.reshape(T, H, W), spec))
    r.check('counted another way')
    hist.free()
    r.sbuf.free()
    r.obuf.free()


def test_refusals_write_nothing(ctx):
    rng = np.random.default_rng(9700)
    tiles, table = C.plane_of(rng.random((2, 20, 30)) < 0.5, rng)
    spec = Spec(8, 2, table)
    r = Run(ctx, tiles, spec)
    plane = r.sbuf.ptr + r.start
    lib, h = ctx.lib, ctx.handle

    def call(plane=plane, cspec=_capi.LabelSpec.of(spec), n=2, H=20, W=30, stride=0, out=r.out, handle=h):
        return lib.dswx_label_device(handle, ctypes.c_void_p(plane), ctypes.byref(cspec) if cspec is not None else None, n, H, W,
                                     stride, ctypes.byref(out) if out is not None else None, None)

    def cs(**kw):
        c = _capi.LabelSpec.of(spec)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def outs(**kw):
        o = _capi.LabelOut.of(**{k: r.obuf.ptr + r.where[k] for k in KEYS})
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    A, L = _capi.ERR_ARG, _capi.ERR_ALIGN
    for rc, kw in ((A, {'cspec': None}), (A, {'out': None}), (A, {'cspec': cs(connectivity=6)}), (A, {'cspec': cs(connectivity=0)}),
                   (A, {'cspec': cs(replace=256)}), (A, {'cspec': cs(replace=-1)}), (A, {'cspec': cs(min_size=0)}),
                   (A, {'n': -1}), (A, {'H': -1}), (A, {'W': -1}), (A, {'stride': -1}), (A, {'stride': 599}),
                   (A, {'H': 1 << 16, 'W': (1 << 15) + 1}), (A, {'plane': None}), (A, {'out': outs(label=None)}),
                   (A, {'out': outs(size=None)}), (A, {'out': outs(size=None, sieved=None)}), (A, {'out': outs(size=None, summary=None)}),
                   (L, {'out': outs(label=r.out.label + 2)}), (L, {'out': outs(size=r.out.size + 1)}),
                   (L, {'out': outs(summary=r.out.summary + 4)}), (A, {'handle': None})):
        assert call(**kw) == rc, (kw, lib.dswx_last_error())
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    # arguments before the context: a bad spec AND no context names the spec
    assert call(cspec=cs(connectivity=5), handle=None) == A and 'connectivity' in lib.dswx_last_error().decode()
    # an empty raster and no tiles are legal and write nothing
    for kw in ({'n': 0}, {'H': 0}, {'W': 0}):
        assert call(**kw) == 0, kw
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    r.run()
    ctx.synchronize()
    r.check('after the refusals')
    r.sbuf.free()
    r.obuf.free()


def download(res, n_tiles, h, w):
    got = {k: res[k].download(_capi.LABEL_DTYPES[k], n_tiles * (SUMMARY_WORDS if k == 'summary' else h * w)) for k in res}
    for k in got:
        got[k] = got[k].reshape((n_tiles, SUMMARY_WORDS) if k == 'summary' else (n_tiles, h, w))
    return got


FORMS = {'packed': {}, 'slide_placed': {'sliding_outputs': True}, 'contiguous': {'tile_align': 1}}


@pytest.mark.parametrize('form', list(FORMS))
def test_batch_label_on_the_wtr_plane_of_a_classified_batch(ctx, form):
    """The WTR plane of a classified packed, placed and contiguous batch: every tile, tile ranges with tile0 > 0,
    DSWX_BATCH_ALL_TILES; the results checked by CHECKSUMS made on the device against the checksums of the host statement, so
    that no result plane is downloaded; DIAG, a band, the counters, a missing plane and ranges outside the batch refused."""
    n_tiles, h, w = 4, 2 * R + 9, CW + 37
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w, **FORMS[form])
    sums = ctx.malloc(8 * n_tiles)
    try:
        batch.synth(SEED, tile0=31)
        p = _capi.default_params()
        if form == 'slide_placed':
            batch.place_slide(p, slack_bytes=24 << 20, step_bytes=2 << 20, spread_gaps=2, refine_passes=1, launches=2, keep_free_bytes=0)
        batch.classify(p)
        tiles = np.stack([batch.read_tile('wtr', t) for t in range(n_tiles)])
        for spec in (wtr_label_spec(3), wtr_label_spec(2, connectivity=4, partial_is_water=False)):
            ref = _capi.label_host(tiles, spec)
            assert ref['summary'][:, 0].min() > 1                     # the layer has water bodies
            for tile0, count in ((0, None), (1, n_tiles - 1), (2, 1), (1, _capi.BATCH_ALL_TILES), (n_tiles, None), (0, 0)):
                res = batch.label('wtr', spec, tile0=tile0, n_tiles=count)
                assert list(res) == list(KEYS)
                last = tile0 + (n_tiles - tile0 if count in (None, _capi.BATCH_ALL_TILES) else count)
                nt = last - tile0
                for k in KEYS:
                    per = SUMMARY_WORDS if k == 'summary' else h * w
                    if nt:
                        ctx.checksum_device(res[k].ptr, EB[k], nt, per, sums.ptr)
                    ctx.synchronize()
                    got = sums.download(np.uint64, nt) if nt else np.zeros(0, dtype=np.uint64)
                    want = [checksum(ref[k][t].reshape(-1)) for t in range(tile0, last)]
                    assert got.tolist() == want, (form, k, tile0, count)
                for b in res.values():
                    b.free()
            res = batch.label('wtr', spec, want=('label',))
            ctx.synchronize()
            assert list(res) == ['label'] and np.array_equal(download(res, n_tiles, h, w)['label'], ref['label'])
            res['label'].free()
        spec = wtr_label_spec(3)
        for name in ('blue', 'swir2', 'diag'):
            with pytest.raises(_capi.DswxError, match=r'band\[|diag') as e:
                batch.label(name, spec)
            assert e.value.code == _capi.ERR_ARG and 'uint8' in str(e.value)
        with pytest.raises(_capi.DswxError, match='counters') as e:
            batch.label('counters', spec)
        assert e.value.code == _capi.ERR_ARG
        for name in ('land', 'browse'):
            with pytest.raises(_capi.DswxError, match=name) as e:
                batch.label(name, spec)
            assert e.value.code == _capi.ERR_ARG and 'no plane' in str(e.value)
        for bad in ((0, n_tiles + 1), (-1, 2), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError, match='outside the batch'):
                batch.label('wtr', spec, tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(ValueError):
            batch.label('water', spec)
    finally:
        sums.free()
        batch.free()


def test_device_plane_label_feeds_histogram_checksum_and_grid(ctx):
    """DevicePlane.label, and its results as planes like any other: the sieved plane histogrammed and gridded on the device,
    label and size checksummed, with no download in between."""
    from proteus_amd.grid import grid_tiles, wtr_grid_spec
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9800)
    try:
        a = rng.choice(np.array([0, 1, 2, 252, 253, 255], dtype=np.uint8), size=(3, R + 20, CW + 30), p=[0.4, 0.3, 0.1, 0.05, 0.1, 0.05])
        p = eng.upload(a)
        spec = wtr_label_spec(4)
        want = label_tiles(a, spec)
        got = p.label(spec)
        assert list(got) == list(KEYS)
        assert np.array_equal(got['sieved'].histogram(), np.bincount(want['sieved'].reshape(-1), minlength=256).astype(np.uint64))
        assert got['label'].checksum() == checksum(want['label'].reshape(-1)) and got['size'].checksum() == checksum(want['size'].reshape(-1))
        share = got['sieved'].grid(wtr_grid_spec(30), want=('share',))['share']
        assert np.array_equal(share.numpy(), grid_tiles(want['sieved'], wtr_grid_spec(30))['share'])
        assert got['sieved']._host is None and got['label']._host is None
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k].numpy(), want[k]), k
        only = p.label(spec, want=('label',))
        assert list(only) == ['label'] and np.array_equal(only['label'].numpy(), want['label'])
        one = eng.upload(a[0]).label(spec, want=('summary',))
        assert list(one) == ['label', 'size', 'summary'] and np.array_equal(one['summary'].numpy(), want['summary'][:1])
        with pytest.raises(ValueError):
            eng.upload(np.zeros((4,), dtype=np.uint8)).label(spec)
        with pytest.raises(ValueError):
            eng.upload(np.zeros((2, 4, 4), dtype=np.uint16)).label(spec)
    finally:
        eng.close()


@pytest.fixture(scope='module')
def product_file(tmp_path_factory):
    """The multi-band product file of the suite's own synthetic product run (tools/make_synthetic_hls.py, 301 x 301)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    from proteus_amd import dswx_hls
    tmp = tmp_path_factory.mktemp('label_product')
    _, files, _, _ = synth_hls.make(str(tmp), size=301, tile=4)
    out = str(tmp / 'product.tif')
    assert dswx_hls.generate_dswx_layers(files, out) is True
    return out


def test_the_command_line_tool(product_file, tmp_path, capsys):
    """bin/dswx_bodies.py on a product file: the JSON is the host statement's summary of band 1, the output a Byte COG that
    holds the host statement's sieved plane and passes the COG validator."""
    spec = importlib.util.spec_from_file_location('dswx_bodies_tool', os.path.join(ROOT, 'bin', 'dswx_bodies.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    bands, info = geotiff.read_geotiff(product_file)
    wtr = bands[0] if bands.ndim == 3 else bands
    for flags, min_size, conn in (([], 5, 8), (['--connectivity', '4'], 2, 4)):
        out = str(tmp_path / f'sieved{min_size}.tif')
        capsys.readouterr()
        assert tool.main(flags + ['--min-size', str(min_size), '-o', out, product_file]) == 0
        said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        ref = _capi.label_host(wtr[None], wtr_label_spec(min_size, connectivity=conn))
        s = ref['summary'][0]
        assert (said['bodies'], said['member_pixels'], said['largest_size'], said['largest_label']) == tuple(int(v) for v in s[:4])
        assert (said['bodies_kept'], said['pixels_kept'], said['min_size'], said['connectivity']) == (int(s[4]), int(s[5]), min_size, conn)
        assert said['bodies_by_log2_size'] == [int(v) for v in s[8:]] and said['bodies'] > 1
        gt = tuple(info.geotransform)
        assert said['pixel_area_m2'] == abs(gt[1] * gt[5]) and said['largest_area_m2'] == int(s[2]) * said['pixel_area_m2']
        arr, meta = geotiff.read_geotiff(out)
        assert arr.dtype == np.uint8 and np.array_equal(arr, ref['sieved'][0])
        assert geotiff.validate_cog(out) == []
        assert tuple(meta.geotransform) == gt and meta.nodata == 255
    capsys.readouterr()
    assert tool.main(['--min-size', '0', '-o', str(tmp_path / 'no.tif'), product_file]) == 1
    assert tool.main(['--min-size', '3', '--band', '99', '-o', str(tmp_path / 'no.tif'), product_file]) == 1
    assert tool.main(['--min-size', '3', '-o', str(tmp_path / 'no.tif'), str(tmp_path / 'missing.tif')]) == 1
    assert not os.path.exists(str(tmp_path / 'no.tif'))


def test_label_example_runs(tmp_path):
    """examples/batch_label.c: its own checks (exit status 0: label, size, sieved and summary of the device against its loop
    over the downloaded layer and against dswx_label_host)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_label')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_label.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '3', '301'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr label: device, loop and host entry agree in every pixel' in r.stdout
    assert '3 tiles of 301 x 301 pixels' in r.stdout
