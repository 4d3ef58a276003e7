"""The outline entry on the GPU: dswx_outline_device byte for byte against the library's scalar walk (dswx_outline_host, which
tests/test_outline.py pins to the numpy statement, to scipy and to matplotlib) -- every pattern of tests/_outline_cases.py
labelled with 4 and with 8 and outlined with both connectivities at every shape, arbitrary uint32 planes, a ring longer than
the scan chunk, edge counts around the chunk, more chunks than one step of the scan, capacities either side of E and R, the
counting call, more tiles than grid.y has blocks, a caller's stream with the outputs reused, the body table of the same plane,
refusals, the DevicePlane and DeviceBatch chains, bin/dswx_outline.py and the C example.  Every byte of every output of every
tile is compared, and every byte outside the outputs checked."""
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
from proteus_amd.bodies import ROW_DTYPE as BODY_ROW, Spec as BodySpec, wtr_body_spec
from proteus_amd.checksum import checksum
from proteus_amd.label import wtr_label_spec
from proteus_amd.outline import ROW_DTYPE, Spec, outline_tiles, polygons
from proteus_amd.synth import SEED
from tests import _body_cases as B
from tests import _label_cases as C
from tests import _outline_cases as OC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK, STEP = _capi.BODY_CHUNK, _capi.BODY_SCAN_STEP
RW, HW = _capi.OUTLINE_ROW_WORDS, _capi.OUTLINE_HEAD_WORDS
SENT = 0xEE                                       # every byte of an output buffer, and of the working memory, beforehand
GUARD = 512
KEYS = ('chain', 'rings', 'head')
EB = {'chain': 4, 'rings': 4, 'head': 8}
OFF = {'chain': 4, 'rings': 12, 'head': 8}        # past a 16-byte boundary: the least alignment the entry accepts


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Run:
    """One call of dswx_outline_device.  The id plane lies guard | 4 bytes past a 256-byte boundary | guard in `ibuf`; the
    wanted outputs lie in `obuf`, chain 4, rings 12 and head 8 bytes past a 16-byte boundary, every byte SENT beforehand; the
    working memory lies 8 bytes past a 16-byte boundary in `wbuf` between guards."""

    def __init__(self, ctx, ids, spec, want=KEYS, bufs=None):
        self.ctx, self.ids, self.spec = ctx, ids, spec
        self.want = tuple(k for k in want if k != 'rings' or spec.max_rings > 0)
        self.T, self.H, self.W = ids.shape
        self.istart = GUARD + 4
        self.ihost = np.full(self.istart + 4 * ids.size + GUARD, SENT, dtype=np.uint8)
        self.ihost[self.istart:self.istart + 4 * ids.size] = ids.reshape(-1).view(np.uint8)
        self.count = {'chain': self.T * spec.max_edges, 'rings': self.T * spec.max_rings * RW, 'head': self.T * HW}
        self.where, cursor = {}, 0
        for k in KEYS:
            begin = -(-cursor // 16) * 16 + OFF[k]
            self.where[k] = begin
            cursor = begin + self.count[k] * EB[k] + 16
        self.osize = cursor + 16
        self.work_bytes = _capi.outline_work_bytes(spec, self.T, self.H, self.W)
        self.wsize = GUARD + 8 + self.work_bytes + GUARD
        self.own = bufs is None
        self.ibuf, self.obuf, self.wbuf = bufs if bufs else (ctx.malloc(self.ihost.size), ctx.malloc(self.osize), ctx.malloc(self.wsize))
        assert self.ibuf.nbytes >= self.ihost.size and self.obuf.nbytes >= self.osize and self.wbuf.nbytes >= self.wsize
        assert self.ibuf.ptr % 256 == 0 and self.obuf.ptr % 16 == 0 and self.wbuf.ptr % 16 == 0
        self.ibuf.upload(self.ihost)
        self.poison()
        self.out = _capi.OutlineOut.of(**{k: self.obuf.ptr + self.where[k] for k in self.want})

    def poison(self):
        self.obuf.upload(np.full(self.osize, SENT, dtype=np.uint8))
        self.wbuf.upload(np.full(self.wsize, SENT, dtype=np.uint8))

    def run(self, stream=None):
        self.ctx.outline_device(self.ibuf.ptr + self.istart, self.spec, self.T, self.H, self.W, self.out, self.wbuf.ptr + GUARD + 8,
                                self.work_bytes, stream=stream)

    def host(self):
        return _capi.outline_host(self.ids, self.spec, self.want)

    def get(self, k):
        return self.obuf.download(_capi.OUTLINE_DTYPES[k], self.count[k], self.where[k])

    def check(self, what, ref=None):
        """The wanted outputs are the host entry's, every other byte of the output buffer is still SENT, the guards of the
        working memory are untouched and the id plane is what was uploaded."""
        ref = self.host() if ref is None else ref
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for k in self.want:
            begin, nb = self.where[k], self.count[k] * EB[k]
            got = raw[begin:begin + nb].copy().view(_capi.OUTLINE_DTYPES[k])
            want = ref[k].reshape(-1)
            assert np.array_equal(got, want), (what, k, np.flatnonzero(got != want)[:6], got[got != want][:6], want[got != want][:6])
            written[begin:begin + nb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted outputs were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.all(self.wbuf.download(np.uint8, GUARD + 8) == SENT), (what, 'below the working memory')
        assert np.all(self.wbuf.download(np.uint8, GUARD, GUARD + 8 + self.work_bytes) == SENT), (what, 'above the working memory')
        assert np.array_equal(self.ibuf.download(np.uint8, self.ihost.size), self.ihost), (what, 'the id plane was written')
        return ref

    def free(self):
        for b in (self.ibuf, self.obuf, self.wbuf):
            b.free()


def once(ctx, ids, spec, what, **kw):
    r = Run(ctx, ids, spec, **kw)
    r.run()
    ctx.synchronize()
    ref = r.check(what)
    r.free()
    return ref


@pytest.mark.parametrize('H,W', OC.SHAPES)
def test_device_entry_against_the_host_entry_every_pattern_and_connectivity(ctx, H, W):
    """One shape: empty, one id, one pixel, checkerboard, frame, nested rings, comb, spiral and noise at 0.3, 0.5 and 0.7,
    labelled by dswx_label_host with 4 and with 8, then two planes of arbitrary uint32; each outlined with both
    connectivities (the crossed combinations included), capacities with room to spare."""
    rng = np.random.default_rng(9100 + 131 * H + W)
    names, members, planes = OC.id_planes(H, W, rng)
    for label_conn in (4, 8):
        ids = planes[label_conn]
        for conn in (4, 8):
            spec = OC.full_spec(ids, conn)
            ref = once(ctx, ids, spec, (H, W, label_conn, conn))
            head = ref['head']
            assert np.all(head[:, 7] == 0) and np.array_equal(head[:, 0], OC.edges_of(ids)) and np.array_equal(head[:, 3], head[:, 0])
            assert head[names.index('empty')].tolist() == [0] * HW
            full = ref['rings'][names.index('full'), 0].view(ROW_DTYPE)[0]
            assert (full['id'], full['start'], full['offset'], full['length'], full['corners'], full['area2']) == (1, 0, 0, 2 * (H + W), 4, 2 * H * W)
            if label_conn == conn:                           # a ring of positive area per body, started at the body's first pixel
                K = B.bodies_of(ids[:len(members)])
                assert np.array_equal(head[:len(members), 4], K)
    info = ctx.last_kernel_info()
    assert 'dswx_outline_count_k' in info and 'dswx_outline_jump_k x ' in info and f'chunk={CHUNK}' in info, info


def test_a_ring_longer_than_the_scan_chunk(ctx):
    """The 96 x 96 spiral: ONE ring, longer than the 4096 edges of a chunk, so that positions in the ring cross chunks and the
    rounds run to the end; and the comb, whose one ring has as many corners as a ring can."""
    rng = np.random.default_rng(9110)
    ids = B.labels_of(np.stack([C.spiral(96, 96), C.serpentine(96, 96)]), rng, 4)
    for conn in (4, 8):
        ref = once(ctx, ids, OC.full_spec(ids, conn), ('spiral', conn))
        assert ref['head'][:, 1].tolist() == [1, 1] and ref['rings'][0, 0, 3] > CHUNK and ref['rings'][0, 0, 3] == ref['head'][0, 0]


@pytest.mark.parametrize('E', [CHUNK - 4, CHUNK, CHUNK + 4])
def test_edge_counts_around_the_scan_chunk(ctx, E):
    """Isolated pixels at 4 edges each: one chunk of edges less a ring, exactly one chunk, one ring more."""
    ids = OC.isolated(E // 4, 64, 66)[None]
    for conn, cap in ((4, E), (8, E + 5)):
        ref = once(ctx, ids, Spec(cap, E // 4, conn), (E, conn))
        assert ref['head'][0].tolist() == [E, E // 4, E // 4, E, E // 4, 0, E, 0]


def test_more_chunks_than_one_step_of_the_scan(ctx):
    """Isolated pixels on the even coordinates of 1024 x 1026: 262,656 rings and 1,050,624 edges, 257 chunks of edges and 257
    of pixels, more than the 256 that the scan launches take per step."""
    H, W = 1024, 1026
    ids = OC.isolated((H // 2) * (W // 2), H, W)[None]
    E = 4 * (H // 2) * (W // 2)
    assert E == 1050624 and E > STEP * CHUNK and H * W > STEP * CHUNK
    ref = once(ctx, ids, Spec(E, E // 4, 4), 'deep')
    assert ref['head'][0].tolist() == [E, 262656, 262656, E, 262656, 0, E, 0]


def test_capacities_either_side_of_e_and_r_and_the_counting_call(ctx):
    """Three tiles, the middle one with the most edges.  max_edges = E - 1 of the middle tile: that tile is zero with head
    word 7 set, its neighbours are unaffected.  max_rings = R - 1: the rows are truncated, the chain is complete.  max_rings 0
    with rings NULL; head alone with and without capacity: the counting call."""
    rng = np.random.default_rng(9120)
    H, W = 40, 70
    ids = B.labels_of(np.stack([C.noise(H, W, 0.3, rng), C.noise(H, W, 0.55, rng), C.noise(H, W, 0.2, rng)]), rng, 8)
    E = OC.edges_of(ids)
    assert E[1] > E[0] and E[1] > E[2]
    full = once(ctx, ids, Spec(int(E[1]), int(E[1]) // 4, 8), 'full')
    R = full['head'][:, 1]
    short = once(ctx, ids, Spec(int(E[1]) - 1, int(E[1]) // 4, 8), 'E - 1')
    assert short['head'][1].tolist() == [E[1], 0, 0, 0, 0, 0, 0, 1] and not short['chain'][1].any() and not short['rings'][1].any()
    for t in (0, 2):
        assert np.array_equal(short['head'][t], full['head'][t]) and np.array_equal(short['chain'][t], full['chain'][t][:-1])
        assert np.array_equal(short['rings'][t], full['rings'][t])
    cut = once(ctx, ids, Spec(int(E[1]), int(R.max()) - 1, 8), 'R - 1')
    assert np.array_equal(cut['chain'], full['chain']) and np.array_equal(cut['rings'], full['rings'][:, :int(R.max()) - 1])
    assert cut['head'][:, 2].tolist() == [min(int(r), int(R.max()) - 1) for r in R] and np.array_equal(cut['head'][:, [0, 1, 3, 4, 5, 6, 7]], full['head'][:, [0, 1, 3, 4, 5, 6, 7]])
    bare = once(ctx, ids, Spec(int(E[1]), 0, 8), 'no rings', want=('chain', 'head'))
    assert np.array_equal(bare['chain'], full['chain']) and bare['head'][:, 2].tolist() == [0, 0, 0]
    counted = once(ctx, ids, Spec(int(E[1]), 0, 8), 'head alone', want=('head',))
    assert np.array_equal(counted['head'], bare['head'])
    asked = once(ctx, ids, Spec(0, 0, 8), 'the counting call', want=('head',))
    assert asked['head'].tolist() == [[int(e), 0, 0, 0, 0, 0, 0, 1] for e in E]
    only = once(ctx, ids, Spec(int(E[1]), int(R.max()), 8), 'chain and rings', want=('chain', 'rings'))
    assert np.array_equal(only['rings'], full['rings'][:, :int(R.max())])


def test_a_workgroup_outlines_a_second_tile_past_the_blocks_of_grid_y(ctx):
    """65535 + 4 tiles of 2 x 3: grid.y is 65535, and the workgroups of tiles 0 .. 3 walk on to tiles 65535 .. 65538 with their
    shared memory as the first tile left it.  The first four tiles dense, the last four sparse, the rest noise, labelled with
    8 and outlined with 4.  A labelled tile of 2 x 3 has 0, 4, 6, 8, 10 or 12 edges in at most 3 rings: capacity 9 edges and 1
    ring, so that some tiles overflow (the full tile has 10 edges), some are truncated (two pixels apart: 8 edges, 2 rings) and
    some fit."""
    rng = np.random.default_rng(9130)
    ids = B.labels_of(C.second_pass_members(2, 3, rng), rng, 8)
    ids[65536] = rng.integers(0, 1 << 32, size=(2, 3), dtype=np.uint64).astype(np.uint32)
    T = len(ids)
    assert T == 65535 + 4
    spec = Spec(9, 1, 4)
    ref = once(ctx, ids, spec, 'second pass')
    info = ctx.last_kernel_info()
    assert ',65535,1)' in info and 'grid=(65535,1,1)' in info, info
    over, cut = ref['head'][:, 7] == 1, ref['head'][:, 1] > ref['head'][:, 2]
    assert 0 < over.sum() < T and 0 < cut.sum() < T and (~over & ~cut).any()
    for i in range(4):
        assert not np.array_equal(ids[65535 + i], ids[i]), i


def test_on_a_callers_stream_twice_with_the_same_outputs(ctx):
    """On a caller's stream, and a second and third call that reuse the outputs and the working memory of the first as they
    are: nothing depends on what they held."""
    if torch is None:
        pytest.skip('no torch')
    rng = np.random.default_rng(9140)
    H, W = 65, 257
    first = B.labels_of(np.stack([C.full(H, W), C.noise(H, W, 0.593, rng), C.checkerboard(H, W)]), rng, 4)
    second = B.labels_of(np.stack([C.noise(H, W, 0.5, rng), C.serpentine(H, W), C.empty(H, W)]), rng, 4)
    E = int(max(OC.edges_of(first).max(), OC.edges_of(second).max()))
    spec = Spec(E, E // 4, 4)
    s = torch.cuda.Stream(device=0)
    r = Run(ctx, first, spec)
    r.run(stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    r.check('first')
    r.ids = second                                                   # the same buffers, another plane, nothing poisoned again
    r.ihost[r.istart:r.istart + 4 * second.size] = second.reshape(-1).view(np.uint8)
    r.ibuf.upload(r.ihost)
    r.run(stream=s.cuda_stream)
    r.run(stream=s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    r.check('second')
    r.free()


def test_the_result_of_tile_0_does_not_depend_on_the_number_of_tiles(ctx):
    """There is no switch for the launch geometry, so: the bytes of tile 0 are the same whether the call has 1 tile or 5, run
    three times each, by checksums."""
    rng = np.random.default_rng(9150)
    H, W = 101, 291
    ids = B.labels_of(np.stack([C.noise(H, W, d, rng) for d in (0.593, 0.1, 0.5, 0.9, 0.6)]), rng, 8)
    E = int(OC.edges_of(ids).max())
    spec = Spec(E, E // 4, 8)
    per = {'chain': spec.max_edges, 'rings': spec.max_rings * RW, 'head': HW}
    seen = set()
    for T in (1, 5, 1, 5, 5, 1):
        r = Run(ctx, ids[:T], spec)
        r.run()
        ctx.synchronize()
        seen.add(tuple(checksum(r.get(k)[:per[k]].copy().view(np.uint8)) for k in KEYS))
        r.free()
    assert len(seen) == 1
    ref = _capi.outline_host(ids[:1], spec)
    assert seen == {tuple(checksum(ref[k].reshape(-1).view(np.uint8)) for k in KEYS)}


def test_against_the_device_body_table_of_the_same_plane(ctx):
    """Consistency without the host entry: E is the body table's sum of perimeters (head word 4), the outer rings are its K,
    and per body the area2 of its rings sum to twice its area and their lengths to its perimeter -- the `dense` plane of the
    body table as ids, so that a ring's id is a row of the table."""
    rng = np.random.default_rng(9160)
    H, W, T = 67, 261, 3
    for conn in (4, 8):
        label = B.labels_of(np.stack([C.noise(H, W, d, rng) for d in (0.4, 0.593, 0.8)]), rng, conn)
        K = int(B.bodies_of(label).max())
        lab, dense, rows, head = ctx.malloc(label.nbytes), ctx.malloc(label.nbytes), ctx.malloc(T * K * 64), ctx.malloc(T * 64)
        lab.upload(label.reshape(-1))
        ctx.body_table_device(lab.ptr, None, BodySpec(0, None, K), T, H, W, _capi.BodyOut.of(dense=dense.ptr, rows=rows.ptr, head=head.ptr))
        ctx.synchronize()
        bhead = head.download(np.uint64, T * 8).reshape(T, 8)
        brows = rows.download(np.uint32, T * K * 16).reshape(T, K, 16).view(BODY_ROW)[..., 0]
        E = int(bhead[:, 4].max())
        got = ctx.outline(dense, Spec(E, E // 4, conn), T, H, W)
        ohead = got['head'].download(np.uint64, T * HW).reshape(T, HW)
        rings = got['rings'].download(np.uint32, T * (E // 4) * RW).reshape(T, E // 4, RW).view(ROW_DTYPE)[..., 0]
        assert np.array_equal(ohead[:, 0], bhead[:, 4]) and np.array_equal(ohead[:, 4], bhead[:, 0]) and np.all(ohead[:, 7] == 0)
        for t in range(T):
            k, r = int(bhead[t, 0]), rings[t, :int(ohead[t, 1])]
            assert np.array_equal(np.bincount(r['id'], weights=r['area2'], minlength=k + 1)[1:], 2.0 * brows['area'][t, :k])
            assert np.array_equal(np.bincount(r['id'], weights=r['length'], minlength=k + 1)[1:], brows['perimeter'][t, :k].astype(np.float64))
            assert np.array_equal(np.bincount(r['id'][r['area2'] > 0], minlength=k + 1)[1:], np.ones(k, dtype=np.int64))
        for b in (lab, dense, rows, head, *got.values()):
            b.free()


def test_refusals_write_nothing(ctx):
    rng = np.random.default_rng(9170)
    ids = B.labels_of(rng.random((2, 20, 30)) < 0.5, rng, 8)
    spec = Spec(600, 150, 8)
    r = Run(ctx, ids, spec)
    lib, h = ctx.lib, ctx.handle
    ip, wp = r.ibuf.ptr + r.istart, r.wbuf.ptr + GUARD + 8

    def cs(**kw):
        c = _capi.OutlineSpec.of(spec)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def outs(**kw):
        o = _capi.OutlineOut.of(**{k: r.obuf.ptr + r.where[k] for k in KEYS})
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(ids=ip, cspec=cs(), n=2, H=20, W=30, out=r.out, work=wp, work_bytes=r.work_bytes, handle=h):
        return lib.dswx_outline_device(handle, ctypes.c_void_p(ids), ctypes.byref(cspec) if cspec is not None else None, n, H, W,
                                       ctypes.byref(out) if out is not None else None, ctypes.c_void_p(work), work_bytes, None)

    A, L = _capi.ERR_ARG, _capi.ERR_ALIGN
    for rc, kw in ((A, {'cspec': None}), (A, {'out': None}), (A, {'cspec': cs(connectivity=6)}), (A, {'cspec': cs(connectivity=0)}),
                   (A, {'cspec': cs(reserved=1)}), (A, {'n': -1}), (A, {'H': -1}), (A, {'W': -1}), (A, {'cspec': cs(max_edges=-1)}),
                   (A, {'cspec': cs(max_rings=-1)}), (A, {'H': 1 << 15, 'W': (1 << 15) + 1}), (A, {'cspec': cs(max_edges=(1 << 31) + 1)}),
                   (A, {'cspec': cs(max_rings=(1 << 31) + 1)}), (A, {'ids': None}), (A, {'out': outs(rings=None)}),
                   (A, {'out': outs(chain=None)}), (A, {'work': None}), (A, {'work_bytes': r.work_bytes - 1}), (A, {'work_bytes': 0}),
                   (L, {'ids': ip + 2}), (L, {'out': outs(chain=r.out.chain + 1)}), (L, {'out': outs(rings=r.out.rings + 2)}),
                   (L, {'out': outs(head=r.out.head + 4)}), (L, {'work': wp + 4}), (A, {'handle': None})):
        assert call(**kw) == rc, (kw, lib.dswx_last_error())
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT) and np.all(r.wbuf.download(np.uint8, r.wsize) == SENT)
    assert call(cspec=cs(connectivity=5), handle=None) == A and 'connectivity' in lib.dswx_last_error().decode()     # arguments before the context
    assert call(n=0) == 0                                            # no tiles: legal, writes nothing
    ctx.synchronize()
    assert np.all(r.obuf.download(np.uint8, r.osize) == SENT)
    r.run()
    ctx.synchronize()
    r.check('after the refusals')
    r.free()


def test_device_plane_and_device_batch_chains(ctx):
    """upload -> label -> outline with no host copy in between, equal to outline.outline_tiles of the label plane; the same
    for the WTR plane of a classified batch, a tile range with tile0 > 0."""
    from proteus_amd.label import label_tiles
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9180)
    try:
        a = rng.choice(np.array([0, 1, 2, 252, 253, 255], dtype=np.uint8), size=(3, 52, 158), p=[0.4, 0.3, 0.1, 0.05, 0.1, 0.05])
        lspec = wtr_label_spec(1)
        label = label_tiles(a, lspec)['label']
        E = int(OC.edges_of(label).max())
        spec = Spec(E + 1, E // 4, 8)
        want = outline_tiles(label, spec)
        got = eng.upload(a).outline(lspec, spec)
        assert list(got) == ['label', 'chain', 'rings', 'head'] and all(p._host is None for p in got.values())
        assert np.array_equal(got['label'].numpy(), label) and np.array_equal(got['chain'].numpy(), want['chain'])
        assert np.array_equal(got['head'].numpy(), want['head']) and np.array_equal(got['rings'].numpy().view(ROW_DTYPE)[..., 0], want['rings'])
        one = eng.upload(label[1]).outline(None, spec)
        assert list(one) == ['chain', 'rings', 'head'] and np.array_equal(one['chain'].numpy(), want['chain'][1:2])
        with pytest.raises(ValueError):
            eng.upload(a).outline(None, spec)
    finally:
        eng.close()
    n_tiles, h, w = 4, 73, 165
    batch = _capi.DeviceBatch(ctx, n_tiles, h, w)
    try:
        batch.synth(SEED, tile0=31)
        batch.classify(_capi.default_params())
        wtr = np.stack([batch.read_tile('wtr', t) for t in range(n_tiles)])
        label = _capi.label_host(wtr, lspec, want=('label',))['label']
        E = int(OC.edges_of(label).max())
        spec = Spec(E, E // 4, 8)
        ref = _capi.outline_host(label, spec)
        for tile0, count in ((0, None), (1, 2)):
            res = batch.outline('wtr', lspec, spec, tile0=tile0, n_tiles=count)
            nt = n_tiles - tile0 if count is None else count
            assert list(res) == ['label', 'chain', 'rings', 'head']
            assert np.array_equal(res['label'].download(np.uint32, nt * h * w).reshape(nt, h, w), label[tile0:tile0 + nt])
            for k in KEYS:
                assert np.array_equal(res[k].download(_capi.OUTLINE_DTYPES[k], ref[k][tile0:tile0 + nt].size), ref[k][tile0:tile0 + nt].reshape(-1)), (k, tile0)
            for b in res.values():
                b.free()
    finally:
        batch.free()


@pytest.fixture(scope='module')
def product_file(tmp_path_factory):
    """The multi-band product file of the suite's own synthetic product run (tools/make_synthetic_hls.py, 301 x 301)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    from proteus_amd import dswx_hls
    tmp = tmp_path_factory.mktemp('outline_product')
    _, files, _, _ = synth_hls.make(str(tmp), size=301, tile=4)
    out = str(tmp / 'product.tif')
    assert dswx_hls.generate_dswx_layers(files, out) is True
    return out


def test_the_command_line_tool_writes_the_polygons(product_file, tmp_path, capsys):
    """bin/dswx_outline.py: the GeoJSON parsed back, every feature equal to what the host path gives -- dswx_label_host of
    the sieved band, dswx_body_table_host, dswx_outline_host, outline.polygons and the file's geotransform."""
    spec = importlib.util.spec_from_file_location('dswx_outline_tool', os.path.join(ROOT, 'bin', 'dswx_outline.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    bands, info = geotiff.read_geotiff(product_file)
    wtr = bands[0] if bands.ndim == 3 else bands
    H, W = wtr.shape
    gt = tuple(float(v) for v in info.geotransform)
    for flags, min_size, conn in (([], 1, 8), (['--connectivity', '4', '--min-size', '5'], 5, 4)):
        out = str(tmp_path / f'bodies{min_size}.geojson')
        capsys.readouterr()
        assert tool.main(flags + ['--out', out, product_file]) == 0
        said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        lspec = wtr_label_spec(min_size, connectivity=conn)
        sieved = _capi.label_host(wtr[None], lspec, want=('sieved',))['sieved']
        label = _capi.label_host(sieved, lspec, want=('label',))['label']
        K = int(B.bodies_of(label)[0])
        rows = _capi.body_table_host(label, sieved, wtr_body_spec(K))['rows'].view(BODY_ROW)[0, :, 0]
        E = int(OC.edges_of(label)[0])
        ref = _capi.outline_host(label, Spec(E, E // 4, conn))
        with open(out) as f:
            doc = json.load(f)
        assert doc['type'] == 'FeatureCollection' and len(doc['features']) == K == said['bodies'] == said['polygons'] and K > 3
        assert said['edges'] == E and said['rings'] == int(ref['head'][0, 1]) and said['vertices'] == int(ref['head'][0, 6])
        if said['epsg'] is not None:
            assert doc['crs']['properties']['name'] == f'urn:ogc:def:crs:EPSG::{said["epsg"]}'
        polys = list(polygons(ref['chain'][0], ref['rings'][0], W))
        assert [p[0] for p in polys] == [int(r['label']) for r in rows]
        for feat, (label_id, outer, holes), row in zip(doc['features'], polys, rows):
            prop, rings = feat['properties'], feat['geometry']['coordinates']
            assert feat['geometry']['type'] == 'Polygon' and prop['label'] == label_id and prop['holes'] == len(holes) == len(rings) - 1
            assert prop['area_m2'] == int(row['area']) * abs(gt[1] * gt[5]) and prop['perimeter_m'] == int(row['perimeter']) * (abs(gt[1]) + abs(gt[5])) / 2
            for ring, pts in zip(rings, [outer] + holes):
                assert ring[0] == ring[-1] and len(ring) == len(pts) + 1
                assert ring[:-1] == [[gt[0] + float(x) * gt[1] + float(y) * gt[2], gt[3] + float(x) * gt[4] + float(y) * gt[5]] for x, y in pts.tolist()]
    assert tool.main(['--min-size', '0', '--out', str(tmp_path / 'no.geojson'), product_file]) == 1
    assert not os.path.exists(str(tmp_path / 'no.geojson'))


def test_outline_example_runs(tmp_path):
    """examples/batch_outline.c: its own checks (exit status 0: chain, rings and head of the device against
    dswx_outline_host on the downloaded label plane)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_outline')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_outline.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '3', '301'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'wtr outlines: device and host entry agree in every byte' in r.stdout
    assert '3 tiles of 301 x 301 pixels' in r.stdout and 'largest ring' in r.stdout
