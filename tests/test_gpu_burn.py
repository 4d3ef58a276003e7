"""The burn entries on the device (include/dswx_hip.h "burn"): dswx_burn_device and dswx_batch_burn against dswx_burn_host,
every output byte of every tile, on the cases of tests/test_burn.py and on shapes built around the seams of the two kernels."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py)
    import torch
except ImportError:
    torch = None

from proteus_amd import _capi
from proteus_amd import burn as BN
from proteus_amd.burn import HEAD_WORDS, Spec
from proteus_amd.label import wtr_label_spec
from proteus_amd.synth import SEED
from tests import _burn_cases as K
from tests import _outline_cases as OC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xEE                                       # every byte of an output buffer beforehand
GUARD = 512
KEYS = ('acc', 'mask', 'head')
EB = {'acc': 4, 'mask': 1, 'head': 8}
OFF = {'acc': 4, 'mask': 1, 'head': 8}            # past a 16-byte boundary: the least alignment the entry accepts


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Run:
    """One call of dswx_burn_device.  The records lie at a 16-byte boundary behind a guard and the table 8 bytes past one, in
    `ibuf`, with `src` (when given) 3 bytes past one; the wanted outputs lie in `obuf`, acc 4, mask 1 and head 8 bytes past a
    16-byte boundary, every byte SENT beforehand."""

    def __init__(self, ctx, c, spec=None, want=KEYS, src=None, in_place=False):
        self.ctx, self.c, self.spec, self.want = ctx, c, spec or Spec(200, 3), tuple(want)
        self.T, self.H, self.W = len(c['first']) - 1, c['H'], c['W']
        n = self.H * self.W
        self.src, self.in_place = src, in_place
        ms = self.spec.mask_tile_stride or n
        self.count = {'acc': self.T * n, 'mask': self.T * ms, 'head': self.T * HEAD_WORDS}
        v = c['verts'].view(np.uint8)
        self.vat = GUARD
        self.fat = -(-(self.vat + max(v.size, 16)) // 16) * 16 + 8
        self.sat = -(-(self.fat + c['first'].nbytes) // 16) * 16 + 3
        self.ihost = np.full(self.sat + (src.size if src is not None else 0) + GUARD, SENT, dtype=np.uint8)
        self.ihost[self.vat:self.vat + v.size] = v
        self.ihost[self.fat:self.fat + c['first'].nbytes] = np.ascontiguousarray(c['first'], dtype=np.int64).view(np.uint8)
        if src is not None:
            self.ihost[self.sat:self.sat + src.size] = src.reshape(-1)
        self.where, cursor = {}, 0
        for k in KEYS:
            begin = -(-cursor // 16) * 16 + OFF[k]
            self.where[k] = begin
            cursor = begin + self.count[k] * EB[k] + 16
        self.osize = cursor + 16
        self.ibuf, self.obuf = ctx.malloc(self.ihost.size), ctx.malloc(self.osize)
        assert self.ibuf.ptr % 256 == 0 and self.obuf.ptr % 16 == 0
        self.ibuf.upload(self.ihost)
        self.poison()
        self.out = _capi.BurnOut.of(**{k: self.obuf.ptr + self.where[k] for k in self.want})

    def poison(self):
        raw = np.full(self.osize, SENT, dtype=np.uint8)
        if self.in_place:                                    # the mask holds the source
            raw[self.where['mask']:self.where['mask'] + self.src.size] = self.src.reshape(-1)
        self.obuf.upload(raw)
        self.before = raw

    def run(self, stream=None):
        src = None if self.src is None else self.obuf.ptr + self.where['mask'] if self.in_place else self.ibuf.ptr + self.sat
        self.ctx.burn_device(self.ibuf.ptr + self.vat, self.ibuf.ptr + self.fat, self.spec, self.T, self.H, self.W, src, self.out, stream=stream)

    def host(self):
        """dswx_burn_host on the same arguments; the mask starts as the bytes the device's mask started as."""
        n, ms = self.H * self.W, self.spec.mask_tile_stride or self.H * self.W
        mask = self.before[self.where['mask']:self.where['mask'] + self.T * ms].copy().reshape(self.T, ms) if 'mask' in self.want else None
        src = mask if self.in_place else self.src
        ref = _capi.burn_host(self.c['verts'], self.c['first'], self.H, self.W, self.spec, src=src, want=self.want, mask=mask)
        return ref

    def check(self, what, ref=None):
        """The wanted outputs are the host entry's -- the bytes between the rasters of a strided mask as they were --, every
        other byte of the output buffer is still SENT and the inputs are what was uploaded."""
        ref = self.host() if ref is None else ref
        raw = self.obuf.download(np.uint8, self.osize)
        written = np.zeros(self.osize, dtype=bool)
        for k in ('acc',) + tuple(k for k in self.want if k != 'acc'):
            begin, nb = self.where[k], self.count[k] * EB[k]
            got = raw[begin:begin + nb].copy().view(_capi.BURN_DTYPES[k])
            want = ref[k].reshape(-1)
            assert np.array_equal(got, want), (what, k, np.flatnonzero(got != want)[:6], got[got != want][:6], want[got != want][:6])
            written[begin:begin + nb] = True
        assert np.all(raw[~written] == SENT), (what, 'bytes outside the wanted outputs were written', np.flatnonzero((raw != SENT) & ~written)[:6])
        assert np.array_equal(self.ibuf.download(np.uint8, self.ihost.size), self.ihost), (what, 'an input was written')
        return ref

    def free(self):
        self.ibuf.free()
        self.obuf.free()


def once(ctx, c, what=None, **kw):
    r = Run(ctx, c, **kw)
    r.run()
    ctx.synchronize()
    ref = r.check(what or c['name'])
    r.free()
    return ref


def test_device_entry_against_the_host_entry_on_the_cases_of_the_host_tests(ctx):
    """The random polygons (ties and clipping on all four sides), one batch per shape, and the named corner cases."""
    for c in K.random_cases() + [K.corner_cases()[1]]:
        ref = once(ctx, c)
        assert ref['head'][:, 3].sum() > 0
    names, c = K.corner_cases()
    rng = np.random.default_rng(1)
    n = len(names)
    src = rng.integers(0, 256, size=(n, c['H'], c['W']), dtype=np.uint8)
    once(ctx, c, 'src apart', src=src, spec=Spec(9, 1))
    once(ctx, c, 'src in place', src=src, spec=Spec(9, 1), in_place=True)
    ms, ss = c['H'] * c['W'] + 7, c['H'] * c['W'] + 3
    wide = rng.integers(0, 256, size=(n, ss), dtype=np.uint8)
    once(ctx, c, 'strides', src=wide, spec=Spec(9, 1, ms, ss))
    wide = rng.integers(0, 256, size=(n, ms), dtype=np.uint8)
    once(ctx, c, 'strides in place', src=wide, spec=Spec(9, 1, ms, ms), in_place=True)
    for want in (('acc',), ('acc', 'head'), ('acc', 'mask')):
        once(ctx, c, f'want {want}', want=want)
    # a table that decreases, or begins below zero: the affected tiles have no records
    sq = K.ring([(2, 2), (6, 2), (6, 5), (2, 5)], 13)
    d = {'name': 'decreasing', 'H': 9, 'W': 11, 'verts': np.concatenate([sq, sq, sq]), 'first': np.array([0, 8, 4, 8, 8, 12, -4, 4, 4])}
    assert once(ctx, d)['head'][:, 0].tolist() == [8, 0, 4, 0, 4, 0, 0, 0]
    # no tiles, no rows, no columns
    for T, H, W in ((0, 5, 7), (2, 0, 5), (2, 5, 0)):
        once(ctx, {'name': 'empty', 'H': H, 'W': W, 'verts': c['verts'][:8], 'first': np.array([0, 4, 8][:T + 1])})


@pytest.mark.parametrize('H,W', OC.SHAPES)
def test_round_trip_through_the_outline_on_the_device(ctx, H, W):
    rng = np.random.default_rng(100 * H + W)
    _, _, planes = OC.id_planes(H, W, rng)
    for conn in (4, 8):
        verts, first, _, _ = K.outline_records(planes[conn], conn)
        ref = once(ctx, {'name': f'round_trip_{conn}', 'H': H, 'W': W, 'verts': verts, 'first': first}, spec=Spec(77, 5))
        assert np.array_equal(ref['acc'], planes[conn])


@pytest.mark.parametrize('W', (255, 256, 257, 513, 1025, 129))
def test_carry_across_the_steps_of_a_row_and_rows_that_begin_anywhere(ctx, W):
    """Widths either side of the DSWX_BURN_SCAN_STEP pixels a wave takes per step, several steps, and 129, whose rows begin at
    every offset in a 16-byte slot: toggles in the first and last columns of every step, three rows."""
    assert _capi.BURN_SCAN_STEP == 256
    c = K.carry_case(W)
    ref = once(ctx, c)
    assert ref['head'][0, 3] == 3 * (len(c['verts']) - 8) // 2 and (ref['acc'][0, :, -1] != 0).all()
    rng = np.random.default_rng(W)
    src = rng.integers(0, 256, size=(2, 3, W), dtype=np.uint8)
    once(ctx, c, f'carry_{W} in place', src=src, in_place=True)
    once(ctx, c, f'carry_{W} src apart', src=src)


def test_edges_shared_out_over_the_wave(ctx):
    """700 x 37: edges from (-3.3, -5) to (W + 2, H + 7) and a fan whose row counts sit at, one below and one above the rows a
    thread finishes alone and 64 times that."""
    c = K.fan_case()
    ref = once(ctx, c)
    assert ref['head'][0, 2] == len(c['verts'][:c['first'][1]]) and ref['head'][0, 4] > 0 and ref['head'][0, 5] > 0
    assert 'thread_rows=4' in ctx.last_kernel_info()


def test_a_workgroup_burns_a_second_tile_past_the_blocks_of_grid_y(ctx):
    """65535 + 4 tiles of 4 x 5 with one or two rings each, some tiles empty: grid.y is 65535."""
    c = K.tiny_tiles_case()
    assert len(c['first']) - 1 == 65535 + 4
    ref = once(ctx, c)
    assert ',65535,1)' in ctx.last_kernel_info()
    counts = np.diff(c['first'])
    assert (counts == 0).sum() > 100 and ref['head'][-1, 3] > 0 and (ref['head'][:, 0] == counts).all()


def test_on_a_callers_stream_on_the_null_stream_and_twice_on_dirty_outputs(ctx):
    names, c = K.corner_cases()
    r = Run(ctx, c)
    r.run()                                                  # NULL: the context's stream
    ctx.synchronize()
    ref = r.check('null stream')
    r.run()                                                  # the outputs as the first call left them
    r.run()
    ctx.synchronize()
    r.check('dirty outputs', ref)
    if torch is not None:
        s = torch.cuda.Stream(device=0)
        r.poison()
        r.run(stream=s.cuda_stream)
        r.run(stream=s.cuda_stream)
        ctx.synchronize(s.cuda_stream)
        r.check('caller stream', ref)
    r.free()


def test_label_outline_burn_on_the_device_gives_the_label_plane_back(ctx):
    """label -> outline -> burn without a plane crossing PCIe: only chain and rings are read back, the records are built from
    them, and dswx_compare_device of acc against the label plane finds no difference (uint32 planes as twice as many
    uint16)."""
    from proteus_amd.compare import RECORD
    rng = np.random.default_rng(9300)
    H, W = 65, 130
    a = (rng.random((2, H, W)) < 0.55).astype(np.uint8)
    lspec = wtr_label_spec(1, connectivity=8)
    plane = ctx.malloc(a.size)
    plane.upload(a)
    label = ctx.malloc(4 * a.size)
    rec = ctx.malloc(2 * RECORD.itemsize)
    res = {}
    try:
        ctx.label_device(plane.ptr, lspec, 2, H, W, _capi.LabelOut.of(label=label.ptr))
        E = 4 * H * W
        res = ctx.outline(label, OC.Spec(E, E // 4, 8), 2, H, W, want=('chain', 'rings'))
        chain = res['chain'].download(np.uint32, 2 * E).reshape(2, E)
        rings = res['rings'].download(np.uint32, 2 * (E // 4) * 8).reshape(2, E // 4, 8)
        verts, first = BN.tiles([BN.records_of_outline(chain[t], rings[t], W) for t in range(2)])
        got = ctx.burn(verts, first, H, W, Spec(), want=('acc', 'head'))
        res.update(got)
        ctx.compare_device(got['acc'].ptr, label.ptr, _capi.CMP_U16, 2, 2 * H * W, rec.ptr)
        ctx.synchronize()
        out = rec.download(RECORD, 2)
        assert out['n_diff'].tolist() == [0, 0]
        head = got['head'].download(np.uint64, 2 * HEAD_WORDS).reshape(2, HEAD_WORDS)
        assert head[:, 6].tolist() == (a != 0).sum(axis=(1, 2)).tolist() and not head[:, 1].any()
    finally:
        for b in [plane, label, rec] + list(res.values()):
            b.free()


def test_batch_burn_into_the_ocean_plane_then_classify(ctx):
    """Polygons burnt into DSWX_PLANE_OCEAN of a masks batch, then dswx_batch_classify: the checksums of all layers and the
    counters equal those of a second batch whose OCEAN plane was uploaded from dswx_burn_host's mask.  And the refusals of the
    batch form."""
    n_tiles, H, W = 4, 73, 165
    rng = np.random.default_rng(9310)
    per_tile = [K.concat_rings(K.ring([(-5, 10), (W + 3, 30), (W / 2, H + 9)], 1), K.ring([(20 + t, 20), (60, 22), (50, 55 - t), (18, 50)], 2))
                for t in range(n_tiles)]
    verts, first = BN.tiles(per_tile)
    spec = Spec(burn=0, background=1)
    a, b = _capi.DeviceBatch(ctx, n_tiles, H, W, masks=True), _capi.DeviceBatch(ctx, n_tiles, H, W, masks=True)
    res = {}
    try:
        ocean = rng.integers(0, 2, size=(n_tiles, H, W), dtype=np.uint8) | (rng.random((n_tiles, H, W)) < 0.01).astype(np.uint8) * 7
        for batch in (a, b):
            batch.synth(SEED, tile0=5)
        ctx.synchronize()
        for t in range(n_tiles):
            a.write_tile('ocean', t, ocean[t])
        ref = _capi.burn_host(verts, first, H, W, spec, src=ocean)
        assert (ref['mask'] != ocean).any()
        for t in range(n_tiles):
            b.write_tile('ocean', t, ref['mask'][t])
        res = a.burn('ocean', verts, first, spec)
        assert np.array_equal(res['acc'].download(np.uint32, n_tiles * H * W), ref['acc'].reshape(-1))
        assert np.array_equal(res['head'].download(np.uint64, n_tiles * HEAD_WORDS), ref['head'].reshape(-1))
        assert all(np.array_equal(a.read_tile('ocean', t), ref['mask'][t]) for t in range(n_tiles))
        params = _capi.default_params()
        a.classify(params)
        b.classify(params)
        ctx.synchronize()
        ca, cb = a.checksums(a.plane_names() + ['counters']), b.checksums(b.plane_names() + ['counters'])
        assert list(ca) == list(cb) and all(np.array_equal(ca[k], cb[k]) for k in ca), [k for k in ca if not np.array_equal(ca[k], cb[k])]
        assert np.array_equal(a.read_counters(), b.read_counters())
        # a tile range: tile_first[0] belongs to tile0
        for buf in res.values():
            buf.free()
        res = b.burn('ocean', verts[first[1]:first[3]], first[1:4] - first[1], Spec(burn=9, background=1), tile0=1, n_tiles=2)
        two = _capi.burn_host(verts[first[1]:first[3]], first[1:4] - first[1], H, W, Spec(burn=9, background=1), src=ref['mask'][1:3])
        assert np.array_equal(b.read_tile('ocean', 0), ref['mask'][0]) and np.array_equal(b.read_tile('ocean', 3), ref['mask'][3])
        assert all(np.array_equal(b.read_tile('ocean', 1 + t), two['mask'][t]) for t in range(2))
        assert np.array_equal(res['head'].download(np.uint64, 2 * HEAD_WORDS), two['head'].reshape(-1))
        # the refusals: the rules of dswx_batch_distance, the strides of the spec, and nothing written
        before = [b.read_tile('ocean', t) for t in range(n_tiles)]
        lib = ctx.lib
        dv, df = ctx.malloc(max(verts.nbytes, 16)), ctx.malloc(first.nbytes)
        res['dv'], res['df'] = dv, df
        dv.upload(verts)
        df.upload(first)

        def call(batch=b.handle, plane=_capi.PLANE_INDEX['ocean'], spec=spec, acc=res['acc'].ptr, head=res['head'].ptr, tile0=0, n=2, v=dv.ptr, f=df.ptr):
            return lib.dswx_batch_burn(batch, plane, ctypes.c_void_p(v), ctypes.c_void_p(f), ctypes.byref(_capi.BurnSpec.of(spec)),
                                       ctypes.c_void_p(acc), ctypes.c_void_p(head), tile0, n, None)

        def refused(rc, code, text):
            assert rc == code and text in lib.dswx_last_error(), (rc, lib.dswx_last_error())
        refused(call(batch=None), _capi.ERR_ARG, b'batch is NULL')
        refused(call(plane=_capi.PLANE_INDEX['counters']), _capi.ERR_ARG, b'counters')
        refused(call(plane=_capi.PLANE_INDEX['blue']), _capi.ERR_ARG, b'uint8 plane')
        refused(call(plane=_capi.PLANE_INDEX['diag']), _capi.ERR_ARG, b'uint8 plane')
        refused(call(plane=_capi.PLANE_INDEX['browse']), _capi.ERR_ARG, b'has no plane')
        refused(call(plane=-1), _capi.ERR_ARG, b'plane -1')
        refused(call(plane=20), _capi.ERR_ARG, b'plane 20')
        refused(call(tile0=3, n=2), _capi.ERR_ARG, b'outside the batch')
        refused(call(tile0=-1), _capi.ERR_ARG, b'outside the batch')
        refused(call(spec=Spec(0, 1, H * W + 8, 0)), _capi.ERR_ARG, b'must be 0')
        refused(call(spec=Spec(0, 1, 0, H * W + 8)), _capi.ERR_ARG, b'must be 0')
        refused(call(acc=None), _capi.ERR_ARG, b'acc is NULL')
        refused(call(v=None), _capi.ERR_ARG, b'verts is NULL')
        refused(call(f=None), _capi.ERR_ARG, b'tile_first is NULL')
        refused(call(acc=res['acc'].ptr + 2), _capi.ERR_ALIGN, b'acc')
        refused(call(head=res['head'].ptr + 4), _capi.ERR_ALIGN, b'head')
        refused(call(v=dv.ptr + 8), _capi.ERR_ALIGN, b'verts')
        refused(call(f=df.ptr + 4), _capi.ERR_ALIGN, b'tile_first')
        ctx.synchronize()
        assert all(np.array_equal(b.read_tile('ocean', t), before[t]) for t in range(n_tiles))
        assert call(n=0) == 0 and call(tile0=4, n=_capi.BATCH_ALL_TILES) == 0            # an empty range: legal, writes nothing
        with pytest.raises(ValueError):
            b.burn('ocean', verts, first, spec, want=('mask',))
    finally:
        for buf in res.values():
            buf.free()
        a.free()
        b.free()


def test_device_plane_burn(ctx):
    """pipeline.DevicePlane.burn: rings in pixel coordinates burnt into a resident plane in place."""
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9320)
    try:
        a = rng.integers(0, 256, size=(2, 41, 67), dtype=np.uint8)
        rings = [[np.array([(3.2, 4.1), (60.7, 9.9), (30.5, 38.0)]), np.array([(20.0, 10.0), (40.0, 10.0), (30.0, 20.0)])],
                 [np.array([(-4.0, -4.0), (70.0, -4.0), (70.0, 20.5), (-4.0, 20.5)])]]
        words = [[1, 1], [4]]
        verts, first = BN.tiles([BN.records([BN.quantise(r) for r in rs], w) for rs, w in zip(rings, words)])
        want = BN.burn_tiles(verts, first, 41, 67, Spec(burn=5), src=a)
        plane = eng.upload(a)
        got = plane.burn(rings, Spec(burn=5), words)
        assert list(got) == ['acc', 'head'] and np.array_equal(plane.numpy(), want['mask'])
        assert np.array_equal(got['acc'].numpy(), want['acc']) and np.array_equal(got['head'].numpy(), want['head'])
        one = eng.upload(a[0])
        one.burn(rings[0], Spec(burn=5))
        assert np.array_equal(one.numpy(), want['mask'][0])
        with pytest.raises(ValueError):
            eng.upload(a.astype(np.uint16)).burn(rings)
        with pytest.raises(ValueError):
            eng.upload(a).burn(rings[:1])
    finally:
        eng.close()


def test_the_command_line_tool_burns_what_the_outline_tool_wrote(tmp_path, capsys):
    """bin/dswx_outline.py, then bin/dswx_burn.py on its GeoJSON: the water bodies of the WTR band of the suite's synthetic
    product come back as the water pixels, one bit per polygon, 32 polygons per call; --buffer-m adds the pixels within the
    radius, as dswx_distance_host says; the file is a Byte COG with the product's georeferencing."""
    import importlib.util
    import json
    import sys
    from proteus_amd import dswx_hls, geotiff
    from proteus_amd.distance import Spec as DistanceSpec
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    _, files, _, _ = synth_hls.make(str(tmp_path / 'in'), size=301, tile=4)
    product = str(tmp_path / 'product.tif')
    assert dswx_hls.generate_dswx_layers(files, product) is True
    tools = {}
    for name in ('dswx_outline', 'dswx_burn'):
        spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'bin', name + '.py'))
        tools[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tools[name])
    bands, info = geotiff.read_geotiff(product)
    wtr = bands[0] if bands.ndim == 3 else bands
    water = np.isin(wtr, (1, 2))
    polys = str(tmp_path / 'bodies.geojson')
    assert tools['dswx_outline'].main(['--out', polys, product]) == 0
    out = str(tmp_path / 'burnt.tif')
    capsys.readouterr()
    assert tools['dswx_burn'].main([product, '--polygons', polys, '--burn', '7', '--background', '2', '--out', out]) == 0
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    got, ginfo = geotiff.read_geotiff(out)
    assert got.dtype == np.uint8 and np.array_equal(got, np.where(water, 7, 2))
    assert said['polygons'] > 32 and said['burnt_pixels'] == int(water.sum()) and (said['height'], said['width']) == wtr.shape
    assert tuple(ginfo.geotransform) == tuple(info.geotransform) and geotiff.validate_cog(out) == []
    px = abs(float(info.geotransform[1]))
    assert tools['dswx_burn'].main([product, '--polygons', polys, '--buffer-m', str(2.5 * px), '--out', out]) == 0
    got, _ = geotiff.read_geotiff(out)
    target = np.zeros(256, dtype=np.uint8)
    target[1] = 1
    ring = _capi.distance_host(water[None].astype(np.uint8), DistanceSpec(target, 2, 1), want=('within',))['within'][0]
    assert np.array_equal(got, ring) and ring.sum() > water.sum()
    assert tools['dswx_burn'].main([product, '--polygons', polys, '--burn', '3', '--background', '3', '--out', str(tmp_path / 'no.tif')]) == 1
    assert tools['dswx_burn'].main([product, '--polygons', str(tmp_path / 'missing.geojson'), '--out', str(tmp_path / 'no.tif')]) == 1
    assert not os.path.exists(str(tmp_path / 'no.tif'))


def test_burn_example_runs(tmp_path):
    """examples/batch_burn.c: its own checks (exit status 0: the OCEAN plane and the head of the device against its scalar
    loop)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_burn')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_burn.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '3', '301'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'burn: device and scalar loop agree in every pixel and every head word' in r.stdout
    assert '3 tiles of 301 x 301 pixels' in r.stdout and 'then classified' in r.stdout
