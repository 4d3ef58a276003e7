"""The reach entries on the device (include/dswx_hip.h "reach"): dswx_reach_device and dswx_batch_reach against dswx_reach_host,
every output byte of every tile, on the cases of tests/test_reach.py."""
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
from proteus_amd.reach import HEAD_WORDS, Spec
from proteus_amd.synth import SEED
from tests import _reach_cases as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xEE                                       # every byte of an output buffer beforehand
GUARD = 512
KEYS = ('acc', 'mask', 'head')
EB = {'acc': 4, 'mask': 1, 'head': 8}
OFF = {'acc': 4, 'mask': 1, 'head': 8}            # past a 16-byte boundary: the least alignment the entry accepts
CASES = K.named_cases()


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


class Run:
    """One call of dswx_reach_device.  The records lie at a 16-byte boundary behind a guard and the table 8 bytes past one, in
    `ibuf`, with `src` (when given) 3 bytes past one; the wanted outputs lie in `obuf`, acc 4, mask 1 and head 8 bytes past a
    16-byte boundary, every byte SENT beforehand."""

    def __init__(self, ctx, c, spec=None, want=KEYS, src=None, in_place=False):
        self.ctx, self.c, self.spec, self.want = ctx, c, spec or K.spec_of(c, burn=200, background=3), tuple(want)
        self.T, self.H, self.W = len(c['first']) - 1, c['H'], c['W']
        n = self.H * self.W
        self.src, self.in_place = src, in_place
        ms = self.spec.mask_tile_stride or n
        self.count = {'acc': self.T * n, 'mask': self.T * ms, 'head': self.T * HEAD_WORDS}
        v = c['verts'].view(np.uint8)
        first = np.ascontiguousarray(c['first'], dtype=np.int64)
        self.vat = GUARD
        self.fat = -(-(self.vat + max(v.size, 16)) // 16) * 16 + 8
        self.sat = -(-(self.fat + first.nbytes) // 16) * 16 + 3
        self.ihost = np.full(self.sat + (src.size if src is not None else 0) + GUARD, SENT, dtype=np.uint8)
        self.ihost[self.vat:self.vat + v.size] = v
        self.ihost[self.fat:self.fat + first.nbytes] = first.view(np.uint8)
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
        self.ctx.reach_device(self.ibuf.ptr + self.vat, self.ibuf.ptr + self.fat, self.spec, self.T, self.H, self.W, src, self.out, stream=stream)

    def host(self):
        """dswx_reach_host on the same arguments; the mask starts as the bytes the device's mask started as."""
        ms = self.spec.mask_tile_stride or self.H * self.W
        mask = self.before[self.where['mask']:self.where['mask'] + self.T * ms].copy().reshape(self.T, ms) if 'mask' in self.want else None
        src = mask if self.in_place else self.src
        return _capi.reach_host(self.c['verts'], self.c['first'], self.H, self.W, self.spec, src=src, want=self.want, mask=mask)

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


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_device_entry_against_the_host_entry(ctx, c):
    """Every named case: all outputs; acc alone, without head, without mask; src apart and src == mask; a second call on the
    outputs of the first."""
    ref = once(ctx, c)
    for want in (('acc',), ('acc', 'mask'), ('acc', 'head')):
        once(ctx, c, f"{c['name']} want {want}", want=want)
    n = len(c['first']) - 1
    rng = np.random.default_rng(len(c['verts']))
    src = rng.integers(0, 256, size=(n, c['H'], c['W']), dtype=np.uint8)
    once(ctx, c, 'src apart', src=src, spec=K.spec_of(c, burn=9, background=1))
    r = Run(ctx, c, src=src, spec=K.spec_of(c, burn=9, background=1), in_place=True)
    r.run()
    ctx.synchronize()
    first = r.check('src in place')
    r.run()                                                  # into its own result: the same bytes
    r.run()
    ctx.synchronize()
    r.check('a second call', first)
    r.free()
    assert np.array_equal(first['acc'], ref['acc']) and np.array_equal(first['head'], ref['head'])


def test_strides_empty_rasters_and_a_callers_stream(ctx):
    c = CASES[1]
    n, H, W = len(c['first']) - 1, c['H'], c['W']
    rng = np.random.default_rng(3)
    ms, ss = H * W + 7, H * W + 3
    once(ctx, c, 'strides', src=rng.integers(0, 256, size=(n, ss), dtype=np.uint8), spec=Spec(c['R'], 9, 1, ms, ss))
    once(ctx, c, 'strides in place', src=rng.integers(0, 256, size=(n, ms), dtype=np.uint8), spec=Spec(c['R'], 9, 1, ms, ms), in_place=True)
    for T, h, w in ((0, 5, 7), (2, 0, 5), (2, 5, 0)):
        once(ctx, {'name': 'empty', 'H': h, 'W': w, 'R': 300, 'verts': c['verts'][:8], 'first': np.array([0, 4, 8][:T + 1])})
    assert 'thread_rows=4' in ctx.last_kernel_info() and 'dswx_reach_scatter_k' in ctx.last_kernel_info()
    if torch is not None:
        s = torch.cuda.Stream(device=0)
        r = Run(ctx, c)
        r.run(stream=s.cuda_stream)
        r.run(stream=s.cuda_stream)
        ctx.synchronize(s.cuda_stream)
        r.check('caller stream')
        r.free()


def test_a_workgroup_reaches_a_second_tile_past_the_blocks_of_grid_y(ctx):
    """65535 + 4 tiles of 8 x 8 with a few segments or points each, some tiles empty: grid.y is 65535; every byte compared."""
    c = K.tiny_tiles_case()
    assert len(c['first']) - 1 == 65535 + 4 and (c['H'], c['W']) == (8, 8)
    ref = once(ctx, c)
    assert ',65535,1)' in ctx.last_kernel_info()
    counts = np.diff(c['first'])
    assert (counts == 0).sum() > 100 and ref['head'][-1, 3] > 0 and (ref['head'][:, 0] == counts).all()


def test_batch_reach_into_the_ocean_plane_then_classify(ctx):
    """A ring burnt and then buffered into DSWX_PLANE_OCEAN of a masks batch, then dswx_batch_classify: the checksums of all
    layers and the counters equal those of a second batch whose OCEAN plane was uploaded from the host entries' mask.  And the
    refusals of the batch form, by code and whole text."""
    n_tiles, H, W = 4, 73, 165
    rng = np.random.default_rng(9410)
    per_tile = [BN.records([BN.quantise([(-5, 10), (W + 3, 30), (W / 2, H + 9)]), BN.quantise([(20 + t, 20), (60, 22), (50, 55 - t), (18, 50)])], [1, 2])
                for t in range(n_tiles)]
    verts, first = BN.tiles(per_tile)
    bspec, rspec = BN.Spec(burn=0, background=1), Spec(3 * 256 + 41, burn=0, background=1)
    a, b = _capi.DeviceBatch(ctx, n_tiles, H, W, masks=True), _capi.DeviceBatch(ctx, n_tiles, H, W, masks=True)
    res = {}
    try:
        ocean = rng.integers(0, 2, size=(n_tiles, H, W), dtype=np.uint8) | (rng.random((n_tiles, H, W)) < 0.01).astype(np.uint8) * 7
        for batch in (a, b):
            batch.synth(SEED, tile0=5)
        ctx.synchronize()
        for t in range(n_tiles):
            a.write_tile('ocean', t, ocean[t])
        burnt = _capi.burn_host(verts, first, H, W, bspec, src=ocean)
        ref = _capi.reach_host(verts, first, H, W, rspec, src=burnt['mask'])
        assert (ref['mask'] != burnt['mask']).any() and (burnt['mask'] != ocean).any()
        for t in range(n_tiles):
            b.write_tile('ocean', t, ref['mask'][t])
        for buf in a.burn('ocean', verts, first, bspec).values():
            buf.free()
        res = a.reach('ocean', verts, first, rspec)
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
        nine = Spec(rspec.radius, burn=9, background=1)
        res = b.reach('ocean', verts[first[1]:first[3]], first[1:4] - first[1], nine, tile0=1, n_tiles=2)
        two = _capi.reach_host(verts[first[1]:first[3]], first[1:4] - first[1], H, W, nine, src=ref['mask'][1:3])
        assert np.array_equal(b.read_tile('ocean', 0), ref['mask'][0]) and np.array_equal(b.read_tile('ocean', 3), ref['mask'][3])
        assert all(np.array_equal(b.read_tile('ocean', 1 + t), two['mask'][t]) for t in range(2))
        assert np.array_equal(res['head'].download(np.uint64, 2 * HEAD_WORDS), two['head'].reshape(-1))
        # the refusals, and nothing written
        before = [b.read_tile('ocean', t) for t in range(n_tiles)]
        lib = ctx.lib
        dv, df = ctx.malloc(max(verts.nbytes, 16)), ctx.malloc(first.nbytes)
        res['dv'], res['df'] = dv, df
        dv.upload(verts)
        df.upload(first)

        def call(batch=b.handle, plane=_capi.PLANE_INDEX['ocean'], spec=rspec, acc=res['acc'].ptr, head=res['head'].ptr, tile0=0, n=2, v=dv.ptr, f=df.ptr,
                 **fields):
            s = _capi.ReachSpec.of(spec)
            for k, val in fields.items():
                setattr(s, k, val)
            return lib.dswx_batch_reach(batch, plane, ctypes.c_void_p(v), ctypes.c_void_p(f), ctypes.byref(s),
                                        ctypes.c_void_p(acc), ctypes.c_void_p(head), tile0, n, None)

        def refused(rc, code, text, whole=False):
            said = lib.dswx_last_error()
            assert rc == code and (said == text if whole else text in said), (rc, said)
        refused(call(batch=None), _capi.ERR_ARG, b'batch is NULL')
        refused(call(plane=_capi.PLANE_INDEX['counters']), _capi.ERR_ARG, b'the counters are not reached into')
        refused(call(plane=_capi.PLANE_INDEX['blue']), _capi.ERR_ARG, b'edges reach into a uint8 plane')
        refused(call(plane=_capi.PLANE_INDEX['diag']), _capi.ERR_ARG, b'edges reach into a uint8 plane')
        refused(call(plane=_capi.PLANE_INDEX['browse']), _capi.ERR_ARG, b'has no plane')
        refused(call(plane=-1), _capi.ERR_ARG, b'plane -1')
        refused(call(plane=20), _capi.ERR_ARG, b'plane 20')
        refused(call(tile0=3, n=2), _capi.ERR_ARG, b'outside the batch')
        refused(call(tile0=-1), _capi.ERR_ARG, b'outside the batch')
        refused(call(mask_tile_stride=H * W + 8), _capi.ERR_ARG,
                b'mask_tile_stride %d and src_tile_stride 0 must be 0: the plane has the stride of the batch' % (H * W + 8), whole=True)
        refused(call(src_tile_stride=H * W + 8), _capi.ERR_ARG,
                b'mask_tile_stride 0 and src_tile_stride %d must be 0: the plane has the stride of the batch' % (H * W + 8), whole=True)
        refused(call(radius=(1 << 20) + 1), _capi.ERR_ARG, b'radius 1048577 above DSWX_REACH_MAX_RADIUS 1048576 (1/256 pixel)', whole=True)
        refused(call(reserved=7), _capi.ERR_ARG, b'reserved 7 must be 0', whole=True)
        refused(call(burn=256), _capi.ERR_ARG, b'burn 256 outside 0 .. 255', whole=True)
        refused(call(acc=None), _capi.ERR_ARG, b'acc is NULL: it is the working array', whole=True)
        refused(call(v=None), _capi.ERR_ARG, b'verts is NULL', whole=True)
        refused(call(f=None), _capi.ERR_ARG, b'tile_first is NULL', whole=True)
        refused(call(acc=res['acc'].ptr + 2), _capi.ERR_ALIGN, b'acc not 4-byte aligned', whole=True)
        refused(call(head=res['head'].ptr + 4), _capi.ERR_ALIGN, b'head not 8-byte aligned', whole=True)
        refused(call(v=dv.ptr + 8), _capi.ERR_ALIGN, b'verts not 16-byte aligned', whole=True)
        refused(call(f=df.ptr + 4), _capi.ERR_ALIGN, b'tile_first not 8-byte aligned', whole=True)
        ctx.synchronize()
        assert all(np.array_equal(b.read_tile('ocean', t), before[t]) for t in range(n_tiles))
        assert call(n=0) == 0 and call(tile0=4, n=_capi.BATCH_ALL_TILES) == 0            # an empty range: legal, writes nothing
        with pytest.raises(ValueError):
            b.reach('ocean', verts, first, rspec, want=('mask',))
    finally:
        for buf in res.values():
            buf.free()
        a.free()
        b.free()


def test_device_plane_reach(ctx):
    """pipeline.DevicePlane.burn then .reach: rings in pixel coordinates grown by a radius in a resident plane in place."""
    from proteus_amd.pipeline import TileEngine
    from proteus_amd.reach import reach_tiles
    eng = TileEngine(ctx)
    rng = np.random.default_rng(9420)
    try:
        a = rng.integers(0, 256, size=(2, 41, 67), dtype=np.uint8)
        rings = [[np.array([(3.2, 4.1), (60.7, 9.9), (30.5, 38.0)]), np.array([(20.0, 10.0), (40.0, 10.0), (30.0, 20.0)])],
                 [np.array([(-4.0, -4.0), (70.0, -4.0), (70.0, 20.5), (-4.0, 20.5)])]]
        verts, first = BN.tiles([BN.records([BN.quantise(r) for r in rs]) for rs in rings])
        spec = Spec(700, burn=5)
        want = reach_tiles(verts, first, 41, 67, spec, src=a)
        plane = eng.upload(a)
        got = plane.reach(rings, spec)
        assert list(got) == ['acc', 'head'] and np.array_equal(plane.numpy(), want['mask'])
        assert np.array_equal(got['acc'].numpy(), want['acc']) and np.array_equal(got['head'].numpy(), want['head'])
        one = eng.upload(a[0])
        one.reach(rings[0], spec)
        assert np.array_equal(one.numpy(), want['mask'][0])
        with pytest.raises(ValueError):
            eng.upload(a.astype(np.uint16)).reach(rings, spec)
    finally:
        eng.close()


def test_rasterise_shoreline_on_a_synthetic_product(tmp_path):
    """generate_dswx_layers with a .shp shoreline and rasterise_shoreline=True on a 64 x 64 product: every layer of the product
    equals that of a run given ocean_mask= from burn_tiles + reach_tiles of the same plan; the metadata name the shapefile."""
    import sys
    from proteus_amd import dswx_hls, geotiff, shoreline
    from tests import _shoreline_cases as S
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    _, files, _, _ = synth_hls.make(str(tmp_path / 'in'), size=64, tile=4)
    gt = (600000.0, 30.0, 0.0, 4000020.0, 0.0, -30.0)        # (of tools/make_synthetic_hls.py, EPSG:32615)
    grid = S.Grid.of(gt, 15, 64)
    land = np.array([(-40000.0, -300.0), (-700.0, -350.0), (-200.0, 100.0), (300.0, -500.0), (40000.0, -450.0), (30000.0, -90000.0), (-35000.0, -80000.0)])
    isle = np.array([(500.0, 600.0), (700.0, 640.0), (620.0, 800.0)])
    recs = [('polygon', [S.clockwise(grid.lonlat(land))]), ('point', (0.0, 0.0)), ('polygonz', [S.clockwise(grid.lonlat(isle))])]
    shp = S.write_shp(str(tmp_path / 'coast.shp'), recs)
    common = dict(apply_ocean_masking=True, ocean_masking_shoreline_distance_km=0.2, scratch_dir=str(tmp_path))
    plan = shoreline.plan(shp, gt, 32615, 64, 64, 200)
    mask = plan.host_mask(64, 64)
    assert 0.2 * 64 * 64 < mask.sum() < 0.8 * 64 * 64 and plan.polygons == 2 and plan.edges_on_clip_sides >= 3
    a, b = str(tmp_path / 'a.tif'), str(tmp_path / 'b.tif')
    assert dswx_hls.generate_dswx_layers(files, a, shoreline_shapefile=shp, shoreline_shapefile_description='Synthetic coast',
                                         rasterise_shoreline=True, **common) is True
    assert dswx_hls.generate_dswx_layers(files, b, ocean_mask=mask, **common) is True
    got, ginfo = geotiff.read_geotiff(a)
    want, winfo = geotiff.read_geotiff(b)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the mask did change pixels, and only beyond the margin
    c = str(tmp_path / 'c.tif')
    assert dswx_hls.generate_dswx_layers(files, c, apply_ocean_masking=False, scratch_dir=str(tmp_path)) is True
    plain, _ = geotiff.read_geotiff(c)
    changed = (got != plain).reshape(-1, 64, 64).any(axis=0)
    assert changed.any() and not changed[mask == 1].any()
    assert ginfo.metadata['SHORELINE_SOURCE'] == 'Synthetic coast' and ginfo.metadata['OCEAN_MASKING_ENABLED'] == 'TRUE'
    for k in ('SPATIAL_COVERAGE', 'SPATIAL_COVERAGE_EXCLUDING_MASKED_OCEAN', 'OCEAN_MASKING_SHORELINE_DISTANCE_KM'):
        assert ginfo.metadata[k] == winfo.metadata[k], k


def test_the_burn_tool_buffers_the_vector(tmp_path, capsys):
    """bin/dswx_burn.py --buffer-vector-m: burn, then reach, against the host entries; --buffer-m stays what it was and the two
    exclude each other."""
    import importlib.util
    import json
    import sys
    from proteus_amd import dswx_hls, geotiff
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import make_synthetic_hls as synth_hls
    _, files, _, _ = synth_hls.make(str(tmp_path / 'in'), size=64, tile=4)
    product = str(tmp_path / 'product.tif')
    assert dswx_hls.generate_dswx_layers(files, product) is True
    spec = importlib.util.spec_from_file_location('dswx_burn_tool2', os.path.join(ROOT, 'bin', 'dswx_burn.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    gt = (600000.0, 30.0, 0.0, 4000020.0, 0.0, -30.0)
    ring = [[600300.0, 3999700.0], [601200.0, 3999500.0], [600900.0, 3998800.0], [600300.0, 3999700.0]]
    polys = str(tmp_path / 'p.geojson')
    with open(polys, 'w') as f:
        json.dump({'type': 'Feature', 'properties': {}, 'geometry': {'type': 'Polygon', 'coordinates': [ring]}}, f)
    out = str(tmp_path / 'buffered.tif')
    capsys.readouterr()
    assert tool.main([product, '--polygons', polys, '--burn', '7', '--background', '2', '--buffer-vector-m', '100', '--out', out]) == 0
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    got, _ = geotiff.read_geotiff(out)
    verts = tool.records_of(tool.polygons_of(json.load(open(polys))), gt)
    first = np.array([0, len(verts)])
    m = _capi.burn_host(verts, first, 64, 64, BN.Spec(7, 2))['mask']
    ref = _capi.reach_host(verts, first, 64, 64, Spec(round(256 * 100 / 30.0), 7, 2), src=m, mask=m)
    assert np.array_equal(got, m[0]) and said['buffer_vector_256ths_of_a_pixel'] == 853 and said['reached_pixels'] == int(ref['head'][0, 6])
    assert said['burnt_pixels'] == int((m[0] == 7).sum()) > said['reached_pixels'] > 0
    assert tool.main([product, '--polygons', polys, '--buffer-vector-m', '100', '--buffer-m', '100', '--out', str(tmp_path / 'no.tif')]) == 1
    assert tool.main([product, '--polygons', polys, '--buffer-vector-m', '-1', '--out', str(tmp_path / 'no.tif')]) == 1
    assert not os.path.exists(str(tmp_path / 'no.tif'))


def test_reach_example_runs(tmp_path):
    """examples/batch_reach.c: its own checks (exit status 0: the OCEAN plane and the head of the device against its loop)."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_reach')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_reach.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    r = subprocess.run([exe, '3', '301'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'reach: device and loop agree in every pixel and every head word' in r.stdout
    assert '3 tiles of 301 x 301 pixels' in r.stdout
