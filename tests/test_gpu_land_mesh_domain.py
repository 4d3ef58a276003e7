"""The land-mesh kernel on the GPU over its whole value domain and over its walk past LM_MAX_GRID_X = 1024 rectangles:
dswx_land_mesh_device byte for byte, land and head, against expected values that no mesh or warp line of the project computes
(tests/_land_mesh_domain_cases.py builds every case backwards from hand-padded rasters and the oracle; tests/
test_land_mesh_domain.py holds the host entry and the numpy statement to the same values and shows that the draws are not
vacuous).  The sweep: every WorldCover, CGLS and `outside` byte, forest classes in every word of the bitset, every threshold
set, year offsets that wrap, every pair of shifts, every count of inside taps, an empty source per map.  The walk: 1031
rectangles in a row, 1031 in a column, 1144 ragged and 2050, where a workgroup takes a second and a third rectangle before its
one set of atomics.  A dozen sweep cases then go through every other way in: DeviceBatch.land_mesh, DevicePlane.land_mesh,
TileEngine.landcover_mask_mesh, Context.land_mesh and the chain dswx_warp_device x 2, dswx_landcover_mask_device."""
import numpy as np
import pytest

try:                                              # before the library is loaded, as the suite's collection does it (test_gpu_streams.py)
    import torch
except ImportError:
    torch = None

from proteus_amd import _capi, pipeline, warp
from tests import _land_mesh_domain_cases as D

pytestmark = pytest.mark.gpu

SENT, PAD = 0xEE, 0xA5
ENTRY = D.entry_cases()


@pytest.fixture(scope='module')
def ctx():
    if torch is None:
        pytest.skip('no torch')
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def engine(ctx):
    e = pipeline.TileEngine(ctx)
    yield e
    e.close()


def dev(a, off=0):
    """(tensor that owns the memory, address) of a host array on the device, `off` bytes past an allocation's start, PAD around it."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    host = np.full(off + raw.size + 64, PAD, dtype=np.uint8)
    host[off:off + raw.size] = raw
    t = torch.from_numpy(host).to('cuda:0')
    return t, t.data_ptr() + off


def run_device(ctx, b, call=0, off=0, stream=None, twice=False, want=('land', 'head')):
    """One call of dswx_land_mesh_device on the windows and meshes of a case against the expected values of call number `call`
    (run_device of tests/test_gpu_land_mesh.py with the oracle in the host entry's place): the planes `off` bytes past an
    allocation's start -- an empty one is a NULL pointer --, the meshes 4-byte aligned and no more, land `off` bytes and head 8
    bytes into a buffer of SENT whose every other byte, the padding of a LAND stride included, stays SENT."""
    c = b.case
    spec = c.spec(call)
    n, (H, W) = c.n, c.shape
    land, head = b.expected(call)
    stride = spec.land_tile_stride or H * W
    exp_land = np.full((n, stride), SENT, np.uint8)
    exp_land[:, :H * W] = land.reshape(n, -1)
    keep = [dev(b.wc, off), dev(b.cg, off + 2), dev(b.m_wc, 4), dev(b.m_cg, 4)]
    land_bytes = n * stride
    head_at = -(-(256 + off + land_bytes + 64) // 256) * 256 + 8
    out = torch.full((head_at + n * 64 + 64,), SENT, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    for _ in range(2 if twice else 1):
        ctx.land_mesh_device(keep[0][1] if b.wc.size else None, b.wc.shape[1:], keep[1][1] if b.cg.size else None, b.cg.shape[1:], spec, n, H, W,
                             keep[2][1], keep[3][1], out.data_ptr() + 256 + off if 'land' in want else None,
                             out.data_ptr() + head_at if 'head' in want else None, stream=stream)
    ctx.synchronize(stream) if stream else ctx.synchronize()
    got = out.cpu().numpy()
    what = (c.name, call, spec.outside_wc, spec.outside_cg)
    written = np.zeros(got.size, dtype=bool)
    if 'land' in want:
        a, e = got[256 + off:256 + off + land_bytes], exp_land.reshape(-1)
        assert np.array_equal(a, e), (what, 'land', np.flatnonzero(a != e)[:8], a[a != e][:8], e[a != e][:8], int((a != e).sum()))
        written[256 + off:256 + off + land_bytes] = True
    if 'head' in want:
        a = got[head_at:head_at + n * 64].view(np.uint64).reshape(n, 8)
        assert np.array_equal(a, head), (what, 'head', a[:4], head[:4])
        written[head_at:head_at + n * 64] = True
    assert (got[~written] == SENT).all(), (what, 'bytes outside the outputs were written', np.flatnonzero((got != SENT) & ~written)[:8])
    for (t, _), src in zip(keep, (b.wc, b.cg)):
        assert (t.cpu().numpy()[:off] == PAD).all()


# ---- the value domain: lattices of at most 1024 rectangles -----------------------------------------------------------------

@pytest.mark.parametrize('k', range(D.N_SWEEP), ids=[c.name for c in D.SWEEP])
def test_device_entry_over_the_domain(ctx, k):
    b = D.built('sweep', k)
    for call in range(D.N_CALLS):
        run_device(ctx, b, call, off=(k + call) % 4)
    info = ctx.last_kernel_info()
    assert 'dswx_land_mesh_k' in info and f'grid=({D.rectangles(b.case.shape)},{b.case.n},1)' in info


# ---- the walk: more than 1024 rectangles -----------------------------------------------------------------------------------

@pytest.mark.parametrize('k', range(len(D.WALK)), ids=[c.name for c in D.WALK])
def test_device_entry_walks_past_the_grid(ctx, k):
    """A workgroup goes on with b += gridDim.x: fresh `cls`, `cnt` and `in` per rectangle, head sums over its two or three
    rectangles, the by / bx split of a large b.  Two tiles, LAND at a stride above the raster."""
    b = D.built('walk', k)
    want, twice = D.WALK_WANT[b.case.name]
    run_device(ctx, b, 0, off=1, twice=twice, want=want)
    info = ctx.last_kernel_info()
    print(f'{b.case.name}: {D.rectangles(b.case.shape)} rectangles: {info}')
    assert 'dswx_land_mesh_k' in info and 'grid=(1024,2,1)' in info and f"head={int('head' in want)}" in info


# ---- every way in ----------------------------------------------------------------------------------------------------------

IDS = [D.SWEEP[k].name for k in ENTRY]


@pytest.mark.parametrize('k', ENTRY, ids=IDS)
def test_batch_entry_with_a_tile_range(ctx, k):
    """DeviceBatch.land_mesh into tiles 1 .. n of a batch of n + 2 tiles: the oracle's bytes there, the other tiles as they were."""
    b = D.built('sweep', k)
    c = b.case
    land, head = b.expected(0)
    H, W = c.shape
    batch = _capi.DeviceBatch(ctx, c.n + 2, H, W, masks=True)
    try:
        for t in range(c.n + 2):
            batch.write_tile('land', t, np.full((H, W), 7, np.uint8))
        keep = [dev(b.wc), dev(b.cg), dev(b.m_wc), dev(b.m_cg)]
        heads = torch.full((c.n * 8,), -1, dtype=torch.int64, device='cuda:0')
        torch.cuda.synchronize()
        batch.land_mesh(keep[0][1], b.wc.shape[1:], keep[1][1], b.cg.shape[1:], c.spec(0), keep[2][1], keep[3][1], tile0=1, n_tiles=c.n,
                        head_ptr=heads.data_ptr())
        ctx.synchronize()
        for t in range(c.n + 2):
            assert np.array_equal(batch.read_tile('land', t), land[t - 1] if 1 <= t <= c.n else np.full((H, W), 7, np.uint8)), (c.name, t)
        assert np.array_equal(heads.cpu().numpy().view(np.uint64).reshape(c.n, 8), head)
    finally:
        batch.free()


@pytest.mark.parametrize('k', ENTRY, ids=IDS)
def test_plane_and_engine_entries(engine, k):
    """DevicePlane.land_mesh and TileEngine.landcover_mask_mesh, one tile at a time."""
    b = D.built('sweep', k)
    c = b.case
    land, head = b.expected(0)
    for t in range(c.n):
        wc, cg = engine.upload(b.wc[t]), engine.upload(b.cg[t])
        made = wc.land_mesh(cg, b.m_wc, b.m_cg, c.shape, c.spec(0))
        assert np.array_equal(made['land'].numpy(), land[t]) and np.array_equal(made['head'].numpy().reshape(-1), head[t]), (c.name, t)
        only = wc.land_mesh(cg, b.m_wc, b.m_cg, c.shape, c.spec(0), want=('land',))
        assert list(only) == ['land'] and np.array_equal(only['land'].numpy(), land[t])
        plane, words = engine.landcover_mask_mesh(wc, cg, b.m_wc, b.m_cg, c.shape, c.spec(0))
        assert np.array_equal(plane.numpy(), land[t]) and np.array_equal(words, head[t]), (c.name, t)
        for p in (wc, cg, made['land'], made['head'], only['land'], plane):
            p.release()


@pytest.mark.parametrize('k', ENTRY, ids=IDS)
def test_context_entry(ctx, k):
    """Context.land_mesh: host arrays in, host arrays out."""
    b = D.built('sweep', k)
    c = b.case
    land, head = b.expected(0)
    for t in range(c.n):
        got_land, got_head = ctx.land_mesh(b.wc[t], b.cg[t], b.m_wc, b.m_cg, c.shape, c.spec(0))
        assert np.array_equal(got_land, land[t]) and np.array_equal(got_head, head[t]), (c.name, t)


@pytest.mark.parametrize('k', ENTRY, ids=IDS)
def test_chain_of_the_existing_device_entries(ctx, k):
    """dswx_warp_device twice and then dswx_landcover_mask_device: the chain the entry is defined as gives the oracle's bytes too."""
    b = D.built('sweep', k)
    c = b.case
    spec = c.spec(0)
    land, _ = b.expected(0)
    n, (H, W) = c.n, c.shape
    keep = [dev(b.wc), dev(b.cg), dev(b.m_wc), dev(b.m_cg)]
    w3 = torch.zeros((n * 9 * H * W,), dtype=torch.uint8, device='cuda:0')
    c1 = torch.zeros((n * H * W,), dtype=torch.uint8, device='cuda:0')
    out = torch.zeros((n * H * W,), dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    ctx.warp_device(keep[0][1], warp.Spec(1, spec.shift_wc, spec.outside_wc), n, b.wc.shape[1], b.wc.shape[2], keep[2][1], 3 * H, 3 * W,
                    _capi.WarpOut.of(w3.data_ptr()))
    ctx.warp_device(keep[1][1], warp.Spec(1, spec.shift_cg, spec.outside_cg), n, b.cg.shape[1], b.cg.shape[2], keep[3][1], H, W,
                    _capi.WarpOut.of(c1.data_ptr()))
    ctx.landcover_mask_device(w3.data_ptr(), c1.data_ptr(), n, H, W, spec.forest_classes, out.data_ptr(), thresholds=spec.thresholds,
                              year_offset=spec.year_offset)
    ctx.synchronize()
    e_w3, e_c1 = b.warped(0)
    assert np.array_equal(w3.cpu().numpy().reshape(e_w3.shape), e_w3) and np.array_equal(c1.cpu().numpy().reshape(e_c1.shape), e_c1), c.name
    assert np.array_equal(out.cpu().numpy().reshape(n, H, W), land), c.name
