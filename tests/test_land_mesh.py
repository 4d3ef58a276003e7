"""The LAND layer read through two coordinate meshes (include/dswx_hip.h "land mesh") without a GPU: the numpy statement
(proteus_amd/landmesh.py), the library's scalar statement (dswx_land_mesh_host) and the chain it is defined as -- warp, warp,
landcover mask -- agree on every byte; the reference's own LAND output through identity meshes; refusals; the plan."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import dswx_oracle as O
from proteus_amd import _capi, geotiff, landmesh, warp
from tests import _golden as G
from tests import _land_mesh_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAND_GOLDENS = sorted(os.path.basename(p)[5:-4] for p in __import__('glob').glob(os.path.join(G.GOLDEN_DIR, 'land_*.npz')))


def chain(wc, cg, m_wc, m_cg, shape, spec, host):
    """The definition: the two warps (warp.warp_tiles, or the host entry dswx_warp_host) and then the oracle's aggregation."""
    H, W = shape
    if host:
        w3 = _capi.warp_host(wc, m_wc, warp.Spec(1, spec.shift_wc, spec.outside_wc, mesh_tile_stride_nodes=spec.mesh_wc_tile_stride_nodes),
                             (3 * H, 3 * W), want=('dst',))['dst']
        c1 = _capi.warp_host(cg, m_cg, warp.Spec(1, spec.shift_cg, spec.outside_cg, mesh_tile_stride_nodes=spec.mesh_cg_tile_stride_nodes),
                             (H, W), want=('dst',))['dst']
    else:
        w3 = warp.warp_tiles(wc, m_wc, spec.shift_wc, (3 * H, 3 * W), spec.outside_wc)['dst']
        c1 = warp.warp_tiles(cg, m_cg, spec.shift_cg, (H, W), spec.outside_cg)['dst']
    return np.stack([O.landcover_mask_from_warped(w3[t], c1[t], spec.forest_classes, year=2000 + spec.year_offset, thresholds=spec.thresholds)
                     for t in range(wc.shape[0])]) if wc.shape[0] else np.zeros((0, H, W), np.uint8)


def check_all(wc, cg, m_wc, m_cg, shape, spec):
    """Every statement on every byte; returns the numpy statement's outputs."""
    ref = C.numpy_land(wc, cg, m_wc, m_cg, shape, spec)
    got = _capi.land_mesh_host(wc, cg, m_wc, m_cg, spec, shape)
    assert np.array_equal(got['land'], ref['land']) and np.array_equal(got['head'], ref['head'])
    if shape[0] * shape[1] and -1000 < spec.year_offset < 1000:          # (the oracle adds the year in Python integers)
        for host in (False, True):
            assert np.array_equal(chain(wc, cg, m_wc, m_cg, shape, spec, host), ref['land']), host
    h = ref['head']
    px = shape[0] * shape[1]
    assert (h[:, 0] == px).all() and (h[:, 1] + h[:, 2] == 9 * px).all() and (h[:, 3] + h[:, 4] == px).all() and (h[:, 7] == 0).all()
    return ref


@pytest.mark.parametrize('name', LAND_GOLDENS)
@pytest.mark.parametrize('shift', (0, 3, 6, 8))
def test_reference_land_through_identity_meshes(name, shift):
    """The inputs of every tests/golden/land_*.npz -- maps the reference warped itself -- through identity meshes (fine pixel
    (x, y) -> the centre of source pixel (x, y)) give the reference's own LAND."""
    z = G.load(f'land_{name}.npz')
    wc, cg = z['worldcover_up3'][None], z['copernicus'][None]
    H, W = cg.shape[1:]
    thr = [int(v) for v in z['thresholds']]
    spec = C.spec_of(shift, 8 - shift if shift else 0, outside_wc=80, outside_cg=111, thresholds=thr, year_offset=int(z['year']) - 2000,
                     forest_classes=[int(v) for v in z['forest_classes']])
    m_wc, m_cg = C.identity_mesh((3 * H, 3 * W), spec.shift_wc), C.identity_mesh((H, W), spec.shift_cg)
    got = _capi.land_mesh_host(wc, cg, m_wc, m_cg, spec, (H, W))
    assert np.array_equal(got['land'][0], z['land'])
    assert got['head'][0].tolist() == [H * W, 9 * H * W, 0, H * W, 0, 0, int((z['land'] == 255).sum()), 0]
    assert np.array_equal(C.numpy_land(wc, cg, m_wc, m_cg, (H, W), spec)['land'][0], z['land'])


@pytest.mark.parametrize('lat', C.LATITUDES)
def test_geographic_meshes(lat):
    """Maps in EPSG:4326 at their real pixel sizes under 40 x 52 HLS pixels, different shifts for the two maps."""
    rng = np.random.default_rng(int(lat * 10))
    for s_wc, s_cg in ((5, 3), (6, 4), (4, 6)):
        wc, cg, m_wc, m_cg = C.geographic_case(rng, lat, shift_wc=s_wc, shift_cg=s_cg)
        ref = check_all(wc, cg, m_wc, m_cg, (40, 52), C.spec_of(s_wc, s_cg, year_offset=21))
        assert ref['head'][0, 2] == 0 and ref['head'][0, 4] == 0          # the windows cover every tap
        assert len(np.unique(ref['land'])) >= 4


@pytest.mark.parametrize('shift', range(9))
def test_every_shift(shift):
    rng = np.random.default_rng(shift)
    H, W = 11, 13
    wc, cg = C.maps(rng, 2, (50, 70), (14, 17))
    m_wc = C.identity_mesh((3 * H, 3 * W), shift, scale=(400, 350), offset=(-900, 300))
    m_cg = C.identity_mesh((H, W), 8 - shift, scale=(300, 310), offset=(40, -500))
    ref = check_all(wc, cg, m_wc, m_cg, (H, W), C.spec_of(shift, 8 - shift, outside_wc=50, outside_cg=113, year_offset=20))
    assert 0 < ref['head'][0, 2] < 9 * H * W and 0 < ref['head'][0, 4] < H * W


def test_garbage_meshes_with_int32_extremes():
    rng = np.random.default_rng(7)
    for shift in (0, 2, 5, 8):
        H, W = 9, 14
        wc, cg = C.maps(rng, 3, (60, 90), (20, 30))
        m_wc, m_cg = C.garbage_mesh(rng, (3 * H, 3 * W), shift, 3), C.garbage_mesh(rng, (H, W), shift, 3)
        mh, mw = warp.mesh_shape((3 * H, 3 * W), shift)
        ch, cw = warp.mesh_shape((H, W), shift)
        m_wc[0, 0, 0], m_wc[0, -1, -1] = (-(1 << 31), (1 << 31) - 1), ((1 << 31) - 1, -(1 << 31))
        spec = C.spec_of(shift, shift, outside_wc=10, outside_cg=111, mesh_wc_tile_stride_nodes=mh * mw, mesh_cg_tile_stride_nodes=ch * cw)
        ref = check_all(wc, cg, m_wc, m_cg, (H, W), spec)
        assert ref['head'][:, 2].sum() > 0 and (shift > 2 or ref['head'][:, 1].sum() > 0)      # (one huge node empties a large cell)


def test_maps_covering_half_the_tile_and_empty_sources():
    rng = np.random.default_rng(11)
    H, W = 12, 16
    wc, cg = C.maps(rng, 1, (36, 24), (6, 16))              # the left half of the fine lattice, the upper half of the HLS lattice
    m_wc, m_cg = C.identity_mesh((3 * H, 3 * W), 3), C.identity_mesh((H, W), 2)
    ref = check_all(wc, cg, m_wc, m_cg, (H, W), C.spec_of(3, 2, outside_wc=0, outside_cg=0))
    assert ref['head'][0].tolist()[:6] == [H * W, 36 * 24, 36 * 24, 6 * 16, 6 * 16, H * W // 2]
    assert (ref['land'][0][:, W // 2:] == 255).all()
    # an empty source: every tap is `outside`
    none_wc, none_cg = np.zeros((1, 0, 5), np.uint8), np.zeros((1, 7, 0), np.uint8)
    water = check_all(none_wc, none_cg, m_wc, m_cg, (H, W), C.spec_of(3, 2, outside_wc=80, outside_cg=111))
    assert (water['land'] == 200).all() and water['head'][0].tolist() == [H * W, 0, 9 * H * W, 0, H * W, H * W, 0, 0]
    nothing = check_all(none_wc, cg, m_wc, m_cg, (H, W), C.spec_of(3, 2, outside_wc=0))
    assert (nothing['land'] == 255).all() and nothing['head'][0, 6] == H * W
    trees = check_all(none_wc, none_cg, m_wc, m_cg, (H, W), C.spec_of(3, 2, outside_wc=10, outside_cg=111))
    assert (trees['land'] == 201).all()


def test_forest_lists_thresholds_and_the_uint8_wrap():
    rng = np.random.default_rng(13)
    H, W = 10, 12
    wc, cg = C.maps(rng, 2, (30, 36), (10, 12))
    m_wc, m_cg = C.identity_mesh((3 * H, 3 * W), 4), C.identity_mesh((H, W), 1)
    no_forest = check_all(wc, cg, m_wc, m_cg, (H, W), C.spec_of(4, 1, forest_classes=()))
    assert not (no_forest['land'] == 201).any()
    assert (check_all(wc, cg, m_wc, m_cg, (H, W), C.spec_of(4, 1))['land'] == 201).any()
    for thr, year in (((6, 3, 7, 3), 21), ((0, 0, 0, 0), 0), ((10, 10, 10, 10), 5), ((-5, 1, 2, 10), 200), ((1, 1, 10, 10), 157),
                      ((10, 1, 1, 10), -1), ((2, 2, 3, 9), 999), ((-(1 << 31), (1 << 31) - 1, 1, 10), 356)):
        ref = check_all(wc, cg, m_wc, m_cg, (H, W), C.spec_of(4, 1, thresholds=thr, year_offset=year))
        assert set(np.unique(ref['land'])) <= {255, 201, 200, year & 255, (100 + year) & 255}
    # beyond what the oracle's Python integers are asked: the library's own wrap of INT32 extremes against the numpy statement
    for year in ((1 << 31) - 1, -(1 << 31)):
        spec = C.spec_of(4, 1, thresholds=(10, 1, 2, 10), year_offset=year)
        got = _capi.land_mesh_host(wc, cg, m_wc, m_cg, spec, (H, W))['land']
        assert np.array_equal(got, C.numpy_land(wc, cg, m_wc, m_cg, (H, W), spec)['land']) and ((got == (year & 255)) | (got == ((100 + year) & 255)) | (got == 255)).all()


@pytest.mark.parametrize('shape', ((1, 1), (3, 5), (0, 4), (4, 0)))
def test_small_and_empty_lattices(shape):
    rng = np.random.default_rng(17)
    H, W = shape
    wc, cg = C.maps(rng, 2, (9, 15), (3, 5))
    m_wc, m_cg = C.identity_mesh((3 * H, 3 * W), 2), C.identity_mesh((H, W), 0)
    ref = check_all(wc, cg, m_wc, m_cg, shape, C.spec_of(2, 0))
    assert ref['land'].shape == (2, H, W)
    if H * W == 0:
        head = np.full((2, 8), 77, np.uint64)              # an empty lattice writes nothing
        spec = _capi.LandMeshSpec.of(C.spec_of(2, 0))
        assert _capi.load_library().dswx_land_mesh_host(wc.ctypes.data, 9, 15, cg.ctypes.data, 3, 5, ctypes.byref(spec), 2, H, W, m_wc.ctypes.data,
                                                        m_cg.ctypes.data, None, head.ctypes.data) == 0
        assert (head == 77).all()


def test_three_tiles_padded_strides_per_tile_meshes_and_a_land_stride():
    rng = np.random.default_rng(19)
    H, W, n = 7, 9, 3
    wc, cg = C.maps(rng, n, (25, 31), (9, 10))
    mh, mw = warp.mesh_shape((3 * H, 3 * W), 3)
    ch, cw = warp.mesh_shape((H, W), 1)
    m_wc = np.stack([C.identity_mesh((3 * H, 3 * W), 3, scale=(256 + 30 * t, 256 - 20 * t), offset=(128 - 400 * t, 128)) for t in range(n)])
    m_cg = np.stack([C.identity_mesh((H, W), 1, scale=(256, 300), offset=(128, 128 - 300 * t)) for t in range(n)])
    packed = C.spec_of(3, 1, mesh_wc_tile_stride_nodes=mh * mw, mesh_cg_tile_stride_nodes=ch * cw, year_offset=21)
    ref = check_all(wc, cg, m_wc, m_cg, (H, W), packed)
    # the same tiles in padded planes, the meshes three nodes apart, LAND 11 bytes apart
    wcp, cgp = np.full((n, 25 * 31 + 13), 80, np.uint8), np.full((n, 9 * 10 + 6), 111, np.uint8)
    wcp[:, :25 * 31], cgp[:, :90] = wc.reshape(n, -1), cg.reshape(n, -1)
    mwp, mcp = np.full((n, mh * mw + 3, 2), 12345, np.int32), np.full((n, ch * cw + 5, 2), -999, np.int32)
    mwp[:, :mh * mw], mcp[:, :ch * cw] = m_wc.reshape(n, -1, 2), m_cg.reshape(n, -1, 2)
    spec = C.spec_of(3, 1, wc_tile_stride=25 * 31 + 13, cg_tile_stride=96, mesh_wc_tile_stride_nodes=mh * mw + 3,
                     mesh_cg_tile_stride_nodes=ch * cw + 5, land_tile_stride=H * W + 11, year_offset=21)
    land = np.full((n, H * W + 11), 0xA5, np.uint8)
    got = _capi.land_mesh_host(wcp, cgp, mwp, mcp, spec, (H, W), wc_raster=(25, 31), cg_raster=(9, 10), land=land)
    assert got['land'] is land and np.array_equal(land[:, :H * W].reshape(n, H, W), ref['land']) and (land[:, H * W:] == 0xA5).all()
    assert np.array_equal(got['head'], ref['head'])
    assert not np.array_equal(ref['land'][0], ref['land'][1])


def test_refusals_write_nothing():
    """Every refusal with its code and its text, in the order of the checks; a refused call leaves land and head as they were."""
    rng = np.random.default_rng(23)
    H, W = 4, 6
    wc, cg = C.maps(rng, 2, (12, 18), (4, 6))
    m_wc, m_cg = C.identity_mesh((3 * H, 3 * W), 2), C.identity_mesh((H, W), 1)
    lib = _capi.load_library()
    land, head = np.full((2, H, W), 0xA5, np.uint8), np.full((2, 8), 0xA5A5, np.uint64)

    def call(spec=None, n=2, h=H, w=W, wc_dims=(12, 18), cg_dims=(4, 6), wc_p=True, cg_p=True, mw_p=True, mc_p=True, null_spec=False, **fields):
        s = _capi.LandMeshSpec.of(spec or C.spec_of(2, 1))
        for k, v in fields.items():
            setattr(s, k, v)
        rc = lib.dswx_land_mesh_host(wc.ctypes.data if wc_p else None, wc_dims[0], wc_dims[1], cg.ctypes.data if cg_p else None, cg_dims[0],
                                     cg_dims[1], None if null_spec else ctypes.byref(s), n, h, w, m_wc.ctypes.data if mw_p else None,
                                     m_cg.ctypes.data if mc_p else None, land.ctypes.data, head.ctypes.data)
        return rc, lib.dswx_last_error().decode()

    big = 1 << 30
    cases = [
        (dict(null_spec=True), 'spec is NULL'),
        (dict(reserved2=1), 'reserved2 is 1, not 0'),
        (dict(outside_wc=256), 'outside 0 .. 255'),
        (dict(outside_cg=1 << 31), 'outside 0 .. 255'),
        (dict(n_forest_classes=-1), 'bad size'),
        (dict(n_forest_classes=2, forest_classes=None), 'bad size'),
        (dict(h=-1), 'negative size'),
        (dict(w=-1), 'negative size'),
        (dict(h=1 << 14, w=(1 << 13) + 1), 'above 2^30 / 9 pixels'),
        (dict(h=big, w=1), 'above 2^30 / 9 pixels'),
        (dict(shift_wc=9), 'shift 9 outside 0 .. 8'),
        (dict(shift_wc=-1), 'shift -1 outside 0 .. 8'),
        (dict(reserved=7), 'reserved is 7, not 0'),
        (dict(n=-1), 'negative size'),
        (dict(wc_dims=(-1, 18)), 'negative size'),
        (dict(wc_tile_stride=-1), 'negative stride'),
        (dict(mesh_wc_tile_stride_nodes=-1), 'negative stride'),
        (dict(wc_dims=(1 << 15, (1 << 15) + 1)), 'above 2^30 pixels'),
        (dict(wc_tile_stride=12 * 18 - 1), 'src_tile_stride smaller than the tile'),
        (dict(mesh_wc_tile_stride_nodes=1), 'mesh_tile_stride_nodes 1 smaller than the mesh'),
        (dict(shift_cg=9), 'shift 9 outside 0 .. 8'),
        (dict(cg_dims=(4, -6)), 'negative size'),
        (dict(cg_tile_stride=-5), 'negative stride'),
        (dict(cg_dims=(big, 2)), 'above 2^30 pixels'),
        (dict(cg_tile_stride=23), 'src_tile_stride smaller than the tile'),
        (dict(mesh_cg_tile_stride_nodes=2), 'mesh_tile_stride_nodes 2 smaller than the mesh'),
        (dict(n=(1 << 32) + 1), 'more than 2^32 tiles'),
        (dict(wc_tile_stride=(1 << 46) + 1), 'plane too large'),
        (dict(land_tile_stride=-1), 'negative stride'),
        (dict(land_tile_stride=H * W - 1), 'land_tile_stride smaller than the raster'),
        (dict(land_tile_stride=(1 << 46) + 1), 'plane too large'),
        (dict(mw_p=False), 'mesh_wc is NULL'),
        (dict(mc_p=False), 'mesh_cg is NULL'),
        (dict(wc_p=False), 'worldcover is NULL'),
        (dict(cg_p=False), 'copernicus is NULL'),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == _capi.ERR_ARG and text in msg, (kw, rc, msg)
        assert (land == 0xA5).all() and (head == 0xA5A5).all(), kw
    # a NULL plane of an empty raster is not an error, and neither is a call with nothing to do
    assert call(wc_p=False, wc_dims=(0, 18))[0] == 0 and (land == 255).all()
    land[:] = 0xA5
    head[:] = 0xA5A5
    assert call(n=0, mw_p=False, mc_p=False, wc_p=False, cg_p=False)[0] == 0 and (land == 0xA5).all() and (head == 0xA5A5).all()
    # the Python forms refuse what they can see
    with pytest.raises(ValueError, match='outside 0 .. 8'):
        C.spec_of(9, 0)
    with pytest.raises(ValueError, match='outside 0 .. 255'):
        C.spec_of(0, 0, outside_cg=256)
    with pytest.raises(ValueError, match='too small'):
        _capi.land_mesh_host(wc, cg, m_wc[:-1], m_cg, C.spec_of(2, 1), (H, W))
    with pytest.raises(ValueError, match='CGLS tiles'):
        _capi.land_mesh_host(wc, cg[:1], m_wc, m_cg, C.spec_of(2, 1), (H, W))


def test_header_says_has_land_mesh_and_the_struct_mirror_matches(tmp_path):
    text = open(os.path.join(ROOT, 'include', 'dswx_hip.h')).read()
    section = text.split('---- land mesh')[1].split('---- device plumbing')[0]
    assert '#define DSWX_HAS_LAND_MESH 1' in section and '#define DSWX_ABI_VERSION 7' in text and _capi.HAS_LAND_MESH == 1
    assert 'STILL REFUSED' in section and 'UNPINNED' in section and 'THE DEFINITION' in section
    for name in ('dswx_land_mesh_device', 'dswx_land_mesh_host'):
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(_capi.load_library(), name)
    S = _capi.LandMeshSpec
    assert ctypes.sizeof(S) == 96 and _capi.LAND_MESH_HEAD_WORDS == 8
    offsets = {f: getattr(S, f).offset for f, _ in S._fields_}
    cxx = shutil.which('g++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('needs a C++ compiler')
    src = tmp_path / 'layout.cpp'
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "dswx_hip.h"\nint main() {\n  printf("{\\"size\\": %zu", sizeof(dswx_land_mesh_spec_t));\n'
                   + ''.join(f'  printf(", \\"{f}\\": %zu", offsetof(dswx_land_mesh_spec_t, {f}));\n' for f in offsets)
                   + '  printf(", \\"has\\": %d, \\"words\\": %d}\\n", DSWX_HAS_LAND_MESH, DSWX_LAND_MESH_HEAD_WORDS);\n  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.run([cxx, '-std=c++17', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True, capture_output=True)
    out = json.loads(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert out.pop('size') == 96 and out.pop('has') == 1 and out.pop('words') == 8 and out == offsets
    # the kernel's geometry that the GPU tests build their shapes around
    hip = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_land_mesh.hip')).read()
    assert f'LM_RECT_H = {_capi.LAND_MESH_RECT_H}, LM_RECT_W = {_capi.LAND_MESH_RECT_W};' in hip


def test_rule_and_host_entry_under_asan_and_ubsan_in_a_program_of_their_own():
    """tests/native/land_mesh_host_san.cpp with proteus_amd/csrc/dswx_land_mesh.hip (and dswx_warp.hip, whose geometry checks it
    shares) compiled into it, host code under ASan + UBSan: the rule header's host form over garbage meshes and tiny rasters on
    heap blocks of exactly the bytes the entry may touch, at odd addresses, against a plain loop with 128-bit positions.  A
    child process; nothing is loaded into this interpreter."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('needs hipcc')
    out_dir = os.path.join(ROOT, 'tests', 'native', '_build')
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, 'land_mesh_host_san')
    csrc = os.path.join(ROOT, 'proteus_amd', 'csrc')
    cmd = [hipcc, '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-ffp-contract=off', '-Wall', '-Wno-unused-function',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           '-I', os.path.join(ROOT, 'include'), '-I', csrc,
           os.path.join(ROOT, 'tests', 'native', 'land_mesh_host_san.cpp'), os.path.join(csrc, 'dswx_land_mesh.hip'), os.path.join(csrc, 'dswx_warp.hip'),
           '-o', exe]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0 and 'libclang_rt.asan' in res.stderr:     # (only the runtime: an error in the sources must fail)
        pytest.skip(f'sanitizer runtime missing: {res.stderr[-300:]}')
    assert res.returncode == 0, res.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-4000:])
    assert 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr and 'LeakSanitizer' not in res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out['failures'] == 0 and out['cases'] >= 200


# ---- the plan ------------------------------------------------------------------------------------------------------------

class Info:
    """What geotiff.open_geotiff(...).info tells the plan about a map file."""

    def __init__(self, gt, epsg, height, width, dtype=np.uint8, bands=1):
        self.geotransform, self.height, self.width, self.dtype, self.bands = gt, height, width, np.dtype(dtype), bands
        self.geo_tags = geotiff.geo_tags_from_geotransform(gt or (0, 1, 0, 0, 0, -1), epsg) if epsg is not None else {}


@pytest.mark.parametrize('lat', C.LATITUDES)
def test_plan_on_the_three_latitudes(lat):
    """The window covers every tap, the shift is the first of 6, 5, 4 whose mesh deviates by at most 1/256 source pixel, and the
    mesh is relative to the window."""
    H, W = 96, 128
    gt, epsg = C.hls_grid(lat, (H, W))
    tags = geotiff.geo_tags_from_geotransform(gt, epsg)
    for pixel, scale in ((C.WC_PIXEL, 3), (C.CG_PIXEL, 1)):
        src_gt = C.map_gt(lat, pixel)
        info = Info(src_gt, 4326, int(round(4.0 / pixel)), int(round(2.0 / pixel)))
        window, mesh, shift, deviation = landmesh.plan(info, gt, tags, H, W, scale)
        assert shift in landmesh.MESH_SHIFTS and deviation <= 1.0
        dst_gt = (gt[0], gt[1] / scale, 0.0, gt[3], 0.0, gt[5] / scale)
        for s in landmesh.MESH_SHIFTS[:landmesh.MESH_SHIFTS.index(shift)]:
            assert warp.mesh_between(src_gt, 4326, dst_gt, epsg, (scale * H, scale * W), s)[1] > 1.0
        full, dev = warp.mesh_between(src_gt, 4326, dst_gt, epsg, (scale * H, scale * W), shift)
        assert dev == deviation and np.array_equal(mesh.astype(np.int64) + 256 * np.array(window[:2]), full.astype(np.int64))
        sx, sy = warp.positions(mesh, shift, (scale * H, scale * W))
        c, r = sx >> 8, sy >> 8
        assert c.min() >= 0 and r.min() >= 0 and c.max() < window[2] and r.max() < window[3]
        # ... and is no larger than the taps, a margin of two pixels and the last cell, whose far nodes lie past the lattice
        m = mesh.astype(np.int64)
        cell_w, cell_h = int(np.abs(np.diff(m[..., 0], axis=1)).max() >> 8) + 1, int(np.abs(np.diff(m[..., 1], axis=0)).max() >> 8) + 1
        assert window[2] <= c.max() - c.min() + 1 + 4 + cell_w and window[3] <= r.max() - r.min() + 1 + 4 + cell_h


def test_plan_takes_and_refuses():
    H, W = 64, 64
    gt, epsg = C.hls_grid(45.0, (H, W))
    tags = geotiff.geo_tags_from_geotransform(gt, epsg)
    geo = C.map_gt(45.0, C.CG_PIXEL)
    # the product's own SRS off the grid, and a neighbouring UTM zone, are taken
    own = Info((gt[0] - 1234.5, 100.0, 0.0, gt[3] + 777.0, 0.0, -100.0), epsg, 400, 400)
    window, mesh, shift, deviation = landmesh.plan(own, gt, tags, H, W, 1)
    assert deviation == 0.0 and shift == 6 and window[2] > 0
    landmesh.plan(Info((300000.0, 100.0, 0.0, gt[3] + 5000.0, 0.0, -100.0), epsg + 1, 4000, 8000), gt, tags, H, W, 1)
    # a map that misses the tile has an empty window
    assert landmesh.plan(Info((geo[0], geo[1], 0.0, 10.0, 0.0, geo[5]), 4326, 100, 100), gt, tags, H, W, 1)[0] == (0, 0, 0, 0)
    for info, text in ((Info((geo[0], geo[1], 1e-9, geo[3], 0.0, geo[5]), 4326, 4000, 2000), 'rotated'),
                       (Info(geo, 3857, 4000, 2000), 'not WGS 84 / UTM'),
                       (Info(geo, None, 4000, 2000), 'names no SRS'),
                       (Info(geo, 4326, 4000, 2000, dtype=np.int16), 'not one uint8 band'),
                       (Info(geo, 4326, 4000, 2000, bands=3), 'not one uint8 band'),
                       (Info(None, 4326, 4000, 2000), 'no geotransform')):
        with pytest.raises(NotImplementedError, match=text) as e:
            landmesh.plan(info, gt, tags, H, W, 1)
        assert 'is taken' in str(e.value)
    # the antimeridian
    _, north = warp.tm_forward(177.0, 45.0, 177.0)
    across = (730000.0, 30.0, 0.0, float(north), 0.0, -30.0)
    with pytest.raises(NotImplementedError, match='antimeridian'):
        landmesh.plan(Info((170.0, C.CG_PIXEL, 0.0, 47.0, 0.0, -C.CG_PIXEL), 4326, 4000, 12000), across, geotiff.geo_tags_from_geotransform(across, 32660), 512, 512, 1)
    # a window above 2^30 pixels: a map of 1/120000 degree under 3 x 1100 pixels
    fine = Info((geo[0], 1e-6, 0.0, geo[3], 0.0, -1e-6), 4326, 4_000_000, 2_000_000)
    g2, _ = C.hls_grid(45.0, (1100, 1100))
    with pytest.raises(NotImplementedError, match='more than 2\\^30 pixels'):
        landmesh.plan(fine, g2, geotiff.geo_tags_from_geotransform(g2, epsg), 1100, 1100, 3)
