"""The land-mesh entry over its whole value domain and over lattices of more than 1024 rectangles, without a GPU: the library's
scalar statement (dswx_land_mesh_host) and the numpy statement (proteus_amd.landmesh.land_tiles) against expected values built
backwards from hand-padded rasters and the oracle (tests/_land_mesh_domain_cases.py says how), and the conditions on those inputs
that keep tests/test_gpu_land_mesh_domain.py from being vacuous."""
import os

import numpy as np
import pytest

from oracle import land_inputs as L
from proteus_amd import _capi, landmesh
from tests import _land_mesh_domain_cases as D
from tests.test_gpu_land_domain import YEAR_OFFSETS, rule_of


def check_head(head, shape):
    px = shape[0] * shape[1]
    assert (head[:, 0] == px).all() and (head[:, 7] == 0).all()
    assert (head[:, 1] + head[:, 2] == 9 * px).all() and (head[:, 3] + head[:, 4] == px).all()


def check_statements(b, call):
    """dswx_land_mesh_host and landmesh.land_tiles on the windows and meshes of a case against the expected values of a call."""
    c = b.case
    spec = c.spec(call)
    land, head = b.expected(call)
    check_head(head, c.shape)
    H, W = c.shape
    got = _capi.land_mesh_host(b.wc, b.cg, b.m_wc, b.m_cg, spec, c.shape,
                               land=np.full((c.n, spec.land_tile_stride), 0xEE, np.uint8) if spec.land_tile_stride else None)
    host_land = got['land'][:, :H * W].reshape(c.n, H, W)
    assert np.array_equal(host_land, land), (c.name, call, 'host land', int((host_land != land).sum()))
    assert np.array_equal(got['head'], head), (c.name, call, 'host head', got['head'], head)
    if spec.land_tile_stride:
        assert (got['land'][:, H * W:] == 0xEE).all()
    ref = landmesh.land_tiles(b.wc, b.cg, b.m_wc, b.m_cg, c.shape, spec.shift_wc, spec.shift_cg, spec.outside_wc, spec.outside_cg,
                              spec.thresholds, spec.year_offset, spec.forest_classes)
    assert np.array_equal(ref['land'], land), (c.name, call, 'numpy land', int((ref['land'] != land).sum()))
    assert np.array_equal(ref['head'], head), (c.name, call, 'numpy head', ref['head'], head)


def test_sweep_is_not_vacuous():
    """Conditions on the inputs, computed from the oracle-side rasters alone: every count 0 .. 9 of water, urban and tree, every
    step of the hierarchy, every byte among the WorldCover taps, among the CGLS taps and as each `outside` value, every count
    0 .. 9 of inside taps, every value of every axis, and both empty sources."""
    counts = [set(), set(), set()]
    rules, taps_wc, taps_cg, inside, out_wc, out_cg = set(), set(), set(), set(), set(), set()
    paired = aliased = 0
    for k, c in enumerate(D.SWEEP):
        b = D.built('sweep', k)
        inside |= set(np.unique(b.taps_inside).tolist())
        for call in range(D.N_CALLS):
            w3, c1 = b.warped(call)
            assert w3.shape == (c.n, 3 * c.shape[0], 3 * c.shape[1]) and c1.shape == (c.n,) + c.shape
            out_wc.add(c.outs[call][0])
            out_cg.add(c.outs[call][1])
            taps_wc |= set(np.unique(w3[:, b.in_wc]).tolist())
            taps_cg |= set(np.unique(c1[:, b.in_cg]).tolist())
            for t in range(c.n):
                for j, cnt in enumerate(L.counts(w3[t])):
                    counts[j] |= set(np.unique(cnt).tolist())
                rules |= set(np.unique(rule_of(w3[t], c1[t], c.forest, c.thresholds)).tolist())
        # the first call of a case with outside taps pairs a counted code with one of the case's forest classes
        if not b.in_wc.all() and not b.in_cg.all() and c.outs[0][0] in L.WC_CODES and c.outs[0][1] in (c.forest or []):
            paired += 1
        # ... and the second flips bit 7 of both bytes: where the oracle's LAND differs, a kernel that dropped the bit is seen
        assert c.outs[1] == (c.outs[0][0] ^ 128, c.outs[0][1] ^ 128)
        aliased += not np.array_equal(b.expected(0)[0], b.expected(1)[0])
    assert aliased >= 30
    assert counts == [set(range(10))] * 3
    assert rules == {0, 1, 2, 3, 4}
    assert taps_wc == set(range(256)) and taps_cg == set(range(256))
    assert out_wc == set(range(256)) and out_cg == set(range(256))
    assert inside == set(range(10))
    assert paired >= 30
    S = D.SWEEP
    assert len(S) == D.N_SWEEP and {c.shape for c in S} == set(D.LATTICES) and {c.modes[0] for c in S} == set(D.WC_MODES)
    assert {c.forest_key for c in S} == set(D.FOREST_KEYS) and {0, 31, 32, 223, 224, 255} < set(D.FOREST_KEYS)
    assert {c.thr_key for c in S} == set(L.THRESHOLD_SETS) and {c.year_offset for c in S} == set(YEAR_OFFSETS)
    assert {c.shifts for c in S} == {(a, b) for a in range(9) for b in range(9)}
    for j in range(4):
        assert {c.sub[j] for c in S} == {128, 0, 255, -1, 256}
    assert {c.n for c in S} == {2, 3} and all(len(set(map(str, c.modes))) == c.n for c in S)
    for j in range(4):                                                     # margins: different per side and per map, some of them 0
        for margins in ([c.margins_wc[j] for c in S], [c.margins_cg[j] for c in S]):
            assert 0 in margins and len(set(margins)) > 3
    assert any(len(set(c.margins_wc)) > 2 for c in S) and any(c.margins_wc != c.margins_cg for c in S)
    assert sum(D.built('sweep', k).wc.size == 0 for k in range(len(S))) == 1 and sum(D.built('sweep', k).cg.size == 0 for k in range(len(S))) == 1
    assert any(c.holes for c in S) and any(D.rectangles(c.shape) > 1 for c in S)
    # the other ways in: a dozen cases, nothing at its default
    E = D.entry_cases()
    assert len(E) == 12
    for k in E:
        c = S[k]
        assert c.thresholds != (6, 3, 7, 3) and c.forest and c.year_offset != 0 and 0 not in c.outs[0]
        assert D.built('sweep', k).wc.size and D.built('sweep', k).cg.size


def test_walk_lattices_pass_the_grid():
    """Each walk lattice has more than LM_MAX_GRID_X rectangles -- in one row, in one column, ragged in both directions, and
    more than twice as many -- and no sweep lattice has; the cuts leave outside taps on every side."""
    assert [D.rectangles(c.shape) for c in D.WALK] == [1031, 1031, 1144, 2050]
    assert all(D.rectangles(s) <= D.MAX_GRID_X for s in D.LATTICES)
    (a, b, c, d) = (w.shape for w in D.WALK)
    assert a[0] == D.RECT_H and b[1] < D.RECT_W and c[0] % D.RECT_H and c[1] % D.RECT_W and D.rectangles(d) > 2 * D.MAX_GRID_X
    hip = open(os.path.join(os.path.dirname(_capi.__file__), 'csrc', 'dswx_land_mesh.hip')).read()
    assert f'LM_MAX_GRID_X = {D.MAX_GRID_X};' in hip and (_capi.LAND_MESH_RECT_H, _capi.LAND_MESH_RECT_W) == (D.RECT_H, D.RECT_W)
    assert {want for want, _ in D.WALK_WANT.values()} == {('land', 'head'), ('head',), ('land',)}
    assert sum(twice for _, twice in D.WALK_WANT.values()) == 1
    assert all(c.n == 2 and c.land_pad > 0 and c.spec().land_tile_stride > c.shape[0] * c.shape[1] for c in D.WALK)


def test_none_and_empty_forest_lists_are_a_null_pointer():
    for key in ('none', 'empty'):
        c = next(c for c in D.SWEEP if c.forest_key == key)
        s = _capi.LandMeshSpec.of(c.spec())
        assert s.forest_classes is None and s.n_forest_classes == 0
    s = _capi.LandMeshSpec.of(next(c for c in D.SWEEP if c.forest_key == 224).spec())
    assert s.forest_classes is not None and s.n_forest_classes == 1


@pytest.mark.parametrize('k', range(D.N_SWEEP), ids=[c.name for c in D.SWEEP])
def test_host_entry_and_numpy_statement_over_the_domain(k):
    b = D.built('sweep', k)
    for call in range(D.N_CALLS):
        check_statements(b, call)


@pytest.mark.parametrize('k', (0, 2), ids=[D.WALK[k].name for k in (0, 2)])
def test_host_entry_and_numpy_statement_on_walk_lattices(k):
    b = D.built('walk', k)
    check_statements(b, 0)
    land, head = b.expected(0)
    assert len(np.unique(land)) >= 4 and 0 < head[0, 2] and 0 < head[0, 4] and 0 < head[0, 5] and 0 < head[0, 6] < land[0].size
