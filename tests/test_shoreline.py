"""proteus_amd.shoreline on the host: the shapefile reader held to files this test writes itself with `struct`; `plan` end to end
on a synthetic coast in degrees at 45 and 70 degrees north, against a floating-point statement in metres through tm_forward;
every refusal text, and the unchanged refusal of a .shp without rasterise_shoreline.  No GPU."""
import os

import numpy as np
import pytest

from proteus_amd import _capi, shoreline
from proteus_amd import dswx_hls as D
from tests import _shoreline_cases as S


def test_read_shp_is_held_to_what_was_written(tmp_path):
    rng = np.random.default_rng(1)
    outer = S.clockwise(rng.uniform(-5, 5, size=(7, 2)))
    hole = S.clockwise(np.array([(0.1, 0.1), (0.4, 0.1), (0.3, 0.5)]), False)
    tri = S.clockwise(np.array([(10.0, 50.0), (11.0, 50.0), (10.5, 51.0)]))
    two = [S.clockwise(np.array([(20.0, 0.0), (21.0, 0.0), (20.5, 1.0)])), S.clockwise(np.array([(30.0, 0.0), (31.0, 0.0), (30.5, 1.0)]))]
    recs = [('null', None), ('polygon', [outer, hole]), ('point', (3.0, 4.0)), ('polygonz', [tri]), ('polygonm', [tri + 1.0]), ('polygon', two)]
    for shx in (True, False):
        path = S.write_shp(str(tmp_path / f'a{int(shx)}.shp'), recs, shx=shx)
        assert os.path.exists(path[:-4] + '.shx') == shx
        with shoreline.read_shp(path) as shp:
            assert len(shp) == 4 and shp.record.tolist() == [1, 3, 4, 5] and shp.skipped_types == 2 and shp.epsg == 4326
            want_box = [[g[0][:, 0].min(), g[0][:, 1].min(), g[0][:, 0].max(), g[0][:, 1].max()] for _, g in (recs[1], recs[3], recs[4])]
            assert np.array_equal(shp.bbox[:3], np.array(want_box)) and shp.bbox[3].tolist() == [20.0, 0.0, 31.0, 1.0]
            got = shp.rings(0)
            assert len(got) == 2 and np.array_equal(got[0], outer) and np.array_equal(got[1], hole)
            assert shoreline.shoelace(got[0]) < 0 < shoreline.shoelace(got[1]) and shoreline.outer_rings(got) == 1
            assert np.array_equal(shp.rings(1)[0], tri) and np.array_equal(shp.rings(2)[0], tri + 1.0)      # x and y of Z and M records
            assert shoreline.outer_rings(shp.rings(3)) == 2
    with pytest.raises(ValueError, match='not a shapefile'):
        bad = tmp_path / 'bad.shp'
        bad.write_bytes(b'\0' * 200)
        shoreline.read_shp(str(bad))
    # the SRS of a .prj: ESRI's and OGC's spellings
    assert shoreline.epsg_of_wkt(S.WGS84_PRJ) == 4326 and shoreline.epsg_of_wkt(S.utm_prj(33)) == 32633
    assert shoreline.epsg_of_wkt(S.utm_prj(7, south=True)) == 32707
    assert shoreline.epsg_of_wkt('PROJCS["WGS 84 / UTM zone 15N",GEOGCS["WGS 84",DATUM["WGS_1984"]],AUTHORITY["EPSG","32615"]]') == 32615
    assert shoreline.epsg_of_wkt('GEOGCS["NAD27",DATUM["North_American_Datum_1927"],AUTHORITY["EPSG","4267"]]') == 4267
    assert shoreline.epsg_of_wkt('PROJCS["NAD83 / UTM zone 15N",GEOGCS["NAD83"],AUTHORITY["EPSG","26915"]]') == 26915
    assert shoreline.epsg_of_wkt('LOCAL_CS["x"]') is None


def test_clip_ring_against_the_scalar_clip_and_the_edges_on_the_sides():
    rng = np.random.default_rng(5)
    rect = (-1.0, -2.0, 3.0, 2.5)
    for trial in range(40):
        ring = rng.uniform(-6, 6, size=(int(rng.integers(3, 12)), 2))
        got, on_side = shoreline.clip_ring(ring, rect)
        want = S.scalar_clip(ring, rect)
        want = want[np.append((want[1:] != want[:-1]).any(axis=1), True)] if len(want) else want
        if len(want) > 1 and (want[0] == want[-1]).all():
            want = want[:-1]
        # (the same cycle: the two begin it at different vertices)
        assert len(got) == len(want) and any(np.array_equal(np.roll(want, k, axis=0), got) for k in range(max(len(want), 1))), trial
        nxt = np.roll(got, -1, axis=0)
        for i in range(len(got)):
            on = any(got[i, a] == v and nxt[i, a] == v for a, v in ((0, rect[0]), (0, rect[2]), (1, rect[1]), (1, rect[3])))
            assert on == on_side[i]
    inside = np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)])
    got, on_side = shoreline.clip_ring(inside, rect)
    assert np.array_equal(got, inside) and not on_side.any()
    assert len(shoreline.clip_ring(inside + 50.0, rect)[0]) == 0


def test_colours_share_a_bit_only_between_disjoint_boxes():
    boxes = np.array([[0, 0, 4, 4], [5, 5, 9, 9], [4, 4, 6, 6], [20, 0, 22, 2], [0, 0, 30, 30]])
    assert shoreline.colours_of(boxes).tolist() == [0, 0, 1, 0, 2]
    assert shoreline.colours_of(np.zeros((0, 4), dtype=np.int64)).tolist() == []


@pytest.mark.parametrize('lat,many', ((45.0, False), (70.0, True)))
def test_plan_end_to_end_against_the_float_statement_in_metres(tmp_path, lat, many):
    """A coast in degrees with islands whose boxes overlap and islands whose boxes do not, a mainland that spans hundreds of
    kilometres beyond the clip rectangle, a record with two outer rings: burn + reach of the plan's tables (numpy statements and
    host entries) equals inside OR distance <= margin wherever the distance is further than 0.05 pixel from the margin; at most
    1 % of the pixels abstain."""
    pytest.importorskip('matplotlib.path')
    grid = S.Grid(lat)
    margin = 1000.0
    recs = S.coast_records(grid, many=many)
    path = S.write_shp(str(tmp_path / 'coast.shp'), recs, shx=not many)
    p = shoreline.plan(path, grid.gt, grid.epsg, grid.size, grid.size, margin)
    assert p.radius == round(256 * margin / 30.0) == 8533 and p.multipolygons_skipped == 1 and p.other_types_skipped == 2
    assert p.polygons == (6 if not many else 40) and p.edges_on_clip_sides >= 3
    assert (p.colours > 32 and len(p.burn_calls) == 2) if many else (2 <= p.colours <= 4 and len(p.burn_calls) == 1)
    for verts, _ in p.burn_calls:
        assert all(bin(int(w)).count('1') == 1 for w in np.unique(verts['word']))
    n = grid.size
    mask = p.host_mask(n, n)
    assert np.array_equal(mask, p.host_mask(n, n, entries=(_capi.burn_host, _capi.reach_host)))
    want, sure = S.float_mask(recs, grid, margin, p.rect)
    print('abstained on', int((~sure).sum()), 'of', n * n, '; land', int(mask.sum()))
    assert np.array_equal(mask.astype(bool)[sure], want[sure])
    assert (~sure).sum() <= 0.01 * n * n and 0 < mask.sum() < n * n
    # the bridging edges and every other edge on a side of the clip rectangle reach nothing: with them, the same mask
    every = p.reach[0].copy()
    dropped = every['next'] == shoreline.DROPPED
    every['next'][dropped] = np.flatnonzero(dropped) + 1     # (never the last record of a ring: a clip leaves two sides at least)
    keep = shoreline.Plan(p.burn_calls, (every, p.reach[1]), p.radius, {}, p.rect)
    head = _capi.reach_host(p.reach[0], p.reach[1], n, n, shoreline._reach.Spec(p.radius))['head'][0]
    assert head[1] == dropped.sum() and np.array_equal(keep.host_mask(n, n, entries=(_capi.burn_host, _capi.reach_host)), mask)


def test_a_shoreline_in_utm_and_in_the_products_own_srs(tmp_path):
    pytest.importorskip('matplotlib.path')
    grid = S.Grid(45.0)
    ring = np.array([(-2000.0, -300.0), (2500.0, 250.0), (2600.0, -3000.0), (-2100.0, -2900.0)])
    for zone in (33, 34):                                    # the product's own zone, and its neighbour
        lonlat = grid.lonlat(ring)
        e, nn = S.warp.tm_forward(lonlat[:, 0], lonlat[:, 1], -183.0 + 6.0 * zone)
        recs = [('polygon', [S.clockwise(np.stack([e + 500000.0, nn], axis=1))])]
        path = S.write_shp(str(tmp_path / f'utm{zone}.shp'), recs, prj=S.utm_prj(zone))
        p = shoreline.plan(path, grid.gt, grid.epsg, grid.size, grid.size, 300.0)
        want, sure = S.float_mask(recs, grid, 300.0, p.rect, epsg_of_records=32600 + zone)
        mask = p.host_mask(grid.size, grid.size)
        assert np.array_equal(mask.astype(bool)[sure], want[sure]) and (~sure).sum() <= 0.01 * grid.size ** 2 and 0 < mask.sum() < mask.size
    # a code that is neither: taken only as the product's own
    path = S.write_shp(str(tmp_path / 'own.shp'), recs, prj='PROJCS["NAD83 / UTM zone 15N",GEOGCS["NAD83"],AUTHORITY["EPSG","26915"]]')
    assert shoreline.plan(path, grid.gt, 26915, grid.size, grid.size, 300.0).polygons == 0      # (zone 34 coordinates: off this grid)


def test_every_refusal_and_the_unchanged_refusal_without_the_keyword(tmp_path):
    grid = S.Grid(45.0)
    recs = [('polygon', [S.clockwise(grid.lonlat(np.array([(-500.0, -500.0), (500.0, -400.0), (0.0, 600.0)])))])]
    good = S.write_shp(str(tmp_path / 'good.shp'), recs)

    def refused(text, path=good, gt=grid.gt, epsg=grid.epsg, margin=1000.0):
        with pytest.raises(NotImplementedError) as e:
            shoreline.plan(path, gt, epsg, grid.size, grid.size, margin)
        assert text in str(e.value), str(e.value)
        return str(e.value)
    said = refused('has no .prj beside it; the SRS of a shoreline must be geographic WGS 84 (EPSG:4326, as GSHHS ships), a WGS 84 / UTM zone '
                   '(EPSG 326zz / 327zz) or the SRS of the product itself (the same EPSG code in the .prj)',
                   path=S.write_shp(str(tmp_path / 'noprj.shp'), recs, prj=None))
    assert said.startswith('shoreline_shapefile: ')
    refused('(EPSG 4267) is not taken; the SRS of a shoreline must be geographic WGS 84',
            path=S.write_shp(str(tmp_path / 'nad27.shp'), recs, prj='GEOGCS["NAD27",DATUM["North_American_Datum_1927"],AUTHORITY["EPSG","4267"]]'))
    refused('(EPSG None) is not taken', path=S.write_shp(str(tmp_path / 'local.shp'), recs, prj='LOCAL_CS["x"]'))
    refused('the product is not in a WGS 84 / UTM zone', epsg=3857)
    refused('the product is not in a WGS 84 / UTM zone', epsg=None)
    refused('are not square and north-up', gt=(grid.gt[0], 30.0, 0.0, grid.gt[3], 0.0, -20.0))
    refused('are not square and north-up', gt=(grid.gt[0], 30.0, 0.1, grid.gt[3], 0.0, -30.0))
    refused('above the 4096 pixels of the reach entries', margin=30.0 * 4097)
    # a tile in zone 1 whose box grown by two margins crosses 180 degrees west
    west = S.Grid(10.0, zone=1, dlon=-2.9)
    refused('the antimeridian is not handled', gt=west.gt, epsg=west.epsg, margin=20000.0)
    # generate_dswx_layers: without the keyword exactly as before, before anything is loaded; with it, a shapefile that cannot
    # be taken is refused before anything is loaded too
    with pytest.raises(NotImplementedError, match='GDAL') as e:
        D.generate_dswx_layers(['nothing.tif'], shoreline_shapefile=good, apply_ocean_masking=True)
    assert 'shoreline' in str(e.value) and 'rasterise_shoreline=True' in str(e.value)
    with pytest.raises(NotImplementedError, match='has no .prj beside it'):
        D.generate_dswx_layers(['nothing.tif'], shoreline_shapefile=str(tmp_path / 'noprj.shp'), apply_ocean_masking=True, rasterise_shoreline=True)
    assert D.get_dswx_hls_cli_parser().parse_args(['x.tif', '--rasterise-shoreline']).rasterise_shoreline is True
    assert D.get_dswx_hls_cli_parser().parse_args(['x.tif']).rasterise_shoreline is False


def test_the_runconfig_key_and_the_command_line_flag():
    from proteus_amd import runconfig as R
    required, accepts = R.SCHEMA['processing']['rasterise_shoreline']
    assert required is R.OPT and accepts(True) and accepts(False) and not accepts('yes') and not accepts(1)
    for flag, want in (([], False), (['--rasterise-shoreline'], True)):
        args = D.get_dswx_hls_cli_parser().parse_args(['x.tif'] + flag)
        D.parse_runconfig_file(None, args)                   # the default runconfig does not have the key
        assert args.rasterise_shoreline is want
