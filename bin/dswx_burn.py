#!/usr/bin/env python3
"""`dswx_burn.py product.tif --polygons FILE.geojson [--burn 1] [--background 0] [--buffer-m M | --buffer-vector-m M] [--device D] --out FILE.tif`

Polygons burnt onto the grid of a DSWx-HLS product on the GPU (include/dswx_hip.h "burn"): the opposite direction of
dswx_outline.py, which writes the files this tool reads, so the two round-trip.  FILE.geojson holds Polygon / MultiPolygon
features in the SRS of the product (read with `json`: there is no GDAL here, nothing is reprojected, and .shp files are not
read); their coordinates go through the inverse of the file's geotransform to pixel coordinates, and the rings are burnt into
a plane of the product's size that starts as --background, 32 polygons per call with one bit each and the holes of a polygon on
its bit, IN PLACE: a pixel whose CENTRE lies inside a polygon (even-odd within one polygon) becomes --burn, and polygons that
overlap union.  16 bytes per vertex cross PCIe, not a plane.  With --buffer-m every pixel within M metres of a burnt pixel is
set to --burn too, through the distance entry's `within` (include/dswx_hip.h "distance"): that buffers the RASTER -- distances
between pixel centres, M rounded down to whole pixels -- not the vector as the reference's Buffer(margin) does.  With
--buffer-vector-m every pixel whose CENTRE lies within M metres of an edge of a polygon is set to --burn too, through the reach
entry (include/dswx_hip.h "reach"): that buffers the VECTOR, exactly, M rounded to 1/256 pixel.  FILE.tif is
written as a Byte COG with the product's georeferencing, usable as --ocean-mask (with --burn 0 --background 1: 0 = ocean).
One line of JSON on standard output says how many polygons, rings and vertices there were and how many pixels were burnt.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import burn as BN   # noqa: E402

POLYGONS_PER_CALL = 32


def polygons_of(doc):
    """The polygons of a GeoJSON document (a FeatureCollection, a Feature or a geometry): a list of polygons, each a list of
    rings -- exterior first, then holes --, each ring a float64 [k, 2] array of map (x, y) without the repeated closing point."""
    def ring(coords):
        r = np.asarray(coords, dtype=np.float64).reshape(-1, np.shape(coords)[-1] if len(coords) else 2)[:, :2]
        return r[:-1] if len(r) > 1 and (r[0] == r[-1]).all() else r

    def geometry(g, out):
        if g is None:
            return
        kind = g.get('type')
        if kind == 'Polygon':
            out.append([ring(r) for r in g['coordinates']])
        elif kind == 'MultiPolygon':
            for p in g['coordinates']:
                out.append([ring(r) for r in p])
        elif kind == 'GeometryCollection':
            for h in g.get('geometries', []):
                geometry(h, out)
        elif kind == 'Feature':
            geometry(g.get('geometry'), out)
        elif kind == 'FeatureCollection':
            for f in g.get('features', []):
                geometry(f, out)
        else:
            raise ValueError(f'ERROR geometry of type {kind!r}: only Polygon and MultiPolygon are burnt')
    out = []
    geometry(doc, out)
    return out


def to_pixels(xy, gt):
    """Map coordinates -> pixel coordinates by the inverse of the geotransform (x = gt0 + c gt1 + r gt2, y = gt3 + c gt4 + r gt5)."""
    det = gt[1] * gt[5] - gt[2] * gt[4]
    if det == 0:
        raise ValueError('ERROR the geotransform of the product is singular')
    dx, dy = xy[:, 0] - gt[0], xy[:, 1] - gt[3]
    return np.stack([(gt[5] * dx - gt[2] * dy) / det, (gt[1] * dy - gt[4] * dx) / det], axis=1)


def rings_of(polys, gt):
    """(rings in pixel coordinates, their words) of at most POLYGONS_PER_CALL polygons: polygon i has bit i, on all its rings."""
    assert len(polys) <= POLYGONS_PER_CALL
    return [to_pixels(r, gt) for p in polys for r in p], [1 << i for i, p in enumerate(polys) for _ in p]


def records_of(polys, gt):
    """The records of one call (burn.VERTEX_DTYPE): what DevicePlane.burn makes of rings_of."""
    rings, words = rings_of(polys, gt)
    return BN.records([BN.quantise(r) for r in rings], words)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Burn the polygons of a GeoJSON file onto the grid of a product, write a Byte COG')
    ap.add_argument('input_file', type=str, help='DSWx-HLS product file: the grid and the georeferencing')
    ap.add_argument('--polygons', type=str, required=True, metavar='FILE.geojson', help='Polygon / MultiPolygon features in the SRS of the product')
    ap.add_argument('--out', type=str, required=True, metavar='FILE.tif', help='the burnt plane, Byte COG')
    ap.add_argument('--burn', type=int, default=1, help='byte of a pixel inside a polygon (default 1)')
    ap.add_argument('--background', type=int, default=0, help='byte of every other pixel (default 0)')
    ap.add_argument('--buffer-m', type=float, default=None, metavar='M', help='also burn every pixel within M metres of a burnt pixel (buffers the RASTER)')
    ap.add_argument('--buffer-vector-m', type=float, default=None, metavar='M',
                    help='also burn every pixel whose centre lies within M metres of a polygon edge (buffers the VECTOR, exactly)')
    ap.add_argument('--device', type=int, default=None, metavar='D', help='GPU to run on (default $DSWX_DEVICE or 0)')
    args = ap.parse_args(argv)
    for f in (args.input_file, args.polygons):
        if not os.path.isfile(f):
            print(f'ERROR file not found: {f}')
            return 1
    if not (0 <= args.burn <= 255 and 0 <= args.background <= 255) or args.burn == args.background:
        print(f'ERROR --burn {args.burn} and --background {args.background}: two different bytes')
        return 1
    if args.buffer_m is not None and not args.buffer_m > 0:
        print(f'ERROR --buffer-m {args.buffer_m}: above 0')
        return 1
    if args.buffer_vector_m is not None and (args.buffer_m is not None or not args.buffer_vector_m >= 0):
        print(f'ERROR --buffer-vector-m {args.buffer_vector_m}: 0 or above, and not together with --buffer-m')
        return 1
    from proteus_amd import dswx_hls, geotiff, pipeline
    from proteus_amd import reach as RC
    from proteus_amd.distance import Spec as DistanceSpec
    try:
        with open(args.polygons) as f:
            polys = polygons_of(json.load(f))
    except ValueError as e:
        print(e)
        return 1
    engine = pipeline.engine_of(dswx_hls.get_context(args.device))
    try:
        info = geotiff.open_geotiff(args.input_file).info           # the grid and the georeferencing: no band is read
    except geotiff.GeoTiffError as e:
        print(f'ERROR {e}')
        return 1
    gt = tuple(float(v) for v in info.geotransform)
    H, W = info.height, info.width
    plane = engine.constant_plane((H, W), args.background)
    spec = BN.Spec(burn=args.burn, background=args.background)
    toggles = rings = vertices = 0
    reach_spec = None
    if args.buffer_vector_m is not None:
        if abs(gt[5]) != abs(gt[1]) or not 256.0 * args.buffer_vector_m / abs(gt[1]) <= RC.MAX_RADIUS:
            print(f'ERROR --buffer-vector-m {args.buffer_vector_m}: needs square pixels (here {abs(gt[1])} x {abs(gt[5])} m) and at most '
                  f'{RC.MAX_RADIUS // 256} pixels')
            return 1
        reach_spec = RC.Spec(int(round(256.0 * args.buffer_vector_m / abs(gt[1]))), burn=args.burn, background=args.background)
    try:
        for at in range(0, len(polys), POLYGONS_PER_CALL):
            px, words = rings_of(polys[at:at + POLYGONS_PER_CALL], gt)
            res = plane.burn(px, spec, words, want=('head',))
            toggles += int(res['head'].numpy()[0, 3])
            rings += len(px)
            vertices += sum(len(r) for r in px)
            for p in res.values():
                p.release()
        if reach_spec is not None:                               # every ring at once: no bit is needed to reach
            res = plane.reach([to_pixels(r, gt) for p in polys for r in p], reach_spec, want=('head',))
            reached = int(res['head'].numpy()[0, 6])
            for p in res.values():
                p.release()
    except ValueError as e:
        print(f'ERROR {e}')
        return 1
    said = {'input_file': os.path.basename(args.input_file), 'polygons': len(polys), 'rings': rings, 'vertices': vertices,
            'toggles': toggles, 'height': H, 'width': W, 'burn': args.burn, 'background': args.background}
    if reach_spec is not None:
        said['buffer_vector_256ths_of_a_pixel'], said['reached_pixels'] = reach_spec.radius, reached
    if args.buffer_m is not None:
        px_m = abs(gt[1])
        if abs(gt[5]) != px_m:
            print(f'ERROR pixels of {px_m} x {abs(gt[5])} m: a Euclidean distance in pixels needs square ones')
            return 1
        radius = int(args.buffer_m // px_m)
        said['buffer_pixels'] = radius
        if radius >= 1:
            target = np.zeros(256, dtype=np.uint8)
            target[args.burn] = 1
            ring = plane.distance(DistanceSpec(target, radius, args.burn), want=('within',))
            plane.release()
            plane = ring['within']
            plane.shape = plane.shape[1:]
            ring['dist2'].release()
    said['burnt_pixels'] = int(plane.histogram()[args.burn])
    md = {'BURN_INPUT_FILE': os.path.basename(args.input_file), 'BURN_POLYGONS_FILE': os.path.basename(args.polygons),
          'BURN_VALUE': str(args.burn), 'BURN_BACKGROUND': str(args.background),
          'BURN_BUFFER_M': str(args.buffer_m) if args.buffer_m is not None else 'none (the raster, not the vector, is buffered)'}
    if reach_spec is not None:
        md['BURN_BUFFER_M'], md['BURN_BUFFER_VECTOR_M'] = 'none', str(args.buffer_vector_m)
    written = []
    dswx_hls._save_array(plane, args.out, md, info.geo_tags, description='Polygons burnt onto the grid of the product',
                         output_files_list=written)
    plane.release()
    for f in written:
        print(f'file saved: {f}')
    print(json.dumps(said))
    return 0


if __name__ == '__main__':
    sys.exit(main())
