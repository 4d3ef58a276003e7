#!/usr/bin/env python3
"""`dswx_outline.py product.tif [--layer WTR | --band B] [--connectivity 4|8] [--min-size N] [--no-partial] [--device D] --out FILE.geojson`

The water bodies of one layer of a DSWx-HLS product as POLYGONS, traced on the GPU (include/dswx_hip.h "outline"): the band of
the layer (default WTR = band 1) is read into a resident plane; its water pixels (open or, unless --no-partial, partial
surface water) are grouped into connected bodies, those of fewer than N pixels dropped (--min-size, default 1); the bodies
are tabulated (include/dswx_hip.h "body table") and their outlines put in order as rings, all on the device: the label plane
never crosses PCIe, what is downloaded is 4 bytes per pixel edge of a shoreline and 32 bytes per ring.  FILE is written as a
GeoJSON FeatureCollection with one Polygon per body, in the order of the bodies' first pixels: the exterior ring first, then
its holes (islands), each closed, collinear points dropped; coordinates are map coordinates of pixel corners by the file's
geotransform, and the CRS is named from the file's EPSG code where it has one.  The properties of a feature are `label` (1 +
the index y * width + x of the body's first pixel), `area_m2`, `perimeter_m` (an edge counted as the mean of the pixel's two
sides) and `holes`.  One line of JSON on standard output says how many bodies, rings, edges and vertices there were.  Only
`json` writes the file: there is no GDAL here.  PROTEUS has no such tool: there is no reference output to be equal to;
proteus_amd/outline.py states what a ring is.
"""
import argparse
import importlib.util
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import dswx_hls, geotiff, pipeline   # noqa: E402
from proteus_amd.bodies import ROW_DTYPE as BODY_ROW, wtr_body_spec   # noqa: E402
from proteus_amd.label import wtr_label_spec   # noqa: E402
from proteus_amd.outline import ROW_DTYPE, Spec, polygons   # noqa: E402

LAYERS = {'WTR': 1, 'WTR-1': 5, 'WTR-2': 6}              # the water-class layers and their bands in the product file


def _bodies_tool():
    spec = importlib.util.spec_from_file_location('dswx_bodies_tool', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dswx_bodies.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def epsg_of(geo_tags):
    """The EPSG code of the GeoKey directory (ProjectedCSTypeGeoKey 3072, else GeographicTypeGeoKey 2048), or None."""
    if geotiff.TAG_GEOKEYS not in geo_tags:
        return None
    keys = [int(v) for v in geo_tags[geotiff.TAG_GEOKEYS][1]]
    found = {keys[i]: keys[i + 3] for i in range(4, len(keys) - 3, 4) if keys[i + 1] == 0}
    code = found.get(3072, found.get(2048))
    return code if code and code != 32767 else None


def features(chain, rings, body_rows, width, gt):
    """The GeoJSON features of one tile: `chain` uint32 [max_edges], `rings` outline.ROW_DTYPE [max_rings], `body_rows`
    bodies.ROW_DTYPE [K] and the geotransform."""
    by_label = {int(r['label']): r for r in body_rows}
    to_map = lambda pts: [[gt[0] + float(x) * gt[1] + float(y) * gt[2], gt[3] + float(x) * gt[4] + float(y) * gt[5]] for x, y in pts.tolist()]
    closed = lambda pts: to_map(pts) + to_map(pts[:1])
    out = []
    for label, outer, holes in polygons(chain, rings, width):
        row = by_label[label]
        out.append({'type': 'Feature',
                    'properties': {'label': label, 'area_m2': int(row['area']) * abs(gt[1] * gt[5]),
                                   'perimeter_m': int(row['perimeter']) * (abs(gt[1]) + abs(gt[5])) / 2, 'holes': len(holes)},
                    'geometry': {'type': 'Polygon', 'coordinates': [closed(outer)] + [closed(h) for h in holes]}})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description='Trace the water bodies of a layer of a product as polygons, write GeoJSON')
    ap.add_argument('input_file', type=str, help='DSWx-HLS product file')
    ap.add_argument('--out', type=str, required=True, metavar='FILE.geojson', help='the FeatureCollection')
    ap.add_argument('--layer', type=str, default='WTR', choices=sorted(LAYERS), help='layer of the product file (default WTR)')
    ap.add_argument('--band', type=int, default=None, metavar='B', help='band of the product file, instead of --layer')
    ap.add_argument('--connectivity', type=int, default=8, choices=(4, 8), help='neighbourhood of a pixel (default 8)')
    ap.add_argument('--min-size', type=int, default=1, metavar='N', help='bodies of fewer than N pixels are dropped (default 1)')
    ap.add_argument('--no-partial', action='store_true', help='partial surface water is not water')
    ap.add_argument('--device', type=int, default=None, metavar='D', help='GPU to run on (default $DSWX_DEVICE or 0)')
    args = ap.parse_args(argv)
    if not os.path.isfile(args.input_file):
        print(f'ERROR file not found: {args.input_file}')
        return 1
    if args.min_size < 1:
        print(f'ERROR --min-size {args.min_size}: at least 1')
        return 1
    band = LAYERS[args.layer] if args.band is None else args.band
    engine = pipeline.engine_of(dswx_hls.get_context(args.device))
    try:
        plane, info = _bodies_tool().read_band(engine, args.input_file, band)
    except ValueError as e:
        print(e)
        return 1
    lspec = wtr_label_spec(args.min_size, connectivity=args.connectivity, partial_is_water=not args.no_partial)
    # label with the small bodies sieved out, then label what is left: the ids of the bodies that stay
    first = plane.label(lspec, want=('sieved',))
    first['sieved'].shape = first['sieved'].shape[1:]
    kept = first['sieved'].label(lspec, want=('label', 'summary'))
    K = int(kept['summary'].numpy()[0, 0])
    kept['label'].shape = kept['label'].shape[1:]
    table = kept['label'].body_table(wtr_body_spec(K), value=first['sieved'])
    body_rows = table['rows'].numpy().view(BODY_ROW)[0, :, 0] if 'rows' in table else np.zeros(0, dtype=BODY_ROW)
    E = int(table['head'].numpy()[0, 4])                  # the perimeters of all bodies: exactly the edges of the outline
    H, W = info.height, info.width
    res = kept['label'].outline(None, Spec(max(E, 4), max(E // 4, 1), args.connectivity))
    head = res['head'].numpy()[0]
    if int(head[0]) != E or int(head[7]) != 0:
        print(f'ERROR the outline has {int(head[0])} edges, the body table counted {E}')
        return 1
    chain = res['chain'].numpy()[0]
    rings = res['rings'].numpy().view(ROW_DTYPE)[0, :, 0] if 'rings' in res else np.zeros(0, dtype=ROW_DTYPE)
    for group in (first, kept, table, res):
        for p in group.values():
            p.release()
    plane.release()
    gt = tuple(float(v) for v in info.geotransform)
    feats = features(chain, rings, body_rows, W, gt)
    doc = {'type': 'FeatureCollection', 'name': os.path.splitext(os.path.basename(args.out))[0]}
    epsg = epsg_of(info.geo_tags)
    if epsg is not None:
        doc['crs'] = {'type': 'name', 'properties': {'name': f'urn:ogc:def:crs:EPSG::{epsg}'}}
    doc['features'] = feats
    with open(args.out, 'w') as f:
        json.dump(doc, f)
    print(f'file saved: {args.out}')
    print(json.dumps({'input_file': os.path.basename(args.input_file), 'band': band, 'min_size': args.min_size,
                      'connectivity': args.connectivity, 'bodies': K, 'polygons': len(feats), 'rings': int(head[1]),
                      'holes': int(head[5]), 'edges': E, 'vertices': int(head[6]), 'epsg': epsg, 'height': H, 'width': W}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
