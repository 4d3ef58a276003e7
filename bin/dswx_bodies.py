#!/usr/bin/env python3
"""`dswx_bodies.py --min-size N [--connectivity 4|8] [--band B] [--no-partial] [--device D] [-o OUTPUT] [--table FILE [--max-bodies M]] product.tif`

The water bodies of one layer of a DSWx-HLS product, labelled on the GPU (include/dswx_hip.h "label"): band B (default 1 =
WTR) of the product file is read into a resident plane; its water pixels (open or, unless --no-partial, partial surface
water) are grouped into connected bodies; every body of fewer than N pixels is turned into "not water" (0), and the result is
written as a Byte COG by the product writer, in the projection of the input (OUTPUT, default <product>_SIEVED.tif).  The
summary is printed as one line of JSON: how many bodies, how many water pixels, the largest body and its label (1 + the index
y * width + x of its first pixel), how many bodies and pixels stay, the bodies per power of two of their size -- and, where
the file's geotransform gives the size of a pixel, the same areas in square metres.  PROTEUS has no such tool: there is no
reference output to be equal to; proteus_amd/label.py states what a body is.

With --table FILE the bodies are also tabulated on the GPU (include/dswx_hip.h "body table", proteus_amd/bodies.py) and FILE is
written as CSV with one line per body KEPT by --min-size, in the order of the bodies' first pixels: rank and label, the first
pixel, the area in pixels, the bounding box and the centroid in pixels (a pixel's coordinate is its column / row index), the
perimeter in pixel edges, the open-water and partial-surface-water pixels; and, where the geotransform is known, the area in
square metres, the perimeter in metres (an edge counted as the mean of the pixel's two sides), the centroid (of pixel
centres) and the bounding box (of pixel outlines) in map coordinates.  --max-bodies M is the capacity of the table (default:
the body count of the summary); bodies of rank M and above are not listed.  The JSON line is the same with and without.
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import dswx_hls, geotiff, pipeline   # noqa: E402
from proteus_amd.bodies import ROW_DTYPE, wtr_body_spec   # noqa: E402
from proteus_amd.label import wtr_label_spec   # noqa: E402


def read_band(engine, path, band):
    """Band `band` of the file -> (DevicePlane uint8 [H, W], GeoTiffInfo)."""
    planes, info = engine.read_bands(path)
    try:
        if not 1 <= band <= info.bands:
            raise ValueError(f'ERROR {path} has {info.bands} bands, band {band} was asked for')
        if planes.dtype != np.uint8:
            raise ValueError(f'ERROR {path} holds {planes.dtype} samples: bodies are labelled in a Byte band')
        plane = engine.plane((info.height, info.width), np.uint8)
        n = info.height * info.width
        if n:
            with engine.lock:
                engine.ctx.copy_2d_device(plane.ptr, n, planes.ptr + (band - 1) * n, n, n, 1)
                engine.ctx.synchronize()
    finally:
        planes.release()
    return plane, info


TABLE_COLUMNS = ('rank', 'label', 'first_x', 'first_y', 'area_px', 'x_min', 'x_max', 'y_min', 'y_max', 'centroid_x_px', 'centroid_y_px',
                 'perimeter_edges', 'open_px', 'partial_px')
TABLE_MAP_COLUMNS = ('area_m2', 'perimeter_m', 'centroid_map_x', 'centroid_map_y', 'map_x_min', 'map_x_max', 'map_y_min', 'map_y_max')


def write_table(path, rows, min_size, width, gt):
    """The rows (bodies.ROW_DTYPE [n]) of at least min_size pixels -> CSV; `gt` is the geotransform or None."""
    with open(path, 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(TABLE_COLUMNS + (TABLE_MAP_COLUMNS if gt else ()))
        for k, r in enumerate(rows):
            a = int(r['area'])
            if a < min_size or a == 0:
                continue
            first = int(r['label']) - 1
            x0, x1, y0, y1 = (int(r[c]) for c in ('x_min', 'x_max', 'y_min', 'y_max'))
            cx, cy, per = int(r['sum_x']) / a, int(r['sum_y']) / a, int(r['perimeter'])
            line = [k, int(r['label']), first % width, first // width, a, x0, x1, y0, y1, repr(cx), repr(cy), per,
                    int(r['count'][0]), int(r['count'][1])]
            if gt:
                # (north-up files: no rotation terms; a row's y decreases downward, so y_min of the map is the LAST row's lower edge)
                line += [repr(a * abs(gt[1] * gt[5])), repr(per * (abs(gt[1]) + abs(gt[5])) / 2), repr(gt[0] + (cx + 0.5) * gt[1]),
                         repr(gt[3] + (cy + 0.5) * gt[5]), repr(gt[0] + x0 * gt[1]), repr(gt[0] + (x1 + 1) * gt[1]),
                         repr(gt[3] + (y1 + 1) * gt[5]), repr(gt[3] + y0 * gt[5])]
            w.writerow(line)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Label the water bodies of a layer of a product, remove the small ones, summarise')
    ap.add_argument('input_file', type=str, help='DSWx-HLS product file')
    ap.add_argument('--min-size', type=int, required=True, metavar='N', help='bodies of fewer than N pixels become "not water"')
    ap.add_argument('--connectivity', type=int, default=8, choices=(4, 8), help='neighbourhood of a pixel (default 8)')
    ap.add_argument('-o', '--output', dest='output', type=str, default=None, help='the sieved layer (default <product>_SIEVED.tif)')
    ap.add_argument('--band', type=int, default=1, metavar='B', help='band of the product file to label (default 1 = WTR)')
    ap.add_argument('--no-partial', action='store_true', help='partial surface water is not water')
    ap.add_argument('--table', type=str, default=None, metavar='FILE', help='write one CSV line per body kept by --min-size')
    ap.add_argument('--max-bodies', type=int, default=None, metavar='M', help='capacity of the table (default: the body count)')
    ap.add_argument('--device', type=int, default=None, metavar='D', help='GPU to run on (default $DSWX_DEVICE or 0)')
    args = ap.parse_args(argv)
    if not os.path.isfile(args.input_file):
        print(f'ERROR file not found: {args.input_file}')
        return 1
    if args.min_size < 1:
        print(f'ERROR --min-size {args.min_size}: at least 1')
        return 1
    if args.max_bodies is not None and args.max_bodies < 0:
        print(f'ERROR --max-bodies {args.max_bodies}: at least 0')
        return 1
    output = args.output or os.path.splitext(args.input_file)[0] + '_SIEVED.tif'
    engine = pipeline.engine_of(dswx_hls.get_context(args.device))
    try:
        plane, info = read_band(engine, args.input_file, args.band)
    except ValueError as e:
        print(e)
        return 1
    res = plane.label(wtr_label_spec(args.min_size, connectivity=args.connectivity, partial_is_water=not args.no_partial))
    s = [int(v) for v in res['summary'].numpy()[0]]
    rows = np.zeros(0, dtype=ROW_DTYPE)
    if args.table is not None:
        res['label'].shape = res['label'].shape[1:]           # [1, H, W] -> the raster of the value plane
        table = res['label'].body_table(wtr_body_spec(s[0] if args.max_bodies is None else args.max_bodies), value=plane)
        if 'rows' in table:
            rows = table['rows'].numpy().view(ROW_DTYPE)[0, :, 0]
        for p in table.values():
            p.release()
    plane.release()
    said = {'input_file': os.path.basename(args.input_file), 'band': args.band, 'min_size': args.min_size,
            'connectivity': args.connectivity, 'bodies': s[0], 'member_pixels': s[1], 'largest_size': s[2], 'largest_label': s[3],
            'bodies_kept': s[4], 'pixels_kept': s[5], 'bodies_by_log2_size': s[8:]}
    tags, gt = info.geo_tags, info.geotransform
    if geotiff.TAG_TRANSFORM in tags or (geotiff.TAG_PIXEL_SCALE in tags and geotiff.TAG_TIEPOINT in tags):
        area = abs(float(gt[1]) * float(gt[5]))
        said.update(pixel_area_m2=area, member_area_m2=s[1] * area, largest_area_m2=s[2] * area, kept_area_m2=s[5] * area,
                    min_area_m2=args.min_size * area)
    md = dict(info.metadata)
    md['BODIES_INPUT_FILE'] = os.path.basename(args.input_file)
    md['BODIES_INPUT_BAND'] = str(args.band)
    md['BODIES_MIN_SIZE_PIXELS'] = str(args.min_size)
    md['BODIES_CONNECTIVITY'] = str(args.connectivity)
    md['BODIES_PARTIAL_SURFACE_WATER_IS_WATER'] = str(not args.no_partial)
    written = []
    res['sieved'].shape = res['sieved'].shape[1:]             # [1, H, W] -> the raster the writer takes
    dswx_hls._save_array(res['sieved'], output, md, info.geo_tags, description=f'Water bodies of at least {args.min_size} pixels',
                         output_files_list=written, no_data_value=255)
    for p in res.values():
        p.release()
    if args.table is not None:
        known = geotiff.TAG_TRANSFORM in tags or (geotiff.TAG_PIXEL_SCALE in tags and geotiff.TAG_TIEPOINT in tags)
        write_table(args.table, rows, args.min_size, info.width, tuple(float(v) for v in gt) if known else None)
        written.append(args.table)
    for f in written:
        print(f'file saved: {f}')
    print(json.dumps(said))
    return 0


if __name__ == '__main__':
    sys.exit(main())
