#!/usr/bin/env python3
"""`dswx_distance.py [--radius-m M] [--band B] [--no-partial] [--device N] --out-distance FILE [--out-buffer FILE] product.tif`

The distance of every pixel of one layer of a DSWx-HLS product to the nearest water, measured on the GPU (include/dswx_hip.h
"distance"): band B (default 1 = WTR) of the product file is read into a resident plane; its water pixels (open or, unless
--no-partial, partial surface water) are the targets; the exact squared Euclidean distance of every pixel to the nearest of
them comes back as integers, and `--out-distance FILE` is written as a Float32 COG in the projection of the input that holds
pixel_size * sqrt(dist2) in metres, computed on the host in float64 and rounded once; a pixel that no water reaches is nodata
(-9999).  With --radius-m M only water within M metres counts (the radius in pixels is M / pixel_size rounded down), and
`--out-buffer FILE` is the layer itself as a Byte COG with every non-water pixel within the radius turned into the byte 200:
the buffer ring.  The summary is printed as one line of JSON: water pixels, reached and not reached pixels, the largest
distance in metres and the pixel (row, column) that holds it, the mean distance of the reached pixels that are not water, and
the pixels per power of two of their squared distance.  Where the file has no geotransform a pixel counts as one metre.
PROTEUS has no such tool: there is no reference output to be equal to; proteus_amd/distance.py states what a distance is.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import dswx_hls, geotiff, pipeline   # noqa: E402
from proteus_amd.distance import NONE, wtr_distance_spec   # noqa: E402

NODATA = -9999.0


def read_band(engine, path, band):
    """Band `band` of the file -> (DevicePlane uint8 [H, W], GeoTiffInfo)."""
    planes, info = engine.read_bands(path)
    try:
        if not 1 <= band <= info.bands:
            raise ValueError(f'ERROR {path} has {info.bands} bands, band {band} was asked for')
        if planes.dtype != np.uint8:
            raise ValueError(f'ERROR {path} holds {planes.dtype} samples: distances are measured in a Byte band')
        plane = engine.plane((info.height, info.width), np.uint8)
        n = info.height * info.width
        if n:
            with engine.lock:
                engine.ctx.copy_2d_device(plane.ptr, n, planes.ptr + (band - 1) * n, n, n, 1)
                engine.ctx.synchronize()
    finally:
        planes.release()
    return plane, info


def main(argv=None):
    ap = argparse.ArgumentParser(description='Distance of every pixel of a layer of a product to the nearest water; a buffer ring')
    ap.add_argument('input_file', type=str, help='DSWx-HLS product file')
    ap.add_argument('--out-distance', type=str, required=True, metavar='FILE', help='distance to water in metres, Float32 COG')
    ap.add_argument('--out-buffer', type=str, default=None, metavar='FILE', help='the layer with the ring within --radius-m marked, Byte COG')
    ap.add_argument('--radius-m', type=float, default=None, metavar='M', help='only water within M metres counts (default: unbounded)')
    ap.add_argument('--band', type=int, default=1, metavar='B', help='band of the product file to measure in (default 1 = WTR)')
    ap.add_argument('--no-partial', action='store_true', help='partial surface water is not water')
    ap.add_argument('--device', type=int, default=None, metavar='N', help='GPU to run on (default $DSWX_DEVICE or 0)')
    args = ap.parse_args(argv)
    if not os.path.isfile(args.input_file):
        print(f'ERROR file not found: {args.input_file}')
        return 1
    if args.out_buffer is not None and args.radius_m is None:
        print('ERROR --out-buffer needs --radius-m: the ring needs a radius')
        return 1
    if args.radius_m is not None and not args.radius_m > 0:
        print(f'ERROR --radius-m {args.radius_m}: above 0')
        return 1
    engine = pipeline.engine_of(dswx_hls.get_context(args.device))
    try:
        plane, info = read_band(engine, args.input_file, args.band)
    except ValueError as e:
        print(e)
        return 1
    tags, gt = info.geo_tags, info.geotransform
    known = geotiff.TAG_TRANSFORM in tags or (geotiff.TAG_PIXEL_SCALE in tags and geotiff.TAG_TIEPOINT in tags)
    px = abs(float(gt[1])) if known else 1.0
    if known and abs(float(gt[5])) != px:
        print(f'ERROR pixels of {px} x {abs(float(gt[5]))} m: a Euclidean distance in pixels needs square ones')
        plane.release()
        return 1
    radius = 0 if args.radius_m is None else int(args.radius_m // px)
    if args.radius_m is not None and radius < 1:
        print(f'ERROR --radius-m {args.radius_m} is below one pixel ({px} m)')
        plane.release()
        return 1
    spec = wtr_distance_spec(radius=radius, partial_is_water=not args.no_partial)
    try:
        res = plane.distance(spec, want=('dist2', 'summary') + (('within',) if args.out_buffer else ()))
    except ValueError as e:
        print(f'ERROR {e}')
        plane.release()
        return 1
    plane.release()
    s = [int(v) for v in res['summary'].numpy()[0]]
    d2 = res['dist2'].numpy()[0]
    metres = np.where(d2 == NONE, NODATA, px * np.sqrt(d2.astype(np.float64))).astype(np.float32)
    ring = d2[(d2 != NONE) & (d2 != 0)]
    said = {'input_file': os.path.basename(args.input_file), 'band': args.band, 'radius_pixels': radius, 'pixel_size_m': px,
            'pixel_size_known': bool(known), 'water_pixels': s[0], 'reached_pixels': s[1], 'not_reached_pixels': s[2],
            'largest_distance_m': px * math.sqrt(s[3]), 'largest_distance_pixel': [s[4] // info.width, s[4] % info.width],
            'mean_distance_m': float(px * np.sqrt(ring.astype(np.float64)).mean()) if ring.size else 0.0,
            'sum_dist2_pixels': s[5], 'pixels_by_log2_dist2': s[8:]}
    md = dict(info.metadata)
    md['DISTANCE_INPUT_FILE'] = os.path.basename(args.input_file)
    md['DISTANCE_INPUT_BAND'] = str(args.band)
    md['DISTANCE_RADIUS_PIXELS'] = str(radius)
    md['DISTANCE_PARTIAL_SURFACE_WATER_IS_WATER'] = str(not args.no_partial)
    written = []
    dswx_hls._save_array(metres, args.out_distance, md, info.geo_tags, description='Distance to the nearest water in metres',
                         output_files_list=written, no_data_value=NODATA)
    if args.out_buffer:
        res['within'].shape = res['within'].shape[1:]         # [1, H, W] -> the raster the writer takes
        dswx_hls._save_array(res['within'], args.out_buffer, md, info.geo_tags,
                             description=f'Layer with the pixels within {radius} pixels of water marked {spec.mark}',
                             output_files_list=written, no_data_value=255)
    for p in res.values():
        p.release()
    for f in written:
        print(f'file saved: {f}')
    print(json.dumps(said))
    return 0


if __name__ == '__main__':
    sys.exit(main())
