#!/usr/bin/env python3
"""`dswx_grid.py --cell N [--band B] [--no-partial] [--device D] -o PREFIX product.tif`

One layer of a DSWx-HLS product aggregated onto square cells of N x N pixels on the GPU (include/dswx_hip.h "grid"): band B
(default 1 = WTR) of the product file is read into a resident plane and one kernel launch turns it into

    PREFIX_SHARE.tif      Byte  100 * water / (water + clear land) of the cell in integer division: its water fraction
                                (water = open or, unless --no-partial, partial surface water; nodata 255 = nothing clear)
    PREFIX_COVERAGE.tif   Byte  100 * (water + clear land) / pixels of the cell: how much of it was observed at all
    PREFIX_MAJOR.tif      Byte  0 = mostly water, 1 = mostly clear land (a tie is water); nodata 255 = nothing clear

written as COGs by the product writer, in the projection of the input: the tie point is the input's, the pixel scale N times
the input's (30 m pixels and --cell 30: 900 m cells; the last row and column of cells are ragged and count the pixels they
have).  PROTEUS has no such tool: there is no reference output to be equal to; proteus_amd/grid.py states what the layers are.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import dswx_hls, geotiff, pipeline   # noqa: E402
from proteus_amd.grid import MAX_CELL_PIXELS, NO_SHARE, NONE, wtr_grid_spec   # noqa: E402


def read_band(engine, path, band):
    """Band `band` of the file -> (DevicePlane uint8 [H, W], GeoTiffInfo)."""
    planes, info = engine.read_bands(path)
    try:
        if not 1 <= band <= info.bands:
            raise ValueError(f'ERROR {path} has {info.bands} bands, band {band} was asked for')
        if planes.dtype != np.uint8:
            raise ValueError(f'ERROR {path} holds {planes.dtype} samples: a grid is made of a Byte band')
        plane = engine.plane((info.height, info.width), np.uint8)
        n = info.height * info.width
        if n:
            with engine.lock:
                engine.ctx.copy_2d_device(plane.ptr, n, planes.ptr + (band - 1) * n, n, n, 1)
                engine.ctx.synchronize()
    finally:
        planes.release()
    return plane, info


def scaled_geo_tags(geo_tags, cell):
    """The GeoTIFF tags of the input with the pixel scale multiplied by `cell`; the tie point stays where it is."""
    tags = dict(geo_tags)
    if geotiff.TAG_PIXEL_SCALE in tags:
        kind, (sx, sy, sz) = tags[geotiff.TAG_PIXEL_SCALE][0], tags[geotiff.TAG_PIXEL_SCALE][1][:3]
        tags[geotiff.TAG_PIXEL_SCALE] = (kind, [float(sx) * cell, float(sy) * cell, float(sz)])
    return tags


def main(argv=None):
    ap = argparse.ArgumentParser(description='Aggregate a layer of a product onto N x N cells: water fraction, observed fraction, '
                                             'majority class')
    ap.add_argument('input_file', type=str, help='DSWx-HLS product file')
    ap.add_argument('-o', '--output-prefix', dest='prefix', type=str, required=True, help='PREFIX of the three output files')
    ap.add_argument('--cell', type=int, required=True, metavar='N', help='pixels per cell side')
    ap.add_argument('--band', type=int, default=1, metavar='B', help='band of the product file to aggregate (default 1 = WTR)')
    ap.add_argument('--no-partial', action='store_true', help='partial surface water counts as clear and not water')
    ap.add_argument('--device', type=int, default=None, metavar='D', help='GPU to run on (default $DSWX_DEVICE or 0)')
    args = ap.parse_args(argv)
    if not os.path.isfile(args.input_file):
        print(f'ERROR file not found: {args.input_file}')
        return 1
    if args.cell < 1:
        print(f'ERROR --cell {args.cell}: at least 1')
        return 1
    engine = pipeline.engine_of(dswx_hls.get_context(args.device))
    try:
        plane, info = read_band(engine, args.input_file, args.band)
    except ValueError as e:
        print(e)
        return 1
    if min(args.cell, info.height) * min(args.cell, info.width) > MAX_CELL_PIXELS:
        plane.release()
        print(f'ERROR --cell {args.cell}: a cell has at most {MAX_CELL_PIXELS} pixels')
        return 1
    res = plane.grid(wtr_grid_spec(args.cell, collapsed=True, partial_is_water=not args.no_partial), want=('share', 'coverage', 'major'))
    plane.release()
    md = dict(info.metadata)
    md['GRID_INPUT_FILE'] = os.path.basename(args.input_file)
    md['GRID_INPUT_BAND'] = str(args.band)
    md['GRID_CELL_PIXELS'] = str(args.cell)
    md['GRID_PARTIAL_SURFACE_WATER_IS_WATER'] = str(not args.no_partial)
    tags = scaled_geo_tags(info.geo_tags, args.cell)
    outputs = (('share', 'SHARE', 'Water fraction of the clear pixels of the cell in percent', NO_SHARE),
               ('coverage', 'COVERAGE', 'Clear fraction of the cell in percent', 255),
               ('major', 'MAJOR', 'Majority of the clear pixels of the cell: 0 water, 1 not water', NONE))
    written = []
    for key, suffix, description, nodata in outputs:
        res[key].shape = res[key].shape[1:]               # [1, GH, GW] -> the raster the writer takes
        dswx_hls._save_array(res[key], f'{args.prefix}_{suffix}.tif', md, tags, description=description,
                             output_files_list=written, no_data_value=nodata)
    for p in res.values():
        p.release()
    for f in written:
        print(f'file saved: {f}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
