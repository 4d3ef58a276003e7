#!/usr/bin/env python3
"""`dswx_stack.py [--band N] [--no-partial] [--device N] -o PREFIX file1.tif file2.tif ...`

The dates of one MGRS tile composited per pixel on the GPU (include/dswx_hip.h "stack"): band N (default 1 = WTR) of every
DSWx-HLS product file, in the order given (= time order), is read into one resident [n, H, W] stack and one kernel launch
turns it into

    PREFIX_COUNT_WATER.tif   UInt16  on how many dates the pixel was water (open or, unless --no-partial, partial)
    PREFIX_COUNT_LAND.tif    UInt16  on how many dates it was clear and not water
    PREFIX_LAST.tif          Byte    its latest clear observation, clouds filled from earlier dates (nodata 255, WTR colours)
    PREFIX_LAST_INDEX.tif    UInt16  which file (0 = the first) that observation came from (nodata 65535)
    PREFIX_SHARE.tif         Byte    100 * water / (water + land) in integer division: surface water occurrence (nodata 255)

written as COGs by the product writer (overviews and blocks made on the device).  PROTEUS has no such tool: there is no
reference output to be equal to; proteus_amd/stack.py states what the layers are.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import dswx_hls, pipeline   # noqa: E402
from proteus_amd.stack import MAX_TILES, NONE, NO_SHARE, wtr_spec   # noqa: E402


def read_stack(engine, files, band, same_geotransform=True, infos=None):
    """The band of every file -> (DevicePlane uint8 [n, H, W], GeoTiffInfo of the first file); files whose size or
    geotransform differ from the first are refused.  same_geotransform=False leaves the geotransforms to the caller
    (bin/dswx_mosaic.py), who finds the GeoTiffInfo of every file appended to the list `infos`."""
    stack = first = None
    for k, path in enumerate(files):
        plane, info = engine.read_bands(path)
        try:
            if not 1 <= band <= info.bands:
                raise ValueError(f'ERROR {path} has {info.bands} bands, band {band} was asked for')
            if plane.dtype != np.uint8:
                raise ValueError(f'ERROR {path} holds {plane.dtype} samples: a stack is made of Byte bands')
            if first is None:
                first = info
                stack = engine.plane((len(files), info.height, info.width), np.uint8)
            if (info.height, info.width) != (first.height, first.width):
                raise ValueError(f'[FAIL] Comparing size\n       * input 1 has size "{first.width} x {first.height}" whereas input '
                                 f'{k + 1} has size "{info.width} x {info.height}".')
            if infos is not None:
                infos.append(info)
            if same_geotransform and not np.array_equal(info.geotransform, first.geotransform):
                raise ValueError(f'[FAIL] Comparing geotransform\n       * input 1 geotransform with content "{first.geotransform}" '
                                 f'differs from input {k + 1} geotransform with content "{info.geotransform}".')
            n = info.height * info.width
            if n:
                with engine.lock:
                    engine.ctx.copy_2d_device(stack.ptr + k * n, n, plane.ptr + (band - 1) * n, n, n, 1)
                    engine.ctx.synchronize()
        except Exception:
            if stack is not None:
                stack.release()
            raise
        finally:
            plane.release()
    return stack, first


def main(argv=None):
    ap = argparse.ArgumentParser(description='Composite the dates of one tile per pixel: water counts, latest clear '
                                             'observation, surface water occurrence')
    ap.add_argument('input_file', type=str, nargs='+', help='DSWx-HLS product files of one tile, in time order')
    ap.add_argument('-o', '--output-prefix', dest='prefix', type=str, required=True, help='PREFIX of the five output files')
    ap.add_argument('--band', type=int, default=1, metavar='N', help='band of the product files to stack (default 1 = WTR)')
    ap.add_argument('--no-partial', action='store_true', help='partial surface water counts as clear and not water')
    ap.add_argument('--device', type=int, default=None, metavar='N', help='GPU to run on (default $DSWX_DEVICE or 0)')
    args = ap.parse_args(argv)
    for f in args.input_file:
        if not os.path.isfile(f):
            print(f'ERROR file not found: {f}')
            return 1
    if len(args.input_file) > MAX_TILES:
        print(f'ERROR {len(args.input_file)} files: at most {MAX_TILES}')
        return 1
    engine = pipeline.engine_of(dswx_hls.get_context(args.device))
    try:
        stack, info = read_stack(engine, args.input_file, args.band)
    except ValueError as e:
        print(e)
        return 1
    spec = wtr_spec(collapsed=True, partial_is_water=not args.no_partial, fill=dswx_hls.UINT8_FILL_VALUE)
    res = stack.stack(spec)
    stack.release()
    md = dict(info.metadata)
    md['STACK_INPUT_FILES'] = ', '.join(os.path.basename(f) for f in args.input_file)
    md['STACK_INPUT_BAND'] = str(args.band)
    md['STACK_PARTIAL_SURFACE_WATER_IS_WATER'] = str(not args.no_partial)
    outputs = (('count0', 'COUNT_WATER', 'Number of dates with water', None, None),
               ('count1', 'COUNT_LAND', 'Number of clear dates without water', None, None),
               ('last', 'LAST', 'Latest clear observation', dswx_hls._get_interpreted_dswx_ctable(True, layer_name='WTR'),
                dswx_hls.UINT8_FILL_VALUE),
               ('last_index', 'LAST_INDEX', 'Index of the file of the latest clear observation', None, NONE),
               ('share', 'SHARE', 'Surface water occurrence in percent of the clear dates', None, NO_SHARE))
    written = []
    for key, suffix, description, ctable, nodata in outputs:
        dswx_hls._save_array(res[key], f'{args.prefix}_{suffix}.tif', md, info.geo_tags, description=description,
                             output_files_list=written, ctable=ctable, no_data_value=nodata)
    for plane in res.values():
        plane.release()
    for f in written:
        print(f'file saved: {f}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
