#!/usr/bin/env python3
"""`dswx_mosaic.py [--band N] [--no-partial] [--reproject] [--device N] [--bodies FILE.json] -o PREFIX file1.tif file2.tif ...`

Neighbouring tiles, and several dates of them, placed on one canvas and composited per canvas pixel on the GPU
(include/dswx_hip.h "mosaic"): band N (default 1 = WTR) of every DSWx-HLS product file is read into one resident [n, H, W]
plane, the geotransforms place every file on the lattice of the first (proteus_amd.mosaic.layout: the canvas is the bounding
box of the footprints), and one kernel launch turns the plane into

    PREFIX_COUNT_WATER.tif   UInt16  on how many covering files the pixel was water (open or, unless --no-partial, partial)
    PREFIX_COUNT_LAND.tif    UInt16  on how many it was clear and not water
    PREFIX_LAST.tif          Byte    its latest clear observation, in the order of the files (nodata 255, WTR colours); a pixel
                                     outside every footprint is 255 too
    PREFIX_LAST_INDEX.tif    UInt16  which file (0 = the first) that observation came from (nodata 65535)
    PREFIX_SHARE.tif         Byte    100 * water / (water + land) in integer division: surface water occurrence (nodata 255)

written as COGs with the geotransform of the canvas by the product writer.  The files are given in priority / time order: where
footprints overlap, the LAST file that saw the pixel clear gives LAST.  They must be of one size and one projection (the
GeoKey tags are compared) and lie on one lattice of whole pixels: without --reproject nothing is resampled or reprojected, so a
neighbour in another UTM zone is refused.  With --reproject an input whose GeoKeys name another WGS 84 / UTM zone, or whose
origin or pixel size is off the lattice of input 1, is first resampled on the GPU (nearest pixel; include/dswx_hip.h "warp",
proteus_amd/warp.py makes the mesh) onto the lattice of input 1 -- into a window of the inputs' size around the centre of its
footprint, so the corners that a rotation of a few degrees turns out of that window are lost -- and then placed like the
others.  With --bodies FILE.json the water bodies of the LAST canvas are labelled on the GPU
(include/dswx_hip.h "label") and the summary is written to FILE.json and printed as one line of JSON: a lake on a seam is ONE
body.  PROTEUS has no such tool: there is no reference output to be equal to; proteus_amd/mosaic.py states what the layers are.
"""
import argparse
import importlib.util
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import _capi, dswx_hls, geotiff, pipeline, warp   # noqa: E402
from proteus_amd.label import wtr_label_spec   # noqa: E402
from proteus_amd.mosaic import layout, wtr_mosaic_spec   # noqa: E402
from proteus_amd.stack import MAX_TILES, NONE, NO_SHARE   # noqa: E402

_spec = importlib.util.spec_from_file_location('dswx_stack_tool', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dswx_stack.py'))
_stack_tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_stack_tool)
read_stack = _stack_tool.read_stack

PROJECTION_TAGS = (geotiff.TAG_GEOKEYS, geotiff.TAG_GEO_DOUBLES, geotiff.TAG_GEO_ASCII)
REPROJECT_SHIFT = 5                     # --reproject: a mesh node every 32 pixels


def same_projection(a, b):
    for tag in PROJECTION_TAGS:
        x, y = a.geo_tags.get(tag), b.geo_tags.get(tag)
        if (x is None) != (y is None) or (x is not None and (x[0] != y[0] or list(x[1]) != list(y[1]))):
            return False
    return True


def reproject_window(gt, epsg, gt1, epsg1, height, width):
    """The geotransform of the height x width window on the lattice of input 1 (gt1, epsg1) around the centre of the footprint
    of an input with geotransform gt and EPSG code epsg (None / equal codes: the same SRS)."""
    cx, cy = gt[0] + width / 2.0 * gt[1], gt[3] + height / 2.0 * gt[5]
    if epsg != epsg1:
        cx, cy = (float(v) for v in warp.utm_to_utm(cx, cy, epsg, epsg1))
    col0 = int(round((cx - gt1[0]) / gt1[1] - width / 2.0))
    row0 = int(round((cy - gt1[3]) / gt1[5] - height / 2.0))
    return (gt1[0] + col0 * gt1[1], gt1[1], 0.0, gt1[3] + row0 * gt1[5], 0.0, gt1[5])


def reproject_inputs(engine, plane, infos):
    """--reproject: every input that is not on the lattice of input 1 -- another WGS 84 / UTM zone, an origin that is not a
    whole number of pixels away, another pixel size -- is resampled on the device, in its slot of `plane`, onto its
    reproject_window.  Returns the geotransforms that place the slots and the (1-based) inputs that were resampled."""
    first = infos[0]
    gt1 = tuple(float(v) for v in first.geotransform)
    H, W = first.height, first.width
    gts, moved = [gt1], []
    for k, info in enumerate(infos[1:], 2):
        gt = tuple(float(v) for v in info.geotransform)
        same = same_projection(first, info)
        col, row = (gt[0] - gt1[0]) / gt1[1], (gt[3] - gt1[3]) / gt1[5]
        if same and gt[1:3] == gt1[1:3] and gt[4:] == gt1[4:] and abs(col - round(col)) <= 1e-6 and abs(row - round(row)) <= 1e-6:
            gts.append(gt)
            continue
        epsg, epsg1 = (None, None) if same else (warp.epsg_of(info.geo_tags), warp.epsg_of(first.geo_tags))
        try:
            window = reproject_window(gt, epsg, gt1, epsg1, H, W)
            mesh, _ = warp.mesh_between(gt, epsg, window, epsg1, (H, W), REPROJECT_SHIFT)
        except ValueError as e:
            raise ValueError(f'[FAIL] Reprojecting input {k}\n       * {e}.') from None
        table, tmp = engine.upload(mesh), engine.plane((H, W), np.uint8)
        try:
            with engine.lock:
                slot = plane.ptr + (k - 1) * H * W
                engine.ctx.warp_device(slot, warp.Spec(1, REPROJECT_SHIFT, dswx_hls.UINT8_FILL_VALUE), 1, H, W, table.ptr, H, W,
                                       _capi.WarpOut.of(dst=tmp.ptr))
                engine.ctx.copy_2d_device(slot, H * W, tmp.ptr, H * W, H * W, 1)
                engine.ctx.synchronize()
        finally:
            table.release()
            tmp.release()
        gts.append(window)
        moved.append(k)
    return gts, moved


def place_files(infos, geotransforms=None, moved=()):
    """(canvas_h, canvas_w, place, canvas geotransform, canvas geo tags) of the files; refused: another projection than the
    first file's, and what proteus_amd.mosaic.layout refuses.  --reproject gives the geotransforms of the slots and the
    (1-based) inputs it has resampled, whose own projection no longer matters."""
    first = infos[0]
    for k, info in enumerate(infos):
        if k + 1 in moved:
            continue
        for tag in PROJECTION_TAGS:
            a, b = first.geo_tags.get(tag), info.geo_tags.get(tag)
            if (a is None) != (b is None) or (a is not None and (a[0] != b[0] or list(a[1]) != list(b[1]))):
                raise ValueError(f'[FAIL] Comparing projection\n       * input 1 GeoTIFF tag {tag} with content "{a}" differs from input '
                                 f'{k + 1} GeoTIFF tag {tag} with content "{b}".')
    try:
        canvas_h, canvas_w, place, gt = layout(geotransforms if geotransforms is not None else
                                               [tuple(float(v) for v in i.geotransform) for i in infos], first.height, first.width)
    except ValueError as e:
        raise ValueError(f'[FAIL] Comparing geotransform\n       * {e}.') from None
    tags = dict(first.geo_tags)
    tags.pop(geotiff.TAG_TRANSFORM, None)
    tags.update({k: v for k, v in geotiff.geo_tags_from_geotransform(gt).items()})
    return canvas_h, canvas_w, place, gt, tags


def main(argv=None):
    ap = argparse.ArgumentParser(description='Mosaic neighbouring tiles and their dates per canvas pixel: water counts, latest '
                                             'clear observation, surface water occurrence')
    ap.add_argument('input_file', type=str, nargs='+', help='DSWx-HLS product files of one size on one lattice, in priority / time order')
    ap.add_argument('-o', '--output-prefix', dest='prefix', type=str, required=True, help='PREFIX of the five output files')
    ap.add_argument('--band', type=int, default=1, metavar='N', help='band of the product files to mosaic (default 1 = WTR)')
    ap.add_argument('--no-partial', action='store_true', help='partial surface water counts as clear and not water')
    ap.add_argument('--reproject', action='store_true', help='resample inputs in another UTM zone or off the lattice of input 1 onto it (nearest pixel)')
    ap.add_argument('--bodies', type=str, default=None, metavar='FILE.json', help='label the water bodies of LAST, write the summary')
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
    infos = []
    try:
        plane, info = read_stack(engine, args.input_file, args.band, same_geotransform=False, infos=infos)
    except ValueError as e:
        print(e)
        return 1
    try:
        gts, moved = reproject_inputs(engine, plane, infos) if args.reproject else (None, ())
        canvas_h, canvas_w, place, gt, tags = place_files(infos, gts, moved)
    except ValueError as e:
        plane.release()
        print(e)
        return 1
    spec = wtr_mosaic_spec(collapsed=True, partial_is_water=not args.no_partial, fill=dswx_hls.UINT8_FILL_VALUE,
                           outside=dswx_hls.UINT8_FILL_VALUE)
    res = plane.mosaic(place, (canvas_h, canvas_w), spec)
    plane.release()
    md = dict(info.metadata)
    md['MOSAIC_INPUT_FILES'] = ', '.join(os.path.basename(f) for f in args.input_file)
    md['MOSAIC_INPUT_BAND'] = str(args.band)
    md['MOSAIC_PARTIAL_SURFACE_WATER_IS_WATER'] = str(not args.no_partial)
    md['MOSAIC_PLACEMENTS_ROW_COL'] = ', '.join(f'{int(r)} {int(c)}' for r, c in place)
    if args.reproject:
        md['MOSAIC_REPROJECTED_INPUTS'] = ', '.join(str(k) for k in moved)
    said = None
    if args.bodies is not None:
        lab = res['last'].label(wtr_label_spec(1, partial_is_water=not args.no_partial), want=('summary',))
        s = [int(v) for v in lab['summary'].numpy()[0]]
        for p in lab.values():
            p.release()
        said = {'input_files': [os.path.basename(f) for f in args.input_file], 'band': args.band, 'canvas_height': canvas_h,
                'canvas_width': canvas_w, 'bodies': s[0], 'member_pixels': s[1], 'largest_size': s[2], 'largest_label': s[3],
                'bodies_by_log2_size': s[8:], 'pixel_area_m2': abs(gt[1] * gt[5])}
    outputs = (('count0', 'COUNT_WATER', 'Number of covering files with water', None, None),
               ('count1', 'COUNT_LAND', 'Number of clear covering files without water', None, None),
               ('last', 'LAST', 'Latest clear observation', dswx_hls._get_interpreted_dswx_ctable(True, layer_name='WTR'),
                dswx_hls.UINT8_FILL_VALUE),
               ('last_index', 'LAST_INDEX', 'Index of the file of the latest clear observation', None, NONE),
               ('share', 'SHARE', 'Surface water occurrence in percent of the clear covering files', None, NO_SHARE))
    written = []
    for key, suffix, description, ctable, nodata in outputs:
        dswx_hls._save_array(res[key], f'{args.prefix}_{suffix}.tif', md, tags, description=description,
                             output_files_list=written, ctable=ctable, no_data_value=nodata)
    for p in res.values():
        p.release()
    if said is not None:
        with open(args.bodies, 'w') as f:
            json.dump(said, f)
        written.append(args.bodies)
    for f in written:
        print(f'file saved: {f}')
    if said is not None:
        print(json.dumps(said))
    return 0


if __name__ == '__main__':
    sys.exit(main())
