#!/usr/bin/env python3
"""`dswx_warp.py product.tif --like other.tif [--band N] [--shift 6] [--outside 255] [--resample nearest] [--device N] -o out.tif`

One layer laid over the lattice of another file on the GPU (include/dswx_hip.h "warp"): band N (default 1) of product.tif is
read into HBM, a mesh of source coordinates is computed on the host from the two geotransforms and GeoKeys -- the same SRS
(a shifted origin, another pixel size: proteus_amd.warp.affine_mesh) or two WGS 84 / UTM zones (EPSG 326zz / 327zz:
proteus_amd.warp.utm_mesh, this project's own transverse Mercator) -- with one node every 1 << shift pixels of other.tif, and
one kernel launch picks for every pixel of other.tif's lattice the NEAREST pixel of the product; pixels that fall outside the
product get --outside (default 255, the product's fill).  out.tif is a COG with the size, the geotransform and the GeoKeys of
other.tif and the metadata of product.tif.  One line of JSON says how many pixels were inside and how far the interpolated
mesh is from the exact mapping at most (in 1/256 pixel of the product): choose a smaller --shift if that is too far.

--resample bilinear | cubic INTERPOLATES a float32 or int16 band instead (include/dswx_hip.h "resample"): the input's nodata
value marks taps that are not valid, and --outside is the value of the pixels without a valid tap.  The input may then be in
EPSG:4326 under a WGS 84 / UTM lattice (proteus_amd.warp.geographic_mesh).  The default, nearest, is the path described above, and refuses such an input as before.

No mode / average resampling; no SRS other than EPSG:4326 and WGS 84 / UTM across files; no antimeridian.  PROTEUS does this through gdal.Warp, which is not part of this project's environment: GDAL's own choice of the
nearest pixel, its approximate transformer (0.125 pixel error threshold) and its handling of a centre exactly on a pixel
boundary are not pinned by execution; proteus_amd/warp.py states what this tool computes.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np   # noqa: E402

from proteus_amd import dswx_hls, geotiff, pipeline, resample, warp   # noqa: E402

PROJECTION_TAGS = (geotiff.TAG_GEOKEYS, geotiff.TAG_GEO_DOUBLES, geotiff.TAG_GEO_ASCII)


def read_band(engine, path, band):
    """(DevicePlane [H, W] of band `band` of the file, its GeoTiffInfo)."""
    plane, info = engine.read_bands(path)
    try:
        if not 1 <= band <= info.bands:
            raise ValueError(f'ERROR {path} has {info.bands} bands, band {band} was asked for')
        if plane.dtype.itemsize not in (1, 2, 4):
            raise ValueError(f'ERROR {path} holds {plane.dtype} samples: elements of 1, 2 or 4 bytes are warped')
        one = engine.plane((info.height, info.width), plane.dtype)
        n = info.height * info.width * plane.dtype.itemsize
        if n:
            with engine.lock:
                engine.ctx.copy_2d_device(one.ptr, n, plane.ptr + (band - 1) * n, n, n, 1)
                engine.ctx.synchronize()
    finally:
        plane.release()
    return one, info


def same_projection(a, b):
    for tag in PROJECTION_TAGS:
        x, y = a.geo_tags.get(tag), b.geo_tags.get(tag)
        if (x is None) != (y is None) or (x is not None and (x[0] != y[0] or list(x[1]) != list(y[1]))):
            return False
    return True


def mesh_for(src_info, dst_info, shift, geographic=False):
    """(mesh, deviation in 1/256 source pixel) that lays src_info's raster onto dst_info's lattice; `geographic`: a source in
    EPSG:4326 is taken (the interpolating methods), not refused (nearest, as before)."""
    src_gt, dst_gt = (tuple(float(v) for v in i.geotransform) for i in (src_info, dst_info))
    shape = (dst_info.height, dst_info.width)
    if same_projection(src_info, dst_info):
        return warp.affine_mesh(src_gt, dst_gt, shape, shift), 0.0
    src_epsg, dst_epsg = warp.epsg_of(src_info.geo_tags), warp.epsg_of(dst_info.geo_tags)
    if geographic and src_epsg == warp.GEOGRAPHIC_EPSG:
        return warp.geographic_mesh(src_gt, dst_gt, dst_epsg, shape, shift)
    return warp.utm_mesh(src_gt, src_epsg, dst_gt, dst_epsg, shape, shift)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Lay one layer over the lattice, size and projection of another file (nearest pixel)')
    ap.add_argument('input_file', type=str, help='the file whose band is warped')
    ap.add_argument('--like', type=str, required=True, metavar='other.tif', help='the file whose lattice, size and GeoKeys the output gets')
    ap.add_argument('-o', '--output', dest='output', type=str, required=True, help='the output COG')
    ap.add_argument('--band', type=int, default=1, metavar='N', help='band of the input file (default 1)')
    ap.add_argument('--shift', type=int, default=6, metavar='S', help='a mesh node every 1 << S output pixels, 0 .. 8 (default 6)')
    ap.add_argument('--outside', type=int, default=dswx_hls.UINT8_FILL_VALUE, metavar='V', help='value of the pixels outside the input (default 255)')
    ap.add_argument('--resample', choices=('nearest', 'bilinear', 'cubic'), default='nearest',
                    help='nearest (default) copies the nearest pixel; bilinear and cubic interpolate a float32 or int16 band')
    ap.add_argument('--device', type=int, default=None, metavar='N', help='GPU to run on (default $DSWX_DEVICE or 0)')
    args = ap.parse_args(argv)
    for f in (args.input_file, args.like):
        if not os.path.isfile(f):
            print(f'ERROR file not found: {f}')
            return 1
    if not 0 <= args.shift <= warp.MAX_SHIFT:
        print(f'ERROR --shift {args.shift} outside 0 .. {warp.MAX_SHIFT}')
        return 1
    try:
        like = geotiff.open_geotiff(args.like).info             # the directory alone: no pixel of --like is read
    except geotiff.GeoTiffError as e:
        print(f'ERROR could not open {args.like}: {e}')
        return 1
    engine = pipeline.engine_of(dswx_hls.get_context(args.device))
    try:
        plane, info = read_band(engine, args.input_file, args.band)
    except ValueError as e:
        print(e)
        return 1
    try:
        mesh, deviation = mesh_for(info, like, args.shift, geographic=args.resample != 'nearest')
    except ValueError as e:
        plane.release()
        print(f'ERROR {e}')
        return 1
    if args.resample != 'nearest':
        try:
            word = resample.outside_word(args.outside, plane.dtype) if plane.dtype in resample.DTYPES.values() else 0
            res = plane.resample(mesh, (like.height, like.width), args.shift, args.resample, nodata=info.nodata, outside=word, want=('dst', 'head'))
        except ValueError as e:
            plane.release()
            print(f'ERROR {e}')
            return 1
    else:
        res = plane.warp(mesh, (like.height, like.width), args.shift, outside=args.outside, want=('dst', 'head'))
    plane.release()
    head = [int(v) for v in res['head'].numpy()[0]]
    res['head'].release()
    md = dict(info.metadata)
    md['WARP_INPUT_FILE'] = os.path.basename(args.input_file)
    md['WARP_INPUT_BAND'] = str(args.band)
    md['WARP_LIKE_FILE'] = os.path.basename(args.like)
    md['WARP_MESH_SHIFT'] = str(args.shift)
    if args.resample != 'nearest':
        md['WARP_RESAMPLE'] = args.resample
    tags = dict(like.geo_tags)
    written = []
    dswx_hls._save_array(res['dst'], args.output, md, tags, output_files_list=written,
                         no_data_value=args.outside if np.dtype(res['dst'].dtype).kind in 'iu' else None)
    res['dst'].release()
    for f in written:
        print(f'file saved: {f}')
    if args.resample != 'nearest':
        print(json.dumps({'pixels': head[0], 'cubic': head[1], 'bilinear': head[2], 'renormalised': head[3], 'outside': head[4],
                          'source_rows': head[5:7], 'resample': args.resample, 'mesh_shift': args.shift, 'mesh_deviation_256ths': deviation}))
        return 0
    print(json.dumps({'pixels': head[0], 'inside': head[1], 'outside': head[2], 'source_rows': head[3:5], 'source_columns': head[5:7],
                      'mesh_shift': args.shift, 'mesh_deviation_256ths': deviation}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
