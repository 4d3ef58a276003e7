#!/usr/bin/env python3
"""Rate of the land-mesh kernel (dswx_land_mesh.hip), in one process, with HIP events on the library's stream: 4 tiles of 3660 x
3660 HLS pixels, every tile with its own synthetic WorldCover and CGLS source window, through five mesh pairs:

  identity      the maps already on their grids (windows 10980 x 10980 and 3660 x 3660)
  lat45, lat70  the real meshes of maps in EPSG:4326 at 1/12000 and 1/1008 degree under a tile of UTM zone 32 at 45 and 70
                degrees N (landmesh.choose_mesh: the product path's shift rule; windows by landmesh.source_window)
  quarter_turn  every fine row a source column: the worst gather
  garbage       int32 noise (almost every tap outside)

Measured per mesh pair, the calls alternating round by round, min - median - max of --reps: the entry with LAND alone and with
LAND and head; alongside, on the same bytes, the chain it is defined as -- dswx_warp_device of the WorldCover windows onto [4][3 H][3
W], dswx_warp_device of the CGLS windows onto [4][H][W], dswx_landcover_mask_device -- whose LAND is compared with the entry's;
and dswx_batch_histogram of a resident WTR plane of the same four tiles as the yardstick.  Then one product's LAND step (a tile
of --product-size pixels, maps written as GeoTIFFs in EPSG:4326): the host's read of the two source windows against the device.

ONE BAR, fixed before the first measurement because it follows from the bytes (the entry moves S + N against the chain's S + 21
N): at the 45-degree meshes the entry's median (LAND alone) must not exceed the chain's median.  Recorded as met or not.

    python tools/land_mesh_rate.py [--tiles 4] [--size 3660] [--reps 20] [--out profiles/land_mesh_rate.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi, geotiff, landmesh, warp          # noqa: E402
from proteus_amd.synth import SEED                              # noqa: E402

from histogram_rate import PEAK, row, timed_alternating        # noqa: E402  (the same timing loop and row format)

WC_PIXEL, CG_PIXEL = 1.0 / 12000.0, 1.0 / 1008.0
WC_CODES = np.array([10, 10, 10, 50, 50, 80, 90, 95, 0, 20, 30, 40, 60, 100], dtype=np.uint8)
CG_CODES = np.array([111, 111, 113, 115, 121, 20, 30, 0, 200], dtype=np.uint8)
FOREST = (111, 113, 115, 121)


def patchy(rng, codes, n, h, w, block):
    """uint8 [n, h, w]: classes per block of `block` pixels, distinct per tile."""
    out = np.empty((n, max(h, 0), max(w, 0)), dtype=np.uint8)
    for t in range(n):
        small = codes[rng.integers(0, codes.size, size=(-(-h // block) + 1, -(-w // block) + 1))]
        out[t] = np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:h, :w]
    return out


def hls_grid(lat, size, zone=32, pixel=30.0):
    lon0 = -183.0 + 6.0 * zone
    _, north = warp.tm_forward(lon0, lat, lon0)
    return (500000.0 - size // 2 * pixel, pixel, 0.0, round(float(north) / pixel) * pixel + size // 2 * pixel, 0.0, -pixel), 32600 + zone


def centre_mesh(shape, shift, fn):
    mh, mw = warp.mesh_shape(shape, shift)
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) << shift, np.arange(mh, dtype=np.int64) << shift)
    c, r = fn(X, Y)
    return np.stack([256 * c + 128, 256 * r + 128], axis=-1).astype(np.int32)


def cases(size, rng):
    """{name: (wc window shape, cg window shape, mesh_wc, mesh_cg, shift_wc, shift_cg, note)}"""
    F = 3 * size
    out = {'identity': ((F, F), (size, size), centre_mesh((F, F), 6, lambda X, Y: (X, Y)), centre_mesh((size, size), 6, lambda X, Y: (X, Y)), 6, 6, {})}
    for lat in (45.0, 70.0):
        gt, epsg = hls_grid(lat, size)
        fine = (gt[0], gt[1] / 3, 0.0, gt[3], 0.0, gt[5] / 3)
        lon0 = -183.0 + 6.0 * 32
        got = []
        for pixel, dst_gt, shape in ((WC_PIXEL, fine, (F, F)), (CG_PIXEL, gt, (size, size))):
            src_gt = (lon0 - 2.0, pixel, 0.0, float(np.floor(lat)) + 2.0, 0.0, -pixel)
            mesh, shift, deviation = landmesh.choose_mesh(src_gt, 4326, dst_gt, epsg, shape)
            window, moved = landmesh.source_window(mesh, deviation, 1 << 26, 1 << 26)
            got.append(((window[3], window[2]), moved, shift, deviation))
        out[f'lat{int(lat)}'] = (got[0][0], got[1][0], got[0][1], got[1][1], got[0][2], got[1][2],
                                 {'deviation_256ths': [round(got[0][3], 3), round(got[1][3], 3)]})
    out['quarter_turn'] = ((F, F), (size, size), centre_mesh((F, F), 6, lambda X, Y: (F - 1 - Y, X)),
                           centre_mesh((size, size), 6, lambda X, Y: (size - 1 - Y, X)), 6, 6, {})
    g = lambda shape: rng.integers(-(1 << 31), 1 << 31, size=warp.mesh_shape(shape, 6) + (2,), dtype=np.int64).astype(np.int32)
    out['garbage'] = ((F, F), (size, size), g((F, F)), g((size, size)), 6, 6, {})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=4)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--product-size', type=int, default=1098)
    ap.add_argument('--only', default='', help='comma-separated mesh names (default: all)')
    ap.add_argument('--out', default=os.path.join('profiles', 'land_mesh_rate.json'))
    a = ap.parse_args()
    T, H = a.tiles, a.size
    N = H * H
    rng = np.random.default_rng(5)
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, T, H, H)
    batch.synth(SEED)
    batch.classify(_capi.default_params())
    ctx.synchronize()
    wtr = _capi.PLANE_INDEX['wtr']
    hist = np.zeros((1, T, 256), dtype=np.uint64)

    def histogram():
        _capi._check(ctx.lib.dswx_batch_histogram(batch.handle, 1 << wtr, 0, T, 0, 6, _capi._host_ptr(hist), None))

    w3, c1 = ctx.malloc(9 * T * N), ctx.malloc(T * N)
    land, land_chain, head = ctx.malloc(T * N), ctx.malloc(T * N), ctx.malloc(64 * T)
    out = {'tool': 'tools/land_mesh_rate.py', 'tiles': T, 'tile': [H, H], 'reps': a.reps, 'hbm_peak_GBps': PEAK,
           'design': 'one workgroup = 8 x 32 HLS pixels, one pixel per thread, at most 1024 workgroups that walk the rectangles: mesh_position for each of '
                     'the nine fine pixels and the HLS pixel; nine WorldCover gathers and one CGLS gather, each behind the comparison of its '
                     'position with the raster; the code table in LDS; one byte stored; no LDS staging, no barrier per rectangle',
           'rates_are': 'bytes of LAND written plus source windows per second: n_tiles x (H W + wc window + cg window)', 'meshes': {}}
    wanted = [k for k in a.only.split(',') if k]
    for name, (wc_shape, cg_shape, m_wc, m_cg, s_wc, s_cg, note) in cases(H, rng).items():
        if wanted and name not in wanted:
            continue
        wc, cg = patchy(rng, WC_CODES, T, wc_shape[0], wc_shape[1], 9), patchy(rng, CG_CODES, T, cg_shape[0], cg_shape[1], 3)
        bufs = [ctx.malloc(max(x.nbytes, 8)) for x in (wc, cg, m_wc, m_cg)]
        for b, x in zip(bufs, (wc, cg, m_wc, m_cg)):
            b.upload(x.view(np.uint8).reshape(-1))
        del wc, cg
        spec = landmesh.Spec(s_wc, s_cg, 0, 0, (6, 3, 7, 3), 21, FOREST)
        w_wc, w_cg = warp.Spec(1, s_wc, 0), warp.Spec(1, s_cg, 0)

        def entry(head_ptr=None):
            ctx.land_mesh_device(bufs[0].ptr, wc_shape, bufs[1].ptr, cg_shape, spec, T, H, H, bufs[2].ptr, bufs[3].ptr, land.ptr, head_ptr)

        def chain():
            ctx.warp_device(bufs[0].ptr, w_wc, T, wc_shape[0], wc_shape[1], bufs[2].ptr, 3 * H, 3 * H, _capi.WarpOut.of(dst=w3.ptr))
            ctx.warp_device(bufs[1].ptr, w_cg, T, cg_shape[0], cg_shape[1], bufs[3].ptr, H, H, _capi.WarpOut.of(dst=c1.ptr))
            ctx.landcover_mask_device(w3.ptr, c1.ptr, T, H, H, FOREST, land_chain.ptr, thresholds=(6, 3, 7, 3), year_offset=21)

        ms = timed_alternating(ctx, {'entry_land': entry, 'entry_land_head': lambda: entry(head.ptr), 'chain_warp_warp_mask': chain,
                                     'histogram_wtr': histogram}, a.reps)
        S = T * (wc_shape[0] * wc_shape[1] + cg_shape[0] * cg_shape[1])
        rec = {'wc_window': list(wc_shape), 'cg_window': list(cg_shape), 'shift_wc': s_wc, 'shift_cg': s_cg, **note,
               'entry_land': row(S + T * N, ms['entry_land']), 'entry_land_head': row(S + T * N, ms['entry_land_head']),
               'chain_warp_warp_mask': row(S + 21 * T * N, ms['chain_warp_warp_mask']), 'histogram_wtr': row(T * N, ms['histogram_wtr'])}
        entry(head.ptr)
        rec['kernel'] = ctx.last_kernel_info()
        chain()
        ctx.synchronize()
        rec['head_of_tile_0'] = [int(v) for v in head.download(np.uint64, 8)]
        rec['entry_equals_chain'] = bool(np.array_equal(land.download(np.uint8, T * N), land_chain.download(np.uint8, T * N)))
        rec['entry_over_chain_median'] = round(rec['entry_land']['ms_median'] / rec['chain_warp_warp_mask']['ms_median'], 4)
        out['meshes'][name] = rec
        print(name, json.dumps({k: rec[k] for k in ('entry_over_chain_median', 'entry_equals_chain', 'wc_window')}), flush=True)
        for b in bufs:
            b.free()
    if 'lat45' in out['meshes']:
        r = out['meshes']['lat45']['entry_over_chain_median']
        out['bar'] = {'statement': 'lat45: entry_land ms_median <= chain_warp_warp_mask ms_median', 'ratio': r, 'met': bool(r <= 1.0)}
    for b in (w3, c1, land, land_chain, head):
        b.free()
    batch.free()

    # one product's LAND step: the host's read of the two windows against the device
    if a.product_size > 0:
        P = a.product_size
        gt, epsg = hls_grid(45.0, P)
        tags = geotiff.geo_tags_from_geotransform(gt, epsg)
        lon0 = -183.0 + 6.0 * 32
        with tempfile.TemporaryDirectory() as tmp:
            files = {}
            for key, pixel, codes, span in (('wc', WC_PIXEL, WC_CODES, 0.6), ('cg', CG_PIXEL, CG_CODES, 0.6)):
                n = int(span / pixel)
                path = os.path.join(tmp, f'{key}.tif')
                src_gt = (lon0 - span / 2, pixel, 0.0, 45.0 + span / 2, 0.0, -pixel)
                geotiff.write_geotiff(path, patchy(rng, codes, 1, n, n, 9)[0], geo_tags=geotiff.geo_tags_from_geotransform(src_gt, 4326), nodata=0)
                files[key] = path
            t0 = time.perf_counter()
            plans = {k: landmesh.plan(geotiff.open_geotiff(files[k]).info, gt, tags, P, P, 3 if k == 'wc' else 1) for k in files}
            t1 = time.perf_counter()
            src = {k: np.ascontiguousarray(geotiff.read_geotiff(files[k], window=plans[k][0])[0]) for k in files}
            t2 = time.perf_counter()
            spec = landmesh.Spec(plans['wc'][2], plans['cg'][2], 0, 0, (6, 3, 7, 3), 21, FOREST)
            ctx.land_mesh(src['wc'], src['cg'], plans['wc'][1], plans['cg'][1], (P, P), spec)          # (first call: allocations warm)
            t3 = time.perf_counter()
            got, hd = ctx.land_mesh(src['wc'], src['cg'], plans['wc'][1], plans['cg'][1], (P, P), spec)
            t4 = time.perf_counter()
            out['product_land_step'] = {'tile': [P, P], 'file_pixels': {k: int(geotiff.open_geotiff(files[k]).info.width) ** 2 for k in files},
                                        'windows': {k: list(plans[k][0]) for k in files}, 'plan_ms': round((t1 - t0) * 1e3, 2),
                                        'host_window_read_ms': round((t2 - t1) * 1e3, 2),
                                        'upload_kernel_download_ms': round((t4 - t3) * 1e3, 2), 'head': [int(v) for v in hd],
                                        'note': 'geotiff.read_geotiff decodes the whole file and crops afterwards'}
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
