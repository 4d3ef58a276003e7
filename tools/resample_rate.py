#!/usr/bin/env python3
"""Rate of the resample kernel (dswx_resample.hip), in one process, with HIP events on the library's stream: one float32 plane
of `--tiles` tiles of 3660 x 3660 (a smooth surface plus noise, the same in every tile) interpolated onto 3760 x 3760 at shift 5

  (a) through five meshes -- the identity (the destination is the source grown by 50 pixels on every side); the geographic mesh
      of a 1-arc-second raster under a 30 m UTM grid at 45 degrees N and at 70 degrees N (proteus_amd.warp.geographic_mesh; 1.4
      and 2.8 source columns per destination pixel, so much of the destination falls outside a source of the same pixel count:
      `head_of_tile_0` says how much); a quarter turn; int32 garbage --
      CUBIC and BILINEAR, each with `dst` alone and with every output;
  (b) alongside, the calls alternating round by round: dswx_warp_device (nearest) of the same plane through the same mesh, `dst`
      alone, and the ratio of the medians;
  (c) the share of the kernel's rectangles whose source window is staged in LDS, computed on the host from the positions by the
      kernel's rule;
  (d) what the entry replaces, on one tile, wall clock: the download of the plane, dswx_resample_host on one core, the upload
      of the result.

No ratio is fixed in advance; the one condition is that the device entry beats (d).

    python tools/resample_rate.py [--tiles 32] [--reps 20] [--out profiles/resample_rate.json]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi, resample, warp                  # noqa: E402

from histogram_rate import PEAK, row, timed_alternating        # noqa: E402  (the same timing loop and row format)

SHIFT, MARGIN, ARC = 5, 50, 1.0 / 3600.0


def geographic(lat, size, dst):
    """The mesh of a `size` x `size` raster of one arc second whose centre lies under the centre of a dst x dst grid of 30 m
    pixels on the central meridian of zone 33 at latitude `lat`."""
    _, north = warp.tm_forward(15.0, lat, 15.0)
    dst_gt = (500000.0 - dst // 2 * 30.0, 30.0, 0.0, round(float(north) / 30.0) * 30.0 + dst // 2 * 30.0, 0.0, -30.0)
    src_gt = (15.0 - size // 2 * ARC, ARC, 0.0, lat + size // 2 * ARC, 0.0, -ARC)
    return warp.geographic_mesh(src_gt, dst_gt, 32633, (dst, dst), SHIFT)


def meshes_for(size, dst, rng):
    mh, mw = warp.mesh_shape((dst, dst), SHIFT)
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) << SHIFT, np.arange(mh, dtype=np.int64) << SHIFT)
    centre = lambda c, r: np.stack([256 * c + 128, 256 * r + 128], axis=-1).astype(np.int32)
    g45, d45 = geographic(45.0, size, dst)
    g70, d70 = geographic(70.0, size, dst)
    return ({'identity': centre(X - MARGIN, Y - MARGIN), 'geographic_45N': g45, 'geographic_70N': g70,
             'quarter_turn': centre(size - 1 - (Y - MARGIN), X - MARGIN),
             'garbage': rng.integers(-(1 << 31), 1 << 31, size=(mh, mw, 2), dtype=np.int64).astype(np.int32)},
            {'geographic_45N': d45, 'geographic_70N': d70})


def lds_share(mesh, dst, size, cubic):
    """The share of the kernel's rectangles whose window is staged in LDS, by the kernel's rule (csrc/dswx_resample.hip, TAPS)."""
    rh, rw, cap = _capi.RESAMPLE_RECT_H, _capi.RESAMPLE_RECT_W, _capi.RESAMPLE_LDS_ELEMS
    sx, sy = warp.positions(mesh, SHIFT, (dst, dst))
    lo, hi = (1, 2) if cubic else (0, 1)
    c0, r0 = (sx - 128) >> 8, (sy - 128) >> 8
    near = (c0 + hi >= 0) & (c0 - lo < size) & (r0 + hi >= 0) & (r0 - lo < size)
    big = 1 << 40
    ph, pw = -(-dst // rh) * rh, -(-dst // rw) * rw

    def blocks(a, fill, op):
        p = np.full((ph, pw), fill, dtype=np.int64)
        p[:dst, :dst] = np.where(near, a, fill)
        return op(op(p.reshape(ph // rh, rh, pw // rw, rw), axis=3), axis=1)

    cl, ch = np.maximum(blocks(c0, big, np.min) - lo, 0), np.minimum(blocks(c0, -big, np.max) + hi, size - 1)
    rl, rhh = np.maximum(blocks(r0, big, np.min) - lo, 0), np.minimum(blocks(r0, -big, np.max) + hi, size - 1)
    elems = np.maximum(ch - cl + 1, 0) * np.maximum(rhh - rl + 1, 0)
    return round(float((elems <= cap).mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=32)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'resample_rate.json'))
    a = ap.parse_args()
    T, size, dst = a.tiles, a.size, a.size + 2 * MARGIN
    n, m = size * size, dst * dst
    ctx = _capi.Context(0)
    rng = np.random.default_rng(5)
    c, r = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32))
    tile = (500.0 + 200.0 * np.sin(c / 90.0) * np.cos(r / 70.0) + rng.normal(0.0, 2.0, (size, size))).astype(np.float32)
    plane = ctx.malloc(4 * T * n)
    for t in range(T):
        plane.upload(tile.view(np.uint8).reshape(-1), offset=4 * t * n)
    meshes, deviations = meshes_for(size, dst, rng)
    dev_mesh = {}
    for k, v in meshes.items():
        dev_mesh[k] = ctx.malloc(v.nbytes)
        dev_mesh[k].upload(v.view(np.uint8).reshape(-1))
    out_dst, out_how, out_head = ctx.malloc(4 * T * m), ctx.malloc(T * m), ctx.malloc(64 * T)
    word = resample.outside_word(-9999.0, np.float32)
    specs = {name: _capi.ResampleSpec.of(resample.Spec(np.float32, name, SHIFT, None, word)) for name in ('bilinear', 'cubic')}
    wspec = _capi.WarpSpec.of(warp.Spec(4, SHIFT, word))
    only = _capi.ResampleOut.of(dst=out_dst.ptr)
    every = _capi.ResampleOut.of(dst=out_dst.ptr, how=out_how.ptr, head=out_head.ptr)
    wonly = _capi.WarpOut.of(dst=out_dst.ptr)

    def res(method, mesh, out, nt=T):
        _capi._check(ctx.lib.dswx_resample_device(ctx.handle, ctypes.c_void_p(plane.ptr), ctypes.byref(specs[method]), nt, size, size,
                                                  ctypes.c_void_p(dev_mesh[mesh].ptr), dst, dst, ctypes.byref(out), None))

    def nearest(mesh):
        _capi._check(ctx.lib.dswx_warp_device(ctx.handle, ctypes.c_void_p(plane.ptr), ctypes.byref(wspec), T, size, size,
                                              ctypes.c_void_p(dev_mesh[mesh].ptr), dst, dst, ctypes.byref(wonly), None))

    fns = {}
    for k in meshes:
        fns[f'nearest_{k}_dst'] = lambda k=k: nearest(k)
        for method in ('bilinear', 'cubic'):
            fns[f'{method}_{k}_dst'] = lambda k=k, method=method: res(method, k, only)
            fns[f'{method}_{k}_all'] = lambda k=k, method=method: res(method, k, every)
    ms = timed_alternating(ctx, fns, a.reps)
    rec = {k: row(4 * T * m, v) for k, v in ms.items()}
    res('cubic', 'identity', only)
    kernel = ctx.last_kernel_info()
    ctx.synchronize()
    heads = {}
    for k in meshes:
        res('cubic', k, every)
        ctx.synchronize()
        heads[k] = [int(v) for v in out_head.download(np.uint64, 8)]
    out = {'tool': 'tools/resample_rate.py', 'kernel': kernel, 'resident_tiles': T, 'tile': [size, size], 'destination': [dst, dst], 'shift': SHIFT,
           'reps': a.reps, 'hbm_peak_GBps': PEAK, 'rates_are': 'bytes of destination written per second: n_tiles x dst pixels x 4',
           'content': 'float32: a smooth surface plus noise, the same in every tile', 'mesh_deviation_256ths': deviations,
           'head_of_tile_0_cubic': heads, 'head_words': 'pixels, cubic, bilinear full, renormalised, outside, min row, max row, 0',
           'lds_share_of_rectangles': {k: {'cubic': lds_share(v, dst, size, True), 'bilinear': lds_share(v, dst, size, False)} for k, v in meshes.items()},
           'rates': rec,
           'ratio_to_nearest_dst': {f'{method}_{k}': round(rec[f'{method}_{k}_dst']['ms_median'] / rec[f'nearest_{k}_dst']['ms_median'], 3)
                                    for k in meshes for method in ('bilinear', 'cubic')}}
    # (d) what the entry replaces: download, one core, upload -- one tile
    spec = resample.Spec(np.float32, 'cubic', SHIFT, None, word)
    t0 = time.perf_counter()
    got = plane.download(np.float32, n).reshape(1, size, size)
    t1 = time.perf_counter()
    ref = _capi.resample_host(got, meshes['geographic_45N'], spec, (dst, dst), want=('dst',))['dst']
    t2 = time.perf_counter()
    out_dst.upload(ref.view(np.uint8).reshape(-1))
    t3 = time.perf_counter()
    res('cubic', 'geographic_45N', only, nt=1)
    ctx.synchronize()
    same = bool(np.array_equal(out_dst.download(np.uint32, m), ref.reshape(-1).view(np.uint32)))
    one = timed_alternating(ctx, {'cubic': lambda: res('cubic', 'geographic_45N', only, nt=1)}, a.reps)['cubic']
    host_ms = [round((t1 - t0) * 1e3, 2), round((t2 - t1) * 1e3, 2), round((t3 - t2) * 1e3, 2)]
    out['d_replaced'] = {'tiles': 1, 'mesh': 'geographic_45N', 'method': 'cubic', 'download_host_upload_ms': host_ms, 'device_dst': row(4 * m, one),
                         'device_dst_equals_host_dst': same, 'speedup_over_download_host_upload': round(sum(host_ms) / one[len(one) // 2], 1),
                         'device_beats_replaced_path': bool(one[len(one) // 2] < sum(host_ms))}
    for b in list(dev_mesh.values()) + [plane, out_dst, out_how, out_head]:
        b.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
