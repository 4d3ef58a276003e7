#!/usr/bin/env python3
"""Rate of the warp kernel (dswx_warp.hip), in one process, with HIP events on the library's stream, on the planes of a resident
batch of 3660 x 3660 tiles (generated and classified: per-pixel class noise) warped onto 3660 x 3660 at shift 6:

  (a) the uint8 WTR plane, `dst` alone and every output, through five meshes: the identity; a whole-pixel shift; the real mesh
      of UTM zone 33 seen from zone 32 at 45 degrees N (proteus_amd.warp.utm_mesh); a quarter turn (every destination row a
      source column: the worst gather); int32 garbage (almost everything outside).
  (b) the int16 NIR plane and a uint32 plane (the src_index of (a), as a caller's plane) through the UTM mesh.
  (c) alongside, the calls alternating round by round: dswx_batch_mosaic of the same tiles at the identity placement with
      `last` alone -- the parent commit's code on the same bytes read -- and dswx_batch_histogram of the same plane.
  (d) what the entry replaces, on the first four tiles, wall clock: the download of the plane, dswx_warp_host on one core, the
      upload of the result.

Rates are in bytes of tiles READ per second (n_tiles x pixels x elem_bytes), although a gather does not read every byte once.
ONE BAR, fixed before the first measurement: at the identity mesh, `dst` alone may take at most 1.5 times the mosaic's median
time.  It is recorded as met or not; DESIGN.md section 5 owes the instructions that cost it where it is not.

    python tools/warp_rate.py [--tiles 32] [--reps 20] [--out profiles/warp_rate.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi, warp                            # noqa: E402
from proteus_amd.mosaic import wtr_mosaic_spec                 # noqa: E402
from proteus_amd.synth import SEED                             # noqa: E402

from histogram_rate import PEAK, row, timed_alternating        # noqa: E402  (the same timing loop and row format)

SHIFT = 6
BAR = 1.5


def meshes_for(size, rng):
    """{name: int32 [mesh_h, mesh_w, 2]} for a destination and a source of size x size."""
    mh, mw = warp.mesh_shape((size, size), SHIFT)
    X, Y = np.meshgrid(np.arange(mw, dtype=np.int64) << SHIFT, np.arange(mh, dtype=np.int64) << SHIFT)
    centre = lambda c, r: np.stack([256 * c + 128, 256 * r + 128], axis=-1).astype(np.int32)
    dst_gt = (699960.0, 30.0, 0.0, 5000040.0, 0.0, -30.0)                    # the east side of zone 32, about 45 degrees N
    cx, cy = warp.utm_to_utm(dst_gt[0] + size * 15.0, dst_gt[3] - size * 15.0, 32632, 32633)
    src_gt = (float(np.round(cx / 30.0) * 30.0) - size * 15.0, 30.0, 0.0, float(np.round(cy / 30.0) * 30.0) + size * 15.0, 0.0, -30.0)
    utm, deviation = warp.utm_mesh(src_gt, 32633, dst_gt, 32632, (size, size), SHIFT)
    return {'identity': centre(X, Y), 'shift': centre(X + 100, Y - 50), 'utm_32_to_33': utm, 'quarter_turn': centre(size - 1 - Y, X),
            'garbage': rng.integers(-(1 << 31), 1 << 31, size=(mh, mw, 2), dtype=np.int64).astype(np.int32)}, deviation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=32)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'warp_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    n, T = batch.n_pixels, a.tiles
    meshes, deviation = meshes_for(a.size, np.random.default_rng(5))
    dev_mesh = {}
    for k, m in meshes.items():
        dev_mesh[k] = ctx.malloc(m.nbytes)
        dev_mesh[k].upload(m.view(np.uint8).reshape(-1))
    dst = ctx.malloc(4 * T * n)                       # room for the uint32 plane of (b)
    index = ctx.malloc(4 * T * n)
    head = ctx.malloc(64 * T)
    canvas = ctx.malloc(n)
    place = ctx.malloc(8 * T)
    place.upload(np.zeros(8 * T, dtype=np.uint8))
    wtr, nir = _capi.PLANE_INDEX['wtr'], _capi.PLANE_INDEX['nir']
    mspec = _capi.MosaicSpec.of(wtr_mosaic_spec())
    specs = {eb: _capi.WarpSpec.of(warp.Spec(eb, SHIFT, 255)) for eb in (1, 2, 4)}
    only_dst, every = _capi.WarpOut.of(dst=dst.ptr), _capi.WarpOut.of(dst=dst.ptr, src_index=index.ptr, head=head.ptr)

    def batch_warp(plane, eb, mesh, out, nt=T):
        _capi._check(ctx.lib.dswx_batch_warp(batch.handle, plane, ctypes.byref(specs[eb]), 0, nt, ctypes.c_void_p(dev_mesh[mesh].ptr),
                                             a.size, a.size, ctypes.byref(out), None))

    def warp_u32():
        _capi._check(ctx.lib.dswx_warp_device(ctx.handle, ctypes.c_void_p(index.ptr), ctypes.byref(specs[4]), T, a.size, a.size,
                                              ctypes.c_void_p(dev_mesh['utm_32_to_33'].ptr), a.size, a.size, ctypes.byref(only_dst), None))

    def mosaic():
        o = _capi.StackOut.of(last=canvas.ptr)
        _capi._check(ctx.lib.dswx_batch_mosaic(batch.handle, wtr, ctypes.byref(mspec), 0, T, ctypes.c_void_p(place.ptr), a.size, a.size,
                                               ctypes.byref(o), None))

    hist = np.zeros((1, T, 256), dtype=np.uint64)

    def histogram():
        _capi._check(ctx.lib.dswx_batch_histogram(batch.handle, 1 << wtr, 0, T, 0, 6, _capi._host_ptr(hist), None))

    batch.synth(SEED)
    batch.classify(_capi.default_params())
    ctx.synchronize()
    out = {'tool': 'tools/warp_rate.py', 'design': 'one workgroup = 4 rows x 1024 columns of the destination, one wave per row, one '
           'thread = 16 pixels; the four mesh nodes of a cell read through the caches, two 64-bit numerators advanced per pixel; a '
           'run of 16 consecutive source elements is one unaligned load, anything else 16 element loads',
           'resident_tiles': T, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride, 'reps': a.reps, 'shift': SHIFT,
           'hbm_peak_GBps': PEAK, 'rates_are': 'bytes of tiles read per second: n_tiles x pixels x elem_bytes',
           'content': 'synthetic batch, classified: class noise', 'utm_mesh_deviation_256ths': deviation}
    fns = {'mosaic_identity_last': mosaic, 'histogram_wtr': histogram}
    for k in meshes:
        fns[f'warp_u8_{k}_dst'] = lambda k=k: batch_warp(wtr, 1, k, only_dst)
        fns[f'warp_u8_{k}_all'] = lambda k=k: batch_warp(wtr, 1, k, every)
    fns['warp_i16_utm_32_to_33_dst'] = lambda: batch_warp(nir, 2, 'utm_32_to_33', only_dst)
    batch_warp(wtr, 1, 'utm_32_to_33', every)                 # src_index of the UTM mesh: the uint32 plane of (b)
    fns['warp_u32_utm_32_to_33_dst'] = warp_u32
    ms = timed_alternating(ctx, fns, a.reps)
    rec = {k: row(T * n * (2 if '_i16_' in k else 4 if '_u32_' in k else 1), v) for k, v in ms.items()}
    batch_warp(wtr, 1, 'identity', only_dst)
    rec['warp_u8_identity_dst']['kernel'] = ctx.last_kernel_info()
    ctx.synchronize()
    heads = {}
    for k in meshes:
        batch_warp(wtr, 1, k, every)
        ctx.synchronize()
        heads[k] = [int(v) for v in head.download(np.uint64, 8)]
    out['head_of_tile_0'] = heads
    ratio = rec['warp_u8_identity_dst']['ms_median'] / rec['mosaic_identity_last']['ms_median']
    out['rates'] = rec
    out['bar'] = {'statement': f'warp_u8_identity_dst ms_median <= {BAR} x mosaic_identity_last ms_median', 'ratio': round(ratio, 4),
                  'met': bool(ratio <= BAR)}
    # (d) what the entry replaces: download, one core, upload -- four tiles
    few = min(T, 4)
    spec = warp.Spec(1, SHIFT, 255)
    host = []
    for _ in range(2):
        t0 = time.perf_counter()
        tiles = np.stack([batch.read_tile('wtr', t).reshape(a.size, a.size) for t in range(few)])
        t1 = time.perf_counter()
        ref = _capi.warp_host(tiles, meshes['utm_32_to_33'], spec, (a.size, a.size), want=('dst',))['dst']
        t2 = time.perf_counter()
        dst.upload(ref.reshape(-1))
        host.append([round((t1 - t0) * 1e3, 2), round((t2 - t1) * 1e3, 2), round((time.perf_counter() - t2) * 1e3, 2)])
    batch_warp(wtr, 1, 'utm_32_to_33', only_dst, nt=few)
    ctx.synchronize()
    same = bool(np.array_equal(dst.download(np.uint8, few * n), ref.reshape(-1)))
    ms_few = timed_alternating(ctx, {'warp': lambda: batch_warp(wtr, 1, 'utm_32_to_33', only_dst, nt=few)}, a.reps)['warp']
    out['d_replaced'] = {'tiles': few, 'download_host_upload_ms': host, 'warp_dst': row(few * n, ms_few), 'device_dst_equals_host_dst': same,
                         'speedup_over_download_host_upload': round(min(sum(h) for h in host) / ms_few[len(ms_few) // 2], 1)}
    for b in list(dev_mesh.values()) + [dst, index, head, canvas, place]:
        b.free()
    batch.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
