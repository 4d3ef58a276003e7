#!/usr/bin/env python3
"""Rate of the mosaic kernel (dswx_mosaic.hip), in one process, with HIP events on the library's stream, on the WTR plane of a
resident batch of 3660 x 3660 tiles (generated and classified: per-pixel class noise):

  (a) identity   every tile at (0, 0) on a canvas of the tile's size, beside dswx_batch_stack on the same bytes, the calls
                 alternating round by round, with `share` alone and with every output.  The mosaic does the same loads and
                 the same arithmetic per byte; the difference is the cost of the cull and of the coverage tests.
  (b) block      the tiles as 2 x 2 neighbours x (tiles / 4) dates, 326 pixels of overlap: a canvas of 6994 x 6994.
  (c) one date   the first four tiles as one 2 x 2 block, against what the call replaces: the download of the four planes
                 and the numpy paste (proteus_amd.mosaic.mosaic_tiles) on one core, wall clock.

Rates are in bytes of tiles READ per second (n_tiles x pixels; every tile byte is covered in all three).  Recorded, not gated:
DESIGN.md section 5 owes an explanation where the mosaic of (a) is slower than the stack's slowest run by more than the stack's
own min - max spread.

    python tools/mosaic_rate.py [--tiles 256] [--reps 20] [--out profiles/mosaic_rate.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi                                  # noqa: E402
from proteus_amd.mosaic import mosaic_tiles, wtr_mosaic_spec   # noqa: E402
from proteus_amd.stack import wtr_spec                         # noqa: E402
from proteus_amd.synth import SEED                             # noqa: E402

from histogram_rate import PEAK, row, timed_alternating        # noqa: E402  (the same timing loop and row format)

OVERLAP = 326


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256, help='resident tiles, a multiple of 4')
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'mosaic_rate.json'))
    a = ap.parse_args()
    if a.tiles % 4 or a.tiles < 4:
        ap.error('--tiles must be a positive multiple of 4')
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    n, T = batch.n_pixels, a.tiles
    step = a.size - OVERLAP
    side = a.size + step
    m = side * side
    sspec, mspec = _capi.StackSpec.of(wtr_spec()), _capi.MosaicSpec.of(wtr_mosaic_spec())
    planes = ctx.malloc(8 * m)                           # count0, count1, last_index (uint16), last, share (uint8)

    def outs(k):
        return (_capi.StackOut.of(count=[planes.ptr, planes.ptr + 2 * k], last_index=planes.ptr + 4 * k, last=planes.ptr + 6 * k,
                                  share=planes.ptr + 7 * k), _capi.StackOut.of(share=planes.ptr + 7 * k))
    corner = [(0, 0), (0, step), (step, 0), (step, step)]
    tables = {'identity': np.zeros((T, 2), dtype=np.int32), 'block': np.array([corner[t % 4] for t in range(T)], dtype=np.int32)}
    place = {}
    for k, tab in tables.items():
        place[k] = ctx.malloc(tab.nbytes)
        place[k].upload(tab.view(np.uint8).reshape(-1))
    wtr = _capi.PLANE_INDEX['wtr']

    def stack(o):
        _capi._check(ctx.lib.dswx_batch_stack(batch.handle, wtr, ctypes.byref(sspec), 0, T, ctypes.byref(o), None))

    def mosaic(o, table, nt, h, w):
        _capi._check(ctx.lib.dswx_batch_mosaic(batch.handle, wtr, ctypes.byref(mspec), 0, nt, ctypes.c_void_p(place[table].ptr), h, w,
                                               ctypes.byref(o), None))

    batch.synth(SEED)
    batch.classify(_capi.default_params())
    ctx.synchronize()
    out = {'tool': 'tools/mosaic_rate.py', 'design': 'one workgroup = 4 rows x 1024 columns of the canvas, one wave per row, one thread '
           '= 16 pixels; placements culled 256 at a time into a list of 512 in LDS; 8 loads in flight; the stack kernel\'s table',
           'resident_tiles': T, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride, 'reps': a.reps, 'hbm_peak_GBps': PEAK,
           'rates_are': 'bytes of tiles read per second: n_tiles x pixels', 'content': 'synthetic batch, classified: class noise'}
    # (a) identity placement beside the stack
    every, share = outs(n)
    ms = timed_alternating(ctx, {'stack_all': lambda: stack(every), 'mosaic_all': lambda: mosaic(every, 'identity', T, a.size, a.size),
                                 'stack_share': lambda: stack(share), 'mosaic_share': lambda: mosaic(share, 'identity', T, a.size, a.size)}, a.reps)
    mosaic(every, 'identity', T, a.size, a.size)
    rec = {k: row(T * n, v) for k, v in ms.items()}
    rec['mosaic_all']['kernel'] = ctx.last_kernel_info()
    for kind in ('all', 'share'):
        s, q = rec[f'stack_{kind}'], rec[f'mosaic_{kind}']
        rec[f'ratio_mosaic_{kind}_over_stack_median_ms'] = round(q['ms_median'] / s['ms_median'], 4)
        rec[f'explanation_owed_{kind}'] = bool(q['ms_median'] - s['ms_max'] > s['ms_max'] - s['ms_min'])
    out['a_identity'] = rec
    # (b) 2 x 2 neighbours x T / 4 dates
    every, share = outs(m)
    ms = timed_alternating(ctx, {'mosaic_all': lambda: mosaic(every, 'block', T, side, side),
                                 'mosaic_share': lambda: mosaic(share, 'block', T, side, side)}, a.reps)
    out['b_block'] = dict({k: row(T * n, v, bytes_written=(8 if k == 'mosaic_all' else 1) * m) for k, v in ms.items()},
                          canvas=[side, side], dates=T // 4, overlap=OVERLAP)
    # (c) one date of 2 x 2 neighbours against download + numpy paste
    ms = timed_alternating(ctx, {'mosaic_all': lambda: mosaic(every, 'block', 4, side, side)}, a.reps)
    ctx.synchronize()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        tiles = np.stack([batch.read_tile('wtr', t).reshape(a.size, a.size) for t in range(4)])
        t1 = time.perf_counter()
        ref = mosaic_tiles(tiles, tables['block'][:4], (side, side), wtr_mosaic_spec())
        host.append((round((t1 - t0) * 1e3, 2), round((time.perf_counter() - t1) * 1e3, 2)))
    got_last = planes.download(np.uint8, m, 6 * m).reshape(side, side)
    out['c_one_date'] = {'mosaic_all': row(4 * n, ms['mosaic_all']), 'download_four_planes_ms': [h[0] for h in host],
                         'numpy_paste_one_core_ms': [h[1] for h in host], 'device_last_equals_numpy_last': bool(np.array_equal(got_last, ref['last'])),
                         'speedup_over_download_plus_paste': round(min(h[0] + h[1] for h in host) / ms['mosaic_all'][len(ms['mosaic_all']) // 2], 1)}
    for b in place.values():
        b.free()
    planes.free()
    batch.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
