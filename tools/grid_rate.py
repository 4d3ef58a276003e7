#!/usr/bin/env python3
"""Rate of the grid kernel (dswx_grid.hip) against the histogram kernel, which reads exactly the same bytes, in one process,
with HIP events on the library's stream.  On the WTR plane of the resident batch of 256 tiles of 3660 x 3660, for two
contents --

  synthetic   the generated batch, classified: per-pixel class noise;
  scene       the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified: classes in
              patches, long runs of one byte -- what a real product looks like

-- dswx_batch_grid at square cells of 3, 30, 128 and 3660 pixels, once with `share` alone and once with every output (two
counts, share, coverage, major), into planes allocated once per cell size, and dswx_batch_histogram of the same plane, the
calls alternating round by round.  The histogram is timed as its C entry is: the records zeroed on the stream, the kernel, and
the download of 2 KiB per tile into a host array allocated once -- what a caller of the parent's read-only entry pays; the
kernel alone is some per cent shorter (a kernel trace has both).  Rates are in bytes READ per second (n_tiles x pixels); what
the grid kernel writes on top is (4 n_cats + 3) / cell^2 of that with every output.  The bar, for cells 30 and 128 with `share` alone: the median rate is
not below the histogram's median rate by more than the histogram's own min-to-max spread in this file; cells 3 (the output is
as large as the input) and 3660 (one workgroup per tile) are recorded, not judged.  Every sample is kept.

    python tools/grid_rate.py [--tiles 256] [--reps 10] [--out profiles/grid_rate.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi                      # noqa: E402
from proteus_amd.grid import grid_shape, wtr_grid_spec   # noqa: E402
from proteus_amd.synth import SEED                 # noqa: E402

from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

JUDGED = (30, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cells', type=int, nargs='*', default=[3, 30, 128, 3660], help='cell sizes to measure')
    ap.add_argument('--out', default=os.path.join('profiles', 'grid_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    read = a.tiles * batch.n_pixels
    wtr = _capi.PLANE_INDEX['wtr']
    records = np.zeros((a.tiles, _capi.HIST_BINS), dtype=np.uint64)

    def histogram():
        _capi._check(ctx.lib.dswx_batch_histogram(batch.handle, 1 << wtr, 0, a.tiles, 0, 6, _capi._host_ptr(records), None))

    out = {'tool': 'tools/grid_rate.py', 'design': 'one workgroup = a rectangle of whole cells counted in LDS; one thread = a unit of '
           '16 columns walked down the rows, 4 loads in flight, packed 8-bit counts widened every 15 rows; 8 lane-indexed replicas '
           'of a 256 x uint32 increment table in LDS', 'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride,
           'reps': a.reps, 'hbm_peak_GBps': PEAK, 'rates_are': 'bytes read per second: n_tiles x pixels; the histogram is the whole C entry (memset of the records, kernel, '
           'download of 2 KiB per tile), the grid entry is its one launch',
           'bar': 'cells 30 and 128, share alone: GBps_median >= histogram GBps_median - (histogram GBps at ms_min - GBps at ms_max)',
           'contents': {}}

    def measure(content):
        rec = {}
        for cell in a.cells:
            spec = wtr_grid_spec(cell)
            cspec = _capi.GridSpec.of(spec)
            gh, gw = grid_shape(a.size, a.size, spec)
            cells = a.tiles * gh * gw
            planes = ctx.malloc(11 * cells + 16)             # count0, count1 (uint32), share, coverage, major (uint8)
            every = _capi.GridOut.of(count=[planes.ptr, planes.ptr + 4 * cells], share=planes.ptr + 8 * cells,
                                     coverage=planes.ptr + 9 * cells, major=planes.ptr + 10 * cells)
            share = _capi.GridOut.of(share=planes.ptr + 8 * cells)

            def grid(o):
                _capi._check(ctx.lib.dswx_batch_grid(batch.handle, wtr, ctypes.byref(cspec), 0, a.tiles, ctypes.byref(o), None))

            ms = timed_alternating(ctx, {'histogram': histogram, 'grid_all': lambda: grid(every),
                                         'grid_share': lambda: grid(share)}, a.reps)
            h = row(read, ms['histogram'], ms_samples=[round(v, 4) for v in ms['histogram']])
            grid(every)
            g_all = row(read, ms['grid_all'], kernel=ctx.last_kernel_info(), bytes_written=11 * cells,
                        written_over_read=round(11 * cells / read, 5), ms_samples=[round(v, 4) for v in ms['grid_all']])
            grid(share)
            g_share = row(read, ms['grid_share'], kernel=ctx.last_kernel_info(), bytes_written=cells,
                          written_over_read=round(cells / read, 5), ms_samples=[round(v, 4) for v in ms['grid_share']])
            ctx.synchronize()
            spread = read / h['ms_min'] / 1e6 - read / h['ms_max'] / 1e6
            r = {'batch_histogram': h, 'batch_grid_all_outputs': g_all, 'batch_grid_share_alone': g_share,
                 'histogram_spread_GBps': round(spread, 1),
                 'ratio_grid_all_over_histogram': round(g_all['GBps_median'] / h['GBps_median'], 4),
                 'ratio_grid_share_over_histogram': round(g_share['GBps_median'] / h['GBps_median'], 4)}
            if cell in JUDGED:
                r['bar_met'] = bool(g_share['GBps_median'] >= h['GBps_median'] - spread)
            rec[f'cell_{cell}'] = r
            planes.free()
        hist = batch.histogram(names=['wtr'], n_tiles=1)['wtr'][0]
        rec['wtr_tile_0_bins'] = {int(b): int(hist[b]) for b in hist.nonzero()[0]}
        out['contents'][content] = rec

    batch.synth(SEED)
    batch.classify(p)
    ctx.synchronize()
    measure('synthetic')
    fill_scene(ctx, batch, a.size)
    batch.classify(p)
    ctx.synchronize()
    measure('scene')
    batch.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
