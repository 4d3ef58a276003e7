#!/usr/bin/env python3
"""Rate of the stack kernel (dswx_stack.hip) against the histogram kernel, which reads exactly the same bytes, in one process,
with HIP events on the library's stream.  On the WTR plane of a resident batch of 3660 x 3660 tiles, over its first 8, 64 and
256 tiles (the addresses a batch of that many tiles would have), for two contents --

  synthetic   the generated batch, classified: per-pixel class noise;
  scene       the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified: classes in
              patches, long runs of one byte -- what a real product looks like

-- dswx_batch_stack with every output (two counts, last, last_index, share) and with `share` alone, into planes allocated
once, and dswx_batch_histogram of the same plane and tiles, the calls alternating round by round.  Rates are in bytes READ
per second (n_tiles x pixels); what the stack kernel writes on top is (2 n_cats + 4) / n_tiles of that with every output.
Recorded, not gated: DESIGN.md section 5 owes an explanation where the ratio at 256 tiles is below 0.8.

    python tools/stack_rate.py [--tiles 256] [--reps 10] [--out profiles/stack_rate.json]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi            # noqa: E402
from proteus_amd.stack import wtr_spec   # noqa: E402
from proteus_amd.synth import SEED       # noqa: E402

from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

EXPLAIN_BELOW = 0.8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--counts', type=int, nargs='*', default=[8, 64, 256], help='tile counts to measure (at most --tiles)')
    ap.add_argument('--out', default=os.path.join('profiles', 'stack_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    n = batch.n_pixels
    spec = wtr_spec()
    cspec = _capi.StackSpec.of(spec)
    planes = ctx.malloc(8 * n)                           # count0, count1, last_index (uint16), last, share (uint8)
    every = _capi.StackOut.of(count=[planes.ptr, planes.ptr + 2 * n], last_index=planes.ptr + 4 * n, last=planes.ptr + 6 * n,
                              share=planes.ptr + 7 * n)
    share = _capi.StackOut.of(share=planes.ptr + 7 * n)
    wtr = _capi.PLANE_INDEX['wtr']
    out = {'tool': 'tools/stack_rate.py', 'design': 'one thread = 16 pixels, 8 tiles in flight, 8 lane-indexed replicas of a '
           '256 x uint64 increment table in LDS', 'resident_tiles': a.tiles, 'tile': [a.size, a.size],
           'tile_stride': batch.tile_stride, 'reps': a.reps, 'hbm_peak_GBps': PEAK, 'explanation_owed_below': EXPLAIN_BELOW,
           'rates_are': 'bytes read per second: n_tiles x pixels', 'contents': {}}

    def stack(o, nt):
        _capi._check(ctx.lib.dswx_batch_stack(batch.handle, wtr, ctypes.byref(cspec), 0, nt, ctypes.byref(o), None))

    def measure(content):
        rec = {}
        for nt in [c for c in a.counts if c <= a.tiles]:
            ms = timed_alternating(ctx, {'histogram': lambda: batch.histogram(names=['wtr'], n_tiles=nt),
                                         'stack_all': lambda: stack(every, nt), 'stack_share': lambda: stack(share, nt)}, a.reps)
            read = nt * n
            h = row(read, ms['histogram'])
            stack(every, nt)
            s_all = row(read, ms['stack_all'], kernel=ctx.last_kernel_info(), bytes_written=8 * n,
                        written_over_read=round(8 / nt, 4))
            stack(share, nt)
            s_share = row(read, ms['stack_share'], kernel=ctx.last_kernel_info(), bytes_written=n, written_over_read=round(1 / nt, 4))
            rec[f'{nt}_tiles'] = {'batch_histogram': h, 'batch_stack_all_outputs': s_all, 'batch_stack_share_alone': s_share,
                                  'ratio_stack_all_over_histogram': round(s_all['GBps_median'] / h['GBps_median'], 4),
                                  'ratio_stack_share_over_histogram': round(s_share['GBps_median'] / h['GBps_median'], 4)}
        ctx.synchronize()
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
