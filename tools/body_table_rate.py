#!/usr/bin/env python3
"""Time of the body table (dswx_body_table.hip) per tile, in one process, with HIP events on the library's stream.  On the WTR
plane of the resident batch of 256 tiles of 3660 x 3660 in ranges of 32 tiles, for the three contents of tools/label_rate.py --

  synthetic    the generated batch, classified: per-pixel class noise, hundreds of thousands of bodies per tile;
  scene        the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified: water in patches;
  all_member   every pixel open water: ONE body per tile, every atomic of a tile on one row

-- the label plane of EVERY tile is made once by dswx_batch_label and stays in HBM; dswx_batch_body_table then runs over it with
WTR itself as the value plane (open and partial water counted), with all three outputs and with dense alone, next to the label
chain that produced its input (all four outputs, and label alone), timed alternately.  Nobody has measured a data-dependent
scatter like this on this part and no rate can be derived, so nothing is judged against a bandwidth.  Two conditions: the
call per tile beats what it replaces -- the download of the label and value planes of one tile plus scipy.ndimage.find_objects
+ sum + center_of_mass on one core -- on every content; and on the scene and on the all-member plane, where the atomics are
few once combined and the streamed budget is a fraction of the chain's, its median does not exceed the median of the label
chain (all four outputs) measured alongside.  Class noise is recorded only.  Every sample is kept.

    python tools/body_table_rate.py [--tiles 256] [--range 32] [--reps 20] [--out profiles/body_table_rate.json] [--once]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi                      # noqa: E402
from proteus_amd.bodies import Spec, wtr_body_spec  # noqa: E402
from proteus_amd.label import wtr_label_spec       # noqa: E402
from proteus_amd.synth import SEED                 # noqa: E402

from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

# bytes per pixel that each launch streams with all three outputs and a value plane
BUDGET = {'dswx_body_count_k': 4.0,       # label read
          'dswx_body_rank_k': 4.0,        # label read; dense written at the roots only
          'dswx_body_fill_k': 9.0}        # label 4 and value 1 read, dense 4 written; the rows above and below re-read from cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--range', dest='span', type=int, default=32, help='tiles per call')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--once', action='store_true', help='one pass per content and nothing timed: the run to put under a kernel trace')
    ap.add_argument('--out', default=os.path.join('profiles', 'body_table_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    px = batch.n_pixels
    read = a.tiles * px
    wtr = _capi.PLANE_INDEX['wtr']
    span = min(a.span, a.tiles)
    lspec = wtr_label_spec(1)
    clspec = _capi.LabelSpec.of(lspec)
    SW = _capi.LABEL_SUMMARY_WORDS
    labels = ctx.malloc(4 * a.tiles * px)                                  # the label plane of every tile
    summaries = ctx.malloc(8 * SW * a.tiles)
    scratch = ctx.malloc(span * 9 * px + 64)                               # dense of a range; or size + sieved + label of a range
    chain_label = ctx.malloc(4 * span * px)
    head = ctx.malloc(8 * _capi.BODY_HEAD_WORDS * span)

    def label_every_tile():
        for t0 in range(0, a.tiles, span):
            n = min(span, a.tiles - t0)
            o = _capi.LabelOut.of(label=labels.ptr + 4 * t0 * px, size=scratch.ptr, summary=summaries.ptr + 8 * SW * t0)
            _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(clspec), t0, n, ctypes.byref(o), None))

    every = _capi.LabelOut.of(label=chain_label.ptr, size=scratch.ptr, sieved=scratch.ptr + 4 * span * px, summary=summaries.ptr)
    alone = _capi.LabelOut.of(label=chain_label.ptr)

    def chain(o):
        for t0 in range(0, a.tiles, span):
            _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(clspec), t0, min(span, a.tiles - t0), ctypes.byref(o), None))

    def table(cspec, o, value):
        for t0 in range(0, a.tiles, span):
            _capi._check(ctx.lib.dswx_batch_body_table(batch.handle, value, ctypes.byref(cspec), t0, min(span, a.tiles - t0),
                                                       ctypes.c_void_p(labels.ptr + 4 * t0 * px), ctypes.byref(o), None))

    out = {'tool': 'tools/body_table_rate.py', 'design': 'count the roots per chunk of 4096 into dense, scan the counts per tile, rank the '
           'roots and begin their rows, then tabulate: runs per thread, equal bodies combined across the wave by leader peeling, one '
           'set of atomics per combined contribution; four launches and two memsets per call, no workgroup waits for another',
           'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride, 'tiles_per_call': span, 'reps': a.reps,
           'connectivity': lspec.connectivity, 'value_plane': 'wtr (open water category 0, partial surface water category 1)',
           'hbm_peak_GBps': PEAK, 'times_are': 'stream events around one pass over all tiles (tiles / tiles_per_call calls); per tile = / tiles',
           'budget_bytes_per_pixel': BUDGET, 'bar': 'scene and all_member: median of the body table (all outputs) <= median of the label '
           'chain (all four outputs) measured alongside; synthetic: recorded only; every content: beats download + scipy',
           'contents': {}}

    def measure(content, judged):
        label_every_tile()
        ctx.synchronize()
        K = int(summaries.download(np.uint64, SW * a.tiles).reshape(a.tiles, SW)[:, 0].max())
        spec = wtr_body_spec(K)
        rows = ctx.malloc(max(64 * K * span, 64))
        cspec, cbare = _capi.BodySpec.of(spec), _capi.BodySpec.of(Spec(0, None, 0))
        o_all = _capi.BodyOut.of(dense=scratch.ptr, rows=rows.ptr if K else None, head=head.ptr)
        o_dense = _capi.BodyOut.of(dense=scratch.ptr)
        if a.once:
            table(cspec, o_all, wtr)
            ctx.synchronize()
            rows.free()
            return
        ms = timed_alternating(ctx, {'label_all': lambda: chain(every), 'label_alone': lambda: chain(alone),
                                     'table_all': lambda: table(cspec, o_all, wtr), 'table_dense': lambda: table(cbare, o_dense, -1)}, a.reps)
        table(cspec, o_all, wtr)
        info = ctx.last_kernel_info()
        ctx.synchronize()
        h = head.download(np.uint64, _capi.BODY_HEAD_WORDS)                  # tile tiles - span of the last pass
        rec = {'bodies_max_per_tile': K, 'head_of_one_tile': {'bodies': int(h[0]), 'rows': int(h[1]), 'member_pixels': int(h[2]),
                                                             'malformed': int(h[3]), 'perimeter': int(h[4])}}
        for k, name in (('label_all', 'batch_label_all_outputs'), ('label_alone', 'batch_label_label_alone'),
                        ('table_all', 'batch_body_table_all_outputs'), ('table_dense', 'batch_body_table_dense_alone')):
            r = row(read, ms[k], ms_samples=[round(v, 4) for v in ms[k]])
            r['ms_per_tile_median'], r['ms_per_tile_min'], r['ms_per_tile_max'] = (round(r[q] / a.tiles, 5) for q in ('ms_median', 'ms_min', 'ms_max'))
            rec[name] = r
        rec['batch_body_table_all_outputs']['kernel'] = info
        ratio = rec['batch_body_table_all_outputs']['ms_median'] / rec['batch_label_all_outputs']['ms_median']
        rec['table_over_label_chain'] = round(ratio, 3)
        rec['bar_table_not_above_label_chain'] = ('met' if ratio <= 1.0 else 'MISSED') if judged else 'recorded only'
        # what the entry replaces: the label and value planes of one tile over PCIe, then scipy on one core
        t0 = time.perf_counter()
        lab = labels.download(np.uint32, px).reshape(a.size, a.size)
        tile = batch.read_tile('wtr', 0)
        t_down = time.perf_counter() - t0
        try:
            from scipy import ndimage
            t0 = time.perf_counter()
            dense, k = ndimage.label(lab != 0, structure=np.ones((3, 3)))    # (the renumbering that the download would need)
            t_label = time.perf_counter() - t0
            t0 = time.perf_counter()
            index = np.arange(1, k + 1)
            boxes = ndimage.find_objects(dense)
            area = ndimage.sum(np.ones_like(tile), dense, index)
            open_water = ndimage.sum(tile == 1, dense, index)
            centre = ndimage.center_of_mass(np.ones_like(tile), dense, index)
            t_scipy = time.perf_counter() - t0
            rec['host_yardstick'] = {'download_label_and_value_of_one_tile_ms': round(t_down * 1e3, 3),
                                     'scipy_find_objects_sum_center_of_mass_ms': round(t_scipy * 1e3, 3),
                                     'scipy_label_for_the_renumbering_ms_not_counted': round(t_label * 1e3, 3), 'bodies': int(k),
                                     'checked': [len(boxes), int(np.sum(area)), int(np.sum(open_water)), len(centre)]}
            rec['table_beats_download_plus_scipy_by'] = round((t_down + t_scipy) * 1e3 / rec['batch_body_table_all_outputs']['ms_per_tile_median'], 1)
        except ImportError:
            rec['host_yardstick'] = {'download_label_and_value_of_one_tile_ms': round(t_down * 1e3, 3), 'scipy': 'not installed'}
        rows.free()
        out['contents'][content] = rec

    batch.synth(SEED)
    batch.classify(p)
    ctx.synchronize()
    measure('synthetic', False)
    fill_scene(ctx, batch, a.size)
    batch.classify(p)
    ctx.synchronize()
    measure('scene', True)
    ptr, _ = batch._plane('wtr')
    _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ptr, 1, a.tiles * batch.tile_stride))
    ctx.synchronize()
    measure('all_member', True)
    for b in (labels, summaries, scratch, chain_label, head):
        b.free()
    batch.free()
    ctx.close()
    if a.once:
        return
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
