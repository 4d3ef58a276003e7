#!/usr/bin/env python3
"""Time of the distance transform (dswx_distance.hip) per tile, in one process, with HIP events on the library's stream.  On the
WTR plane of the resident batch of 256 tiles of 3660 x 3660, transformed in tile ranges whose uint32 planes fit, for six
contents --

  synthetic    (a) the generated batch, classified: per-pixel class noise, water everywhere a few pixels away;
  scene        (b) the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified;
  all_target   (c) every pixel open water: every distance 0;
  one_corner   (d) ONE water pixel, in the first corner of each tile: every search is as long as it can be;
  no_target    (e) no water at all: nothing is reached;
  one_column   (f) one full column of water: the column pass finds a target in one column only

-- dswx_batch_distance with dist2 alone and with every output, unbounded (R = 0: dist2, nearest, summary) and within 17 pixels
(R = 17, 500 m at 30 m: dist2, nearest, within, summary), against three yardsticks measured alongside: dswx_batch_histogram
of the same bytes (one read pass: the traffic floor of 13 bytes per pixel for dist2 alone is stated at ITS rate), dswx_batch_label
with all four outputs on the same planes, and what the entry replaces: the download of one tile plus
scipy.ndimage.distance_transform_edt of it on one host core, for (a), (b) and (d).  Nobody had measured this and no rate can
be derived -- the search depends on the data -- so nothing is judged against a rate; the condition is that the entry per tile
beats download + scipy on every content.  Every sample is kept.  Per-launch times come from a separate run under a kernel
trace (--once, then --trace-csv merges the trace's dispatches with the budget of DESIGN.md section 5).

    python tools/distance_rate.py [--tiles 256] [--range 32] [--reps 20] [--out profiles/distance_rate.json] [--trace-csv FILE]
"""
import argparse
import csv
import ctypes
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi                          # noqa: E402
from proteus_amd.distance import wtr_distance_spec     # noqa: E402
from proteus_amd.label import wtr_label_spec           # noqa: E402
from proteus_amd.synth import SEED                     # noqa: E402

from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

# bytes per pixel that each launch streams for dist2 alone (nearest adds 4 written, within 1 read and 1
# written in the row launch); the band launch writes one word per 64 rows, the column launch reads those of the other bands
BUDGET = {'dswx_distance_column_k<false>': 1.0,     # plane 1 read
          'dswx_distance_column_k<true>': 5.0,      # plane 1 read again; the entry 4 written
          'dswx_distance_row_k': 8.0}               # the entry 4 read, dist2 4 written
FLOOR_BYTES_PER_PIXEL = 13.0                        # 1 read + 4 written + 4 read + 4 written: the band launch is on top of it
CONTENTS = ('synthetic', 'scene', 'all_target', 'one_corner', 'no_target', 'one_column')
RADIUS = 17


def merge_trace(out, trace_csv):
    """The dispatches of the traced run (--once) in time order -- six contents, one pass each, the same launches in each -- as
    time per tile and launch, with the budget's bytes per pixel and the rate that follows."""
    tiles, px = out['tiles'], out['tile'][0] * out['tile'][1]
    with open(trace_csv) as f:
        rows = sorted((r for r in csv.DictReader(f) if 'dswx_distance_' in r['Kernel_Name']), key=lambda r: int(r['Start_Timestamp']))
    share = len(rows) // len(CONTENTS)
    for i, content in enumerate(CONTENTS):
        per = {}
        for name, bpp in BUDGET.items():
            ns = [int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in rows[i * share:(i + 1) * share] if name in r['Kernel_Name']]
            if ns:
                per[name] = {'launches': len(ns), 'us_per_tile': round(sum(ns) / 1e3 / tiles, 2), 'budget_bytes_per_pixel': bpp,
                             'GBps_of_budget': round(bpp * px * tiles / sum(ns), 1)}
        out['contents'][content]['per_launch_from_kernel_trace_all_outputs_R0'] = per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--range', dest='span', type=int, default=32, help='tiles per call: the uint32 planes of a range must fit')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--once', action='store_true', help='one pass per content and nothing timed: the run to put under a kernel trace')
    ap.add_argument('--trace-csv', default=None, help='the kernel trace of such a run (Kernel_Name, Start_Timestamp, End_Timestamp): merged into --out, no device needed')
    ap.add_argument('--out', default=os.path.join('profiles', 'distance_rate.json'))
    a = ap.parse_args()
    if a.trace_csv:                                  # no device: the file of an earlier run and the trace of a --once run
        with open(a.out) as f:
            out = json.load(f)
        merge_trace(out, a.trace_csv)
        with open(a.out, 'w') as f:
            f.write(json.dumps(out, indent=1) + '\n')
        return
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    px = batch.n_pixels
    read = a.tiles * px
    wtr = _capi.PLANE_INDEX['wtr']
    records = np.zeros((a.tiles, _capi.HIST_BINS), dtype=np.uint64)
    specs = {0: wtr_distance_spec(), RADIUS: wtr_distance_spec(radius=RADIUS)}
    cspecs = {r: _capi.DistanceSpec.of(s) for r, s in specs.items()}
    lspec = _capi.LabelSpec.of(wtr_label_spec(4))
    span = min(a.span, a.tiles)
    planes = ctx.malloc(span * (9 * px + 8 * 40) + 64)
    summary = planes.ptr
    first = summary + span * 8 * 40
    second = first + 4 * span * px
    third = second + 4 * span * px
    outs = {'R0_dist2_alone': (0, _capi.DistanceOut.of(dist2=first)),
            'R0_all_outputs': (0, _capi.DistanceOut.of(dist2=first, nearest=second, summary=summary)),
            f'R{RADIUS}_dist2_alone': (RADIUS, _capi.DistanceOut.of(dist2=first)),
            f'R{RADIUS}_all_outputs': (RADIUS, _capi.DistanceOut.of(dist2=first, nearest=second, within=third, summary=summary))}
    label_out = _capi.LabelOut.of(label=first, size=second, sieved=third, summary=summary)

    def histogram():
        _capi._check(ctx.lib.dswx_batch_histogram(batch.handle, 1 << wtr, 0, a.tiles, 0, 6, _capi._host_ptr(records), None))

    def label():
        for t0 in range(0, a.tiles, span):
            _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(lspec), t0, min(span, a.tiles - t0), ctypes.byref(label_out), None))

    def distance(key):
        r, o = outs[key]
        for t0 in range(0, a.tiles, span):
            _capi._check(ctx.lib.dswx_batch_distance(batch.handle, wtr, ctypes.byref(cspecs[r]), t0, min(span, a.tiles - t0), ctypes.byref(o), None))

    out = {'tool': 'tools/distance_rate.py', 'date': datetime.date.today().isoformat(),
           'design': 'separable exact transform: bands of 64 rows x 4 columns a thread note their targets, then write the vertical '
           'offset to the nearest target of the column with the carry read from the notes; one workgroup a row keeps the offsets in '
           'LDS, every lane looks 32 columns to either side and then walks blocks of 64 columns pruned by their minimum; four '
           'launches and one memset per call, no workgroup waits for another',
           'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride, 'tiles_per_call': span, 'reps': a.reps,
           'radius': RADIUS, 'hbm_peak_GBps': PEAK, 'floor_bytes_per_pixel_dist2_alone': FLOOR_BYTES_PER_PIXEL,
           'times_are': 'stream events around one pass over all tiles (tiles / tiles_per_call calls); per tile = / tiles',
           'budget_bytes_per_pixel': BUDGET, 'contents': {}}

    def measure(content, host_yardstick):
        if a.once:
            distance('R0_all_outputs')
            ctx.synchronize()
            return
        fns = {'histogram': histogram, 'label_all': label}
        fns.update({k: (lambda k=k: distance(k)) for k in outs})
        ms = timed_alternating(ctx, fns, a.reps)
        distance('R0_all_outputs')
        info = ctx.last_kernel_info()
        ctx.synchronize()
        words = planes.download(np.uint64, 40)                        # the first tile of the last range
        rec = {'batch_histogram': row(read, ms['histogram'], ms_samples=[round(v, 4) for v in ms['histogram']]),
               'batch_label_all_outputs': row(read, ms['label_all'], ms_samples=[round(v, 4) for v in ms['label_all']]),
               'summary_of_one_tile_R0': {'targets': int(words[0]), 'reached': int(words[1]), 'not_reached': int(words[2]),
                                          'largest_dist2': int(words[3]), 'sum_dist2': int(words[5])}}
        hist = rec['batch_histogram']['ms_median']
        floor_ms = FLOOR_BYTES_PER_PIXEL * hist                        # the histogram streams 1 byte per pixel
        rec['floor_ms_per_tile_at_the_histogram_rate'] = round(floor_ms / a.tiles, 5)
        for k in outs:
            r = rec['batch_distance_' + k] = row(read, ms[k], kernel=info if k == 'R0_all_outputs' else None, ms_samples=[round(v, 4) for v in ms[k]])
            r['ms_per_tile_median'], r['ms_per_tile_min'], r['ms_per_tile_max'] = (round(r[q] / a.tiles, 5) for q in ('ms_median', 'ms_min', 'ms_max'))
            r['multiple_of_histogram'] = round(r['ms_median'] / hist, 2)
            r['multiple_of_label_all_outputs'] = round(r['ms_median'] / rec['batch_label_all_outputs']['ms_median'], 2)
            if k.endswith('dist2_alone'):
                r['fraction_of_the_floor'] = round(floor_ms / r['ms_median'], 3)
        if host_yardstick:
            # what the entry replaces: one tile over PCIe, scipy.ndimage.distance_transform_edt on one core
            t0 = time.perf_counter()
            tile = batch.read_tile('wtr', 0)
            t_down = time.perf_counter() - t0
            try:
                from scipy import ndimage
                t0 = time.perf_counter()
                edt = ndimage.distance_transform_edt(specs[0].target_of_byte[tile] == 0)
                t_scipy = time.perf_counter() - t0
                rec['host_yardstick'] = {'download_one_tile_ms': round(t_down * 1e3, 3), 'scipy_distance_transform_edt_ms': round(t_scipy * 1e3, 3),
                                         'largest_distance': float(edt.max())}
                for k in ('R0_all_outputs', f'R{RADIUS}_all_outputs'):
                    rec[f'{k}_beats_download_plus_scipy_by'] = round((t_down + t_scipy) * 1e3 / rec['batch_distance_' + k]['ms_per_tile_median'], 1)
            except ImportError:
                rec['host_yardstick'] = {'download_one_tile_ms': round(t_down * 1e3, 3), 'scipy': 'not installed'}
        out['contents'][content] = rec
        print(content, {k: rec['batch_distance_' + k]['ms_per_tile_median'] for k in outs}, flush=True)

    ptr, _ = batch._plane('wtr')
    stride = batch.tile_stride

    def fill(byte):
        _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ptr, byte, a.tiles * stride))

    batch.synth(SEED)
    batch.classify(p)
    ctx.synchronize()
    measure('synthetic', True)
    fill_scene(ctx, batch, a.size)
    batch.classify(p)
    ctx.synchronize()
    measure('scene', True)
    fill(1)
    ctx.synchronize()
    measure('all_target', False)
    fill(0)
    for t in range(a.tiles):
        _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ptr + t * stride, 1, 1))
    ctx.synchronize()
    measure('one_corner', True)
    fill(0)
    ctx.synchronize()
    measure('no_target', False)
    column = np.zeros((a.size, a.size), dtype=np.uint8)
    column[:, a.size // 3] = 1
    _capi._check(ctx.lib.dswx_memcpy_h2d(ctx.handle, ptr, _capi._host_ptr(column), column.size))
    for t in range(1, a.tiles):
        ctx.copy_2d_device(ptr + t * stride, stride, ptr, stride, px, 1)
    ctx.synchronize()
    measure('one_column', False)
    planes.free()
    batch.free()
    ctx.close()
    if a.once:
        return
    c = out['contents']
    med = lambda name, k='R0_all_outputs': c[name]['batch_distance_' + k]['ms_per_tile_median']
    out['ratios_R0_all_outputs'] = {'one_corner_to_scene': round(med('one_corner') / med('scene'), 2),
                                    'no_target_to_scene': round(med('no_target') / med('scene'), 2),
                                    'synthetic_to_scene': round(med('synthetic') / med('scene'), 2)}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(json.dumps(out['ratios_R0_all_outputs']))


if __name__ == '__main__':
    main()
