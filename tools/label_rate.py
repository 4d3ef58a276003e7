#!/usr/bin/env python3
"""Time of the label chain (dswx_label.hip) per tile, in one process, with HIP events on the library's stream.  On the WTR plane
of the resident batch of 256 tiles of 3660 x 3660, labelled in tile ranges whose label and size planes fit, for three
contents --

  synthetic    the generated batch, classified: per-pixel class noise, many tiny bodies;
  scene        the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified: water in patches;
  all_member   every pixel open water: ONE body per tile, the worst contention on one root

-- dswx_batch_label with all four outputs (and once with label alone), connectivity 8, against two yardsticks: dswx_batch_
histogram of the same bytes (one read pass; the chain is reported as a multiple of it), and what the chain replaces: the
download of one tile plus scipy.ndimage.label + np.bincount of it on one host core.  Nobody had measured this and no rate can
be derived -- the root chase depends on the data -- so nothing is judged against a rate; the condition is that the chain per
tile beats download + scipy.  Every sample is kept.  Per-launch times come from a separate run under a kernel trace
(--trace-csv merges the trace's dispatches with the budget of DESIGN.md section 5: bytes per pixel of each launch).

    python tools/label_rate.py [--tiles 256] [--range 32] [--reps 20] [--out profiles/label_rate.json] [--trace-csv FILE]
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi                      # noqa: E402
from proteus_amd.label import wtr_label_spec       # noqa: E402
from proteus_amd.synth import SEED                 # noqa: E402

from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

# bytes per pixel that each launch streams with all four outputs (what the root chase and the atomics
# add on top depends on the data and is what the measurement shows)
BUDGET = {'dswx_label_local_k': 9.0,      # plane 1 read; label 4, size 4 written
          'dswx_label_seam_k': 0.625,     # (1/128 + 1/32) of the pixels are seam pixels, four labels of 4 bytes each
          'dswx_label_flatten_k': 8.0,    # label 4 read, 4 written
          'dswx_label_finish_k': 14.0}    # label 4, size of the root 4, plane 1 read; size 4, sieved 1 written


def merge_trace(out, trace_csv):
    """The dispatches of the traced run (--once) in time order -- three contents, one pass each, the same launches in each --
    as time per tile and launch, with the budget's bytes per pixel and the rate that follows."""
    tiles, px = out['tiles'], out['tile'][0] * out['tile'][1]
    with open(trace_csv) as f:
        rows = sorted((r for r in csv.DictReader(f) if 'dswx_label_' in r['Kernel_Name']), key=lambda r: int(r['Start_Timestamp']))
    third = len(rows) // 3
    for i, content in enumerate(('synthetic', 'scene', 'all_member')):
        per = {}
        for name, bpp in BUDGET.items():
            ns = [int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in rows[i * third:(i + 1) * third] if name in r['Kernel_Name']]
            if ns:
                per[name] = {'launches': len(ns), 'us_per_tile': round(sum(ns) / 1e3 / tiles, 2), 'budget_bytes_per_pixel': bpp,
                             'GBps_of_budget': round(bpp * px * tiles / sum(ns), 1)}
        out['contents'][content]['per_launch_from_kernel_trace'] = per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--range', dest='span', type=int, default=32, help='tiles per call: the label and size planes of a range must fit')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--min-size', type=int, default=4)
    ap.add_argument('--once', action='store_true', help='one pass per content and nothing timed: the run to put under a kernel trace')
    ap.add_argument('--trace-csv', default=None, help='the kernel trace of such a run (Kernel_Name, Start_Timestamp, End_Timestamp): merged into --out, no device needed')
    ap.add_argument('--out', default=os.path.join('profiles', 'label_rate.json'))
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
    spec = wtr_label_spec(a.min_size)
    cspec = _capi.LabelSpec.of(spec)
    span = min(a.span, a.tiles)
    planes = ctx.malloc(span * (9 * px + 8 * _capi.LABEL_SUMMARY_WORDS) + 64)
    summary = planes.ptr
    label = summary + span * 8 * _capi.LABEL_SUMMARY_WORDS
    size = label + 4 * span * px
    every = _capi.LabelOut.of(label=label, size=size, sieved=size + 4 * span * px, summary=summary)
    alone = _capi.LabelOut.of(label=label)

    def histogram():
        _capi._check(ctx.lib.dswx_batch_histogram(batch.handle, 1 << wtr, 0, a.tiles, 0, 6, _capi._host_ptr(records), None))

    def chain(o):
        for t0 in range(0, a.tiles, span):
            _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(cspec), t0, min(span, a.tiles - t0), ctypes.byref(o), None))

    out = {'tool': 'tools/label_rate.py', 'design': 'label-equivalence union-find: a 32 x 128 rectangle per workgroup in LDS, seams '
           'united on the global plane by atomicMin, flatten + count with roots combined per thread and per wave, finish = size '
           'broadcast + sieve + summary; five launches and one memset per call, no workgroup waits for another',
           'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride, 'tiles_per_call': span, 'reps': a.reps,
           'connectivity': spec.connectivity, 'min_size': spec.min_size, 'hbm_peak_GBps': PEAK,
           'times_are': 'stream events around one pass over all tiles (tiles / tiles_per_call calls); per tile = / tiles',
           'budget_bytes_per_pixel': BUDGET, 'contents': {}}

    def measure(content):
        if a.once:
            chain(every)
            ctx.synchronize()
            return
        ms = timed_alternating(ctx, {'histogram': histogram, 'label_all': lambda: chain(every), 'label_alone': lambda: chain(alone)}, a.reps)
        chain(every)
        info = ctx.last_kernel_info()
        ctx.synchronize()
        words = planes.download(np.uint64, _capi.LABEL_SUMMARY_WORDS)        # tile tiles - span of the last pass
        # what the chain replaces: one tile over PCIe, scipy.ndimage.label + np.bincount on one core
        t0 = time.perf_counter()
        tile = batch.read_tile('wtr', 0)
        t_down = time.perf_counter() - t0
        rec = {'batch_histogram': row(read, ms['histogram'], ms_samples=[round(v, 4) for v in ms['histogram']]),
               'batch_label_all_outputs': row(read, ms['label_all'], kernel=info, ms_samples=[round(v, 4) for v in ms['label_all']]),
               'batch_label_label_alone': row(read, ms['label_alone'], ms_samples=[round(v, 4) for v in ms['label_alone']]),
               'summary_of_one_tile': {'bodies': int(words[0]), 'member_pixels': int(words[1]), 'largest_size': int(words[2]),
                                       'bodies_kept': int(words[4])}}
        for k in ('batch_label_all_outputs', 'batch_label_label_alone'):
            r = rec[k]
            r['ms_per_tile_median'], r['ms_per_tile_min'], r['ms_per_tile_max'] = (round(r[q] / a.tiles, 5) for q in ('ms_median', 'ms_min', 'ms_max'))
            r['multiple_of_histogram'] = round(r['ms_median'] / rec['batch_histogram']['ms_median'], 2)
        try:
            from scipy import ndimage
            t0 = time.perf_counter()
            lab, k = ndimage.label(spec.member_of_byte[tile] != 0, structure=np.ones((3, 3)))
            sizes = np.bincount(lab.reshape(-1))
            t_scipy = time.perf_counter() - t0
            rec['host_yardstick'] = {'download_one_tile_ms': round(t_down * 1e3, 3), 'scipy_label_bincount_ms': round(t_scipy * 1e3, 3),
                                     'bodies': int(k), 'largest_size': int(sizes[1:].max()) if k else 0}
            rec['chain_beats_download_plus_scipy_by'] = round((t_down + t_scipy) * 1e3 / rec['batch_label_all_outputs']['ms_per_tile_median'], 1)
        except ImportError:
            rec['host_yardstick'] = {'download_one_tile_ms': round(t_down * 1e3, 3), 'scipy': 'not installed'}
        out['contents'][content] = rec

    batch.synth(SEED)
    batch.classify(p)
    ctx.synchronize()
    measure('synthetic')
    fill_scene(ctx, batch, a.size)
    batch.classify(p)
    ctx.synchronize()
    measure('scene')
    ptr, _ = batch._plane('wtr')
    _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ptr, 1, a.tiles * batch.tile_stride))
    ctx.synchronize()
    measure('all_member')
    planes.free()
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
