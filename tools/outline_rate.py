#!/usr/bin/env python3
"""Time of the outline (dswx_outline.hip) per tile, in one process, with HIP events on the library's stream.  On the `label`
plane of the WTR layer of the resident batch of 256 tiles of 3660 x 3660 in ranges of 32 tiles, for the three contents of
tools/label_rate.py --

  synthetic    the generated batch, classified: per-pixel class noise, hundreds of thousands of bodies per tile;
  scene        the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified: water in patches;
  all_member   every pixel open water: ONE body per tile, ONE ring of 4 * 3660 edges

-- the label plane of EVERY tile is made once by dswx_batch_label and stays in HBM; the counting call (head alone, no capacity)
says how many edges the tiles have, and dswx_outline_device then runs over the plane with that capacity and all three outputs,
next to the label chain that produced its input (label alone), timed alternately.  Recorded: E and R per tile, the rounds of
pointer jumping that the capacity fixes and those that actually ran (read from the flags in the working memory), the bytes of
working memory, and what the entry replaces: the download of the label plane of one tile plus dswx_outline_host on one core.
Nobody has measured dependent gathers like these on this part and no rate can be derived, so nothing is judged against a
bandwidth and no bar was fixed in advance.  Every sample is kept.

    python tools/outline_rate.py [--tiles 256] [--range 32] [--reps 20] [--out profiles/outline_rate.json] [--once]
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
from proteus_amd.label import wtr_label_spec       # noqa: E402
from proteus_amd.outline import Spec               # noqa: E402
from proteus_amd.synth import SEED                 # noqa: E402

from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

# what a launch streams or gathers, bytes per pixel (p) or per edge (e)
BUDGET = {'dswx_outline_count_k': '4 p read (the neighbours from cache), 1 p written',
          'dswx_outline_base_k': '1 p read, 4 p written',
          'dswx_outline_emit_k': '9 p read; per edge 3 ids, a base and a mask gathered, 16 e written',
          'dswx_outline_jump_k': 'per round 16 e read in order, 16 e gathered, 16 e written',
          'dswx_outline_ring_count_k/ring_rank_k': '16 e read each; per ring 16 gathered and 16 written',
          'dswx_outline_scatter_k': '16 e read, 16 e gathered, 4 e scattered'}
INFO_BYTES, INFO_FLAGS_AT, MAX_ROUNDS = 256, 24, 31   # csrc/dswx_outline.hip OutlineInfo: E, R (uint64), ok, fin, flag[32] (uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--range', dest='span', type=int, default=32, help='tiles per call')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--connectivity', type=int, default=8)
    ap.add_argument('--once', action='store_true', help='one pass per content and nothing timed: the run to put under a kernel trace')
    ap.add_argument('--out', default=os.path.join('profiles', 'outline_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    px = batch.n_pixels
    wtr = _capi.PLANE_INDEX['wtr']
    span = min(a.span, a.tiles)
    lspec = wtr_label_spec(1, connectivity=a.connectivity)
    clspec = _capi.LabelSpec.of(lspec)
    HW = _capi.OUTLINE_HEAD_WORDS
    labels = ctx.malloc(4 * a.tiles * px)                                  # the label plane of every tile
    chain_label = ctx.malloc(4 * span * px)
    head = ctx.malloc(8 * HW * a.tiles)

    def label_every_tile():
        for t0 in range(0, a.tiles, span):
            o = _capi.LabelOut.of(label=labels.ptr + 4 * t0 * px)
            _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(clspec), t0, min(span, a.tiles - t0), ctypes.byref(o), None))

    alone = _capi.LabelOut.of(label=chain_label.ptr)

    def chain():
        for t0 in range(0, a.tiles, span):
            _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(clspec), t0, min(span, a.tiles - t0), ctypes.byref(alone), None))

    def outline(spec, work, work_bytes, out_of):
        for t0 in range(0, a.tiles, span):
            ctx.outline_device(labels.ptr + 4 * t0 * px, spec, min(span, a.tiles - t0), a.size, a.size, out_of(t0), work.ptr, work_bytes)

    out = {'tool': 'tools/outline_rate.py', 'design': 'count the edges per chunk of 4096 pixels, scan, number the first edge of every pixel, '
           'emit a 16-byte state per edge, ceil(log2 capacity) rounds of pointer jumping between two copies of the states (a tile '
           'whose round changed nothing skips the rest), count / scan / rank the ring starts, scatter the keys into the chain with the '
           'sums of a ring combined per run of lanes, finish the rows and the head; 9 + rounds launches and two memsets per call, no '
           'workgroup waits for another',
           'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride, 'tiles_per_call': span, 'reps': a.reps,
           'connectivity': a.connectivity, 'hbm_peak_GBps': PEAK,
           'times_are': 'stream events around one pass over all tiles (tiles / tiles_per_call calls); per tile = / tiles',
           'budget': BUDGET, 'bar': 'none fixed in advance: recorded next to the label chain (label alone) measured alongside',
           'contents': {}}

    def measure(content):
        label_every_tile()
        ctx.synchronize()
        counting = Spec(0, 0, a.connectivity)
        wb = _capi.outline_work_bytes(counting, span, a.size, a.size)
        work = ctx.malloc(wb)
        outline(counting, work, wb, lambda t0: _capi.OutlineOut.of(head=head.ptr + 8 * HW * t0))
        ctx.synchronize()
        work.free()
        E = head.download(np.uint64, HW * a.tiles).reshape(a.tiles, HW)[:, 0]
        cap = int(E.max())
        spec = Spec(max(cap, 4), max(cap // 4, 1), a.connectivity)
        wb = _capi.outline_work_bytes(spec, span, a.size, a.size)
        work = ctx.malloc(wb)
        chain_buf, rings = ctx.malloc(4 * spec.max_edges * span), ctx.malloc(32 * spec.max_rings * span)
        out_of = lambda t0: _capi.OutlineOut.of(chain=chain_buf.ptr, rings=rings.ptr, head=head.ptr + 8 * HW * t0)
        if a.once:
            outline(spec, work, wb, out_of)
            ctx.synchronize()
        else:
            ms = timed_alternating(ctx, {'label_alone': chain, 'outline_all': lambda: outline(spec, work, wb, out_of)}, a.reps)
            outline(spec, work, wb, out_of)
            info = ctx.last_kernel_info()
            ctx.synchronize()
            h = head.download(np.uint64, HW * a.tiles).reshape(a.tiles, HW)
            assert np.array_equal(h[:, 0], E) and not h[:, 7].any()
            # the rounds that ran for the tiles of the last call: round 0, then one more per flag that the round before raised
            n_last = a.tiles - (a.tiles - 1) // span * span
            per_tile = (wb - 16) // span
            base = (-work.ptr) % 16
            rounds_fixed = max(int(np.ceil(np.log2(min(spec.max_edges, 4 * px)))), 0)
            ran = []
            for t in range(n_last):
                flags = work.download(np.uint32, MAX_ROUNDS + 1, base + (t + 1) * per_tile - INFO_BYTES + INFO_FLAGS_AT)
                ran.append(int(h[a.tiles - n_last + t, 0] > 0) + int(np.count_nonzero(flags[:max(rounds_fixed - 1, 0)])))
            rec = {'edges_per_tile': {'min': int(E.min()), 'median': int(np.median(E)), 'max': int(E.max())},
                   'rings_per_tile': {'min': int(h[:, 1].min()), 'median': int(np.median(h[:, 1])), 'max': int(h[:, 1].max())},
                   'outer_rings_per_tile_max': int(h[:, 4].max()), 'holes_per_tile_max': int(h[:, 5].max()),
                   'capacity_edges': spec.max_edges, 'capacity_rings': spec.max_rings, 'work_bytes_per_call': wb,
                   'work_bytes_per_tile': per_tile, 'rounds_fixed_by_the_capacity': rounds_fixed,
                   'rounds_run_in_the_tiles_of_the_last_call': {'min': min(ran), 'max': max(ran)}}
            for k, name in (('label_alone', 'batch_label_label_alone'), ('outline_all', 'outline_all_outputs')):
                r = row(4 * a.tiles * px, ms[k], ms_samples=[round(v, 4) for v in ms[k]])
                r['ms_per_tile_median'], r['ms_per_tile_min'], r['ms_per_tile_max'] = (round(r[q] / a.tiles, 5) for q in ('ms_median', 'ms_min', 'ms_max'))
                rec[name] = r
            rec['outline_all_outputs']['kernel'] = info
            rec['outline_over_label_chain'] = round(rec['outline_all_outputs']['ms_median'] / rec['batch_label_label_alone']['ms_median'], 3)
            rec['label_chain_then_outline_ms_per_tile'] = round(rec['outline_all_outputs']['ms_per_tile_median'] + rec['batch_label_label_alone']['ms_per_tile_median'], 5)
            # what the entry replaces: the label plane of one tile over PCIe, then the scalar walk on one core
            t0 = time.perf_counter()
            lab = labels.download(np.uint32, px).reshape(1, a.size, a.size)
            t_down = time.perf_counter() - t0
            one = Spec(max(int(E[0]), 4), max(int(E[0]) // 4, 1), a.connectivity)
            t0 = time.perf_counter()
            ref = _capi.outline_host(lab, one)
            t_host = time.perf_counter() - t0
            rec['host_yardstick'] = {'download_label_of_one_tile_ms': round(t_down * 1e3, 3), 'dswx_outline_host_one_core_ms': round(t_host * 1e3, 3),
                                     'edges': int(ref['head'][0, 0]), 'rings': int(ref['head'][0, 1])}
            rec['outline_beats_download_plus_host_walk_by'] = round((t_down + t_host) * 1e3 / rec['outline_all_outputs']['ms_per_tile_median'], 1)
            out['contents'][content] = rec
        for b in (work, chain_buf, rings):
            b.free()

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
    for b in (labels, chain_label, head):
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
