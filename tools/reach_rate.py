#!/usr/bin/env python3
"""Time of the reach (dswx_reach.hip) per tile, in one process, with HIP events on the library's stream: dswx_reach_device with
`acc`, `mask` and `head` over one range of tiles of 3660 x 3660, at radius 0, 10 pixels and 1 km (33.33 pixels of 30 m), for

  zero_records   no record at all: the floor -- the memset of `acc` and the scan, 13 bytes per pixel with `mask`;
  coastline      the synthetic polygon of 100 003 vertices of tools/burn_rate.py, the same in every tile;
  scene          the rings that dswx_outline_device returns for the label plane of the WTR layer of the coherent scene.

Measured alongside, in the same run and on the same records: dswx_burn_device, and the raster chain that `dswx_burn.py --buffer-m`
runs -- burn, then dswx_distance_device with `within` at the radius rounded down to whole pixels.  The chain computes ANOTHER
mask (distances between pixel centres), so no ratio to it was fixed in advance: the ratio is recorded, and on how many pixels of
tile 0 the two masks differ.

THE ONE CONDITION, fixed in advance: one tile's OCEAN step on the device -- the upload of both record tables, the memset of the
plane, burn, reach in place, and the wait -- must beat what it replaces, measured in the same run: dswx_burn_host +
dswx_reach_host of that tile on one core plus the upload of the mask.  Every sample is kept.

    python tools/reach_rate.py [--tiles 32] [--reps 20] [--out profiles/reach_rate.json]
"""
import argparse
import ctypes
import datetime
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi                      # noqa: E402
from proteus_amd import burn as BN                 # noqa: E402
from proteus_amd import reach as RC                # noqa: E402
from proteus_amd.compare import RECORD             # noqa: E402
from proteus_amd.distance import Spec as DistanceSpec   # noqa: E402
from proteus_amd.label import wtr_label_spec       # noqa: E402
from proteus_amd.outline import Spec as OutlineSpec   # noqa: E402

from burn_rate import coastline                    # noqa: E402  (the same polygon)
from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

PIXEL_M = 30.0
RADII = (('0', 0), ('10_pixels', 10 * 256), ('1_km', int(round(256 * 1000.0 / PIXEL_M))))
BUDGET = {'hipMemsetAsync(acc)': '4 p written',
          'dswx_reach_scatter_k': '16 per record read in order, 16 gathered; per (edge, row) two 4-byte atomic adds (one when the interval '
                                  'ends at the last column): at least 2 R / 256 + 1 rows per edge',
          'dswx_reach_scan_k': '4 p read, 4 p written, 1 p written to mask (1 p read of src when there is one)'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=32, help='tiles of the one range')
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--connectivity', type=int, default=8)
    ap.add_argument('--machine', default='MI355X (gfx950)')
    ap.add_argument('--out', default=os.path.join('profiles', 'reach_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    T, S = a.tiles, a.size
    px = S * S
    acc, mask, head = ctx.malloc(4 * T * px), ctx.malloc(T * px), ctx.malloc(8 * _capi.REACH_HEAD_WORDS * T)
    chain_mask, within, dist2 = ctx.malloc(T * px), ctx.malloc(T * px), ctx.malloc(4 * T * px)
    cmp_rec = ctx.malloc(64)
    out3 = _capi.BurnOut.of(acc=acc.ptr, mask=mask.ptr, head=head.ptr)
    bspec = BN.Spec(burn=1, background=0)
    target = np.zeros(256, dtype=np.uint8)
    target[1] = 1

    def per_tile(r):
        r['ms_per_tile_median'], r['ms_per_tile_min'], r['ms_per_tile_max'] = (round(r[q] / T, 5) for q in ('ms_median', 'ms_min', 'ms_max'))
        return r

    def ocean_step(one, rspec):
        """One tile's OCEAN step on the device, and what it replaces; wall clock, the better of three."""
        first = np.array([0, len(one)], dtype=np.int64)
        dev, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            tables = [(ctx.malloc(max(one.nbytes, 16)), ctx.malloc(first.nbytes)) for _ in range(2)]
            for dv, df in tables:
                if one.nbytes:
                    dv.upload(one)
                df.upload(first)
            _capi._check(ctx.lib.dswx_memset_d(ctx.handle, mask.ptr, 0, px))
            o = _capi.BurnOut.of(acc=acc.ptr, mask=mask.ptr)
            ctx.burn_device(tables[0][0].ptr, tables[0][1].ptr, bspec, 1, S, S, mask.ptr, o)
            ctx.reach_device(tables[1][0].ptr, tables[1][1].ptr, rspec, 1, S, S, mask.ptr, o)
            ctx.synchronize()
            dev.append(time.perf_counter() - t0)
            for dv, df in tables:
                dv.free()
                df.free()
        got = mask.download(np.uint8, px)
        for _ in range(1 if len(one) > 500000 else 3):
            t0 = time.perf_counter()
            m = np.zeros((1, S, S), dtype=np.uint8)
            _capi.burn_host(one, first, S, S, bspec, src=m, mask=m, want=('mask',))
            _capi.reach_host(one, first, S, S, rspec, src=m, mask=m, want=('mask',))
            t1 = time.perf_counter()
            chain_mask.upload(m)
            ctx.synchronize()
            host.append((time.perf_counter() - t0, t1 - t0))
        assert np.array_equal(got, m.reshape(-1)), 'the OCEAN plane of the device differs from the host entries'
        best = min(host)
        rec = {'device_upload_2_tables_memset_burn_reach_wait_ms': round(min(dev) * 1e3, 3),
               'host_burn_host_plus_reach_host_one_core_ms': round(best[1] * 1e3, 3), 'host_upload_of_the_mask_ms': round((best[0] - best[1]) * 1e3, 3),
               'host_total_ms': round(best[0] * 1e3, 3), 'ocean_pixels_equal': True}
        rec['device_beats_what_it_replaces_by'] = round(rec['host_total_ms'] / rec['device_upload_2_tables_memset_burn_reach_wait_ms'], 1)
        rec['condition_met'] = bool(rec['device_beats_what_it_replaces_by'] > 1.0)
        return rec

    def measure(one):
        verts, first = np.tile(one, T), np.arange(T + 1, dtype=np.int64) * len(one)
        dv, df = ctx.malloc(max(verts.nbytes, 16)), ctx.malloc(first.nbytes)
        if verts.nbytes:
            dv.upload(verts)
        df.upload(first)
        rec = {'records_per_tile': int(len(one)), 'radii': {}}
        for name, R in RADII:
            rspec = RC.Spec(R, burn=1, background=0)
            whole = R // 256
            dspec = DistanceSpec(target, max(whole, 1), 1)
            dout = _capi.DistanceOut.of(dist2=dist2.ptr, within=within.ptr)

            def chain():
                ctx.burn_device(dv.ptr, df.ptr, bspec, T, S, S, None, _capi.BurnOut.of(acc=acc.ptr, mask=chain_mask.ptr))
                if whole >= 1:
                    ctx.distance_device(chain_mask.ptr, dspec, T, S, S, dout)

            def burn_reach():
                ctx.burn_device(dv.ptr, df.ptr, bspec, T, S, S, None, _capi.BurnOut.of(acc=acc.ptr, mask=mask.ptr))
                ctx.reach_device(dv.ptr, df.ptr, rspec, T, S, S, mask.ptr, _capi.BurnOut.of(acc=acc.ptr, mask=mask.ptr))
            fns = {'reach': lambda: ctx.reach_device(dv.ptr, df.ptr, rspec, T, S, S, None, out3),
                   'burn': lambda: ctx.burn_device(dv.ptr, df.ptr, bspec, T, S, S, None, out3),
                   'burn_then_reach_in_place': burn_reach, 'burn_then_distance_within': chain}
            ms = timed_alternating(ctx, fns, a.reps)
            fns['reach']()
            info = ctx.last_kernel_info()
            ctx.synchronize()
            h = head.download(np.uint64, _capi.REACH_HEAD_WORDS * T).reshape(T, -1)
            assert (h == h[0]).all(), 'the tiles hold the same records'
            chain()
            burn_reach()
            ctx.compare_device(mask.ptr, (within if whole >= 1 else chain_mask).ptr, _capi.CMP_U8, 1, px, cmp_rec.ptr)
            ctx.synchronize()
            differ = int(cmp_rec.download(RECORD, 1)['n_diff'][0])
            r = {'radius_256ths': R, 'head_of_a_tile': [int(v) for v in h[0]], 'kernel': info,
                 'reach_acc_mask_head': per_tile(row(13 * T * px, ms['reach'], ms_samples=[round(v, 4) for v in ms['reach']])),
                 'burn_acc_mask_head': per_tile(row(13 * T * px, ms['burn'], ms_samples=[round(v, 4) for v in ms['burn']])),
                 'burn_then_reach_in_place': per_tile(row(0, ms['burn_then_reach_in_place'])),
                 'burn_then_distance_within': per_tile(row(0, ms['burn_then_distance_within'], radius_whole_pixels=whole)),
                 'pixels_of_tile_0_on_which_the_two_masks_differ': differ}
            r['vector_buffer_over_raster_chain_time'] = round(r['burn_then_reach_in_place']['ms_median'] / r['burn_then_distance_within']['ms_median'], 3)
            if h[0][3]:
                r['atomics_per_interval'] = 2
                r['intervals_per_us'] = round(float(h[0][3]) * T / (r['reach_acc_mask_head']['ms_median'] * 1e3), 1)
            r['ocean_step_of_one_tile'] = ocean_step(one, rspec)
            rec['radii'][name] = r
        dv.free()
        df.free()
        return rec

    out = {'tool': 'tools/reach_rate.py', 'date': datetime.date.today().isoformat(), 'machine': a.machine,
           'design': 'one memset each of acc and head; dswx_reach_scatter_k: one thread per record, the rows of an edge shared out over the '
           '64 lanes of its wave, per row two integer square roots, the ends of the slab estimated in double and moved with the exact 128-bit '
           'predicate, two non-returning atomic adds; dswx_reach_scan_k: the prefix sum of every row in place, fused with the mask and the '
           'count of the pixels; no workgroup waits for another',
           'tiles': T, 'tile': [S, S], 'reps': a.reps, 'hbm_peak_GBps': PEAK, 'pixel_m': PIXEL_M,
           'times_are': 'stream events around one call over all tiles; per tile = / tiles; GB/s counts 13 bytes per pixel; the OCEAN step is '
           'wall clock of one tile',
           'budget': BUDGET,
           'bar': 'none against the raster chain (it computes another mask); the one condition: the OCEAN step of one tile on the device beats '
           'dswx_burn_host + dswx_reach_host on one core plus the upload of the mask',
           'contents': {}}
    out['contents']['zero_records'] = measure(np.zeros(0, dtype=BN.VERTEX_DTYPE))
    out['contents']['coastline'] = measure(BN.records([BN.quantise(coastline(S))]))

    # the outline rings of the coherent scene: label and outline of tile 0 on the device, records on the host
    batch = _capi.DeviceBatch(ctx, 1, S, S)
    fill_scene(ctx, batch, S)
    batch.classify(_capi.default_params())
    ctx.synchronize()
    label = ctx.malloc(4 * px)
    wtr = _capi.PLANE_INDEX['wtr']
    _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(_capi.LabelSpec.of(wtr_label_spec(1, connectivity=a.connectivity))), 0, 1,
                                          ctypes.byref(_capi.LabelOut.of(label=label.ptr)), None))
    counting = ctx.outline(label, OutlineSpec(0, 0, a.connectivity), 1, S, S, want=('head',))
    E = int(counting['head'].download(np.uint64, 8)[0])
    counting['head'].free()
    ospec = OutlineSpec(max(E, 4), max(E // 4, 1), a.connectivity)
    res = ctx.outline(label, ospec, 1, S, S)
    one = BN.records_of_outline(res['chain'].download(np.uint32, ospec.max_edges), res['rings'].download(np.uint32, ospec.max_rings * 8).reshape(-1, 8), S)
    for b in list(res.values()) + [label]:
        b.free()
    batch.free()
    out['contents']['scene'] = dict(measure(one), edges_of_the_outline=E)

    conditions = [r['ocean_step_of_one_tile']['condition_met'] for c in out['contents'].values() for r in c['radii'].values()]
    out['the_one_condition_met_in_every_case'] = bool(all(conditions))
    for b in (acc, mask, head, chain_mask, within, dist2, cmp_rec):
        b.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
