#!/usr/bin/env python3
"""Time of the burn (dswx_burn.hip) per tile, in one process, with HIP events on the library's stream: dswx_burn_device with
`acc`, `mask` and `head` over one range of tiles of 3660 x 3660, for

  zero_records   no record at all: the floor -- the memset of `acc` and the scan, 13 bytes per pixel with `mask` (4 cleared, 4
                 read, 4 + 1 written) -- reported as GB/s next to dswx_batch_histogram of one uint8 plane of a batch of the same
                 tiles, measured alternately in the same run;
  synthetic / scene / all_member
                 the rings that dswx_outline_device returns for the `label` plane of the WTR layer of the three standard
                 contents (tools/outline_rate.py): per-pixel class noise, the coherent scene, one body.  The outline of tile 0
                 is traced on the device, read back (chain and rings), turned into records on the host and used for EVERY tile
                 of the range; dswx_compare_device then finds acc of the first and the last tile equal to the label plane;
  coastline      one synthetic polygon of about 100 000 vertices that leaves the tile on two sides, the same in every tile.

Each is set beside what it replaces, measured in the same run: dswx_burn_host of one tile on one core plus the upload of its
mask.  Nothing about this kernel had been measured and the guides give no rate for 32-bit integer XOR atomics, so no bar was
fixed in advance -- except one: the zero-record floor must reach 0.5 of the histogram's GB/s measured alongside (the scan moves
its bytes once with unit stride).  Every sample is kept.

    python tools/burn_rate.py [--tiles 32] [--reps 20] [--out profiles/burn_rate.json]
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
from proteus_amd.label import wtr_label_spec       # noqa: E402
from proteus_amd.outline import Spec as OutlineSpec   # noqa: E402
from proteus_amd.synth import SEED                 # noqa: E402

from histogram_rate import PEAK, fill_scene, row, timed_alternating   # noqa: E402  (the same timing loop and row format)

FLOOR_BAR = 0.5
BUDGET = {'hipMemsetAsync(acc)': '4 p written',
          'dswx_burn_toggle_k': '16 per record read in order, 16 gathered (in ring order the neighbour); per crossing one 4-byte atomic XOR',
          'dswx_burn_scan_k': '4 p read, 4 p written, 1 p written to mask (1 p read of src when there is one)'}


def coastline(size, n=100000, seed=7):
    """One ring in pixel coordinates: a wiggling shore from beyond the left side to beyond the top, closed around the lower
    right outside of the tile."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)
    x = size * (-0.05 + 0.9 * t) + 60 * np.sin(2 * np.pi * 37 * t) + 9 * np.sin(2 * np.pi * 911 * t) + rng.normal(0, 0.7, n)
    y = size * (0.85 - 0.9 * t) + 60 * np.cos(2 * np.pi * 53 * t) + 9 * np.cos(2 * np.pi * 1201 * t) + rng.normal(0, 0.7, n)
    shore = np.stack([x, y], axis=1)
    return np.concatenate([shore, [[size * 1.2, -0.1 * size], [size * 1.2, size * 1.2], [-0.1 * size, size * 1.2]]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=32, help='tiles of the one range')
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--connectivity', type=int, default=8)
    ap.add_argument('--machine', default='MI355X (gfx950)')
    ap.add_argument('--out', default=os.path.join('profiles', 'burn_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    T, S = a.tiles, a.size
    batch = _capi.DeviceBatch(ctx, T, S, S)
    p = _capi.default_params()
    px = batch.n_pixels
    wtr = _capi.PLANE_INDEX['wtr']
    spec = BN.Spec(burn=1, background=0)
    acc, mask, head = ctx.malloc(4 * T * px), ctx.malloc(T * px), ctx.malloc(8 * _capi.BURN_HEAD_WORDS * T)
    bout = _capi.BurnOut.of(acc=acc.ptr, mask=mask.ptr, head=head.ptr)
    hist = np.zeros((1, T, _capi.HIST_BINS), dtype=np.uint64)

    def histogram():
        _capi._check(ctx.lib.dswx_batch_histogram(batch.handle, 1 << wtr, 0, T, 0, 6, _capi._host_ptr(hist), None))

    def burn_of(d_verts, d_first):
        return lambda: ctx.burn_device(d_verts.ptr, d_first.ptr, spec, T, S, S, None, bout)

    def upload_records(one):
        """The records of one tile for every tile of the range."""
        verts, first = np.tile(one, T), np.arange(T + 1, dtype=np.int64) * len(one)
        dv, df = ctx.malloc(max(verts.nbytes, 16)), ctx.malloc(first.nbytes)
        if verts.nbytes:
            dv.upload(verts)
        df.upload(first)
        return dv, df

    def yardstick(one):
        """What the entry replaces: dswx_burn_host of one tile on one core, then the upload of its mask."""
        t0 = time.perf_counter()
        ref = _capi.burn_host(one, np.array([0, len(one)]), S, S, spec, want=('mask', 'head'))
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        mask.upload(ref['mask'])
        ctx.synchronize()
        t_up = time.perf_counter() - t0
        return ref, {'dswx_burn_host_one_core_ms': round(t_host * 1e3, 3), 'upload_mask_of_one_tile_ms': round(t_up * 1e3, 3)}

    def per_tile(r):
        r['ms_per_tile_median'], r['ms_per_tile_min'], r['ms_per_tile_max'] = (round(r[q] / T, 5) for q in ('ms_median', 'ms_min', 'ms_max'))
        return r

    def measure(one, with_histogram=False):
        dv, df = upload_records(one)
        fns = {'burn': burn_of(dv, df)}
        if with_histogram:
            fns['histogram'] = histogram
        ms = timed_alternating(ctx, fns, a.reps)
        fns['burn']()
        info = ctx.last_kernel_info()
        ctx.synchronize()
        h = head.download(np.uint64, _capi.BURN_HEAD_WORDS * T).reshape(T, -1)
        ref, yard = yardstick(one)
        assert np.array_equal(h, np.repeat(ref['head'], T, axis=0)), 'the head of the device differs from the host entry'
        rec = {'records_per_tile': int(len(one)), 'head_of_a_tile': [int(v) for v in h[0]],
               'burn_acc_mask_head': per_tile(row(13 * T * px, ms['burn'], ms_samples=[round(v, 4) for v in ms['burn']])), 'kernel': info,
               'host_yardstick': yard}
        rec['burn_beats_host_entry_plus_upload_by'] = round(sum(yard.values()) / rec['burn_acc_mask_head']['ms_per_tile_median'], 1)
        if with_histogram:
            rec['batch_histogram_one_uint8_plane'] = per_tile(row(T * px, ms['histogram'], ms_samples=[round(v, 4) for v in ms['histogram']]))
        dv.free()
        df.free()
        return rec

    out = {'tool': 'tools/burn_rate.py', 'date': datetime.date.today().isoformat(), 'machine': a.machine,
           'design': 'one memset each of acc and head; dswx_burn_toggle_k: one thread per record, the first crossing by one 64-bit '
           'division, further rows by adding a quotient and a remainder, edges of more than 4 rows shared out over the 64 lanes of the '
           'wave, one atomic XOR per crossing; dswx_burn_scan_k: the XOR prefix of every row in place, 16 bytes of acc per lane and '
           'step, fused with the mask and the count of the pixels; no workgroup waits for another',
           'tiles': T, 'tile': [S, S], 'reps': a.reps, 'hbm_peak_GBps': PEAK,
           'times_are': 'stream events around one call over all tiles; per tile = / tiles; GB/s of the burn counts 13 bytes per pixel',
           'budget': BUDGET, 'bar': f'none fixed in advance, but: zero_records GB/s >= {FLOOR_BAR} of dswx_batch_histogram GB/s measured alongside',
           'contents': {}}

    batch.synth(SEED)
    batch.classify(p)
    ctx.synchronize()
    floor = measure(np.zeros(0, dtype=BN.VERTEX_DTYPE), with_histogram=True)
    floor['floor_over_histogram_GBps'] = round(floor['burn_acc_mask_head']['GBps_median'] / floor['batch_histogram_one_uint8_plane']['GBps_median'], 3)
    floor['floor_bar_met'] = bool(floor['floor_over_histogram_GBps'] >= FLOOR_BAR)
    out['contents']['zero_records'] = floor

    lspec = wtr_label_spec(1, connectivity=a.connectivity)
    label = ctx.malloc(4 * px)
    cmp_rec = ctx.malloc(64)
    from proteus_amd.compare import RECORD

    def rings_content(name):
        """The outline of the label plane of tile 0 of the batch's WTR layer as records."""
        _capi._check(ctx.lib.dswx_batch_label(batch.handle, wtr, ctypes.byref(_capi.LabelSpec.of(lspec)), 0, 1,
                                              ctypes.byref(_capi.LabelOut.of(label=label.ptr)), None))
        counting = ctx.outline(label, OutlineSpec(0, 0, a.connectivity), 1, S, S, want=('head',))
        E = int(counting['head'].download(np.uint64, 8)[0])
        counting['head'].free()
        ospec = OutlineSpec(max(E, 4), max(E // 4, 1), a.connectivity)
        res = ctx.outline(label, ospec, 1, S, S)
        chain = res['chain'].download(np.uint32, ospec.max_edges)
        rings = res['rings'].download(np.uint32, ospec.max_rings * 8).reshape(-1, 8)
        R = int(res['head'].download(np.uint64, 8)[1])
        for b in res.values():
            b.free()
        t0 = time.perf_counter()
        one = BN.records_of_outline(chain, rings, S)
        t_rec = time.perf_counter() - t0
        rec = measure(one)
        for t in (0, T - 1):                                 # acc IS the label plane (uint32 compared as twice as many uint16)
            ctx.compare_device(acc.ptr + 4 * t * px, label.ptr, _capi.CMP_U16, 1, 2 * px, cmp_rec.ptr)
            ctx.synchronize()
            assert int(cmp_rec.download(RECORD, 1)['n_diff'][0]) == 0, (name, t)
        rec.update(edges_of_the_outline=E, rings_of_the_outline=R, records_of_outline_on_the_host_ms=round(t_rec * 1e3, 1),
                   acc_equals_the_label_plane=True)
        out['contents'][name] = rec

    rings_content('synthetic')
    fill_scene(ctx, batch, S)
    batch.classify(p)
    ctx.synchronize()
    rings_content('scene')
    ptr, _ = batch._plane('wtr')
    _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ptr, 1, T * batch.tile_stride))
    ctx.synchronize()
    rings_content('all_member')
    shore = BN.records([BN.quantise(coastline(S))])
    out['contents']['coastline'] = measure(shore)
    for b in (acc, mask, head, label, cmp_rec):
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
