#!/usr/bin/env python3
"""Rate of the crosstab kernel (dswx_crosstab.hip) against the histogram kernel over the same two planes, in one process,
with HIP events on the library's stream.  On the 256-tile 3660 x 3660 headline batch, for three contents --

  synthetic   the generated batch, classified: per-pixel noise;
  scene       the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified: classes in
              patches, long runs of one byte -- what a real product looks like;
  constant    every plane overwritten with one byte: every lane of every wave meets in one cell, the worst case for a
              shared counter

-- and three pairs -- WTR-2 x WTR, swir1 (folded to 16 rows) x WTR, DIAG x WTR-1 -- dswx_batch_crosstab of the pair and
dswx_batch_histogram of the same two planes in one call, alternating call by call (the time of the CALL on the stream:
allocation, zeroing, kernel, read-back).  The bytes are the same; the crosstab does one LDS add per pair and two table
lookups where the histogram does two adds.  THE EXPECTATION to report against: the crosstab call is no slower than that
histogram call, within the project's run-to-run spread of about 3 %; and the constant content is no slower than the noise.

    python tools/crosstab_rate.py [--tiles 256] [--reps 10] [--out profiles/crosstab_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from proteus_amd import _capi                                              # noqa: E402
from proteus_amd.crosstab import WTR_CLASSES, WTR_VALUES, Spec, classes, fold   # noqa: E402
from proteus_amd.histogram import HIST_DIAG, HIST_I16                      # noqa: E402
from proteus_amd.synth import SEED                                         # noqa: E402
from histogram_rate import fill_constant, fill_scene, row, timed_alternating     # noqa: E402

SPREAD = 0.03
PAIRS = {'wtr2_x_wtr': ('wtr2', 'wtr', WTR_CLASSES),
         'swir1_x_wtr': ('swir1', 'wtr', Spec(HIST_I16, 0, 6, 4, fold(16), classes(WTR_VALUES, other=7))),
         'diag_x_wtr1': ('diag', 'wtr1', Spec(HIST_DIAG, col_bits=3, row_of_bin=np.minimum(np.arange(256), 31),
                                              col_of_byte=classes(WTR_VALUES, other=7)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join('profiles', 'crosstab_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    px = a.tiles * a.size * a.size
    names = batch.plane_names()
    width = {n: 2 if n in _capi.BAND_NAMES or n == 'diag' else 1 for n in names}
    out = {'tool': 'tools/crosstab_rate.py', 'design': 'lane-indexed replicas (32 sets of 256 uint32 counters per block in LDS, bank = '
           'lane & 31), two uint16 tables of 256 entries in LDS, the row premultiplied; one add per step whose units of both planes '
           'hold one value', 'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride, 'reps': a.reps,
           'expectation_crosstab_over_histogram': 1.0, 'run_to_run_spread': SPREAD, 'contents': {}}

    def measure(content):
        rec = {}
        for label, (na, nb, spec) in PAIRS.items():
            nbytes = px * (width[na] + width[nb])
            ms = timed_alternating(ctx, {'histogram': lambda: batch.histogram(names=[na, nb]),
                                         'crosstab': lambda: batch.crosstab([(na, nb, spec)])}, a.reps)
            info = ctx.last_kernel_info()
            h, c = row(nbytes, ms['histogram']), row(nbytes, ms['crosstab'], kernel=info)
            rec[label] = {'batch_histogram_of_both_planes': h, 'batch_crosstab': c,
                          'ratio_crosstab_over_histogram': round(c['GBps_median'] / h['GBps_median'], 4)}
        rec['ratio_min'] = min(v['ratio_crosstab_over_histogram'] for v in rec.values())
        rec['no_slower_than_histogram'] = bool(rec['ratio_min'] >= 1.0 - SPREAD)
        table = WTR_CLASSES.table(batch.crosstab([PAIRS['wtr2_x_wtr']], n_tiles=1)[0, 0])[:8]
        rec['wtr2_x_wtr_tile_0'] = table.tolist()
        out['contents'][content] = rec

    batch.synth(SEED)
    batch.classify(p)
    ctx.synchronize()
    measure('synthetic')
    fill_scene(ctx, batch, a.size)
    batch.classify(p)
    ctx.synchronize()
    measure('scene')
    fill_constant(ctx, batch, names)
    measure('constant')
    syn, con = out['contents']['synthetic'], out['contents']['constant']
    out['constant_over_synthetic_crosstab'] = {k: round(con[k]['batch_crosstab']['GBps_median'] / syn[k]['batch_crosstab']['GBps_median'], 4)
                                               for k in PAIRS}
    out['constant_no_slower_than_noise'] = all(v >= 1.0 - SPREAD for v in out['constant_over_synthetic_crosstab'].values())
    out['no_slower_than_histogram'] = all(v['no_slower_than_histogram'] for v in out['contents'].values())
    batch.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
