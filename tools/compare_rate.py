#!/usr/bin/env python3
"""Rate of the compare kernel (dswx_compare.hip) against the checksum kernel on the same bytes, in one process, with HIP
events on the library's stream.  On a pair of 256-tile 3660 x 3660 batches (same seed; classified with the same parameters,
then the second one again with other thresholds):

  - dswx_batch_compare over the seven output planes and over the seven input planes of the pair -- the time of the CALL on
    the stream: its allocation, the initialisation of the records, the kernel, the read-back of 32 bytes per tile and plane;
  - dswx_batch_checksum called once on EACH batch over the same planes: two launches that move the same bytes;
  - their ratio.  The compare's bytes are those of both planes of every pair.

    python tools/compare_rate.py [--tiles 256] [--reps 10] [--out profiles/compare_rate.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi            # noqa: E402
from proteus_amd.synth import SEED       # noqa: E402

PEAK = 8000.0           # GB/s, MI355X HBM3E


def timed(ctx, fn, reps):
    fn()
    ctx.synchronize()
    ms = []
    for _ in range(reps):
        a, b = ctx.event(), ctx.event()
        ctx.record(a)
        fn()
        ctx.record(b)
        ctx.synchronize()
        ms.append(ctx.elapsed_ms(a, b))
        ctx.destroy_event(a)
        ctx.destroy_event(b)
    return sorted(ms)


def row(nbytes, ms, **extra):
    med = ms[len(ms) // 2]
    return dict(extra, bytes=int(nbytes), ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                GBps_median=round(nbytes / med / 1e6, 1), GBps_best=round(nbytes / ms[0] / 1e6, 1),
                frac_of_hbm_peak_median=round(nbytes / med / 1e6 / PEAK, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join('profiles', 'compare_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    ba = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    bb = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    q = _capi.make_params({**{k: getattr(p, k) for k in _capi.THRESHOLD_NAMES}, 'wigt': 0.2, 'pswt_1_nir': 1400.0})
    for b in (ba, bb):
        b.synth(SEED)
        b.classify(p)
    ctx.synchronize()
    px = a.tiles * a.size * a.size
    names = ba.plane_names()
    inputs, layers = names[:7], names[7:]
    width = {n: 2 if n in _capi.BAND_NAMES or n == 'diag' else 1 for n in names}
    nbytes = lambda ns: 2 * px * sum(width[n] for n in ns)                               # noqa: E731  (both batches)
    out = {'tool': 'tools/compare_rate.py', 'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': ba.tile_stride,
           'reps': a.reps, 'hbm_peak_GBps': PEAK}

    def compare_call(ns, **tol):
        ms = timed(ctx, lambda: ba.compare(bb, names=ns, **tol), a.reps)
        rec = ba.compare(bb, names=ns, **tol)
        return row(nbytes(ns), ms, planes=len(ns), kernel=ctx.last_kernel_info(),
                   pairs_not_close=int(sum(int(r['n_diff'].sum()) for r in rec.values())))

    def checksum_pair(ns):
        def fn():
            ba.checksums(names=ns)
            bb.checksums(names=ns)
        return row(nbytes(ns), timed(ctx, fn, a.reps), planes=len(ns), kernel=ctx.last_kernel_info())
    out['checksum_pair_7_output_planes'] = checksum_pair(layers)
    out['checksum_pair_7_input_planes'] = checksum_pair(inputs)
    out['batch_compare_7_input_planes'] = compare_call(inputs)
    out['identical_layers'] = {'batch_compare_7_output_planes': compare_call(layers)}
    bb.classify(q)
    ctx.synchronize()
    out['other_thresholds'] = {'batch_compare_7_output_planes': compare_call(layers),
                               'batch_compare_7_output_planes_atol_1': compare_call(layers, atol=1.0)}
    out['checksum_pair_7_output_planes_again'] = checksum_pair(layers)
    ref_out = max(out['checksum_pair_7_output_planes']['GBps_median'], out['checksum_pair_7_output_planes_again']['GBps_median'])
    out['ratio_compare_to_checksum_pair'] = {
        '7 input planes': round(out['batch_compare_7_input_planes']['GBps_median'] / out['checksum_pair_7_input_planes']['GBps_median'], 4),
        '7 output planes, identical': round(out['identical_layers']['batch_compare_7_output_planes']['GBps_median'] / ref_out, 4),
        '7 output planes, other thresholds': round(out['other_thresholds']['batch_compare_7_output_planes']['GBps_median'] / ref_out, 4),
        '7 output planes, other thresholds, atol 1': round(
            out['other_thresholds']['batch_compare_7_output_planes_atol_1']['GBps_median'] / ref_out, 4)}
    ba.free()
    bb.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
