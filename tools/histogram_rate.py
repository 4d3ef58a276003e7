#!/usr/bin/env python3
"""Rate of the histogram kernel (dswx_histogram.hip) against the checksum kernel, a read-only reduction over the same bytes,
in one process, with HIP events on the library's stream.  On the 256-tile 3660 x 3660 headline batch, for three contents --

  synthetic   the generated batch, classified: per-pixel noise, the hardest content for a run counter;
  scene       the spatially coherent scene of tools/make_synthetic_hls.py --scene in every tile, classified: classes in
              patches, long runs of one byte -- what a real product looks like;
  constant    every plane overwritten with one byte: every lane of every wave meets in one bin, the worst case for a
              shared counter

-- dswx_batch_histogram and dswx_batch_checksum over the seven output planes, the seven input planes and WTR alone, the
two entries alternating call by call (the time of the CALL on the stream: allocation, zeroing, kernel, read-back), and both
device entries over the seven output planes, one launch per plane queued back to back (the kernels' own rates).  Beside
them the project's read-only yardstick, dswx_stream_probe of libdswx_lab.so in its read-only mode over the input planes.
THE BAR: on each content the histogram's median rate is at least half the checksum's on the same planes.

    python tools/histogram_rate.py [--tiles 256] [--reps 10] [--out profiles/histogram_rate.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from proteus_amd import _capi            # noqa: E402
from proteus_amd.synth import SEED       # noqa: E402

PEAK = 8000.0           # GB/s, MI355X HBM3E
BAR = 0.5
CONSTANT_BYTE = 0x01    # bands 257 (inside the default band bins), DIAG 257 (bin 33), class planes 1


def timed_alternating(ctx, fns, reps):
    """{name: sorted ms}: the functions called in turn, `reps` rounds after one untimed round."""
    for fn in fns.values():
        fn()
    ctx.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = ctx.event(), ctx.event()
            ctx.record(a)
            fn()
            ctx.record(b)
            ms[k].append(ctx.elapsed_ms(a, b))
            ctx.destroy_event(a)
            ctx.destroy_event(b)
    return {k: sorted(v) for k, v in ms.items()}


def row(nbytes, ms, **extra):
    med = ms[len(ms) // 2]
    return dict(extra, bytes=int(nbytes), ms_median=round(med, 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4),
                GBps_median=round(nbytes / med / 1e6, 1), GBps_best=round(nbytes / ms[0] / 1e6, 1),
                frac_of_hbm_peak_median=round(nbytes / med / 1e6 / PEAK, 4))


def fill_scene(ctx, batch, size):
    """The coherent scene (tile 0 of the tool's recipe) into every tile of the input planes: uploaded once, copied on the device."""
    from make_synthetic_hls import scene_tile
    s = scene_tile(0, size)
    for name, arr in list(zip(_capi.BAND_NAMES, s['bands'])) + [('fmask', s['fmask'])]:
        batch.write_tile(name, 0, arr)
        ptr, dt = batch._plane(name)
        step = batch.tile_stride * np.dtype(dt).itemsize
        for t in range(1, batch.n_tiles):
            ctx.copy_2d_device(ptr + t * step, step, ptr, step, batch.n_pixels * np.dtype(dt).itemsize, 1)
    ctx.synchronize()


def fill_constant(ctx, batch, names):
    for name in names:
        ptr, dt = batch._plane(name)
        _capi._check(ctx.lib.dswx_memset_d(ctx.handle, ptr, CONSTANT_BYTE, batch.n_tiles * batch.tile_stride * np.dtype(dt).itemsize))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tiles', type=int, default=256)
    ap.add_argument('--size', type=int, default=3660)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join('profiles', 'histogram_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    p = _capi.default_params()
    px = a.tiles * a.size * a.size
    names = batch.plane_names()
    inputs, layers = names[:7], names[7:]
    width = {n: 2 if n in _capi.BAND_NAMES or n == 'diag' else 1 for n in names}
    nbytes = lambda ns: px * sum(width[n] for n in ns)                                   # noqa: E731
    out = {'tool': 'tools/histogram_rate.py', 'design': 'lane-indexed replicas: 32 sets of 256 uint32 counters per block in LDS, '
           'bank = lane & 31; one add per 16-byte unit of one value', 'tiles': a.tiles, 'tile': [a.size, a.size],
           'tile_stride': batch.tile_stride, 'reps': a.reps, 'hbm_peak_GBps': PEAK, 'bar_histogram_over_checksum': BAR,
           'constant_byte': CONSTANT_BYTE, 'contents': {}}
    scratch = ctx.malloc(8 * _capi.HIST_BINS * a.tiles * len(layers))

    def kind_of(n):
        return (_capi.HIST_DIAG, 0, 0) if n == 'diag' else (_capi.HIST_I16, 0, 6) if n in _capi.BAND_NAMES else (_capi.HIST_U8, 0, 0)

    def hist_entries(ns):
        for k, n in enumerate(ns):
            ptr, _ = batch._plane(n)
            kind, lo, shift = kind_of(n)
            ctx.histogram_device(ptr, kind, a.tiles, batch.n_pixels, scratch.ptr + 8 * _capi.HIST_BINS * a.tiles * k, lo=lo,
                                 shift=shift, tile_stride=batch.tile_stride)

    def cks_entries(ns):
        for k, n in enumerate(ns):
            ptr, dt = batch._plane(n)
            ctx.checksum_device(ptr, dt().itemsize, a.tiles, batch.n_pixels, scratch.ptr + 8 * a.tiles * k,
                                tile_stride=batch.tile_stride)

    def measure(content):
        rec = {}
        for label, ns in (('7_output_planes', layers), ('7_input_planes', inputs), ('one_plane_wtr', ['wtr'])):
            ms = timed_alternating(ctx, {'checksum': lambda: batch.checksums(names=ns), 'histogram': lambda: batch.histogram(names=ns)},
                                   a.reps)
            info = ctx.last_kernel_info()
            c, h = row(nbytes(ns), ms['checksum']), row(nbytes(ns), ms['histogram'], kernel=info)
            rec[label] = {'batch_checksum': c, 'batch_histogram': h,
                          'ratio_histogram_over_checksum': round(h['GBps_median'] / c['GBps_median'], 4)}
        ms = timed_alternating(ctx, {'checksum': lambda: cks_entries(layers), 'histogram': lambda: hist_entries(layers)}, a.reps)
        c, h = row(nbytes(layers), ms['checksum']), row(nbytes(layers), ms['histogram'])
        rec['device_entries_7_output_planes_7_launches'] = {'checksum': c, 'histogram': h,
                                                            'ratio_histogram_over_checksum': round(h['GBps_median'] / c['GBps_median'], 4)}
        rec['ratio_min'] = min(v['ratio_histogram_over_checksum'] for v in rec.values())
        rec['meets_bar'] = bool(rec['ratio_min'] >= BAR)
        hist = batch.histogram(names=['wtr'], n_tiles=1)['wtr'][0]
        rec['wtr_tile_0_bins'] = {int(b): int(hist[b]) for b in np.flatnonzero(hist)}
        out['contents'][content] = rec

    batch.synth(SEED)
    batch.classify(p)
    ctx.synchronize()
    measure('synthetic')
    # the yardstick on the bytes of the input planes: read-only mode (1 << 9) of the stream probe, its four access shapes
    probe = {}
    for ppt16 in (0, 1):
        for nt in (0, 2):
            variant = (1 << 9) | ppt16 | nt
            ms = timed_alternating(ctx, {'probe': lambda: ctx.stream_probe(a.tiles, batch.n_pixels, batch.pin, batch.pout, variant,
                                                                           tile_stride=batch.tile_stride)}, a.reps)['probe']
            probe[f'ppt={16 if ppt16 else 8} nt={nt >> 1}'] = row(nbytes(inputs), ms)
    best = max(probe, key=lambda k: probe[k]['GBps_median'])
    out['read_only_probe_7_input_planes'] = dict(probe[best], shape=best, all_shapes={k: v['GBps_median'] for k, v in probe.items()})
    ref = out['read_only_probe_7_input_planes']['GBps_median']
    syn = out['contents']['synthetic']['7_input_planes']
    out['ratio_to_read_only_probe_7_input_planes_synthetic'] = {
        'dswx_batch_histogram': round(syn['batch_histogram']['GBps_median'] / ref, 4),
        'dswx_batch_checksum': round(syn['batch_checksum']['GBps_median'] / ref, 4)}

    fill_scene(ctx, batch, a.size)
    batch.classify(p)
    ctx.synchronize()
    measure('scene')
    fill_constant(ctx, batch, names)
    measure('constant')
    out['meets_bar'] = all(v['meets_bar'] for v in out['contents'].values())
    scratch.free()
    batch.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
