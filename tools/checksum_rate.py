#!/usr/bin/env python3
"""Rate of the checksum kernel (dswx_checksum.hip) against the project's read-only yardstick, in one process, with HIP
events on the library's stream.  On the 256-tile 3660 x 3660 headline batch:

  - dswx_batch_checksum over the seven output planes (27.4 GB), over all fourteen planes, and over one plane alone --
    the time of the CALL on the stream: its allocation, the zeroing, the kernel, the read-back of 8 bytes per tile and plane;
  - the same planes through dswx_checksum_device, one launch per plane queued back to back -- no host work between the
    events: the kernel's own rate;
  - 32 tiles with every plane at an odd address (each plane taken as bytes from its address + 1), next to the same planes
    at their own addresses;
  - the yardstick: dswx_stream_probe of libdswx_lab.so in its read-only mode (reads the seven input planes, 13 bytes
    per pixel, with trivial arithmetic), best of its access shapes -- on the same bytes as the input-plane checksums.

    python tools/checksum_rate.py [--tiles 256] [--reps 10] [--out profiles/checksum_rate.json]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument('--out', default=os.path.join('profiles', 'checksum_rate.json'))
    a = ap.parse_args()
    ctx = _capi.Context(0)
    batch = _capi.DeviceBatch(ctx, a.tiles, a.size, a.size)
    batch.synth(SEED)
    p = _capi.default_params()
    batch.classify(p)
    ctx.synchronize()
    px = a.tiles * a.size * a.size
    names = batch.plane_names()
    inputs, layers = names[:7], names[7:]
    width = {n: 2 if n in _capi.BAND_NAMES or n == 'diag' else 1 for n in names}
    nbytes = lambda ns: px * sum(width[n] for n in ns)                                   # noqa: E731
    out = {'tool': 'tools/checksum_rate.py', 'tiles': a.tiles, 'tile': [a.size, a.size], 'tile_stride': batch.tile_stride,
           'reps': a.reps, 'hbm_peak_GBps': PEAK}

    def call(ns):
        t0 = time.perf_counter()
        ms = timed(ctx, lambda: batch.checksums(names=ns), a.reps)
        wall = (time.perf_counter() - t0) / (a.reps + 1)
        return row(nbytes(ns), ms, planes=len(ns), kernel=ctx.last_kernel_info(), host_wall_ms_per_call=round(wall * 1e3, 3))
    out['batch_checksum_7_output_planes'] = call(layers)
    out['batch_checksum_14_planes'] = call(names)
    out['batch_checksum_7_input_planes'] = call(inputs)
    out['batch_checksum_one_plane_wtr'] = call(['wtr'])
    out['batch_checksum_one_plane_nir'] = call(['nir'])

    scratch = ctx.malloc(8 * a.tiles * len(names))

    def per_plane(ns, tiles, shift=0, as_bytes=False):
        def fn():
            for k, n in enumerate(ns):
                ptr, dt = batch._plane(n)
                eb = 1 if as_bytes else dt().itemsize
                scale = dt().itemsize // eb
                ctx.checksum_device(ptr + shift, eb, tiles, batch.n_pixels * scale, scratch.ptr + 8 * a.tiles * k,
                                    tile_stride=batch.tile_stride * scale)
        return fn
    out['device_entry_7_output_planes_7_launches'] = row(nbytes(layers), timed(ctx, per_plane(layers, a.tiles), a.reps))
    out['device_entry_7_input_planes_7_launches'] = row(nbytes(inputs), timed(ctx, per_plane(inputs, a.tiles), a.reps))
    t32 = min(32, a.tiles - 1)
    b32 = nbytes(names) * t32 // a.tiles
    out['device_entry_32_tiles_14_planes_own_addresses'] = row(b32, timed(ctx, per_plane(names, t32, 0, True), a.reps), tiles=t32)
    out['device_entry_32_tiles_14_planes_odd_addresses'] = row(b32, timed(ctx, per_plane(names, t32, 1, True), a.reps), tiles=t32)
    scratch.free()

    # the yardstick on the bytes of the input planes: read-only mode (1 << 9) of the stream probe, its four access shapes
    probe = {}
    for ppt16 in (0, 1):
        for nt in (0, 2):
            variant = (1 << 9) | ppt16 | nt
            ms = timed(ctx, lambda: ctx.stream_probe(a.tiles, batch.n_pixels, batch.pin, batch.pout, variant,
                                                     tile_stride=batch.tile_stride), a.reps)
            probe[f'ppt={16 if ppt16 else 8} nt={nt >> 1}'] = row(nbytes(inputs), ms)
    best = max(probe, key=lambda k: probe[k]['GBps_median'])
    out['read_only_probe_7_input_planes'] = dict(probe[best], shape=best, all_shapes={k: v['GBps_median'] for k, v in probe.items()})
    ref = out['read_only_probe_7_input_planes']['GBps_median']
    out['ratio_to_read_only_probe'] = {
        'same_bytes: device entry, 7 input planes': round(out['device_entry_7_input_planes_7_launches']['GBps_median'] / ref, 4),
        'same_bytes: dswx_batch_checksum, 7 input planes': round(out['batch_checksum_7_input_planes']['GBps_median'] / ref, 4),
        'device entry, 7 output planes': round(out['device_entry_7_output_planes_7_launches']['GBps_median'] / ref, 4),
        'dswx_batch_checksum, 7 output planes': round(out['batch_checksum_7_output_planes']['GBps_median'] / ref, 4),
        'dswx_batch_checksum, 14 planes': round(out['batch_checksum_14_planes']['GBps_median'] / ref, 4),
        'odd addresses / own addresses, 32 tiles': round(out['device_entry_32_tiles_14_planes_odd_addresses']['GBps_median']
                                                         / out['device_entry_32_tiles_14_planes_own_addresses']['GBps_median'], 4)}
    batch.free()
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
