"""What the nine resident-batch entries refuse, in which order and in which words: dswx_batch_checksum, _compare, _histogram,
_crosstab, _stack, _grid, _label, _body_table and _distance called through the C-ABI with a NULL batch, plane indices and mask
bits either side of the table, the counters, a 2-byte band, DIAG, a plane the batch does not have, tile ranges outside the
batch, batches of different tile size and a NULL `out` -- the status code, the full text of dswx_last_error() and every
output byte still the sentinel.  The texts are written out here: they are the library's interface to the person who reads
the log, and the selection rules behind them (csrc/dswx_batch_select.h) are shared by all nine."""
import ctypes

import numpy as np
import pytest

try:                                              # before the library is loaded (test_gpu_streams.py)
    import torch                                  # noqa: F401
except ImportError:
    torch = None

from proteus_amd import _capi, bodies, crosstab, distance, grid, label, stack
from proteus_amd.checksum import checksum

pytestmark = pytest.mark.gpu

N, H, W = 3, 8, 16
ALL, MAXP, SENT = _capi.BATCH_ALL_TILES, _capi.BATCH_MAX_PLANES, 0xEE
P = _capi.PLANE_INDEX
RANGES = (((0, N + 1), 'tiles 0 .. +4 outside %s (3 resident)'), ((-1, 2), 'tiles -1 .. +2 outside %s (3 resident)'),
          ((N + 1, 0), 'tiles 4 .. +0 outside %s (3 resident)'), ((N + 1, ALL), 'tiles 4 .. +-1 outside %s (3 resident)'))
PAST = 'plane_mask 0x%x names planes past 19'
NO_LAND = 'the batch has no plane 7 (land)'
# per single-plane entry: what it says of the counters, and of a plane that is not one byte wide
PHRASES = {
    'stack': ('the counters are not stacked', 'a stack is a uint8 plane'),
    'grid': ('the counters are not gridded', 'a grid is made of a uint8 plane'),
    'label': ('the counters are not labelled', 'bodies are labelled in a uint8 plane'),
    'body_table': ('the counters are not tabulated', 'bodies are tabulated against a uint8 plane'),
    'distance': ('the counters have no distances', 'distances are measured in a uint8 plane'),
}


def test_every_batch_entry_refuses_in_the_same_words_and_writes_nothing():
    ctx = _capi.Context(0)
    lib = ctx.lib
    a = _capi.DeviceBatch(ctx, N, H, W)                                                   # no masks: `land` is absent
    full = _capi.DeviceBatch(ctx, N, H, W, extra_layers=('wtr1_aerosol', 'browse'))
    small = _capi.DeviceBatch(ctx, N, H, W // 2)
    host = np.full(1 << 16, SENT, dtype=np.uint8)                                         # `out` of the four read-back entries
    dev = ctx.malloc(1 << 16)                                                             # every output plane of the other five
    dev.upload(host)
    out = _capi._host_ptr(host)
    cases = [0]

    def refused(rc, text):
        assert rc == _capi.ERR_ARG, (rc, text, lib.dswx_last_error())
        assert lib.dswx_last_error().decode() == text
        cases[0] += 1

    def accepted(rc):
        assert rc == _capi.OK, lib.dswx_last_error()
        cases[0] += 1

    def bit(*names):
        m = 0
        for n in names:
            m |= 1 << P[n]
        return m

    # ---- checksum: the counters are a plane like any other
    cs = lambda b, mask, t0, nt, o=out: lib.dswx_batch_checksum(b, mask, t0, nt, o, None)
    refused(cs(None, bit('wtr'), 0, ALL), 'batch is NULL')
    refused(cs(a.handle, 1 << MAXP, 0, ALL), 'plane_mask 0x100000 names planes past 19')
    refused(cs(a.handle, bit('land') | 1 << MAXP, N + 1, ALL), PAST % 0x100080)
    for (t0, nt), text in RANGES:
        refused(cs(a.handle, bit('land'), t0, nt), text % 'the batch')                    # the range before the planes
    refused(cs(a.handle, bit('blue', 'land'), 0, ALL), NO_LAND)
    refused(cs(a.handle, bit('land'), 0, 0), NO_LAND)                                     # an empty range still names real planes
    refused(cs(a.handle, bit('wtr1_aerosol'), 0, ALL), 'the batch has no plane 12 (wtr1_aerosol)')
    refused(cs(a.handle, bit('browse'), 1, 1), 'the batch has no plane 18 (browse)')
    accepted(cs(a.handle, 0, 0, ALL, None))
    accepted(cs(a.handle, bit('blue'), N, ALL, None))
    accepted(cs(a.handle, bit('blue'), 1, 0, None))
    refused(cs(a.handle, bit('blue'), 0, ALL, None), 'out is NULL')
    assert np.all(host == SENT)
    got = np.zeros((3, 2), dtype=np.uint64)
    accepted(cs(full.handle, bit('blue', 'diag', 'counters'), 1, ALL, _capi._host_ptr(got)))
    counters = full.read_counters()
    for i, t in enumerate((1, 2)):
        assert got[:, i].tolist() == [checksum(full.read_tile('blue', t)), checksum(full.read_tile('diag', t)), checksum(counters[t])]

    # ---- compare
    cmp_ = lambda x, y, mask, t0, nt, o=out, atol=0.0: lib.dswx_batch_compare(x, y, mask, t0, nt, atol, 0.0, 1, o, None)
    not_compared = ('the counters are not compared here (24 bytes per tile): compare their checksums instead '
                    '(dswx_batch_checksum with DSWX_PLANE_COUNTERS)')
    refused(cmp_(None, a.handle, bit('wtr'), 0, ALL), 'batch is NULL')
    refused(cmp_(a.handle, None, bit('wtr'), 0, ALL), 'batch is NULL')
    refused(cmp_(a.handle, small.handle, 1 << MAXP | bit('counters'), 0, ALL), PAST % 0x180000)
    refused(cmp_(a.handle, small.handle, bit('counters', 'wtr'), 0, ALL), not_compared)
    refused(cmp_(a.handle, small.handle, bit('wtr'), 0, ALL, atol=-1.0), 'the batches differ in tile size: 8 x 16 against 8 x 8')
    refused(cmp_(small.handle, a.handle, bit('wtr'), 0, ALL), 'the batches differ in tile size: 8 x 8 against 8 x 16')
    refused(cmp_(a.handle, full.handle, bit('land'), N + 1, 0, atol=-1.0), 'atol and rtol must be finite and not negative (atol -1, rtol 0)')
    for (t0, nt), text in RANGES:
        refused(cmp_(a.handle, full.handle, bit('land'), t0, nt), text % 'a batch')
    refused(cmp_(a.handle, full.handle, bit('blue', 'land'), 0, ALL), 'batch a (nor b) has no plane 7 (land)')
    refused(cmp_(a.handle, full.handle, bit('wtr1_aerosol'), 0, 0), 'batch a has no plane 12 (wtr1_aerosol)')
    refused(cmp_(full.handle, a.handle, bit('wtr', 'browse'), 0, ALL), 'batch b has no plane 18 (browse)')
    accepted(cmp_(a.handle, full.handle, 0, 0, ALL, None))
    accepted(cmp_(a.handle, full.handle, bit('blue'), N, ALL, None))
    refused(cmp_(a.handle, full.handle, bit('blue'), 0, ALL, None), 'out is NULL')
    assert np.all(host == SENT)
    from proteus_amd.compare import RECORD
    rec = np.zeros((2, N), dtype=RECORD)
    rec['n_diff'] = -1
    accepted(cmp_(full.handle, full.handle, bit('blue', 'diag'), 0, ALL, _capi._host_ptr(rec)))
    assert np.all(rec['n_diff'] == 0)

    # ---- histogram
    hist = lambda b, mask, t0, nt, o=out, shift=6: lib.dswx_batch_histogram(b, mask, t0, nt, 0, shift, o, None)
    refused(hist(None, bit('wtr'), 0, ALL), 'batch is NULL')
    refused(hist(a.handle, 1 << MAXP | bit('counters'), 0, ALL), PAST % 0x180000)
    refused(hist(a.handle, bit('counters', 'land'), N + 1, ALL, shift=9),
            'the counters are not histogrammed (three int64 per tile): read them (dswx_batch_planes)')
    refused(hist(a.handle, bit('land'), N + 1, ALL, shift=9), 'shift 9 outside 0 .. 8')
    for (t0, nt), text in RANGES:
        refused(hist(a.handle, bit('land'), t0, nt), text % 'the batch')
    refused(hist(a.handle, bit('blue', 'land'), 0, ALL), NO_LAND)
    refused(hist(a.handle, bit('land'), 2, 0), NO_LAND)
    accepted(hist(a.handle, 0, 0, ALL, None))
    accepted(hist(a.handle, bit('blue'), 1, 0, None))
    refused(hist(a.handle, bit('blue'), 0, ALL, None), 'out is NULL')
    assert np.all(host == SENT)
    bins = np.zeros((2, 1, _capi.HIST_BINS), dtype=np.uint64)
    accepted(hist(a.handle, bit('blue', 'diag'), 2, 1, _capi._host_ptr(bins)))
    assert np.array_equal(bins[0, 0], _capi.histogram_host(a.read_tile('blue', 2), _capi.HIST_I16, 0, 6))
    assert np.array_equal(bins[1, 0], _capi.histogram_host(a.read_tile('diag', 2), _capi.HIST_DIAG))

    # ---- crosstab: plane indices in pairs
    def xt(x, y, planes, t0, nt, o=out, kind=_capi.HIST_U8, n_pairs=None, col_bits=4):
        arr = (_capi.CrosstabPair * max(len(planes), 1))()
        for k, (pa, pb) in enumerate(planes):
            arr[k].plane_a, arr[k].plane_b = pa, pb
            arr[k].spec = _capi.CrosstabSpec.of(crosstab.Spec(a_kind=kind, a_shift=6 if kind == _capi.HIST_I16 else 0))
            arr[k].spec.col_bits = col_bits
        return lib.dswx_batch_crosstab(x, y, arr, len(planes) if n_pairs is None else n_pairs, t0, nt, o, None)
    uncrossed = 'the counters are not cross-tabulated (three int64 per tile): read them (dswx_batch_planes)'
    wf = (P['wtr'], P['fmask'])
    refused(xt(None, a.handle, [wf], 0, ALL), 'batch is NULL')
    refused(xt(a.handle, None, [wf], 0, ALL), 'batch is NULL')
    refused(xt(a.handle, a.handle, [wf], 0, ALL, n_pairs=-1), '-1 pairs: 0 .. 6 per call (their tables ride in the kernel arguments)')
    refused(xt(a.handle, a.handle, [wf], 0, ALL, n_pairs=7), '7 pairs: 0 .. 6 per call (their tables ride in the kernel arguments)')
    refused(lib.dswx_batch_crosstab(a.handle, a.handle, None, 1, 0, ALL, out, None), 'pairs is NULL')
    refused(xt(a.handle, small.handle, [wf, (-1, P['fmask'])], 0, ALL), 'pair 1 names plane -1: not 0 .. 19')
    refused(xt(a.handle, small.handle, [(P['wtr'], MAXP)], 0, ALL), 'pair 0 names plane 20: not 0 .. 19')
    refused(xt(a.handle, small.handle, [(P['counters'], P['fmask'])], 0, ALL), uncrossed)
    refused(xt(a.handle, small.handle, [wf, (P['wtr'], P['counters'])], 0, ALL), uncrossed)
    refused(xt(a.handle, small.handle, [wf], 0, ALL, col_bits=9), 'the batches differ in tile size: 8 x 16 against 8 x 8')
    refused(xt(a.handle, full.handle, [(P['land'], P['fmask'])], N + 1, 0, col_bits=9), 'col_bits 9 outside 0 .. 8')
    for (t0, nt), text in RANGES:
        refused(xt(a.handle, full.handle, [(P['land'], P['fmask'])], t0, nt), text % 'a batch')
    refused(xt(a.handle, full.handle, [(P['land'], P['land'])], 0, ALL), 'batch a has no plane 7 (land)')
    refused(xt(full.handle, a.handle, [wf, (P['browse'], P['browse'])], 0, 0), 'batch b has no plane 18 (browse)')
    refused(xt(a.handle, a.handle, [(P['blue'], P['fmask'])], 0, ALL), 'pair 0: a_kind 0 does not bin plane 0 (band[0]), 2 bytes per pixel')
    refused(xt(a.handle, a.handle, [(P['diag'], P['fmask'])], 0, ALL), 'pair 0: a_kind 0 does not bin plane 10 (diag), 2 bytes per pixel')
    refused(xt(a.handle, a.handle, [(P['wtr'], P['blue'])], 0, ALL), 'pair 0: plane b must be a uint8 plane, plane 0 (band[0]) has 2 bytes per pixel')
    refused(xt(a.handle, a.handle, [wf, (P['wtr'], P['diag'])], 0, ALL), 'pair 1: plane b must be a uint8 plane, plane 10 (diag) has 2 bytes per pixel')
    accepted(xt(a.handle, a.handle, [], 0, ALL, None))
    accepted(xt(a.handle, a.handle, [wf], N, ALL, None))
    refused(xt(a.handle, a.handle, [wf], 0, ALL, None), 'out is NULL')
    assert np.all(host == SENT)
    cells = np.zeros((1, 1, _capi.CROSSTAB_CELLS), dtype=np.uint64)
    accepted(xt(a.handle, full.handle, [(P['blue'], P['fmask'])], 1, 1, _capi._host_ptr(cells), kind=_capi.HIST_I16))
    assert np.array_equal(cells[0, 0], _capi.crosstab_host(a.read_tile('blue', 1), full.read_tile('fmask', 1),
                                                           crosstab.Spec(a_kind=_capi.HIST_I16, a_shift=6)))

    # ---- the five entries that take one uint8 plane by its index
    zeros, ones = np.zeros(256, dtype=np.uint8), np.ones(256, dtype=np.uint8)
    specs = {'stack': _capi.StackSpec.of(stack.Spec(1, zeros)), 'grid': _capi.GridSpec.of(grid.Spec(1, 4, 4, zeros)),
             'label': _capi.LabelSpec.of(label.Spec(8, 1, ones)), 'body_table': _capi.BodySpec.of(bodies.Spec(1, zeros, 0)),
             'distance': _capi.DistanceSpec.of(distance.Spec(ones))}
    outs = {'stack': _capi.StackOut.of(count=[dev.ptr], last=dev.ptr, last_index=dev.ptr, share=dev.ptr),
            'grid': _capi.GridOut.of(count=[dev.ptr], share=dev.ptr, coverage=dev.ptr, major=dev.ptr),
            'label': _capi.LabelOut.of(label=dev.ptr, size=dev.ptr, sieved=dev.ptr, summary=dev.ptr),
            'body_table': _capi.BodyOut.of(dense=dev.ptr, head=dev.ptr),
            'distance': _capi.DistanceOut.of(dist2=dev.ptr, nearest=dev.ptr, summary=dev.ptr)}
    for entry, (no_counters, one_byte) in PHRASES.items():
        fn = getattr(lib, f'dswx_batch_{entry}')
        if entry == 'body_table':
            call = lambda b, plane, t0, nt: fn(b, plane, ctypes.byref(specs[entry]), t0, nt, ctypes.c_void_p(dev.ptr),
                                               ctypes.byref(outs[entry]), None)
        else:
            call = lambda b, plane, t0, nt: fn(b, plane, ctypes.byref(specs[entry]), t0, nt, ctypes.byref(outs[entry]), None)
        lowest = -1 if entry == 'body_table' else 0
        refused(call(None, P['wtr'], 0, ALL), 'batch is NULL')
        refused(call(a.handle, lowest - 1, N + 1, ALL), f'plane {lowest - 1}: not {lowest} .. 19')
        refused(call(a.handle, MAXP, N + 1, ALL), f'plane 20: not {lowest} .. 19')
        refused(call(a.handle, P['counters'], N + 1, ALL), f'{no_counters} (three int64 per tile): read them (dswx_batch_planes)')
        refused(call(a.handle, P['blue'], N + 1, ALL), f'{one_byte}, plane 0 (band[0]) has 2 bytes per pixel')
        refused(call(a.handle, P['diag'], N + 1, ALL), f'{one_byte}, plane 10 (diag) has 2 bytes per pixel')
        refused(call(a.handle, P['land'], N + 1, ALL), NO_LAND)
        refused(call(a.handle, P['browse'], 0, 0), 'the batch has no plane 18 (browse)')
        for (t0, nt), text in RANGES:
            refused(call(a.handle, P['wtr'], t0, nt), text % 'the batch')
        if entry == 'body_table':                                                         # "no value plane" has a range too
            refused(call(a.handle, -1, N + 1, ALL), RANGES[3][1] % 'the batch')
    ctx.synchronize()
    assert np.all(dev.download(np.uint8, dev.nbytes) == SENT)
    assert cases[0] == 134
    for b in (a, full, small):
        b.free()
    dev.free()
    ctx.close()
