"""The compare entries on the GPU: dswx_compare_device and dswx_batch_compare against np.isclose + argmax + max on host
copies -- every kind, tile lengths either side of every seam of the kernel (read from the constants in its source), tile
counts up to the launch split, strides and addresses of their own for the two planes, planted differences, the float
boundary set of tests/test_compare.py, a caller's stream; the batch forms; the product comparison; the C example."""
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

from proteus_amd import _capi, geotiff
from proteus_amd.compare import RECORD, compare, kind_of
from proteus_amd.synth import SEED
from tests.test_compare import KINDS, TOLERANCES, boundary_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, 'proteus_amd', 'csrc', 'dswx_compare.hip')).read()


def _const(name):
    return int(re.search(rf'constexpr int {name} = (\d+);', _SRC).group(1))


BLOCK, UNROLL, MAX_PASSES = _const('CMP_BLOCK'), _const('CMP_UNROLL'), _const('CMP_MAX_PASSES')
ROUND = BLOCK * UNROLL                 # 16-byte units of one unrolled round of a block = a block's chunk in a small launch


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def oracle(a, b, atol=0.0, rtol=0.0, equal_nan=True):
    """(n_diff, first, max_abs_diff) of one tile by np.isclose, argmax and max."""
    with np.errstate(all='ignore'):
        bad = ~np.isclose(a, b, rtol=rtol, atol=atol, equal_nan=equal_nan)
        n = int(bad.sum())
        first = int(np.argmax(bad)) if n else -1
        x, y = a[bad].astype(np.float64), b[bad].astype(np.float64)
        ok = ~(np.isnan(x) | np.isnan(y))
        mx = float(np.abs(x[ok] - y[ok]).max()) if ok.any() else 0.0
    return n, first, mx


def as_tuple(rec):
    assert int(rec['reserved']) == 0
    return int(rec['n_diff']), int(rec['first']), float(rec['max_abs_diff'])


class Pair:
    """Two planes in one device buffer, each guard | plane at its own element offset past a 256-byte boundary | guard, with
    its own stride; every byte that is not tile data is poison, a different one in each plane."""
    GUARD = 512

    def __init__(self, ctx, a_tiles, b_tiles, sa=None, sb=None, offa=1, offb=3, buf=None):
        self.ctx, self.dt = ctx, a_tiles[0].dtype
        eb = self.dt.itemsize
        self.n, self.T = a_tiles[0].size, len(a_tiles)
        self.sa, self.sb = (self.n if sa is None else sa), (self.n if sb is None else sb)
        self.a_tiles, self.b_tiles = a_tiles, b_tiles

        def lay(tiles, stride, off, poison, base):
            span = ((self.T - 1) * stride + self.n) * eb
            host = np.full(self.GUARD + off * eb + span + self.GUARD, poison, dtype=np.uint8)
            start = self.GUARD + off * eb
            for t, d in enumerate(tiles):
                at = start + t * stride * eb
                host[at:at + self.n * eb] = d.view(np.uint8)
            return host, base + start
        ha, self.a_at = lay(a_tiles, self.sa, offa, 0xA5, 0)
        b_base = -(-ha.size // 256) * 256
        hb, self.b_at = lay(b_tiles, self.sb, offb, 0x5A, b_base)
        self.out_at = -(-(b_base + hb.size) // 256) * 256
        need = self.out_at + 32 * max(self.T, 1)
        self.own = buf is None
        self.buf = ctx.malloc(need) if buf is None else buf
        assert self.buf.nbytes >= need and self.buf.ptr % 256 == 0
        self.buf.upload(ha, 0)
        self.buf.upload(hb, b_base)
        self.buf.upload(np.full(4 * max(self.T, 1), 0x1111111111111111, dtype=np.uint64), self.out_at)   # stale records

    def run(self, atol=0.0, rtol=0.0, equal_nan=True, stream=None, same_pointer=False):
        p = self.buf.ptr
        self.ctx.compare_device(p + self.a_at, p + (self.a_at if same_pointer else self.b_at), kind_of(self.dt), self.T, self.n,
                                p + self.out_at, a_stride=self.sa, b_stride=self.sa if same_pointer else self.sb, atol=atol, rtol=rtol,
                                equal_nan=equal_nan, stream=stream)

    def records(self):
        return self.buf.download(RECORD, self.T, self.out_at)

    def check(self, atol=0.0, rtol=0.0, equal_nan=True, note=()):
        self.run(atol, rtol, equal_nan)
        self.ctx.synchronize()
        got = [as_tuple(r) for r in self.records()]
        want = [oracle(a, b, atol, rtol, equal_nan) for a, b in zip(self.a_tiles, self.b_tiles)]
        assert got == want, (self.dt, self.n, self.T, atol, rtol, equal_nan, note, got[:3], want[:3])
        return got

    def free(self):
        if self.own:
            self.buf.free()


def _random(dt, n, rng):
    dt = np.dtype(dt)
    if dt.kind == 'f':
        a = (rng.normal(size=n) * 1000).astype(dt)
        if n:
            a[rng.integers(0, n, size=n // 50 + 1)] = np.nan
            a[rng.integers(0, n, size=n // 90 + 1)] = np.inf
        return a
    return rng.integers(np.iinfo(dt).min, np.iinfo(dt).max + 1, size=n).astype(dt)


def _plant(a, idx):
    """A copy of `a` whose elements `idx` are another value (by more than any tolerance used here, never NaN)."""
    b = a.copy()
    if len(idx):
        idx = np.asarray(idx)
        if a.dtype.kind == 'f':
            b[idx] = np.where(np.isfinite(a[idx]), a[idx] + a.dtype.type(100), a.dtype.type(7))
        else:
            b[idx] = a[idx] ^ a.dtype.type(64)
    return b


def seam_sizes(eb):
    """Tile lengths in elements: 0, 1, 15, 16, 17 bytes-worth, and one block pass / one unrolled round (= a block's chunk in a
    small launch) / two rounds, each - 1, + 0 and + 1 unit, without and with elements behind the last whole unit."""
    sizes = {0, 1, 15 // eb, 16 // eb, 16 // eb + 1, 17 // eb}
    for units in (BLOCK, ROUND, 2 * ROUND):
        for u in (units - 1, units, units + 1):
            sizes.add(u * 16 // eb)
            sizes.add(u * 16 // eb + 1)
            sizes.add((u * 16 + 15) // eb)
    return sorted(sizes)


@pytest.mark.parametrize('dtype', KINDS, ids=lambda d: np.dtype(d).name)
def test_every_seam_count_stride_address_and_planted_difference(ctx, dtype):
    dt = np.dtype(dtype)
    eb = dt.itemsize
    rng = np.random.default_rng(8201 + eb)
    epu = 16 // eb
    buf = ctx.malloc(2 * (4 * Pair.GUARD + 3 * (2 * ROUND + 8) * 16 + 4096) + 4096)
    cases = 0
    for n in seam_sizes(eb):
        for T in (1, 3):
            a = [_random(dt, n, rng) for _ in range(T)]
            tail0 = n // epu * epu                                         # first element behind the last whole unit
            patterns = {'none': [[]] * T, 'index 0': [[0]] * T, 'last': [[n - 1]] * T,
                        'trailing': [list(range(tail0, n))] * T,
                        'several tiles': [[(7 * t + 3) % n, n - 1 - t] if t != 1 else [] for t in range(T)] if n > 3 else None,
                        'many': [sorted(set(rng.integers(0, n, size=n // 3 + 1).tolist())) for _ in range(T)] if n else None}
            for name, idx in patterns.items():
                if idx is None or (n == 0 and name != 'none') or (name == 'trailing' and tail0 == n):
                    continue
                b = [_plant(a[t], idx[t]) for t in range(T)]
                p = Pair(ctx, a, b, sa=n + 3, sb=n + 8, offa=1 + cases % 3, offb=3 + cases % 5, buf=buf)
                got = p.check(note=name)
                if name == 'many':
                    assert [g[0] for g in got] == [len(i) for i in idx]          # the count is exact
                    p.check(atol=2.5, rtol=0.01, note=name)
                    p.check(equal_nan=False, note=name)
                if name == 'none' and n:
                    assert got == [(0, -1, 0.0)] * T
                    nans = [int(np.isnan(t.astype(np.float64)).sum()) for t in a]
                    p.run(equal_nan=False, same_pointer=True)                   # a == b: only NaN pairs can differ
                    ctx.synchronize()
                    assert [int(r['n_diff']) for r in p.records()] == nans
                cases += 1
    assert cases > 150
    assert 'dswx_compare_k' in ctx.last_kernel_info() and f'passes={UNROLL}' in ctx.last_kernel_info()
    buf.free()


def test_a_blocks_chunk_in_a_large_launch(ctx):
    """Enough blocks that the launch keeps more than one round per block (passes = 2 UNROLL): tiles one unit and one
    element longer than a block's chunk, differences planted either side of the chunk's end and behind the last unit."""
    passes = 2 * UNROLL
    assert passes <= MAX_PASSES
    chunk = passes * BLOCK * 2                                             # float64 elements of a block's chunk
    n, T = chunk + 2 + 1, 16384 // 2 + 8
    rng = np.random.default_rng(8202)
    a = rng.normal(size=(T, n))
    b = a.copy()
    planted = {0: [chunk - 1], 1: [chunk], 2: [chunk + 1], 3: [chunk + 2], 5: [chunk - 2, chunk + 2], T - 1: [0, chunk - 1, chunk, n - 1],
               T // 2: list(range(chunk - 40, n))}
    for t, idx in planted.items():
        b[t, idx] += 1.0 + np.arange(len(idx))
    p = Pair(ctx, list(a), list(b), sa=n + 1, sb=n + 5, offa=1, offb=3)
    p.run(atol=1e-6, rtol=1e-5)
    ctx.synchronize()
    assert f'passes={passes}' in ctx.last_kernel_info() and f'grid=(2,{T},1)' in ctx.last_kernel_info(), ctx.last_kernel_info()
    got = p.records()
    with np.errstate(all='ignore'):
        bad = ~np.isclose(a, b, rtol=1e-5, atol=1e-6, equal_nan=True)
    assert np.array_equal(got['n_diff'], bad.sum(axis=1))
    assert np.array_equal(got['first'], np.where(bad.any(axis=1), bad.argmax(axis=1), -1))
    assert np.array_equal(got['max_abs_diff'], np.where(bad, np.abs(a - b), 0.0).max(axis=1))
    assert sorted(np.flatnonzero(got['n_diff']).tolist()) == sorted(planted) and not got['reserved'].any()
    p.free()


def test_65537_one_element_tiles_cross_the_launch_split(ctx):
    T = 65537
    rng = np.random.default_rng(8203)
    a = rng.integers(0, 256, size=T).astype(np.uint8)
    b = a.copy()
    changed = [0, 1, 65534, 65535, 65536, 40000]
    b[changed] ^= 0x10
    p = Pair(ctx, list(a.reshape(T, 1)), list(b.reshape(T, 1)), sa=2, sb=3, offa=1, offb=5)
    p.run()
    ctx.synchronize()
    got = p.records()
    want = np.zeros(T, dtype=RECORD)
    want['first'] = -1
    want['n_diff'][changed], want['first'][changed], want['max_abs_diff'][changed] = 1, 0, 16.0
    assert np.array_equal(got, want)
    assert oracle(a[65536:], b[65536:]) == as_tuple(got[65536])
    p.free()


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_float_boundaries_through_the_device(ctx, dtype):
    """The boundary / NaN / infinity / denormal set of the CPU test: float32 arithmetic on the device is numpy's."""
    rng = np.random.default_rng(8101)
    for atol, rtol in TOLERANCES:
        a, b = boundary_pairs(dtype, atol, rtol, rng)
        p = Pair(ctx, [a, b], [b, a], sa=a.size + 1, sb=a.size + 2)
        for equal_nan in (True, False):
            got = p.check(atol, rtol, equal_nan)
            assert got[0] == as_tuple(compare(a, b, atol, rtol, equal_nan)) == as_tuple(_capi.compare_host(a, b, atol, rtol, equal_nan))
        p.free()


def test_on_a_callers_stream_beside_a_classify_on_the_contexts_stream(ctx):
    """Asynchronous on the caller's stream with no synchronisation inside: the stream is held, a copy that REPLACES plane b is
    queued on it, then the entry -- it returns while the hold is pending and its records are those of the replaced plane --
    while a classification runs on the context's stream; neither disturbs the other (no scratch of the context)."""
    torch = pytest.importorskip('torch')
    rng = np.random.default_rng(8204)
    n, T, sa, sb = 300 * 257, 5, 300 * 257 + 5, 300 * 257 + 11
    a = rng.integers(-3000, 3000, size=T * sa).astype(np.int16)
    old = rng.integers(-3000, 3000, size=T * sb).astype(np.int16)
    new = old.copy()
    for t in range(T):
        new[t * sb:t * sb + n] = a[t * sa:t * sa + n]
    new[2 * sb + 77] += 9
    new[4 * sb + n - 1] -= 4
    da, db, dnew = (torch.from_numpy(v.copy()).to('cuda:0') for v in (a, old, new))
    out = torch.zeros((T, 4), dtype=torch.int64, device='cuda:0')
    batch = _capi.DeviceBatch(ctx, 4, 400, 300)
    params = _capi.default_params()
    try:
        batch.synth(SEED)
        batch.classify(params)
        before = batch.checksums()
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=0)
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(1.2e9))                       # some hundreds of milliseconds at any shader clock
            held = torch.cuda.Event()
            held.record(s)
            db.copy_(dnew)
        batch.classify(params)                                  # on the context's stream, not held
        t0 = time.perf_counter()
        ctx.compare_device(da.data_ptr(), db.data_ptr(), _capi.CMP_I16, T, n, out.data_ptr(), a_stride=sa, b_stride=sb,
                           atol=2.0, stream=s.cuda_stream)
        dt = time.perf_counter() - t0
        assert not held.query(), f'the entry took {dt * 1e3:.1f} ms on the host: it waited for the stream'
        ctx.synchronize(s.cuda_stream)
        ctx.synchronize()
        got = out.cpu().numpy().view(RECORD).reshape(T)
        want = [oracle(a[t * sa:t * sa + n], new[t * sb:t * sb + n], atol=2.0) for t in range(T)]
        assert [as_tuple(r) for r in got] == want and [w[0] for w in want] == [0, 0, 1, 0, 1]
        after = batch.checksums()
        assert all(np.array_equal(after[k], before[k]) for k in before)
    finally:
        batch.free()


def _batch_oracle(ba, bb, names, n_tiles, **tol):
    return {n: [oracle(ba.read_tile(n, t).ravel(), bb.read_tile(n, t).ravel(), **tol) for t in range(n_tiles)] for n in names}


@pytest.mark.parametrize('n_tiles,h,w', [(3, 64, 64), (2, 100, 37)], ids=['3x64x64', '2x100x37'])
def test_batch_compare(ctx, n_tiles, h, w):
    kw = dict(masks=True, extra_layers=('wtr1_aerosol', 'browse'))
    p = _capi.default_params()
    q = _capi.make_params({**{k: getattr(p, k) for k in _capi.THRESHOLD_NAMES}, 'wigt': 0.2, 'pswt_1_nir': 1400.0, 'awgt': 0.05})
    a = _capi.DeviceBatch(ctx, n_tiles, h, w, tile_align=1280, **kw)                   # padded stride (64 x 64 is a multiple of 256), packed
    same = _capi.DeviceBatch(ctx, n_tiles, h, w, tile_align=1, **kw)                   # contiguous tiles
    other = _capi.DeviceBatch(ctx, n_tiles, h, w, tile_align=1, separate_outputs=True, **kw)
    plain = _capi.DeviceBatch(ctx, n_tiles, h, w)                                      # no masks, no extra layers
    wide = _capi.DeviceBatch(ctx, n_tiles, h, w + 1, **kw)
    try:
        for b in (a, same, other, plain):
            b.synth(SEED, tile0=11)
        a.classify(p)
        same.classify(p)
        other.classify(q)
        plain.classify(p)
        names = a.plane_names()
        assert len(names) == 10 + 9 and a.tile_stride != same.tile_stride
        # same seed and parameters, padded against contiguous: all zero
        rec = a.compare(same)
        assert 'dswx_compare_k' in ctx.last_kernel_info() and f',{n_tiles},{len(names)})' in ctx.last_kernel_info()
        assert list(rec) == names
        for n in names:
            assert rec[n].dtype == RECORD and [as_tuple(r) for r in rec[n]] == [(0, -1, 0.0)] * n_tiles, n
        # different thresholds, packed + padded against separate outputs + contiguous: the numpy statement on downloads
        for tol in ({}, {'atol': 1.0}, {'atol': 0.5, 'rtol': 0.25}):
            rec = a.compare(other, **tol)
            want = _batch_oracle(a, other, names, n_tiles, **tol)
            for n in names:
                assert [as_tuple(r) for r in rec[n]] == want[n], (n, tol)
                assert [as_tuple(r) for r in rec[n]] == [as_tuple(compare(a.read_tile(n, t), other.read_tile(n, t), **tol))
                                                         for t in range(n_tiles)]
        assert sum(int(rec_n['n_diff'].sum()) for rec_n in a.compare(other).values()) > 0
        assert all(int(a.compare(other)[n]['n_diff'].sum()) == 0 for n in names[:10])     # the inputs are the same tiles
        # a few planes, from tile0 > 0; a batch against itself
        part = other.compare(a, names=['wtr', 'diag', 'nir'], tile0=1, n_tiles=n_tiles - 1)
        assert list(part) == ['nir', 'diag', 'wtr']
        for n in part:
            assert [as_tuple(r) for r in part[n]] == [oracle(other.read_tile(n, t).ravel(), a.read_tile(n, t).ravel())
                                                      for t in range(1, n_tiles)]
        assert all(not r['n_diff'].any() for r in a.compare(a).values())
        assert a.compare(same, names=['wtr'], tile0=n_tiles)['wtr'].shape == (0,)
        # what is refused
        for x, y in ((a, plain), (plain, a)):
            with pytest.raises(_capi.DswxError, match='browse') as e:
                x.compare(y, names=['wtr', 'browse'])
            assert e.value.code == _capi.ERR_ARG
        assert [as_tuple(r) for r in plain.compare(a, names=['wtr'])['wtr']] == _batch_oracle(plain, a, ['wtr'], n_tiles)['wtr']
        with pytest.raises(_capi.DswxError, match='checksums') as e:
            a.compare(same, names=['wtr', 'counters'])
        assert e.value.code == _capi.ERR_ARG
        with pytest.raises(_capi.DswxError, match='tile size') as e:
            a.compare(wide, names=['wtr'])
        assert e.value.code == _capi.ERR_ARG
        for bad in ((0, n_tiles + 1), (-1, 1), (n_tiles + 1, 0)):
            with pytest.raises(_capi.DswxError):
                a.compare(same, names=['wtr'], tile0=bad[0], n_tiles=bad[1])
        with pytest.raises(_capi.DswxError):
            a.compare(same, names=['wtr'], atol=-1.0)
    finally:
        for b in (a, same, other, plain, wide):
            b.free()


def test_device_plane_compare(ctx):
    from proteus_amd.pipeline import TileEngine
    eng = TileEngine(ctx)
    rng = np.random.default_rng(8205)
    for dt in KINDS:
        x = _random(dt, 3 * 211 * 97, rng).reshape(3, 211, 97)
        y = x.copy()
        y[1].reshape(-1)[[5, 4000]] = _plant(x[1].reshape(-1), [5, 4000])[[5, 4000]]
        px, py = eng.upload(x), eng.upload(y)
        got = px.compare(py, atol=1e-6, rtol=1e-5)
        assert [as_tuple(r) for r in got] == [oracle(x[t].ravel(), y[t].ravel(), 1e-6, 1e-5) for t in range(3)]
        assert px.element(211 * 97 + 5) == x[1].reshape(-1)[5] or np.isnan(px.element(211 * 97 + 5))
        one, two = eng.upload(x[1]), eng.upload(y[1])
        assert as_tuple(one.compare(two)[0]) == oracle(x[1].ravel(), y[1].ravel())
        for p in (px, py, one, two):
            p.release()
    eng.close()


def _product(path, array, **kw):
    geotiff.write_geotiff(str(path), array, metadata={'PRODUCT': 'DSWx-HLS', 'SPACECRAFT_NAME': 'test'},
                          descriptions=[f'layer {k}' for k in range(1 if array.ndim == 2 else array.shape[0])],
                          geo_tags=geotiff.geo_tags_from_geotransform((500000.0, 30.0, 0.0, 4000000.0, 0.0, -30.0), 32611), **kw)


@pytest.mark.parametrize('kind', ['u8 classes', 'float32', 'float32 with NaN nodata'])
def test_product_compare_on_the_device_prints_what_the_host_path_prints(ctx, kind, tmp_path, capsys):
    from proteus_amd.dswx_hls import compare_dswx_hls_products
    rng = np.random.default_rng(8206)
    H, W = 70, 53
    if kind == 'u8 classes':
        base = rng.choice(np.array([0, 1, 2, 252, 253, 254, 255], dtype=np.uint8), size=(2, H, W))
        kw = {'nodata': 255}
    else:
        base = (rng.normal(size=(2, H, W)) * 50).astype(np.float32)
        kw = {}
        if 'NaN' in kind:
            base[:, :9, :] = np.nan
            base[1, 20:30, 40:] = np.nan
            kw = {'nodata': float('nan')}
        base[1, 50, 50] = np.float32(5e-7)
    cases = {'identical': base.copy()}
    one = base.copy()
    one[1, 33, 17] = one[1, 33, 17] + 3 if kind != 'u8 classes' else (1 if base[1, 33, 17] != 1 else 2)
    cases['one differing pixel' if kind == 'u8 classes' else 'a float difference outside the tolerance'] = one
    if kind != 'u8 classes':
        inside = base.copy()
        inside[0, 40, 5] = np.nextafter(inside[0, 40, 5], np.float32(np.inf))      # one float32 ulp: inside rtol |y|
        inside[1, 50, 50] = np.float32(0.0)                                         # |diff| = 5e-7 below atol, y = 0
        cases['a float difference inside the tolerance'] = inside
    cases['a different band count'] = base[:1].copy()
    _product(tmp_path / 'base.tif', base, **kw)
    for name, arr in cases.items():
        path = tmp_path / (name.replace(' ', '_') + '.tif')
        _product(path, arr, **kw)
        capsys.readouterr()
        host = compare_dswx_hls_products(str(tmp_path / 'base.tif'), str(path))
        host_text = capsys.readouterr().out
        dev = compare_dswx_hls_products(str(tmp_path / 'base.tif'), str(path), device=0)
        dev_text = capsys.readouterr().out
        assert dev_text == host_text, name
        assert dev == host == (name in ('identical', 'a float difference inside the tolerance')), name
        if name in ('one differing pixel', 'a float difference outside the tolerance'):
            assert '(x: 17, y: 33)' in dev_text and '[FAIL]      Band 2' in dev_text and '[OK]        Band 1' in dev_text
    # the command-line tool takes the device
    import importlib.util
    spec = importlib.util.spec_from_file_location('dswx_compare_cli', os.path.join(ROOT, 'bin', 'dswx_compare.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.main([str(tmp_path / 'base.tif'), str(tmp_path / 'identical.tif'), '--device', '0']) == 0
    assert cli.main([str(tmp_path / 'base.tif'), str(tmp_path / 'a_different_band_count.tif'), '--device', '0']) == 1
    capsys.readouterr()


def test_compare_example_runs_and_agrees_with_the_numpy_statement(tmp_path):
    """examples/batch_compare.c: its own check (exit status 0), and n_diff / first of every layer it prints against the
    same two classifications made here."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    exe = str(tmp_path / 'batch_compare')
    lib_dir = os.path.dirname(_capi.library_path())
    subprocess.run(['gcc', '-std=c11', '-O2', '-Wall', '-Wextra', '-Werror', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'examples', 'batch_compare.c'), '-L', lib_dir, '-ldswx_hip', f'-Wl,-rpath,{lib_dir}',
                    '-o', exe], check=True)
    n_tiles, size = 3, 301
    r = subprocess.run([exe, str(n_tiles), str(size)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert 'diag: device and host records agree' in r.stdout
    got = {(m.group(1), int(m.group(2))): (int(m.group(3)), int(m.group(4)))
           for m in re.finditer(r'^compare (\w+) (\d+) n_diff (-?\d+) first (-?\d+) max \S+$', r.stdout, re.M)}
    layers = ('diag', 'wtr1', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud')
    assert len(got) == n_tiles * len(layers) and sum(v[0] for v in got.values()) > 0
    c = _capi.Context(0)
    a, b = _capi.DeviceBatch(c, n_tiles, size, size), _capi.DeviceBatch(c, n_tiles, size, size, tile_align=1)
    try:
        p = _capi.default_params()
        q = _capi.make_params({**{k: getattr(p, k) for k in _capi.THRESHOLD_NAMES}, 'wigt': 0.2, 'pswt_1_nir': 1400.0})
        for x, params in ((a, p), (b, q)):
            x.synth(20251010)
            x.classify(params)
        for name in layers:
            for t in range(n_tiles):
                assert got[(name, t)] == oracle(a.read_tile(name, t).ravel(), b.read_tile(name, t).ravel())[:2], (name, t)
    finally:
        a.free()
        b.free()
        c.close()
