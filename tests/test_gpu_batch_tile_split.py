"""The batch forms of the analytic entries on a batch of MORE tiles than one launch takes: dswx_batch_checksum, _histogram,
_crosstab and _compare run one launch per 65535 tiles with several planes in each (blockIdx.z x out_pitch together with a
shifted base and a shifted record), dswx_batch_label and dswx_batch_body_table loop over the tiles inside their kernels.
One DeviceBatch of 65535 + 9 tiles of 7 x 11 pixels with the masks, synthesised and classified once; every tile of every
call is compared -- against the numpy statements of proteus_amd/ on the downloaded planes, or against the host entries --
and each entry is called again on tiles 7 .. 7 + 65536, a range that crosses the split with its first launch at tile 7."""
import ctypes

import numpy as np
import pytest

from proteus_amd import _capi
from proteus_amd.bodies import wtr_body_spec
from proteus_amd.checksum import checksum, checksum_tiles
from proteus_amd.compare import compare
from proteus_amd.crosstab import CELLS, WTR_VALUES, Spec, cell_of, classes, crosstab
from proteus_amd.histogram import BINS, HIST_DIAG, HIST_I16, HIST_U8, bin_of, histogram
from proteus_amd.label import SUMMARY_WORDS, wtr_label_spec
from proteus_amd.synth import SEED

pytestmark = pytest.mark.gpu

SPLIT = 65535                                     # the blocks of grid.y
T, H, W = SPLIT + 9, 7, 11
EDGE_TILES = (0, 1, SPLIT - 1, SPLIT, SPLIT + 1, T - 1)
CHANGED_TILES = (0, SPLIT - 1, SPLIT, SPLIT + 1, T - 1)
SUB = (7, SPLIT + 1)                              # tile0, n_tiles: crosses the split, its first launch starts at tile 7


@pytest.fixture(scope='module')
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def make_batch(ctx):
    batch = _capi.DeviceBatch(ctx, T, H, W, masks=True)
    batch.synth(SEED, tile0=5)
    batch.classify(_capi.default_params())
    ctx.synchronize()
    return batch


@pytest.fixture(scope='module')
def batches(ctx):
    """(batch, other): two batches of one geometry and seed, `other` with ONE element of every plane changed in each of
    CHANGED_TILES; both freed afterwards."""
    batch, other = make_batch(ctx), make_batch(ctx)
    for k, name in enumerate(other.plane_names()):
        for j, t in enumerate(CHANGED_TILES):
            tile = other.read_tile(name, t)
            tile.reshape(-1)[(5 * k + 13 * j) % (H * W)] ^= 1
            other.write_tile(name, t, tile)
    yield batch, other
    other.free()
    batch.free()


@pytest.fixture(scope='module')
def planes(ctx, batches):
    """name -> [T, H * W]: every plane of `batch` downloaded whole (the padding of the tile stride cut off), on demand."""
    batch = batches[0]
    cache = {}

    def get(name):
        if name not in cache:
            ptr, dt = batch._plane(name)
            raw = np.empty((T, batch.tile_stride), dtype=dt)
            _capi._check(ctx.lib.dswx_memcpy_d2h(ctx.handle, ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(ptr), raw.nbytes))
            cache[name] = np.ascontiguousarray(raw[:, :H * W])
        return cache[name]
    return get


def test_the_batch_is_what_the_tests_below_assume(ctx, batches, planes):
    batch, other = batches
    assert batch.tile_stride == 256 and len(batch.plane_names()) == 17 and other.plane_names() == batch.plane_names()
    for name in ('wtr', 'nir', 'diag'):
        for t in EDGE_TILES:
            assert np.array_equal(planes(name)[t], batch.read_tile(name, t).reshape(-1)), (name, t)
    assert len(np.unique(planes('wtr'))) > 2 and len(np.unique(checksum_tiles(planes('nir')))) == T      # tiles differ


def test_checksums_every_plane_every_tile(ctx, batches, planes):
    batch = batches[0]
    names = batch.plane_names()
    sums = batch.checksums()
    info = ctx.last_kernel_info()
    assert 'dswx_checksum_k' in info and f',{SPLIT},{len(names)})' in info, info
    assert list(sums) == names
    for name in names:
        assert sums[name].shape == (T,)
        for t in EDGE_TILES:
            assert int(sums[name][t]) == checksum(batch.read_tile(name, t)), (name, t)
    for name in ('wtr', 'swir1', 'diag', 'fmask'):            # (a byte layer, a band, the uint16 layer, a byte input)
        want = checksum_tiles(planes(name))
        bad = np.flatnonzero(sums[name] != want)
        assert bad.size == 0, (name, bad[:4], sums[name][bad[:4]], want[bad[:4]])
    part = batch.checksums(tile0=SUB[0], n_tiles=SUB[1])
    assert list(part) == names and f',{SPLIT},{len(names)})' in ctx.last_kernel_info()
    for name in names:
        bad = np.flatnonzero(part[name] != sums[name][SUB[0]:SUB[0] + SUB[1]])
        assert part[name].shape == (SUB[1],) and bad.size == 0, (name, bad[:4])


def tiled_bincount(index, width):
    """uint64 [T, width]: per tile (row of `index`, int64 [T, n], -1 = not counted) the counts of its values."""
    flat = (index + np.arange(len(index))[:, None] * width)[index >= 0]
    return np.bincount(flat, minlength=len(index) * width).astype(np.uint64).reshape(len(index), width)


def test_histogram_three_kinds_in_one_call_every_tile(ctx, batches, planes):
    batch = batches[0]
    names = ['nir', 'fmask', 'diag', 'wtr']                   # (in the order of PLANE_INDEX)
    lo, shift = -512, 5
    hist = batch.histogram(names=names, band_lo=lo, band_shift=shift)
    info = ctx.last_kernel_info()
    assert info.count('dswx_histogram_k') == 1 and f',{SPLIT},{len(names)})' in info, info
    assert list(hist) == names
    kinds = {'nir': (HIST_I16, lo, shift), 'fmask': (HIST_U8, 0, 0), 'diag': (HIST_DIAG, 0, 0), 'wtr': (HIST_U8, 0, 0)}
    for name in names:
        want = tiled_bincount(bin_of(planes(name), *kinds[name]), BINS)
        for t in EDGE_TILES:
            assert np.array_equal(want[t], histogram(batch.read_tile(name, t), *kinds[name])), (name, t)
        bad = np.argwhere(hist[name] != want)
        assert hist[name].shape == (T, BINS) and bad.size == 0, (name, bad[:4])
        if name != 'nir':
            assert np.all(hist[name].sum(axis=1) == H * W), name
    assert np.count_nonzero(hist['nir']) > T                  # (the band is noise: it fills more than one bin per tile)
    part = batch.histogram(names=names, tile0=SUB[0], n_tiles=SUB[1], band_lo=lo, band_shift=shift)
    assert f',{SPLIT},{len(names)})' in ctx.last_kernel_info()
    for name in names:
        assert part[name].shape == (SUB[1], BINS) and np.array_equal(part[name], hist[name][SUB[0]:SUB[0] + SUB[1]]), name


def test_crosstab_two_pairs_in_one_call_every_tile(ctx, batches, planes):
    batch = batches[0]
    wtr_by_conf = Spec(HIST_U8, col_bits=4, row_of_bin=classes(WTR_VALUES, other=7), col_of_byte=np.arange(256) % 16)
    diag_by_wtr = Spec(HIST_DIAG, col_bits=3, row_of_bin=np.minimum(np.arange(256), 31), col_of_byte=classes(WTR_VALUES, other=7))
    pairs = [('wtr', 'conf', wtr_by_conf), ('diag', 'wtr', diag_by_wtr)]
    got = batch.crosstab(pairs)
    info = ctx.last_kernel_info()
    assert info.count('dswx_crosstab_k') == 1 and f',{SPLIT},{len(pairs)})' in info, info
    assert got.shape == (len(pairs), T, CELLS)
    for k, (na, nb, spec) in enumerate(pairs):
        want = tiled_bincount(cell_of(planes(na), planes(nb), spec), CELLS)
        for t in EDGE_TILES:
            assert np.array_equal(want[t], crosstab(batch.read_tile(na, t), batch.read_tile(nb, t), spec)), (na, nb, t)
        bad = np.argwhere(got[k] != want)
        assert bad.size == 0, (na, nb, bad[:4])
        assert np.all(got[k].sum(axis=1) == H * W), (na, nb)  # nothing is excluded by these tables
    assert not np.array_equal(got[0], got[1])
    part = batch.crosstab(pairs, tile0=SUB[0], n_tiles=SUB[1])
    assert f',{SPLIT},{len(pairs)})' in ctx.last_kernel_info()
    assert part.shape == (len(pairs), SUB[1], CELLS) and np.array_equal(part, got[:, SUB[0]:SUB[0] + SUB[1]])


def test_compare_finds_the_changed_tiles_of_every_plane_and_no_other(ctx, batches):
    batch, other = batches
    names = batch.plane_names()
    recs = batch.compare(other)
    info = ctx.last_kernel_info()
    assert 'dswx_compare_k' in info and f',{SPLIT},{len(names)})' in info, info
    assert list(recs) == names
    for k, name in enumerate(names):
        rec = recs[name]
        assert rec.shape == (T,)
        assert np.flatnonzero(rec['n_diff']).tolist() == list(CHANGED_TILES), (name, np.flatnonzero(rec['n_diff'])[:8])
        for j, t in enumerate(CHANGED_TILES):
            want = compare(batch.read_tile(name, t), other.read_tile(name, t))
            assert rec[t] == want and rec[t]['n_diff'] == 1 and rec[t]['first'] == (5 * k + 13 * j) % (H * W), (name, t, rec[t], want)
        rest = np.ones(T, dtype=bool)
        rest[list(CHANGED_TILES)] = False
        assert np.all(rec['first'][rest] == -1) and np.all(rec['max_abs_diff'][rest] == 0.0), name
    part = batch.compare(other, tile0=SUB[0], n_tiles=SUB[1])
    assert f',{SPLIT},{len(names)})' in ctx.last_kernel_info()
    for name in names:
        assert part[name].shape == (SUB[1],) and np.array_equal(part[name], recs[name][SUB[0]:SUB[0] + SUB[1]]), name


def test_label_and_body_table_of_the_wtr_layer_every_tile(ctx, batches, planes):
    """dswx_batch_label on WTR, then dswx_batch_body_table on its label plane with WTR as the value plane: all four and all
    three outputs of every tile against the host entries on the downloaded layer; then both again on the sub-range."""
    batch = batches[0]
    wtr = planes('wtr').reshape(T, H, W)
    lspec, bspec = wtr_label_spec(2), wtr_body_spec(3)
    lref = _capi.label_host(wtr, lspec)
    assert 0 < np.count_nonzero(lref['summary'][:, 0]) and len(np.unique(lref['summary'][:, 0])) > 2     # the layer has water bodies
    bref = _capi.body_table_host(lref['label'], wtr, bspec)
    assert 0 < np.count_nonzero(bref['head'][:, 0] > bref['head'][:, 1]) < T                                # some tables are truncated

    def both(tile0, count):
        made = []
        try:
            res = batch.label('wtr', lspec, tile0=tile0, n_tiles=count)
            made += list(res.values())
            info = ctx.last_kernel_info()
            assert 'dswx_label_local_k' in info and f',{SPLIT},1)' in info, info
            tab = batch.body_table('wtr', bspec, res['label'], tile0=tile0, n_tiles=count)
            made += list(tab.values())
            info = ctx.last_kernel_info()
            assert 'dswx_body_fill_k' in info and f',{SPLIT},1)' in info, info
            ctx.synchronize()
            nt = T - tile0 if count is None else count
            for k, ref in lref.items():
                want = ref[tile0:tile0 + nt].reshape(-1)
                got = res[k].download(_capi.LABEL_DTYPES[k], want.size)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, ('label', k, tile0, bad[:4], got[bad[:4]], want[bad[:4]])
            for k, ref in bref.items():
                want = ref[tile0:tile0 + nt].reshape(-1)
                got = tab[k].download(_capi.BODY_DTYPES[k], want.size)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, ('body table', k, tile0, bad[:4], got[bad[:4]], want[bad[:4]])
            assert set(res) == set(lref) and set(tab) == set(bref) and lref['summary'].shape[1] == SUMMARY_WORDS
        finally:
            for b in made:
                b.free()

    both(0, None)
    both(*SUB)
