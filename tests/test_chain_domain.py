"""The decision domain of the post-test chain (oracle/chain_inputs.py), shown on the CPU to be what the GPU tests of
tests/test_gpu_chain_domain.py need: the two oracles agree on it for every parameter set, every table cell that can
exist is held by a pixel, and every bit of the aerosol lists decides a pixel.

The cells are counted by chain_inputs.table_cells from the inputs and the C oracle's uncollapsed layers.  With the
default lists and aerosol_max_nir = 1000 (set S0, what every deterministic tile of the suite had before) 58 of the 66
pre16 cells and 58 of the 72 chainm cells exist: remap needs nir <= 1000 and the LAND partial-surface-water rule
nir > 1200, and no byte of the default lists has a shadow, cloud or snow bit.  The tests state those gaps and that the
sets with aerosol_max_nir > lcmask_nir and hashed lists close them."""
import functools

import numpy as np
import pytest

from oracle import chain_inputs as ch
from oracle import dswx_oracle as o

LAYERS = tuple(ch.ABI_NAME.values())


@functools.lru_cache(maxsize=None)
def raw_layers(name):
    return ch.c_expected(name, ch.tile_of(name), collapse=False)


def test_vector_pairs_and_layout():
    """60 (DIAG pattern, nir zone) pairs over 30 patterns under the defaults, 62 at aerosol_max_nir = 1400; every
    combination once; neighbours in memory hold unrelated cells; the variants' sizes."""
    t = ch.tile_of('S0')
    assert t['n_pairs'] == 60 and len(set(t['diag'][:60].tolist())) == 30 and len(t['vectors']) == 66
    assert ch.tile_of('S2')['n_pairs'] == 62
    for k in range(6):                                   # the six added vectors are fill in exactly band k
        assert (t['vectors'][60 + k] == -9999).tolist() == [j == k for j in range(6)]
    assert not (t['vectors'][:60] == -9999).any()
    n = t['fmask'].size
    assert n == 66 * ch.CELLS_PER_VECTOR == 1_520_640 and t['fmask'].shape == (n // ch.WIDTH, ch.WIDTH)
    lut = {v: i for i, v in enumerate(ch.LAND_VALUES)}
    land_i = np.vectorize(lut.get)(t['land'].ravel())
    mask_i = lambda a: np.searchsorted(ch.MASK_VALUES, a.ravel())
    cell = (((t['vec'].ravel().astype(np.int64) * 256 + t['fmask'].ravel()) * 10 + land_i) * 3 + mask_i(t['shad'])) * 3 + \
        mask_i(t['ocean'])
    assert np.array_equal(np.sort(cell), np.arange(n))
    # the 8 pixels of a group (and so the 4 of a transpose and the 64 lanes of a wave) are a random draw: groups whose
    # pixels share a vector or an Fmask byte are as rare as chance makes them
    g = lambda a: np.sort(a.ravel().reshape(-1, 8), axis=1)
    for a, distinct in ((t['vec'], 66), (t['fmask'], 256)):
        p_all_differ = np.prod(1 - np.arange(8) / distinct)
        share = (np.diff(g(a), axis=1) != 0).all(axis=1).mean()
        assert abs(share - p_all_differ) < 0.01, (share, p_all_differ)
    tail = ch.tile_of('S0', 'tail')
    assert tail['fmask'].shape == (1, n - 3) and (n - 3) % 8 == 5
    assert all(np.array_equal(tail[k].ravel(), t[k].ravel()[:-3]) for k in ('fmask', 'land', 'shad', 'ocean'))
    r = ch.tile_of('S0', 'reduced')
    assert r['fmask'].shape[1:] == (1, 7) and 66 * 256 <= r['fmask'].size < 66 * 256 + 7
    pairs = np.unique(r['vec'].ravel().astype(np.int64) * 256 + r['fmask'].ravel())
    assert np.array_equal(pairs, np.arange(66 * 256))
    for m in ('land', 'shad', 'ocean'):
        assert set(np.unique(r[m]).tolist()) == set(ch.LAND_VALUES if m == 'land' else ch.MASK_VALUES)


def test_list_families():
    h = ch.hashed(7)
    m = ch.matrix(h)
    assert m.shape == (4, 256) and 400 < m.sum() < 624 and ch.lists_of(m) == h
    assert np.array_equal(ch.matrix(ch.complement(h)), ~m) and ch.hashed(7) == h and ch.hashed(11) != h
    assert ch.matrix(ch.all_bytes()).all() and not ch.matrix(ch.empty()).any()
    assert ch.default() == {c: sorted(v) for c, v in o.DEFAULT_AEROSOL_FMASK_VALUES.items()}
    f = ch.matrix(ch.one_bit_flipped(h, 2, 16))
    assert (f != m).sum() == 1 and f[2, 16] != m[2, 16]
    from proteus_amd import _capi
    d, s0 = _capi.default_params(), ch.params_of('S0')
    assert bytes(d.aerosol_fmask_lut) == bytes(s0.aerosol_fmask_lut)
    s1, s6 = ch.params_of('S1'), ch.params_of('S6')
    a, b = (np.frombuffer(bytes(p.aerosol_fmask_lut), np.uint8).reshape(4, 256) for p in (s1, s6))
    assert set(np.unique(a).tolist()) == {0, 1} and set(np.unique(b).tolist()) == {0, 2, 128, 255}
    assert np.array_equal(a != 0, b != 0) and np.array_equal(a != 0, m)


@pytest.mark.parametrize('name', list(ch.SETS))
def test_oracles_agree(name):
    """The C oracle and the numpy oracle on all eight layers, the browse layer and the counters, both collapse settings
    ('cover' mode, which the C oracle does not do: the numpy oracle with scipy's dilation against its second statement of
    it, and the C oracle in 'ignore' mode on the layers in front of the dilation)."""
    tile = ch.tile_of(name)
    for collapse in (True, False):
        e = ch.numpy_expected(name, tile, collapse)
        if name == 'S7':
            c = ch.numpy_expected(name, tile, collapse, binary_dilation=o.masked_dilation_by_shifts)
            front = ch.c_expected(name, tile, collapse, mask_adjacent_to_cloud_mode='ignore')
            for k in ('diag', 'wtr1', 'wtr1_aerosol', 'wtr2'):
                assert np.array_equal(front[k], e[k]), (k, collapse)
            assert front['counters'] == e['counters']
        else:
            c = ch.c_expected(name, tile, collapse)
        for k in LAYERS + ('browse',):
            assert c[k].dtype == e[k].dtype and np.array_equal(c[k], e[k]), (name, k, collapse)
        assert c['counters'] == e['counters'], (name, collapse)


def test_float32_set_holds_every_class_in_every_nir_zone():
    """S8 (the float32 chain; the coverage conditions belong to the integer chain): all five WTR-1 classes occur in each of
    the three nir zones of its tile."""
    tile = ch.tile_of('S8')
    p = ch.params_of('S8', False)
    w1 = raw_layers('S8')['wtr1']
    zone = ch.nir_zone(tile['bands'][3], p)
    for z in range(3):
        assert set(np.unique(w1[zone == z]).tolist()) >= {0, 1, 2, 3, 4}, z


# set -> (holds every pre16 cell, holds every chainm cell): what each set is there for
CLOSED = {'S0': (False, False), 'S1': (False, True), 'S2': (True, True), 'S3': (True, True), 'S6': (False, True),
          'S7': (False, True)}


@pytest.mark.parametrize('name', ch.INTEGER_SETS)
def test_every_reachable_cell_is_held_by_a_pixel(name):
    p = ch.params_of(name, False)
    tile = ch.tile_of(name)
    cells = ch.table_cells(p, tile, raw_layers(name))
    r = ch.reachable(p)
    got = {k: set(np.unique(cells[k]).tolist()) for k in r}
    assert {k: len(v) for k, v in r.items()} == dict(
        pre16=66, chainm=72, extram=108 if p.mask_adjacent_to_cloud_mode == 0 else 144,
        joint=28_672 if name in ('S1', 'S6') else 28_576)
    for k in r:
        assert got[k] <= r[k], (k, sorted(got[k] - r[k])[:8])          # the enumeration holds every cell that occurs
    assert got['joint'] == r['joint']
    if name not in CLOSED:
        return
    pre16_closed, chainm_closed = CLOSED[name]
    assert p.aerosol_max_nir > p.lcmask_nir if pre16_closed else p.aerosol_max_nir <= p.lcmask_nir
    if pre16_closed:
        assert got['pre16'] == r['pre16']
    else:       # the stated gap: the eight cells "remap and the LAND partial-surface-water rule on one pixel"
        assert r['pre16'] - got['pre16'] == ch.remap_and_psw_rule(r['pre16']) and len(got['pre16']) == 58
    if chainm_closed:
        assert got['chainm'] == r['chainm'] and got['extram'] == r['extram']
    else:       # the stated gap: the fourteen cells "remapped pixel under Fmask shadow / cloud / snow"
        assert r['chainm'] - got['chainm'] == ch.remap_under_fmask_bits(r['chainm']) and len(got['chainm']) == 58


@pytest.mark.parametrize('fill, bits', [(None, 1024), (255.0, 1020)])
def test_every_list_bit_decides(fill, bits):
    """For every (row, byte) a pixel whose WTR-1-AEROSOL or CLOUD differs between a list and one_bit_flipped of it: seen
    through hashed(7) against its complement, which differ in every bit, on the pixels that read that bit alone."""
    tile = ch.tile_of('S1')
    a = ch.c_expected('S1', tile, False, fmask_fill=fill)
    b = ch.c_expected('S1', tile, False, lists=ch.complement(ch.hashed(7)), fmask_fill=fill)
    assert np.array_equal(a['wtr1'], b['wtr1'])
    decided = ch.decided_bits(tile, a['wtr1'], a, b)
    assert decided.sum() == bits
    if fill is not None:
        assert not decided[:, 255].any() and decided[:, :255].all()


@pytest.mark.parametrize('row, byte', [(0, 0), (1, 255), (2, 16), (3, 14), (2, 224)])
def test_one_flipped_bit_changes_its_pixels_only(row, byte):
    """one_bit_flipped itself: the pixels that change are of that class and Fmask byte, and there are some."""
    tile = ch.tile_of('S1')
    a = raw_layers('S1')
    b = ch.c_expected('S1', tile, False, lists=ch.one_bit_flipped(ch.hashed(7), row, byte))
    diff = np.zeros(tile['fmask'].shape, bool)
    for k in LAYERS:
        diff |= a[k] != b[k]
    assert diff.any() and (tile['fmask'][diff] == byte).all() and (a['wtr1'][diff] == ch.CLASSES[row]).all()
    assert ((a['wtr1_aerosol'] != b['wtr1_aerosol']) | (a['cloud'] != b['cloud']))[diff].all()
    only = ch.decided_bits(tile, a['wtr1'], a, b)
    assert only.sum() == 1 and only[row, byte]


@pytest.mark.parametrize('oracle', ['c', 'numpy'])
def test_remapping_off_equals_empty_lists(oracle):
    f = ch.c_expected if oracle == 'c' else ch.numpy_expected
    tile = ch.tile_of('S4')
    for collapse in (True, False):
        off = f('S4', tile, collapse)
        emp = f('S4', tile, collapse, lists=ch.empty(), apply_aerosol_class_remapping=True)
        hashed_on = f('S4', tile, collapse, apply_aerosol_class_remapping=True)
        for k in LAYERS + ('browse',):
            assert np.array_equal(off[k], emp[k]), (k, collapse)
        assert off['counters'] == emp['counters']
        assert not np.array_equal(off['wtr1_aerosol'], hashed_on['wtr1_aerosol'])


def test_any_nonzero_lut_byte_is_a_member():
    """The C ABI: aerosol_fmask_lut[k][v] != 0.  The LUT written as 2 / 128 / 255 (S6) equals the same lists written as 1."""
    tile = ch.tile_of('S6')
    for collapse in (True, False):
        one, other = ch.c_expected('S1', tile, collapse), ch.c_expected('S6', tile, collapse)
        for k in LAYERS + ('browse',):
            assert np.array_equal(one[k], other[k]), (k, collapse)
        assert one['counters'] == other['counters']
