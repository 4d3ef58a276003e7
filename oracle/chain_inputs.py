"""TEST INFRASTRUCTURE -- the decision domain of the classifier's post-test chain (aerosol remap, the LAND / SHAD rules,
cloud / snow, WTR, BWTR, CONF, `cover` state, browse), shared by tests/test_chain_domain.py and
tests/test_gpu_chain_domain.py.  Imports nothing from the reference.

The chain is a finite function of: the WTR-1 outcome, the Fmask byte, the LAND class, SHAD == 0, OCEAN == 0, two nir
comparisons (nir <= aerosol_max_nir, nir > lcmask_nir) and the run's options.  The table-driven kernel evaluates it as the
small tables dswx_build_tables fills (dswx_tables.h: lut1, fm16, land8, chain, pre16, chainm, extra, extram), the direct
and generic kernels per pixel.  The aerosol lists are 4 x 256 bits of caller data.

`cells_tile` is a tile that holds every cell of that function once: band vectors of tests/golden/diag_vectors.npz -- one
for every (DIAG pattern, nir zone) pair the fixture reaches, and six that are fill in one band each -- x all 256 Fmask
bytes x LAND_VALUES x SHAD (0, 1, 255) x OCEAN (0, 1, 255), laid out through a seeded permutation.  `table_cells` is a CPU
model of the table indices of every pixel, computed from the inputs and the oracle's UNCOLLAPSED layers (never from the
device), `reachable` the cells that can exist, enumerated from first principles.  The list families are `hashed`,
`complement`, `all_bytes`, `empty`, `default`, `one_bit_flipped`; SETS are the parameter sets both test files run.
"""
import functools
import os

import numpy as np

from oracle import dswx_oracle as o

CLASSES = (0, 2, 3, 4)                                      # row k of a list matrix is the list of WTR-1 class CLASSES[k]
LAND_VALUES = (0, 1, 99, 100, 101, 199, 200, 201, 202, 255)
MASK_VALUES = (0, 1, 255)
CELLS_PER_VECTOR = 256 * len(LAND_VALUES) * len(MASK_VALUES) ** 2
WIDTH = 512                                                 # of the 2-D form (CELLS_PER_VECTOR = 45 * 512)
FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'diag_vectors.npz')
ABI_NAME = {'DIAG': 'diag', 'WTR-1': 'wtr1', 'WTR-1-AEROSOL': 'wtr1_aerosol', 'WTR-2': 'wtr2', 'WTR': 'wtr', 'BWTR': 'bwtr',
            'CONF': 'conf', 'CLOUD': 'cloud'}
BROWSE_DEFAULT = (True, False, False, False, True)      # exclude_psw_aggressive, not_water, cloud, snow, ocean -> nodata


# ---- list families: {class: [bytes]} dicts; matrix() is the 4 x 256 boolean form ----------------------------------------
def lists_of(m):
    m = np.asarray(m, bool)
    assert m.shape == (4, 256)
    return {c: np.flatnonzero(m[k]).tolist() for k, c in enumerate(CLASSES)}


def matrix(lists):
    m = np.zeros((4, 256), bool)
    for k, c in enumerate(CLASSES):
        m[k, list(lists[c])] = True
    return m


def hashed(seed):
    """Each of the 1,024 bits drawn with probability 1/2."""
    return lists_of(np.random.default_rng([1024, seed]).random((4, 256)) < 0.5)


def complement(lists):
    return lists_of(~matrix(lists))


def all_bytes():
    return lists_of(np.ones((4, 256), bool))


def empty():
    return lists_of(np.zeros((4, 256), bool))


def default():
    return {c: sorted(v) for c, v in o.DEFAULT_AEROSOL_FMASK_VALUES.items()}


def one_bit_flipped(lists, row, byte):
    m = matrix(lists)
    m[row, byte] ^= True
    return lists_of(m)


# ---- the parameter sets ---------------------------------------------------------------------------------------------------
# kw: proteus_amd._capi.make_params arguments (the lists are added by params_of); member: the byte written into
# aerosol_fmask_lut for "member" (the C ABI says non-zero); f32: the float32 chain
SETS = {
    'S0': dict(lists=('default',), kw=dict()),
    'S1': dict(lists=('hashed', 7), kw=dict(aerosol_max_nir=1000, mask_adjacent_to_cloud_mode='mask', fmask_fill=None)),
    'S2': dict(lists=('complement', 7), kw=dict(aerosol_max_nir=1400, mask_adjacent_to_cloud_mode='ignore')),
    'S3': dict(lists=('hashed', 11), kw=dict(aerosol_max_nir=1400, mask_adjacent_to_cloud_mode='mask', fmask_fill=64)),
    'S4': dict(lists=('hashed', 7), kw=dict(apply_aerosol_class_remapping=False)),
    'S5a': dict(lists=('all_bytes',), kw=dict(aerosol_max_nir=32767)),
    'S5b': dict(lists=('empty',), kw=dict(aerosol_max_nir=-32768)),
    'S6': dict(lists=('hashed', 7), kw=dict(aerosol_max_nir=1000, mask_adjacent_to_cloud_mode='mask', fmask_fill=None),
               member=(2, 128, 255)),
    'S7': dict(lists=('hashed', 7), kw=dict(mask_adjacent_to_cloud_mode='cover')),
    'S8': dict(lists=('hashed', 7), kw=dict(offset_and_scale=[(1.0, 0.0)] * 6)),
}
INTEGER_SETS = tuple(k for k in SETS if 'offset_and_scale' not in SETS[k]['kw'])


def lists_of_set(name):
    kind, *arg = SETS[name]['lists']
    return {'default': default, 'all_bytes': all_bytes, 'empty': empty, 'hashed': hashed,
            'complement': lambda s: complement(hashed(s))}[kind](*arg)


def make_params(kw, lists, collapse=True, member=None):
    """A dswx_params_t for make_params arguments `kw` and `lists`; with `member`, the LUT's "member" bytes are rewritten
    straight in the struct as member[(row + byte) % len(member)] instead of 1."""
    from proteus_amd import _capi
    p = _capi.make_params(aerosol_fmask_values=lists, collapse_wtr_classes=collapse, **kw)
    if member:
        for row in range(4):
            for v in range(256):
                if p.aerosol_fmask_lut[row][v]:
                    p.aerosol_fmask_lut[row][v] = member[(row + v) % len(member)]
    return p


def params_of(name, collapse=True, lists=None, **over):
    s = SETS[name]
    return make_params(dict(s['kw'], **over), lists_of_set(name) if lists is None else lists, collapse, s.get('member'))


def tile_key(name):
    """What the tile of a set depends on: (aerosol_max_nir, float32 chain)."""
    kw = SETS[name]['kw']
    return float(kw.get('aerosol_max_nir', o.AEROSOL_MAX_NIR)), 'offset_and_scale' in kw


# ---- band vectors ---------------------------------------------------------------------------------------------------------
def nir_zone(nir, params):
    """0, 1, 2: the three intervals that aerosol_max_nir (nir <= a) and lcmask_nir (nir > l) cut on the clipped nir."""
    nir = np.asarray(nir, np.float64)
    if params.clip_negative_reflectance:
        nir = np.maximum(nir, 1.0)
    lo, hi = sorted((params.aerosol_max_nir, params.lcmask_nir))
    return (nir > lo).astype(np.int64) + (nir > hi)


def pick_vectors(params):
    """(vectors int16 [V, 6], diag [V], zone [V], n_pairs): one vector of the fixture (the first, no band at its fill) for
    every (DIAG pattern, nir zone) pair that the C oracle finds on the vectors alone under `params`, ordered by (DIAG,
    zone); then six made from the first six by putting one band each at its fill (diag 65535)."""
    from oracle import c_oracle
    vec = np.load(FIXTURE, allow_pickle=False)['bands']
    fills = [params.band_fill[k] for k in range(6)]
    assert all(f == int(f) for f in fills), fills
    ok = np.all(vec != np.array(fills), axis=1)
    vec = vec[ok]
    cols = [np.ascontiguousarray(vec[:, k]) for k in range(6)]
    fm = np.full(vec.shape[0], 1 if params.fmask_fill == 0 else 0, np.uint8)
    diag = c_oracle.classify(params, cols, fm, layers=('diag',))['diag'].astype(np.int64)
    assert (diag != 65535).all()
    zone = nir_zone(vec[:, 3], params)
    _, first = np.unique(diag * 3 + zone, return_index=True)
    out, d, z = vec[first], diag[first], zone[first]
    filled = out[:6].copy()
    for k in range(6):
        filled[k, k] = int(fills[k])
    return (np.concatenate([out, filled]), np.concatenate([d, np.full(6, 65535)]),
            np.concatenate([z, nir_zone(filled[:, 3], params)]), len(first))


# ---- the tile -------------------------------------------------------------------------------------------------------------
def _hash(i):
    return ((np.asarray(i, np.uint64) + np.uint64(0x9e3779b9)) * np.uint64(0x9e3779b97f4a7c15)) >> np.uint64(29)


def cells_tile(params_kw=None, seed=0, variant='full'):
    """The constructed tile for make_params arguments `params_kw` (they decide the vectors: thresholds, fills, clip,
    aerosol_max_nir, the float32 chain): dict(bands [6 x int16], fmask, land, shad, ocean, vec (the vector index of every
    pixel), vectors, diag, zone, n_pairs).

    'full'     every vector x Fmask byte x LAND_VALUES x SHAD x OCEAN once, permuted, as [V * 45, 512]
    'tail'     the same pixels without the last three, as [1, N - 3]: N % 8 == 5
    'reduced'  every vector x Fmask byte, LAND / SHAD / OCEAN hashed from the cell, permuted, the first pixels repeated
               up to a multiple of 7, as [T, 1, 7]"""
    from proteus_amd import _capi
    vectors, diag, zone, n_pairs = pick_vectors(_capi.make_params(**(params_kw or {})))
    V = len(vectors)
    rng = np.random.default_rng([V, seed])
    if variant == 'reduced':
        cell = rng.permutation(V * 256)
        cell = np.concatenate([cell, cell[:-cell.size % 7]])
        h = _hash(cell)
        fm, vi = cell % 256, cell // 256
        land, shad, ocean = (np.array(LAND_VALUES)[h % 10], np.array(MASK_VALUES)[(h // 10) % 3],
                             np.array(MASK_VALUES)[(h // 30) % 3])
        shape = (-1, 1, 7)
    else:
        cell = rng.permutation(V * CELLS_PER_VECTOR)
        c = cell
        ocean, c = np.array(MASK_VALUES)[c % 3], c // 3
        shad, c = np.array(MASK_VALUES)[c % 3], c // 3
        land, c = np.array(LAND_VALUES)[c % 10], c // 10
        fm, vi = c % 256, c // 256
        shape = (-1, WIDTH)
        if variant == 'tail':
            vi, fm, land, shad, ocean = (a[:-3] for a in (vi, fm, land, shad, ocean))
            shape = (1, -1)
            assert vi.size % 8 == 5
        else:
            assert variant == 'full', variant
    u8 = lambda a: np.ascontiguousarray(np.asarray(a).astype(np.uint8).reshape(shape))
    out = dict(bands=[np.ascontiguousarray(vectors[vi, k].reshape(shape)) for k in range(6)], fmask=u8(fm), land=u8(land),
               shad=u8(shad), ocean=u8(ocean), vec=vi.astype(np.int16).reshape(shape), vectors=vectors, diag=diag, zone=zone, n_pairs=n_pairs)
    for a in out['bands'] + [out[k] for k in ('fmask', 'land', 'shad', 'ocean')]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=16)
def tile_of(name, variant='full'):
    """cells_tile of a set of SETS (seed 0), shared by the sets with the same tile_key."""
    return _tile_of_key(tile_key(name), variant)


@functools.lru_cache(maxsize=16)
def _tile_of_key(key, variant):
    kw = dict(aerosol_max_nir=key[0])
    if key[1]:
        kw['offset_and_scale'] = [(1.0, 0.0)] * 6
    return cells_tile(kw, 0, variant)


def masks_of(tile):
    return {m: tile[m] for m in ('land', 'shad', 'ocean')}


# ---- the oracles ----------------------------------------------------------------------------------------------------------
def numpy_expected(name, tile, collapse=True, masks=True, lists=None, binary_dilation=None, **over):
    """The numpy oracle's layers by C-ABI name, 'counters' as the list of three, and 'browse', for a set of SETS."""
    s = SETS[name]
    kw = dict(s['kw'], **over)
    with np.errstate(all='ignore'):
        run = lambda c: o.classify_tile(
            tile['bands'], tile['fmask'], landcover=tile['land'] if masks else None, shadow=tile['shad'] if masks else None,
            ocean_mask=tile['ocean'] if masks else None, fmask_fill=kw.get('fmask_fill', 255.0),
            mask_adjacent_to_cloud_mode=kw.get('mask_adjacent_to_cloud_mode', 'mask'),
            apply_aerosol=kw.get('apply_aerosol_class_remapping', True),
            aerosol_fmask_values=lists_of_set(name) if lists is None else lists, collapse=c,
            offset_and_scale=kw.get('offset_and_scale'), aerosol_max_nir=kw.get('aerosol_max_nir'),
            binary_dilation=binary_dilation)
        e = run(False)
    raw = e['WTR']
    if collapse:                                # as classify_tile itself does at its end
        e = dict(e, **{k: o.collapse_wtr_classes(e[k]) for k in ('WTR', 'WTR-1', 'WTR-1-AEROSOL', 'WTR-2')})
    out = {key: e[layer] for layer, key in ABI_NAME.items()}
    c = e['counters']
    out['counters'] = [c['n_valid'], c['n_cloud_and_valid'], c['n_not_ocean']]
    out['browse'] = o.compute_browse_array(raw, collapse, *BROWSE_DEFAULT)
    return out


def c_expected(name, tile, collapse=True, masks=True, lists=None, **over):
    """The C oracle's layers, 'browse' and 'counters' (a list) for a set of SETS ('cover' mode: the numpy oracle's)."""
    from oracle import c_oracle
    if dict(SETS[name]['kw'], **over).get('mask_adjacent_to_cloud_mode') == 'cover':
        return numpy_expected(name, tile, collapse, masks, lists, **over)
    p = params_of(name, collapse, lists, **over)
    layers = tuple(ABI_NAME.values()) + ('browse',)
    out = c_oracle.classify(p, tile['bands'], tile['fmask'], layers=layers, **(masks_of(tile) if masks else {}))
    out['counters'] = out['counters'].tolist()
    return out


# ---- the CPU model of the table indices -----------------------------------------------------------------------------------
def _code(cls):
    """WTR class byte -> table code: 0..4 class, 5 ocean masked (254), 6 fill (255)."""
    cls = np.asarray(cls, np.int64)
    assert np.isin(cls, (0, 1, 2, 3, 4, 254, 255)).all()
    return np.where(cls <= 4, cls, np.where(cls == 254, 5, 6))


def table_cells(params, inputs, layers):
    """The cells of every pixel, from the inputs (dict: bands, fmask, and land / shad where given) and the oracle's
    UNCOLLAPSED layers by C-ABI name (diag, wtr1, wtr1_aerosol, wtr2):

    lut1    T1 | T2 << 1 | !T3 << 2 | T4 << 3 | T5 << 4 | invalid << 5 | ocean masked << 6 (the test bits of an invalid
            pixel are not in the layers and do not decide: 0, !T3 too)
    pre16   WTR-1 code | remap << 3 | SHAD rule << 4 | LAND partial-surface-water rule << 5 | LAND high-dev rule << 6
    chainm  WTR-2 code | remap << 3 | Fmask shadow << 4 | cloud << 5 | snow << 6
    extram  chainm | Fmask adjacent << 7
    joint   ((((WTR-1 code * 256 + Fmask byte) * 4 + LAND class) * 2 + (SHAD == 0)) * 2 + (nir > lcmask_nir)), LAND class
            0: 200, 1: 201 or < 100, 2: 100..199, 3: other

    A pixel counts as remapped when the remap changed it (classes 0, 2, 3, 4 become 1), whatever a kernel's index bit says
    for the codes that no list has a row for."""
    fm = np.asarray(inputs['fmask'], np.int64)
    nir = np.asarray(inputs['bands'][3], np.float64)
    if params.clip_negative_reflectance:
        nir = np.maximum(nir, 1.0)
    bright = nir > params.lcmask_nir
    land = np.asarray(inputs['land'], np.int64) if inputs.get('land') is not None else np.full(fm.shape, 255)
    shad0 = (np.asarray(inputs['shad']) == 0) if inputs.get('shad') is not None else np.zeros(fm.shape, bool)
    w1, w1a, w2 = (np.asarray(layers[k], np.int64) for k in ('wtr1', 'wtr1_aerosol', 'wtr2'))
    code1, code2 = _code(w1), _code(w2)
    remap = w1a != w1
    psw_class = (land == 201) | (land < 100)
    high = (land >= 100) & (land < 200)
    land_class = np.where(land == 200, 0, np.where(psw_class, 1, np.where(high, 2, 3)))
    shadow_bits = 12 if params.mask_adjacent_to_cloud_mode == 0 else 8
    d = np.asarray(layers['diag'], np.int64)
    invalid = d == 65535
    digit = lambda k: (d // 10 ** k) % 10
    tests = np.where(invalid, 0, digit(0) | digit(1) << 1 | (1 - digit(2)) << 2 | digit(3) << 3 | digit(4) << 4)
    i = lambda b: np.asarray(b, bool).astype(np.int64)
    chainm = code2 | i(remap) << 3 | i(fm & shadow_bits) << 4 | i(fm & 2) << 5 | i(fm & 16) << 6
    return dict(
        lut1=tests | i(invalid) << 5 | i(code1 == 5) << 6,
        pre16=code1 | i(remap) << 3 | i(shad0 & (land != 200)) << 4 | i(psw_class & bright) << 5 | i(high) << 6,
        chainm=chainm, extram=chainm | i(fm & 4) << 7,
        joint=(((code1 * 256 + fm) * 4 + land_class) * 2 + i(shad0)) * 2 + i(bright))


def reachable(params):
    """The cells of table_cells that can exist under `params`, from first principles: a list has rows for the classes
    0, 2, 3, 4 only (no remap of class 1, ocean masked or fill); the two LAND rules exclude each other (201 or < 100
    against 100..199); a remapped pixel is class 1, so its WTR-2 is 1 or, where a rule hits, 0; a pixel whose Fmask byte
    is the fill byte is fill (code 6); in 'mask' mode the adjacent bit is one of the shadow bits.  (Whether remap and the
    partial-surface-water rule meet on one pixel is a matter of the thresholds -- nir <= aerosol_max_nir and nir >
    lcmask_nir -- and of the lists, not of the function: those cells count as reachable.)"""
    pre16 = {code | remap << 3 | shadrule << 4 | lcpsw << 5 | lchigh << 6
             for code in range(7) for remap in (0, 1) for shadrule in (0, 1) for lcpsw in (0, 1) for lchigh in (0, 1)
             if not (remap and code not in CLASSES) and not (lcpsw and lchigh)}
    chainm = {code | remap << 3 | bits << 4 for code in range(7) for remap in (0, 1) for bits in range(8)
              if not (remap and code > 1)}
    mask_mode = params.mask_adjacent_to_cloud_mode == 0
    extram = {c | adj << 7 for c in chainm for adj in (0, 1) if not (mask_mode and adj and not (c >> 4) & 1)}
    fill = int(params.fmask_fill) if params.fmask_fill == params.fmask_fill else -1
    joint = {(((code * 256 + fm) * 4 + lc) * 2 + s0) * 2 + br for code in range(7) for fm in range(256) for lc in range(4)
             for s0 in (0, 1) for br in (0, 1) if not (fm == fill and code != 6)}
    return dict(pre16=pre16, chainm=chainm, extram=extram, joint=joint)


def remap_and_psw_rule(cells):
    """The pre16 cells of `cells` in which remap and the LAND partial-surface-water rule meet."""
    return {c for c in cells if (c >> 3) & 1 and (c >> 5) & 1}


def remap_under_fmask_bits(cells):
    """The chainm cells of `cells` of a remapped pixel under Fmask shadow, cloud or snow."""
    return {c for c in cells if (c >> 3) & 1 and (c >> 4) & 7}


def decided_bits(tile, wtr1_raw, a, b):
    """bool [4, 256]: for (row, byte), is there a pixel of WTR-1 class CLASSES[row] with that Fmask byte whose
    WTR-1-AEROSOL or CLOUD differs between the layer dicts `a` and `b` (runs whose lists differ in that bit: such a pixel's
    remap reads no other bit of the lists)."""
    diff = (np.asarray(a['wtr1_aerosol']) != np.asarray(b['wtr1_aerosol'])) | (np.asarray(a['cloud']) != np.asarray(b['cloud']))
    fm, w1 = np.asarray(tile['fmask'])[diff], np.asarray(wtr1_raw)[diff]
    out = np.zeros((4, 256), bool)
    for k, c in enumerate(CLASSES):
        out[k, np.unique(fm[w1 == c])] = True
    return out
