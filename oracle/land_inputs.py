"""TEST INFRASTRUCTURE -- seeded input draws for the LAND layer (create_landcover_mask :994-1115) over the whole byte
range, shared by oracle/gen_golden.py and tests/test_gpu_land_domain.py.

synth_landcover_inputs (the product's synthetic scenes) draws 13 WorldCover and 16 CGLS class codes; these draws cover
every byte 0..255, the five WorldCover codes the layer counts (10, 50, 80, 90, 95) and their +-1 neighbours, and 3x3
blocks holding each count 0..9 of every code.
"""
import numpy as np

WC_CODES = np.array([10, 50, 80, 90, 95], np.uint8)                 # tree, urban, water x 3
WC_NEAR = np.array([9, 10, 11, 49, 50, 51, 79, 80, 81, 89, 90, 91, 94, 95, 96], np.uint8)
WC_CLASSES = np.array([10, 20, 30, 40, 50, 60, 70, 80, 90, 95, 100], np.uint8)   # the ESA WorldCover legend
DEFAULT_FOREST = [20, 50, 111, 113, 115, 116, 121, 123, 125, 126]
# 0 and 255, duplicates, and classes outside 0..255 (the reference compares a uint8 raster with them: never equal)
EDGE_FOREST = [0, 255, 20, 20, -1, 256, 300, 111, 111, 126]
ALL_FOREST = list(range(256))
FOREST_SETS = {'default': DEFAULT_FOREST, 'edge': EDGE_FOREST, 'all': ALL_FOREST, 'none': None, 'empty': []}
# (tree, low, high, water): the reference's two sets and edge sets (all pass, none pass, a negative one)
THRESHOLD_SETS = {'standard': (6, 3, 7, 3), 'water heavy': (6, 3, 7, 1), 'zeros': (0, 0, 0, 0), 'tens': (10, 10, 10, 10),
                  '1991': (1, 9, 9, 1), 'negative': (-3, 2, 5, 3), 'int32': (-2 ** 31, 4, 2 ** 31 - 1, 5)}


def _dense_blocks(rng, h, w, rest):
    """`rest` [3h, 3w] with k (uniform 0..9) bytes of every 3x3 block replaced by one of the five counted codes."""
    code = rng.choice(WC_CODES, (h, w))
    k = rng.integers(0, 10, (h, w))
    rank = rng.permuted(np.tile(np.arange(9), (h * w, 1)), axis=1).reshape(h, w, 3, 3)
    blocks = rest.reshape(h, 3, w, 3).transpose(0, 2, 1, 3)
    blocks = np.where(rank < k[..., None, None], code[..., None, None], blocks)
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(3 * h, 3 * w), dtype=np.uint8)


def worldcover(rng, h, w, mode):
    """A WorldCover raster [3h, 3w] u8.  mode: 'classes' (the legend), 'full' (uniform 0..255), 'near' (the five codes
    +-1), 'dense' (blocks of k codes in a mix of 'near' and 'full'), or an int: a uniform plane of that byte."""
    shape = (3 * h, 3 * w)
    if isinstance(mode, (int, np.integer)):
        return np.full(shape, mode, np.uint8)
    if mode == 'classes':
        return _dense_blocks(rng, h, w, rng.choice(WC_CLASSES, shape))
    if mode == 'full':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if mode == 'near':
        return rng.choice(WC_NEAR, shape)
    if mode == 'dense':
        rest = np.where(rng.random(shape) < 0.5, rng.choice(WC_NEAR, shape), rng.integers(0, 256, shape))
        return _dense_blocks(rng, h, w, rest)
    if mode == 'blocks':
        # cheap enough for full-size tiles: uniform 3x3 blocks of the codes and their neighbours, a share of whose bytes
        # (0 in the first row, nearly all in the last) is replaced by uniform bytes, so the counts run from 9 down to 0
        coarse = WC_NEAR[rng.integers(0, len(WC_NEAR), (h, w), dtype=np.uint8)]
        wc = np.repeat(np.repeat(coarse, 3, axis=0), 3, axis=1)
        share = (np.arange(3 * h, dtype=np.int64) * 256 // max(3 * h, 1)).astype(np.uint8)[:, None]
        replace = rng.integers(0, 256, shape, dtype=np.uint8) < share
        return np.where(replace, rng.integers(0, 256, shape, dtype=np.uint8), wc)
    raise ValueError(mode)


def copernicus(rng, h, w):
    """A CGLS raster [h, w] u8: half uniform over 0..255, half drawn from the default forest classes, 0 and 255; a raster
    of at least 256 pixels holds every byte."""
    picks = np.array(DEFAULT_FOREST + [0, 255, 19, 21, 110, 127], np.uint8)
    cg = np.where(rng.random((h, w)) < 0.5, rng.choice(picks, (h, w)), rng.integers(0, 256, (h, w))).astype(np.uint8)
    m = min(h * w, 256)
    cg.ravel()[rng.choice(h * w, m, replace=False)] = rng.permutation(256)[:m]
    return cg


def counts(wc):
    """The three 3x3 counts (water, urban, tree) of create_landcover_mask, as int arrays [h, w]."""
    h, w = wc.shape[0] // 3, wc.shape[1] // 3
    blocks = wc.reshape(h, 3, w, 3)
    return (np.isin(blocks, [80, 90, 95]).sum(axis=(1, 3)), (blocks == 50).sum(axis=(1, 3)),
            (blocks == 10).sum(axis=(1, 3)))
