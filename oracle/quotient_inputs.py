"""TEST INFRASTRUCTURE -- thresholds of the quotient tests (MNDWI > wigt / pswt_1_mndwi / pswt_2_mndwi, NDVI < pswt_1_ndvi)
and of the AWESH test over the domain dswx_make_dev_params accepts (t == 0 or 1e-290 <= |t| <= 1e100), and the pixels that
can tell a threshold from its neighbours: pure numpy, seeded, no GPU (tests/test_quotient_domain.py; the sets are cut
for GPU runs as well: rows that divide into 8-pixel groups and into tiles of 7).

The device never divides: fl64(n / d) > t is a division-free predicate there (dswx_device.h quot_gt / quot_lt,
dswx_tables.h lut_group).  The predicate is monotonic in n for a fixed d, so only the reachable n nearest t * d can be
misjudged: `pairs(t)` has those for every d, plus the ends of the range.  Reachable: with the clip off,
n = wrap16(green - swir1) and d = wrap16(green + swir1) have the same parity, so only n = d (mod 2) exists.
`planes_of_pairs` gives the (green, swir1) -- or (nir, red) -- int16 values that make a pair.
"""
import math

import numpy as np

SEED = 4242
INF = math.inf
DEFAULTS = (0.124, -0.44, -0.5, 0.7)            # wigt, pswt_1_mndwi, pswt_2_mndwi, pswt_1_ndvi
DYADIC = (0.125, -0.125, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -7.5, 2.0 ** -15, 32767.0, -32767.0, 32768.0,
          -32768.0)
N_RANDOM = 32
N_FIXED = (0, 1, -1, 2, -2, 32767, 32766, -32768, -32767)
PIXEL_CAP = 700_000


def _around(t):
    return [math.nextafter(t, -INF), t, math.nextafter(t, INF)]


def random_pairs():
    """32 seeded (n0, d0), same parity, d0 != 0, small enough that k * (n0, d0) stays in int16 for |k| <= 4."""
    rng = np.random.default_rng(SEED)
    out = []
    while len(out) < N_RANDOM:
        n0, d0 = int(rng.integers(-8000, 8001)), int(rng.integers(-8000, 8001))
        if d0 != 0 and n0 != 0 and (n0 - d0) % 2 == 0 and abs(n0) != abs(d0) and (n0, d0) not in out:
            out.append((n0, d0))
    return out


RANDOM_PAIRS = random_pairs()


def _key(t):
    return np.float64(t).tobytes()


def _thresholds():
    vals = [0.0, -0.0, *DEFAULTS]
    for t in DYADIC:
        vals += _around(t)
    vals += [1.0 / 3.0, 2.0 / 3.0, 0.1]
    vals += _around(32767.0 / 32768.0) + _around(1.0 / 32767.0)
    vals += [1e-5, 1e-290, -1e-290, 32768.5, 65536.0, 1e9, 1e100, -1e100]
    exact = {}
    for n0, d0 in RANDOM_PAIRS:
        t = n0 / d0
        exact[_key(t)] = (n0, d0)
        vals += _around(t)
    seen, out = set(), []
    for t in vals:
        if _key(t) not in seen:              # by bit pattern: 0.0 and -0.0 both stay
            seen.add(_key(t))
            out.append(float(t))
    return out, exact


THRESHOLDS, _EXACT = _thresholds()
_RANDOM_KEYS = {_key(x): p for p in RANDOM_PAIRS for x in _around(p[0] / p[1])}


def exact_pair(t):
    """(n0, d0) when `t` was built as fl64(n0 / d0), else None."""
    return _EXACT.get(_key(t))


def random_pair_of(t):
    """(n0, d0) when `t` is fl64(n0 / d0) or one of its two neighbours, else None."""
    return _RANDOM_KEYS.get(_key(t))


def _to_parity(n, d):
    """n clamped to int16 and, where its parity is not d's, moved one step towards zero."""
    n = np.clip(n, -32768, 32767)
    odd = ((n - d) & 1) != 0
    return np.where(odd, np.where(n < 0, n + 1, n - 1), n)


def pairs(t):
    """The (n, d) int64 arrays of threshold `t`, every pair reachable and distinct.  For every d (the thresholds around a
    random pair: the multiples of its reduced denominator and 4096 seeded d): the reachable n nearest t * d, two on each
    side and t * d itself where it is one, and N_FIXED."""
    t = float(t)
    rp = random_pair_of(t)
    if rp is None:
        d = np.arange(-32768, 32768, dtype=np.int64)
    else:
        d0 = abs(rp[1]) // math.gcd(rp[0], rp[1])
        rng = np.random.default_rng(SEED + abs(rp[0]) * 65536 + abs(rp[1]))
        d = np.unique(np.concatenate([np.arange(-(32768 // d0) * d0, 32768, d0, dtype=np.int64),
                                      rng.integers(-32768, 32768, 4096), [0]]))
    with np.errstate(all='ignore'):
        x = np.clip(t * d.astype(np.float64), -40000.0, 40000.0)
    m = np.floor(x).astype(np.int64)
    m -= (m - d) & 1                                     # the largest reachable n <= t * d (as float64 sees it)
    near = np.stack([_to_parity(m + k, d) for k in (-4, -2, 0, 2, 4)])
    fixed = np.stack([np.full(d.shape, v, np.int64) for v in N_FIXED])
    n = np.concatenate([near, fixed]).ravel()
    dd = np.tile(d, near.shape[0] + fixed.shape[0])
    keep = ((n - dd) & 1) == 0
    key = np.unique((dd[keep] + 32768) * 65536 + (n[keep] + 32768))          # sorted by d, then n
    return (key & 0xffff) - 32768, (key >> 16) - 32768


def wrap16(v):
    return ((np.asarray(v, np.int64) + 32768) & 0xffff) - 32768


def planes_of_pairs(n, d, alternate=True):
    """int16 (a, b) with wrap16(a - b) == n and wrap16(a + b) == d: a = (n + d) / 2 (mod 2^15), the two solutions of which
    alternate from pixel to pixel (so that wrapped sums occur; without `alternate` a >= 0), b = wrap16(d - a)."""
    n, d = np.asarray(n, np.int64), np.asarray(d, np.int64)
    assert not ((n - d) & 1).any()
    a = ((n + d) >> 1) & 0x7fff
    if alternate:
        a = np.where(np.arange(a.size) & 1, a - 32768, a)
    b = wrap16(d - a)
    return a.astype(np.int16), b.astype(np.int16)


def pairs_of_planes(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return wrap16(a - b), wrap16(a + b)


# Constants of the bands a section does not sweep (clip off).  In the MNDWI sections NDVI = -2 / 0 = -inf passes
# "NDVI < t" for every finite t; in the NDVI section MNDWI = 2 / 0 = +inf passes "MNDWI > t": DIAG bits 0, 3 and 4 then
# each equal one quotient test.  blue and swir2 are plain.
_NIR_RED_PASS = (-1, 1)
_GREEN_SWIR1_PASS = (1, -1)
# With the default clip every band is >= 1: NDVI = -999 / 1001 passes "< t" for t in (0, 1); MNDWI = 32765 / 32767 passes
# "> t" for t < 0.9999.
_NIR_RED_PASS_CLIP = (1, 1000)
_GREEN_SWIR1_PASS_CLIP = (32766, 1)
BLUE, SWIR2 = 300, 50


def tile(mndwi_thresholds=(), ndvi_threshold=None, clip=False):
    """One row of pixels: a section of pairs(t) on (green, swir1) for each of `mndwi_thresholds`, then one on (nir, red)
    for `ndvi_threshold`.  With `clip`, only the pairs whose two planes are both >= 1 (what the default clip leaves as
    drawn).  Returns (bands [six int16 arrays of [1, N]], sections [(kind, t, start, stop)]); N is a multiple of 56 (the
    tail repeats the last pixel) so that it cuts into tiles of 7 and into whole 8-pixel groups."""
    cols = [[] for _ in range(6)]
    sections, at = [], 0
    jobs = [('mndwi', t) for t in mndwi_thresholds] + ([('ndvi', ndvi_threshold)] if ndvi_threshold is not None else [])
    for kind, t in jobs:
        a, b = planes_of_pairs(*pairs(t), alternate=not clip)
        if clip:
            keep = (a >= 1) & (b >= 1)
            a, b = a[keep], b[keep]
        k = a.size
        other = (_NIR_RED_PASS_CLIP if clip else _NIR_RED_PASS) if kind == 'mndwi' else \
            (_GREEN_SWIR1_PASS_CLIP if clip else _GREEN_SWIR1_PASS)
        full = lambda v: np.full(k, v, np.int16)
        if kind == 'mndwi':
            planes = [full(BLUE), a, full(other[1]), full(other[0]), b, full(SWIR2)]
        else:
            planes = [full(BLUE), full(other[0]), b, a, full(other[1]), full(SWIR2)]
        for c, p in zip(cols, planes):
            c.append(p)
        sections.append((kind, float(t), at, at + k))
        at += k
    bands = [np.concatenate(c) for c in cols]
    pad = -at % 56
    bands = [np.ascontiguousarray(np.concatenate([b, np.repeat(b[-1:], pad)]).reshape(1, -1)) for b in bands]
    return bands, sections


# ---- AWESH ----------------------------------------------------------------------------------------------------------------
AWESH4_MAX = 4 * 32767 + 10 * 32767 + 6 * 32768 + 32768        # 688,114
AWESH4_MIN = -(4 * 32768 + 10 * 32768 + 6 * 32767 + 32767)     # -688,121
AWGT = tuple(dict.fromkeys([0.0, 0.124, *_around(0.25), *_around(-0.25), 0.1, -0.3, 1e-290, -1e-290, 172031.75, 172032.0,
                            1e5, -1e5, 1e9, -1e9, 1e100, -1e100])) + (-0.0,)
# (green, nir, swir1): plain, negative, the extremes of 10 g - 6 wrap16(nir + swir1) both ways, and nir + swir1 wrapping
AWESH_BASES = ((400, 300, 100), (-5, 7, -3), (32767, -32768, 0), (-32768, 32767, 0), (1000, 32767, 5), (0, 20000, 20000),
               (-32768, -30000, -30000))


def awesh4(blue, green, nir, swir1, swir2):
    """4 * AWESH as the exact integer 4 b + 10 g - 6 wrap16(nir + swir1) - s2."""
    i = lambda a: np.asarray(a, np.int64)
    return 4 * i(blue) + 10 * i(green) - 6 * wrap16(i(nir) + i(swir1)) - i(swir2)


def awesh_targets(awgt):
    """The values of 4 * AWESH a threshold is probed with, clamped to what is reachable."""
    f = math.floor(4.0 * awgt)
    f = int(max(min(f, 10 ** 7), -10 ** 7))
    want = {f - 1, f, f + 1, f + 2, AWESH4_MIN, AWESH4_MAX} | set(range(-8, 9))
    return sorted({max(AWESH4_MIN, min(AWESH4_MAX, v)) for v in want})


def awesh_tile(awgt):
    """Pixels whose 4 * AWESH takes awesh_targets(awgt) (where a base can reach a value): for every base the blue / swir2
    that give the target -- swir2 takes the remainder mod 4 and what blue cannot reach -- padded to a multiple of 56 pixels.
    red is 200.  Returns six int16 planes of [1, N]."""
    rows = []
    for g, n, s1 in AWESH_BASES:
        base = 10 * g - 6 * int(wrap16(n + s1))
        for v in awesh_targets(awgt):
            rest = v - base                               # = 4 b - s2
            for s2_0 in (0, 32767, -32768):
                s2 = s2_0 - (s2_0 + rest) % 4                # s2 = -rest (mod 4), at or just below s2_0
                if s2 < -32768:
                    s2 += 4
                b = (rest + s2) // 4
                if (rest + s2) % 4 == 0 and -32768 <= b <= 32767 and -32768 <= s2 <= 32767:
                    rows.append((b, g, 200, n, s1, s2))
    a = np.array(rows, np.int64)
    pad = -len(rows) % 56
    a = np.concatenate([a, np.repeat(a[-1:], pad, axis=0)])
    return [np.ascontiguousarray(a[:, k].astype(np.int16).reshape(1, -1)) for k in range(6)]


# ---- parameter sets -------------------------------------------------------------------------------------------------------
# the integer thresholds out of the way (every "band < t" holds), so that DIAG bits 0, 3 and 4 are quotient tests
INT_OFF = dict(pswt_1_nir=1e9, pswt_1_swir1=1e9, pswt_2_blue=1e9, pswt_2_nir=1e9, pswt_2_swir1=1e9, pswt_2_swir2=1e9,
               lcmask_nir=1200.0, awgt=0.0)


def _fmt(t):
    """A threshold in a test id: its repr where that is short, else its hex form (both unique per double)."""
    return repr(float(t)) if len(repr(float(t))) <= 8 else float(t).hex()


def _sets_of(values, idle):
    """[(id, (wigt, pswt_1_mndwi, pswt_2_mndwi), pswt_1_ndvi, thresholds with an MNDWI section)]: `values` three to a set as
    the MNDWI thresholds, the first of the three as the NDVI threshold too; then, for each of the other two, a set with an
    NDVI section only (MNDWI thresholds `idle`).  A last set that is not full is padded with idle[0], which gets no section."""
    trios = [tuple(values[i:i + 3]) for i in range(0, len(values), 3)]
    full = [(' '.join(map(_fmt, trio)), (trio + (idle[0],) * 2)[:3], trio[0], trio) for trio in trios]
    ndvi_only = [(f'ndvi {_fmt(t)}', tuple(idle), t, ()) for trio in trios for t in trio[1:]]
    return full + ndvi_only


def quotient_sets():
    """Every value of THRESHOLDS once as an MNDWI threshold and once as the NDVI threshold; first the defaults and the
    zeros as sets of their own."""
    named = [('defaults', DEFAULTS[:3], DEFAULTS[3], DEFAULTS[:3]), ('zeros', (0.0, -0.0, 0.0), -0.0, (0.0, -0.0)),
             ('zero ndvi', DEFAULTS[:3], 0.0, ())]
    return named + _sets_of(THRESHOLDS, DEFAULTS[:3])


def clip_sets():
    """The thresholds in (0, 1), for the runs with the default clip.  Those above 0.9999 come first in their set, the wigt
    slot: as pswt_1_mndwi they would fail the constant MNDWI of the NDVI section (see _GREEN_SWIR1_PASS_CLIP)."""
    vals = [t for t in THRESHOLDS if 0.0 < t < 1.0]
    big, small = [t for t in vals if t >= 0.9999], [t for t in vals if t < 0.9999]
    k = len(big)
    head = [t for trio in zip(big, small[0:2 * k:2], small[1:2 * k:2]) for t in trio]
    return _sets_of(head + small[2 * k:], (DEFAULTS[0],) * 3)


def thresholds_of(mndwi3, ndvi, **more):
    """The twelve thresholds of a set as a dict."""
    return dict(INT_OFF, wigt=mndwi3[0], pswt_1_mndwi=mndwi3[1], pswt_2_mndwi=mndwi3[2], pswt_1_ndvi=ndvi, **more)
