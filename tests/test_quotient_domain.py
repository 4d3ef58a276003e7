"""The threshold domain of the quotient and AWESH tests on the CPU (oracle/quotient_inputs.py): that the builder's pixels
separate every threshold from its neighbours, that the scalar C oracle (true division) agrees with numpy's
n / d > t, n / d < t and awesh > awgt on every one of its sets, and that both device forms of the division-free predicate
-- restated in oracle/dswx_oracle.c -- equal the reference on the builder's pairs of every threshold."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import c_oracle
from oracle import quotient_inputs as qi
from proteus_amd import _capi
from tests.test_c_oracle import binary_repr

IDS = [qi._fmt(t) for t in qi.THRESHOLDS]


def quotient(n, d):
    with np.errstate(all='ignore'):
        return n.astype(np.float64) / d.astype(np.float64)


# ---- the builder's invariants -------------------------------------------------------------------------------------------
def test_threshold_list():
    T = qi.THRESHOLDS
    keys = {qi._key(t) for t in T}
    assert len(keys) == len(T)
    must = [0.0, -0.0, *qi.DEFAULTS, 1 / 3, 2 / 3, 0.1, 1e-5, 1e-290, -1e-290, 32768.5, 65536.0, 1e9, 1e100, -1e100]
    for t in (0.125, -0.125, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -7.5, 2.0 ** -15, 32767.0, -32767.0, 32768.0,
              -32768.0, 32767 / 32768, 1 / 32767):
        must += [t, math.nextafter(t, math.inf), math.nextafter(t, -math.inf)]
    assert len(qi.RANDOM_PAIRS) == 32
    for n0, d0 in qi.RANDOM_PAIRS:
        assert (n0 - d0) % 2 == 0 and d0 != 0
        must += [n0 / d0, math.nextafter(n0 / d0, math.inf), math.nextafter(n0 / d0, -math.inf)]
    for t in must:
        assert qi._key(t) in keys, t
    # all inside what dswx_make_dev_params accepts
    assert all(t == 0.0 or 1e-290 <= abs(t) <= 1e100 for t in T)
    used_m = [qi._key(t) for s in qi.quotient_sets() for t in s[3]]
    used_v = [qi._key(s[2]) for s in qi.quotient_sets()]
    assert set(used_m) >= keys and set(used_v) >= keys         # every threshold on a > test and on the < test
    for sets in (qi.quotient_sets(), qi.clip_sets()):
        ids = [s[0] for s in sets]
        assert len(set(ids)) == len(ids)
        assert all(len(s[1]) == 3 and set(map(qi._key, s[3])) <= set(map(qi._key, s[1])) for s in sets)
    in_clip = {qi._key(t) for s in qi.clip_sets() for t in s[3]}
    assert in_clip == {qi._key(t) for t in T if 0.0 < t < 1.0} == {qi._key(s[2]) for s in qi.clip_sets()}


@pytest.mark.parametrize('t', qi.THRESHOLDS, ids=IDS)
def test_pairs_of_a_threshold(t):
    n, d = qi.pairs(t)
    assert n.size <= qi.PIXEL_CAP
    assert len(set(zip(n[:1000].tolist(), d[:1000].tolist()))) == min(n.size, 1000)
    # reachable, and the planes give the pairs back through the int16 wrap
    assert not ((n - d) & 1).any() and n.min() >= -32768 and n.max() <= 32767 and d.min() >= -32768 and d.max() <= 32767
    a, b = qi.planes_of_pairs(n, d)
    assert a.dtype == np.int16 and b.dtype == np.int16
    with np.errstate(over='ignore'):
        assert np.array_equal((a - b).astype(np.int64), n) and np.array_equal((a + b).astype(np.int64), d)   # int16 arithmetic wraps
    wrapped = (a.astype(np.int64) + b != d) | (a.astype(np.int64) - b != n)
    assert wrapped.any() and not wrapped.all()
    assert (d == 0).any()
    q = quotient(n, d)
    finite = np.isfinite(q)
    for less in (False, True):
        ref = (q < t) if less else (q > t)
        if abs(t) == 32767 and less == (t < 0):
            # the one quotient beyond +-32767, -32768 / -1 (-32768 / 1), has n even and d odd: not reachable.  The largest
            # reachable quotient is 32767 / 1 itself, which must compare equal: neither greater nor less
            assert not ref[finite].any() and (q == t).any(), (t, less)
        elif abs(t) <= 32767:
            assert ref[finite].any() and not ref[finite].all(), (t, less)
        elif abs(t) > 32767:
            # beyond every reachable quotient (32768 = -32768 / -1 is not one): one outcome only (n / 0 = +-inf aside)
            assert (ref[finite] == ((t > 0) == less)).all(), (t, less)
    if qi.exact_pair(t) is not None:
        assert np.count_nonzero(q == t) >= 8, t
        n0, d0 = qi.exact_pair(t)
        hit = set(zip(n[q == t].tolist(), d[q == t].tolist()))
        assert {(k * n0, k * d0) for k in (1, -1, 2, -2, 3, -3, 4, -4)} <= hit
    if qi.random_pair_of(t) is None:
        # for every d the two reachable n on each side of t * d (t * d itself counts as below), as far as int16 goes
        for dv in (1, -1, 2, 3, -32768, 32767, 12345, -20001):
            have = set(n[d == dv].tolist())
            x = min(max(Fraction(t) * dv, -40000), 40000)                 # exact
            m = math.floor(x) - (math.floor(x) - dv) % 2                   # the largest reachable n <= t * d
            near = [v for v in (m - 2, m, m + 2, m + 4) if -32768 <= v <= 32767]
            assert set(near) <= have and (len(near) == 4 or abs(x) > 32760), (t, dv)
            assert {v for v in qi.N_FIXED if (v - dv) % 2 == 0} <= have


def test_neighbour_thresholds_flip_exactly_one_test():
    """At t = fl64(n0 / d0) both tests are false on the multiples of (n0, d0); at nextafter(t, +inf) only '<' turns true
    there, at nextafter(t, -inf) only '>'."""
    for n0, d0 in qi.RANDOM_PAIRS:
        t = n0 / d0
        k = np.array([1, -1, 2, -2, 3, -3, 4, -4])
        q = quotient(k * n0, k * d0)
        assert (q == t).all()
        up, dn = math.nextafter(t, math.inf), math.nextafter(t, -math.inf)
        assert not (q > t).any() and not (q < t).any()
        assert (q < up).all() and not (q > up).any() and (q > dn).all() and not (q < dn).any()


@pytest.mark.parametrize('awgt', qi.AWGT, ids=[qi._fmt(t) for t in qi.AWGT])
def test_awesh_pixels(awgt):
    b, g, r, n, s1, s2 = qi.awesh_tile(awgt)
    v = qi.awesh4(b, g, n, s1, s2)
    got = set(v.ravel().tolist())
    f = math.floor(4.0 * awgt)
    for want in (f, f + 1):
        if qi.AWESH4_MIN <= want <= qi.AWESH4_MAX:
            assert want in got, (awgt, want)
    assert {qi.AWESH4_MIN, qi.AWESH4_MAX} <= got and set(range(-8, 9)) <= got
    assert b.size % 56 == 0
    wraps = n.astype(np.int64) + s1 != qi.wrap16(n.astype(np.int64) + s1)
    assert wraps.any() and not wraps.all()
    awesh = 0.25 * v
    if abs(4.0 * awgt) < qi.AWESH4_MAX:
        assert (awesh > awgt).any() and not (awesh > awgt).all()


# ---- the C oracle against numpy -----------------------------------------------------------------------------------------
def numpy_diag(bands, thr):
    """DIAG of the five tests with numpy's float64 true division (clip off, no fills), as the saved decimal digits."""
    b, g, r, n, s1, s2 = [x.astype(np.int64) for x in bands]
    w = qi.wrap16
    mndwi, ndvi = quotient(w(g - s1), w(g + s1)), quotient(w(n - r), w(n + r))
    mbsrv, mbsrn = w(g + r), w(n + s1)
    awesh = b + 2.5 * g - 1.5 * mbsrn - 0.25 * s2
    t1 = mndwi > thr['wigt']
    t2 = mbsrv > mbsrn
    t3 = awesh > thr['awgt']
    t4 = (mndwi > thr['pswt_1_mndwi']) & (s1 < thr['pswt_1_swir1']) & (n < thr['pswt_1_nir']) & (ndvi < thr['pswt_1_ndvi'])
    t5 = (mndwi > thr['pswt_2_mndwi']) & (b < thr['pswt_2_blue']) & (s1 < thr['pswt_2_swir1']) & \
        (s2 < thr['pswt_2_swir2']) & (n < thr['pswt_2_nir'])
    bits = t1 * 1 + t2 * 2 + t3 * 4 + t4 * 8 + t5 * 16
    return binary_repr(bits), (mndwi, ndvi)


def plain_params(thr, **kw):
    return _capi.make_params(thr, band_fills=[None] * 6, fmask_fill=None, clip_negative_reflectance=False, **kw)


SETS = qi.quotient_sets()


@pytest.mark.parametrize('k', range(len(SETS)), ids=[s[0] for s in SETS])
def test_c_oracle_against_numpy_on_quotient_sets(k):
    _, m3, v, sections = SETS[k]
    bands, secs = qi.tile(sections, v)
    thr = qi.thresholds_of(m3, v)
    want, (mndwi, ndvi) = numpy_diag(bands, thr)
    got = c_oracle.classify(plain_params(thr), bands, np.zeros(bands[0].shape, np.uint8), layers=('diag',))['diag']
    assert np.array_equal(got, want)
    # in its own section a DIAG digit is one quotient test
    digit = lambda i: (want.ravel() // 10 ** i) % 10
    for (kind, t, lo, hi), slot in zip(secs, (0, 3, 4, 3)):
        if kind == 'ndvi':
            assert np.array_equal(digit(3)[lo:hi], (ndvi.ravel() < t)[lo:hi])
            assert np.isposinf(mndwi.ravel()[lo:hi]).all()
        else:
            assert np.array_equal(digit(slot)[lo:hi], (mndwi.ravel() > t)[lo:hi]), (kind, t, slot)
            assert np.isneginf(ndvi.ravel()[lo:hi]).all()


CLIP_SETS = qi.clip_sets()


@pytest.mark.parametrize('k', range(len(CLIP_SETS)), ids=[s[0] for s in CLIP_SETS])
def test_c_oracle_against_numpy_on_clipped_sets(k):
    """The sets of the default clip: every plane >= 1, so the clip leaves them as drawn and the two settings agree."""
    _, m3, v, sections = CLIP_SETS[k]
    assert all(0.0 < t < 1.0 for t in m3 + (v,)) and m3[1] < 0.9999
    bands, secs = qi.tile(sections, v, clip=True)
    assert min(int(b.min()) for b in bands) >= 1 and all(hi - lo > 100_000 or qi.random_pair_of(t) for _, t, lo, hi in secs)
    thr = qi.thresholds_of(m3, v)
    want, (mndwi, ndvi) = numpy_diag(bands, thr)
    fm = np.zeros(bands[0].shape, np.uint8)
    for clip in (True, False):
        p = _capi.make_params(thr, band_fills=[None] * 6, fmask_fill=None, clip_negative_reflectance=clip)
        assert np.array_equal(c_oracle.classify(p, bands, fm, layers=('diag',))['diag'], want)
    for kind, t, lo, hi in secs:
        q = (ndvi if kind == 'ndvi' else mndwi).ravel()[lo:hi]
        ref = q < t if kind == 'ndvi' else q > t
        # (planes >= 1 reach no quotient above 32766 / 32768: -32766 / -32768 of green 1, swir1 32767)
        assert (not ref.all() if kind == 'mndwi' else ref.any()) and (t >= 0.9999 or (ref.any() and not ref.all())), (kind, t)
    # the constant bands pass the other quotient tests: digit 3 is the swept test in the pswt_1 sections
    digit3 = (want.ravel() // 1000) % 10
    for (kind, t, lo, hi), slot in zip(secs, (0, 3, 4, 3)):
        if kind == 'ndvi':
            assert np.array_equal(digit3[lo:hi], (ndvi.ravel() < t)[lo:hi])
        elif slot == 3:
            assert np.array_equal(digit3[lo:hi], (mndwi.ravel() > t)[lo:hi])


@pytest.mark.parametrize('awgt', qi.AWGT, ids=[qi._fmt(t) for t in qi.AWGT])
def test_c_oracle_against_numpy_on_awesh_sets(awgt):
    bands = qi.awesh_tile(awgt)
    thr = qi.thresholds_of(qi.DEFAULTS[:3], qi.DEFAULTS[3], awgt=awgt)
    want, _ = numpy_diag(bands, thr)
    got = c_oracle.classify(plain_params(thr), bands, np.zeros(bands[0].shape, np.uint8), layers=('diag', 'awesh'))
    assert np.array_equal(got['diag'], want)
    v = qi.awesh4(bands[0], bands[1], bands[3], bands[4], bands[5])
    assert np.array_equal(got['awesh'], 0.25 * v)
    assert np.array_equal((want // 100) % 10, 0.25 * v > awgt)


# ---- both device forms of the predicate on the builder's pairs ----------------------------------------------------------
@pytest.mark.parametrize('t', qi.THRESHOLDS, ids=IDS)
def test_both_predicate_forms_on_the_pairs(t):
    n, d = qi.pairs(t)
    for less in (0, 1):
        for forms in (1, 2):
            bad, first = c_oracle.check_quotient_pairs(t, less, n, d, forms=forms)
            assert bad == 0, (t, less, forms, first)
