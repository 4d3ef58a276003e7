"""The named shadow domains of oracle/shadow_inputs.py, on the CPU alone: every case runs through the numpy oracle in both
promotions, and each domain does what it is for -- the thresholds cut through the data where the terrain is steep enough
for that, the `on_threshold` cases have at least a hundred pixels inside the filter's uncertainty band, the mixed-scale DEM
has pixels on both sides of the filter's S < 2^60 gate, and the two promotions are told apart.  These are the conditions
that keep tests/test_gpu_shadow_domain.py from passing vacuously.  Run with -s to see the figures."""
import numpy as np
import pytest

from oracle import shadow_inputs as si

MARGIN = 3        # the smaller of the two margins the GPU tests give the filter kernel an odd and an even one with: 3, 2


def _fraction(case, legacy):
    return 1.0 - float(si.expected(case, legacy, MARGIN).mean())


@pytest.mark.parametrize('domain', si.DOMAINS)
def test_every_case_runs_through_the_oracle_in_both_promotions(domain):
    names = [c.name for c in si.cases(domain)]
    assert len(set(names)) == len(names)
    for c in si.cases(domain):
        assert c.dem.dtype == np.float32 and c.dem.flags.c_contiguous
        assert all(type(v) is float for v in c[2:]), c.name          # Python floats, as the reference's caller passes them
        for legacy in (False, True):
            for margin in (0, MARGIN):
                e = si.expected(c, legacy, margin)
                assert e.dtype == np.uint8 and e.shape == (c.dem.shape[0] - 2 * margin, c.dem.shape[1] - 2 * margin)
                assert set(np.unique(e).tolist()) <= {0, 1}
            print(f'{domain} {c.name} {"legacy" if legacy else "nep50"}: shadow fraction {_fraction(c, legacy):.3f}')


def test_domains_hold_what_the_issue_lists():
    mag = [c.name for c in si.cases('magnitudes')]
    assert [f'scale_{s:g}' for s in (1e-30, 1e-12, 1e-3, 1, 1e3, 1e6, 1e9, 1e12, 1e15, 1e18, 1e19, 1e25)] == mag[:12]
    assert {'mixed_scales', 'offset_8000', 'zeros_denormals', 'special_pixels', 'special_rows_columns', 'special_blocks'} <= set(mag)
    off = si.case('magnitudes', 'offset_8000').dem
    assert off.min() >= 7999.99 and off.max() <= 8000.01 and len(np.unique(off)) > 20
    for name in ('special_pixels', 'special_rows_columns', 'special_blocks'):
        bits = set(si.case('magnitudes', name).dem.view(np.uint32).ravel().tolist())
        for key, v in si.SPECIALS.items():
            assert int(np.array([v], np.float32).view(np.uint32)[0]) in bits, (name, key)
    assert np.signbit(si.SPECIALS['neg_nan']) and np.isnan(si.SPECIALS['neg_nan']) and not np.signbit(si.SPECIALS['nan'])
    assert {(c.sx, c.sy) for c in si.cases('spacings')} == {
        (30.0, -30.0), (-30.0, 30.0), (-30.0, -30.0), (2.77e-4, 2.77e-4), (30.1, 1 / 3), (1e-20, 1e20), (1e30, 1e30),
        (3e38, 1e-38), (0.0, 30.0)}
    sun = si.cases('sun')
    assert {(c.el, c.az) for c in sun} == {(el, az) for el in (0, 1e-6, 45, 89.999, 90, -10, 100)
                                           for az in (0, 90, 180, 270, 360, -45, 720.5)}
    assert {c.min_slope for c in sun} == {0, -5, 5, -90, 90, 1e-30, -1e-30}
    assert {0.0, 90.0, 180.0, -1.0} <= {c.max_inc for c in sun} and any(c.max_inc == 90.0 - c.el for c in sun)
    for el, az in {(c.el, c.az) for c in sun}:                        # both terrains under every sun
        assert {c.name.split('_')[2] for c in sun if (c.el, c.az) == (el, az)} == {'rough', 'gentle'}
    assert set(si.GEOMETRY_SHAPES) == {(oh, ow) for oh in range(1, 18) for ow in list(range(1, 10)) + [255, 256, 257, 260, 261]}
    assert si.GEOMETRY_MARGINS == (0, 1, 2, 3, 50)
    assert max(c.dem.shape[0] for d in si.DOMAINS for c in si.cases(d)) <= 300
    assert max(c.dem.shape[1] for d in si.DOMAINS for c in si.cases(d)) <= 420


def test_thresholds_cut_through_the_data():
    """Shadow fraction strictly between 0.02 and 0.98 in both promotions: `magnitudes` at scales 1e3 ... 1e25, `spacings`
    but (1e30, 1e30), `on_threshold`, and the geometry tiles (about half).  (Scales <= 1e-3 and spacing 1e30 are flat
    ground at these thresholds: all 'not shadow'.)"""
    todo = [c for c in si.cases('magnitudes') if c.name.startswith('scale_') and float(c.name[6:]) >= 1e3]
    assert len(todo) == 8
    todo += [c for c in si.cases('spacings') if (c.sx, c.sy) != (1e30, 1e30)]
    todo += list(si.cases('on_threshold')) + list(si.cases('geometry'))
    for c in todo:
        for legacy in (False, True):
            f = _fraction(c, legacy)
            print(f'{c.name} {"legacy" if legacy else "nep50"}: shadow fraction {f:.3f}')
            assert 0.02 < f < 0.98, (c.name, legacy, f)
    for c in si.cases('geometry'):
        assert 0.4 < _fraction(c, False) < 0.6, c.name
    # ... and under the edge suns too, on a good part of the cases
    cut = sum(0.02 < _fraction(c, False) < 0.98 for c in si.cases('sun'))
    print(f'sun: {cut} of {len(si.cases("sun"))} cases with a shadow fraction in (0.02, 0.98)')
    assert cut >= 30


def test_on_threshold_cases_sit_inside_the_uncertainty_band():
    """At least 100 pixels per case with |q - inc_q_min| <= 4e-6 or |t - slope_arg_max| <= 2^-18 (|n0 sin| + |n1 cos|),
    counted in float64; across the domain both bands are populated, and the two promotions differ somewhere."""
    n_q = n_t = n_differ = 0
    for c in si.cases('on_threshold'):
        in_q, in_t, either = si.band_counts(c, MARGIN)
        differ = int(np.count_nonzero(si.expected(c, False, MARGIN) != si.expected(c, True, MARGIN)))
        print(f'on_threshold {c.name}: min_slope {c.min_slope:.9g} max_inc {c.max_inc:.9g}: {in_q} pixels in the q band, '
              f'{in_t} in the t band, {either} in either; nep50 and legacy differ on {differ}')
        assert either >= 100, (c.name, in_q, in_t, either)
        n_q, n_t, n_differ = n_q + in_q, n_t + in_t, n_differ + differ
    assert n_q >= 100 and n_t >= 100
    assert n_differ >= 1


def test_mixed_scales_straddle_the_sane_gate_and_the_overflow():
    c = si.case('magnitudes', 'mixed_scales')
    _, _, n0, n1 = (a[MARGIN:-MARGIN, MARGIN:-MARGIN] for a in si.arguments(c))
    S = n0 ** 2 + n1 ** 2 + 1
    below, above = S < si.S_SANE, S >= si.S_SANE
    overflow = (n0 ** 2 > si.FLT_MAX) | (n1 ** 2 > si.FLT_MAX)
    print(f'mixed_scales: {int(below.sum())} interior pixels with S < 2^60, {int(above.sum())} with S >= 2^60, '
          f'{int(overflow.sum())} whose n0^2 or n1^2 overflows float32')
    assert below.sum() >= 100 and above.sum() >= 100 and overflow.sum() >= 100
    # side by side: some aligned group of four pixels (a quad of the filter kernel at margin 3) has both kinds
    quads = below[:, :below.shape[1] // 4 * 4].reshape(below.shape[0], -1, 4)
    assert np.any(quads.any(axis=2) & ~quads.all(axis=2))
    # the single-scale cases: 1e3 ... 1e9 stay below the gate (the filter decides), 1e12 and up are above it everywhere
    # the terrain is not flat
    for s, filt in ((1e3, True), (1e6, True), (1e9, True), (1e12, False), (1e19, False)):
        _, _, n0, n1 = si.arguments(si.case('magnitudes', f'scale_{s:g}'))
        assert bool(np.median(n0 ** 2 + n1 ** 2 + 1) < si.S_SANE) == filt, s


def test_geometry_cut_from_the_whole_tile_is_the_oracle_on_the_cut():
    """geometry_expected cuts the layers of a case with a margin from the oracle's layer of the whole tile; the oracle
    run on the cut itself gives the same."""
    for oh, ow in ((1, 1), (1, 4), (2, 7), (9, 5), (17, 257), (8, 261)):
        for margin in (1, 2, 3, 50):
            for legacy in (False, True):
                dems = si.geometry_dems(oh, ow, margin)
                assert dems.shape == (si.GEOMETRY_TILES, oh + 2 * margin, ow + 2 * margin)
                direct = np.stack([si.expected(c._replace(dem=dems[t]), legacy, margin)
                                   for t, c in enumerate(si.cases('geometry'))])
                assert np.array_equal(si.geometry_expected(oh, ow, margin, legacy), direct), (oh, ow, margin, legacy)
    assert si.geometry_expected(2, 2, 0, False).shape == (si.GEOMETRY_TILES, 2, 2)
