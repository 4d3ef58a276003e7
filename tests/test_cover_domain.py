"""The named 'cover' domains of oracle/cover_inputs.py, on the CPU alone: the numpy oracle's scipy dilation against its
second statement (shifted arrays, oracle/dswx_oracle.py masked_dilation_by_shifts) on every domain at every shape that
tests/test_gpu_cover_domain.py runs, and the proof that each domain does what it is for -- the dilations change CLOUD, the
corridors' snow ends exactly 10 cells past its seed, and the near pixel of every 17-pixel chain follows its far seed.
A windowed restatement of the device code (cover_inputs.windowed_cloud) shows that the chains tell a halo of 17 from one
of 16, 15 or 14."""
import functools

import numpy as np
import pytest

from oracle import cover_inputs as ci
from oracle import dswx_oracle as o

from oracle.cover_inputs import (KERNEL_SHAPES, THIN_SHAPES, ENTRY_SHAPES, STALE_SHAPES, SNOW, CLEAR,       # noqa: E402
                                 expected)


def all_cases():
    """Every (domain, H, W, nw) that a GPU test classifies."""
    out = []
    for dom in ci.DOMAINS:
        for nw, shapes in KERNEL_SHAPES.items():
            out += [(dom, h, w, (nw,)) for h, w in shapes]
        out += [(dom, h, w, (8, 4)) for h, w in THIN_SHAPES + ENTRY_SHAPES + STALE_SHAPES]
    return out


@functools.lru_cache(maxsize=None)
def _cloud(dom, h, w, nw, k=0, mode='cover'):
    return expected(ci.scenes(dom, h, w, nw)[k], False, mode)['CLOUD']


@pytest.mark.parametrize('dom', ci.DOMAINS)
def test_second_statement_of_the_dilation(dom):
    """scipy's binary_dilation and the shifted-array statement give the same layers on every domain at every shape."""
    n = 0
    for _, h, w, nw in [c for c in all_cases() if c[0] == dom]:
        for k, scene in enumerate(ci.scenes(dom, h, w, nw)):
            for edge in (False, True):
                s = ci.with_edge_rows(scene) if edge else scene
                a, b = expected(s), expected(s, binary_dilation=o.masked_dilation_by_shifts)
                for layer in ('DIAG', 'WTR-1', 'WTR-1-AEROSOL', 'WTR-2', 'WTR', 'BWTR', 'CONF', 'CLOUD'):
                    assert np.array_equal(a[layer], b[layer]), (dom, h, w, k, edge, layer)
                assert a['counters'] == b['counters']
                n += 1
    assert n >= 2 * len(THIN_SHAPES)


def test_second_statement_alone():
    """The statement itself on known answers: a diamond of radius n after n steps, the raster edge, a mask that is
    left alone outside and respected inside."""
    x = np.zeros((9, 9), bool)
    x[4, 4] = True
    yy, xx = np.mgrid[0:9, 0:9]
    for n in range(6):
        assert np.array_equal(o.masked_dilation_by_shifts(x, n), np.abs(yy - 4) + np.abs(xx - 4) <= n)
    corner = np.zeros((3, 4), bool)
    corner[0, 3] = True
    assert o.masked_dilation_by_shifts(corner, 2).tolist() == [[0, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1]]
    mask = np.zeros((1, 6), bool)
    mask[0, 1:4] = True
    seed = np.array([[1, 0, 0, 0, 0, 1]], bool)             # the seed at 5 lies outside the mask and stays
    assert o.masked_dilation_by_shifts(seed, 10, mask).tolist() == [[1, 1, 1, 1, 0, 1]]
    assert o.masked_dilation_by_shifts(seed, 2, mask).tolist() == [[1, 1, 1, 0, 0, 1]]


@pytest.mark.parametrize('dom', ['diamonds', 'corridors', 'bytes256', 'holes'])
def test_the_dilations_change_cloud(dom):
    for nw, shapes in KERNEL_SHAPES.items():
        for h, w in shapes:
            cover, ignore = _cloud(dom, h, w, (nw,)), _cloud(dom, h, w, (nw,), mode='ignore')
            assert np.count_nonzero(cover != ignore) > 50, (dom, h, w)


def test_diamonds_cross_every_seam_and_stop_at_the_edge():
    for nw, shapes in KERNEL_SHAPES.items():
        for h, w in shapes:
            scene = ci.scenes('diamonds', h, w, (nw,))[0]
            snow = o.masked_dilation_by_shifts(scene['fmask'] == ci.SEED, 10, scene['fmask'] != ci.FILL)
            rows, cols = ci.seams(h, w, nw)
            assert rows or cols
            for s in rows:
                # seeds on both sides whose diamonds reach over the seam: snow of a seed at s - 11 stops at s - 1
                assert snow[s - 1].any() and snow[s].any() and (s - 11, 11) in scene['meta'][0]['seeds']
            for s in cols:
                assert snow[:, s - 1].any() and snow[:, s].any()
            assert snow[0, 0] and snow[h - 1, w - 1] and snow[0, 10] and not snow[0, 11] and snow[10, 0]


def test_corridor_snow_reaches_exactly_ten_cells():
    for nw, shapes in KERNEL_SHAPES.items():
        for h, w in shapes:
            scene = ci.scenes('corridors', h, w, (nw,))[0]
            cloud = _cloud('corridors', h, w, (nw,))
            rows, cols = ci.seams(h, w, nw)
            long_across = set()
            assert len(scene['meta']) >= 40, (h, w, len(scene['meta']))
            for c in scene['meta']:
                cells = c['cells']
                got = [int(cloud[y, x]) for y, x in cells]
                assert got == [SNOW] * min(11, len(cells)) + [CLEAR] * max(len(cells) - 11, 0), (h, w, c)
                if len(cells) >= 25:
                    ys, xs = [y for y, _ in cells[:11]], [x for _, x in cells[:11]]
                    for s in rows:
                        if min(ys) < s <= max(ys):
                            long_across.add(('row', s, c['dir']))
                    for s in cols:
                        if min(xs) < s <= max(xs):
                            long_across.add(('col', s, c['dir']))
            # the snow front itself crosses every seam in both directions of its axis, on corridors of 25 cells or more
            for s in rows:
                assert {('row', s, (1, 0)), ('row', s, (-1, 0))} <= long_across, (h, w, s, sorted(long_across))
            for s in cols:
                assert {('col', s, (0, 1)), ('col', s, (0, -1))} <= long_across, (h, w, s, sorted(long_across))
            assert any(c['turn'] and len(c['cells']) >= 25 for c in scene['meta'])


def test_chain17_near_pixel_follows_the_far_seed():
    for nw, shapes in KERNEL_SHAPES.items():
        for h, w in shapes:
            a, b = ci.scenes('chain17', h, w, (nw,))[0], ci.scenes('chain17_toggled', h, w, (nw,))[0]
            ca, cb = _cloud('chain17', h, w, (nw,)), _cloud('chain17_toggled', h, w, (nw,))
            rows, cols = ci.seams(h, w, nw)
            # every placement fits: 2 directions x 3 shifts x the seams of halos 17, 16, 15, 14, for every real seam
            assert len(a['meta']) == len(b['meta']) == 6 * len(ci.CHAIN_HALOS) * (len(rows) + len(cols)), (h, w, len(a['meta']))
            for pa, pb in zip(a['meta'], b['meta']):
                assert pa['cells'] == pb['cells'] and pa['far_seed'] != pb['far_seed']
                for p, cloud in ((pa, ca), (pb, cb)):
                    cells, near, far = p['cells'], p['near'], p['far']
                    assert abs(near[0] - far[0]) + abs(near[1] - far[1]) == ci.HALO
                    want = [SNOW] * len(cells) if p['far_seed'] else [SNOW] * 4 + [CLEAR] * (len(cells) - 4)
                    assert [int(cloud[c]) for c in cells] == want, (h, w, p)
                    assert (cloud[near] == SNOW) == p['far_seed']
            # c4 on the first and on the last output row / column of a window, c21 on the window's outermost halo; and
            # the same at the seams a halo of 16, 15, 14 would make (224 / 96, 226 / 98, 228 / 100 for the first seam)
            for axis, real, out in ((0, rows, 222), (1, cols, 32 * nw - 34)):
                for s17 in real:
                    for halo in ci.CHAIN_HALOS:
                        s = ci.seam_for_halo(s17, halo, out)
                        assert s17 % out == 0 and s == s17 + (s17 // out) * 2 * (17 - halo)
                        assert {(p['near'][axis], p['far'][axis]) for p in a['meta']
                                if p['axis'] == axis and p['shift'] == 0 and p['seam'] == s and p['halo'] == halo} == \
                            {(s, s - 17), (s - 1, s + 16)}, (h, w, s17, halo)


@pytest.mark.parametrize('dom', ci.DOMAINS)
def test_windows_with_halo_17_give_the_oracles_answer(dom):
    """The windowed restatement (what the device code does, stated with the oracle's own dilation) is exact at halo 17, on
    every domain, for both window widths."""
    for nw, shapes in KERNEL_SHAPES.items():
        for h, w in shapes:
            for k, scene in enumerate(ci.scenes(dom, h, w, (nw,))):
                assert np.array_equal(ci.windowed_cloud(scene, 17, nw), _cloud(dom, h, w, (nw,), k)), (dom, h, w, k)


@pytest.mark.parametrize('halo', [16, 15, 14])
def test_chains_tell_a_smaller_halo_from_17(halo):
    """A kernel built with a halo of 16 (15, 14) is self-consistent -- its output size follows its halo -- and wrong only
    for a 17-pixel dependency across ITS seams.  Every chain aimed at such a seam (shift 0) that carries its far seed
    comes out wrong at its near pixel under that halo; chain17 and chain17_toggled together carry the far seed on every
    placement."""
    for nw, shapes in KERNEL_SHAPES.items():
        for h, w in shapes:
            wrong = 0
            for dom in ('chain17', 'chain17_toggled'):
                scene = ci.scenes(dom, h, w, (nw,))[0]
                truth, got = _cloud(dom, h, w, (nw,)), ci.windowed_cloud(scene, halo, nw)
                for p in scene['meta']:
                    if p['halo'] == halo and p['shift'] == 0 and p['far_seed']:
                        assert truth[p['near']] == SNOW and got[p['near']] == CLEAR, (halo, nw, h, w, p)
                        wrong += 1
            rows, cols = ci.seams(h, w, nw)
            assert wrong == 2 * (len(rows) + len(cols)), (halo, nw, h, w, wrong)


def test_bytes256_and_saturated_are_what_they_say():
    for h, w in [(250, 250), (160, 112), (250, 140)]:
        s = ci.scenes('bytes256', h, w)[0]
        assert len(np.unique(s['fmask'])) == 256 and 3 <= s['meta'][0]['smax'] <= 20
        assert s['water'].any() and not s['water'].all()
    snow, none, checker, row = ci.scenes('saturated', 60, 70)
    assert (_cloud('saturated', 60, 70, (8,), 0) == SNOW).all() and (_cloud('saturated', 60, 70, (8,), 1) == CLEAR).all()
    c = _cloud('saturated', 60, 70, (8,), 2)
    assert np.array_equal(c == SNOW, checker['fmask'] == ci.SEED) and (checker['fmask'] == ci.SEED).sum() > 100
    c = _cloud('saturated', 60, 70, (8,), 3)
    # (byte 255 has the snow bit: the fill rows either side seed the whole row in one step)
    assert (np.delete(c, 30, axis=0) == 255).all() and set(c[30].tolist()) == {SNOW}
    assert (row['fmask'] != ci.FILL).sum() == 70


def test_holes_masks_cut_through_the_diamonds():
    for h, w, nw in [(250, 250, 8), (250, 220, 4)]:
        s = ci.scenes('holes', h, w, (nw,))[0]
        base = dict(s, ocean=None, shad=None)
        full, cut = expected(s, False)['CLOUD'], expected(base, False)['CLOUD']
        assert np.count_nonzero(full != cut) > 50                  # ocean and shadow change the result
        assert (s['fmask'] == ci.FILL).sum() > 50 and (s['ocean'] == 0).sum() > 50 and (s['shad'] == 0).sum() > 50
