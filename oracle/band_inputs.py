"""TEST INFRASTRUCTURE -- seeded draws of the six int16 reflectance planes over their whole range, shared by
oracle/gen_golden.py and tests/test_gpu_band_domain.py.

synth_tile (the product's synthetic scenes, matched bit for bit by the device generator) draws band values near
realistic means: its only int16 wraps are on green and swir1, and no band is ever -32768, 32767 or between -9999 and
-256.  These functions rewrite the six band planes of a synth_tile into named domains; Fmask, the mask planes and the
tile geometry stay as in the recipe.

  int16      uniform over -32768..32767, every band
  positive   uniform over 1..32767: all four int16 sums (g +- s1, n +- r, g + r, n + s1) wrap often
  edges      per pixel and band a pick from EDGES, plus every band threshold of the parameter set in use +-1
  mix        per pixel the recipe, `edges` or `int16` (realistic WTR classes next to edge values)
  f32_ties   for flag_offset_and_scale_inputs: values equal to a band's offset, and pairs that cancel exactly in float32
             (fg + fs1 == 0, fn + fr == 0, fg == fs1 == 0): +-inf and NaN indices
"""
import numpy as np

BAND_NAMES = ('blue', 'green', 'red', 'nir', 'swir1', 'swir2')
EDGES = (-32768, -32767, -9999, -256, -1, 0, 1, 2, 999, 1000, 1001, 1199, 1200, 1201, 1499, 1500, 2499, 2500,
         16383, 16384, 16385, 32766, 32767)
# the threshold that compares each band with a constant (HlsThresholds names; aerosol_max_nir is a parameter)
BAND_THRESHOLDS = {'blue': ('pswt_2_blue',), 'green': (), 'red': (),
                   'nir': ('pswt_1_nir', 'pswt_2_nir', 'lcmask_nir', 'aerosol_max_nir'),
                   'swir1': ('pswt_1_swir1', 'pswt_2_swir1'), 'swir2': ('pswt_2_swir2',)}
DOMAINS = ('recipe', 'int16', 'positive', 'edges', 'mix', 'f32_ties')


def edge_values(band, thr=None):
    """EDGES plus floor(t) - 1 .. ceil(t) + 1 of every threshold `thr` (dict) holds for `band`, inside int16."""
    vals = set(EDGES)
    for name in BAND_THRESHOLDS[band]:
        t = (thr or {}).get(name)
        if t is None or not np.isfinite(t):
            continue
        for v in range(int(np.floor(t)) - 1, int(np.ceil(t)) + 2):
            if -32768 <= v <= 32767:
                vals.add(v)
    return np.array(sorted(vals), np.int16)


def _cancel(a_vals, sa, oa, sb, ob):
    """For each value a, the int16 b whose float32 sb * (b - ob) is exactly -(sa * (a - oa)) where one exists (else the
    nearest b: a denominator of a few ulps)."""
    f32 = np.float32
    fa = f32(sa) * (a_vals.astype(f32) - f32(oa))
    with np.errstate(all='ignore'):
        b = np.where(sb != 0, np.rint(f32(ob) - fa.astype(np.float64) / (sb if sb != 0 else 1.0)), ob)
    b = np.clip(np.nan_to_num(b, nan=0.0), -32768, 32767).astype(np.int16)
    return b


def f32_ties(rng, shape, scale_offset):
    """Band planes for the float32 chain with `scale_offset` = six (scale_factor, add_offset) pairs: per pixel one of
    uniform int16 values, values equal to a band's offset (f == 0), green / swir1 and nir / red pairs that cancel
    (fg + fs1 == 0, fn + fr == 0; exact where float32 allows), both members of a pair at the offset (0 / 0), and edges."""
    n = int(np.prod(shape))
    out = [rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(6)]
    kind = rng.integers(0, 6, (6, n))
    for k, (sf, off) in enumerate(scale_offset):
        at_off = int(np.clip(np.rint(off), -32768, 32767))
        out[k] = np.where(kind[k] == 1, np.int16(at_off), out[k])
        out[k] = np.where(kind[k] == 2, rng.choice(np.array(EDGES, np.int16), n), out[k])
        near = np.clip(at_off + rng.integers(-3, 4, n), -32768, 32767).astype(np.int16)
        out[k] = np.where(kind[k] == 3, near, out[k])
    pair_kind = rng.integers(0, 4, (2, n))
    for p, (a, b) in enumerate(((1, 4), (3, 2))):          # green + swir1, nir + red
        # positive values, so that the reference's clip to >= 1 leaves them as drawn
        a_vals = np.where(rng.random(n) < 0.5, rng.integers(1, 32768, n),
                          np.clip(np.rint(scale_offset[a][1]) + rng.integers(-2000, 2001, n), 1, 32767)).astype(np.int16)
        b_vals = _cancel(a_vals, *scale_offset[a], *scale_offset[b])
        sel = pair_kind[p] == 1
        out[a] = np.where(sel, a_vals, out[a])
        out[b] = np.where(sel, b_vals, out[b])
        sel = pair_kind[p] == 2                           # both at their offsets: 0 / 0
        out[a] = np.where(sel, np.int16(np.clip(np.rint(scale_offset[a][1]), -32768, 32767)), out[a])
        out[b] = np.where(sel, np.int16(np.clip(np.rint(scale_offset[b][1]), -32768, 32767)), out[b])
    return [np.ascontiguousarray(o.reshape(shape)) for o in out]


def bands_in(domain, rng, shape, recipe=None, thr=None, scale_offset=None):
    """Six int16 band planes of `shape` in `domain`; `recipe` (six planes) is the 'recipe' part of 'mix', `thr` a dict
    of thresholds for the 'edges' picks, `scale_offset` the six pairs of 'f32_ties'."""
    if domain == 'recipe':
        return [np.ascontiguousarray(b, np.int16) for b in recipe]
    if domain == 'int16':
        return [rng.integers(-32768, 32768, shape).astype(np.int16) for _ in range(6)]
    if domain == 'positive':
        return [rng.integers(1, 32768, shape).astype(np.int16) for _ in range(6)]
    if domain == 'edges':
        return [rng.choice(edge_values(name, thr), shape) for name in BAND_NAMES]
    if domain == 'mix':
        pick = rng.integers(0, 3, shape)
        edges = bands_in('edges', rng, shape, thr=thr)
        wide = bands_in('int16', rng, shape)
        return [np.where(pick == 0, r, np.where(pick == 1, e, w)).astype(np.int16)
                for r, e, w in zip(recipe, edges, wide)]
    if domain == 'f32_ties':
        return f32_ties(rng, shape, scale_offset)
    raise ValueError(domain)


def with_bands(s, domain, seed, thr=None, scale_offset=None):
    """A copy of synth_tile(..., with_masks=True) whose six band planes are in `domain` (seeded by `seed`)."""
    out = dict(s)
    out['bands'] = bands_in(domain, np.random.default_rng(seed), s['fmask'].shape, recipe=s['bands'], thr=thr,
                            scale_offset=scale_offset)
    return out
