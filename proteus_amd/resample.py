"""float32 and int16 planes INTERPOLATED onto another lattice through a mesh of source coordinates, include/dswx_hip.h
("resample"), stated in numpy: bilinear and cubic, where proteus_amd.warp copies the nearest pixel.

THE DEFINITION.  Source, destination, mesh and the POSITION (sx, sy) of a destination pixel in 1/256 source pixel are those of
proteus_amd.warp (warp.positions, 64-bit integers).  ux = sx - 128, c0 = ux >> 8, fx = ux & 255 and likewise uy, r0, fy.  A
source pixel (c, r) is a VALID tap iff it lies in the raster, its value is finite and -- with a nodata value -- differs from
it; its value is taken as a float64, exactly.

    CUBIC      all 16 taps (c0 - 1 .. c0 + 2) x (r0 - 1 .. r0 + 2) valid: with the integer weights N(f) of weights() over 2^25,
                   h_r = ((Nx0 p[r][0] + Nx1 p[r][1]) + Nx2 p[r][2]) + Nx3 p[r][3],   v = ((Ny0 h_0 + Ny1 h_1) + Ny2 h_2) + Ny3 h_3
               result = v * 2^-50; every product and sum one float64 operation.  Otherwise the pixel takes the bilinear rule.
    BILINEAR   taps (c0, r0), (c0 + 1, r0), (c0, r0 + 1), (c0 + 1, r0 + 1) with weights (256 - fx)(256 - fy), fx (256 - fy),
               (256 - fx) fy, fx fy; from S = 0.0, Wt = 0 over the valid taps in that order S = S + w * p, Wt += w.  Wt == 0: the
               pixel is OUTSIDE; Wt == 65536: result = S * 2^-16; otherwise result = S / Wt.

    dst    float32: the result rounded to float32; int16: rint, clamped to -32768 .. 32767; `outside` where OUTSIDE
    how    0 outside, 1 bilinear with all four taps valid, 2 bilinear with fewer, 3 cubic                          uint8
    head   [pixels, cubic, bilinear full, renormalised, outside, min row, max row, 0]: the rows of the valid taps of the window
           used (H and 0 if none)                                                                                  uint64 [n, 8]

resample_tiles calls neither dswx_resample_host nor the device: the tests pin the three to each other and to a loop in Python
floats.  UNPINNED: GDAL is not part of this project's environment; gdal.Warp's double-precision positions (ours are quantised
to 1/256 pixel), its border and nodata weighting and its integer rounding are not pinned by execution.
"""
import numpy as np

from . import warp

OUTPUTS = ('dst', 'how', 'head')
HEAD_WORDS = 8
KIND_F32, KIND_I16 = 0, 1
BILINEAR, CUBIC = 1, 2
METHODS = {'bilinear': BILINEAR, 'cubic': CUBIC}
DTYPES = {KIND_F32: np.dtype(np.float32), KIND_I16: np.dtype(np.int16)}
HOW_OUTSIDE, HOW_BILINEAR, HOW_RENORMALISED, HOW_CUBIC = 0, 1, 2, 3


def kind_of(dtype):
    """KIND_F32 / KIND_I16 of a numpy dtype; anything else is refused."""
    dtype = np.dtype(dtype)
    for kind, dt in DTYPES.items():
        if dt == dtype:
            return kind
    raise ValueError(f'only float32 and int16 planes are interpolated, not {dtype}')


def method_of(method):
    """BILINEAR / CUBIC of a name or a code."""
    code = METHODS.get(method, method)
    if code not in (BILINEAR, CUBIC):
        raise ValueError(f'method {method!r}: not bilinear or cubic (nearest is proteus_amd.warp)')
    return code


def outside_word(value, dtype):
    """The uint32 whose low bytes are `value` as an element of `dtype`: the `outside` of a Spec."""
    raw = np.array([value], dtype=np.dtype(dtype).newbyteorder('<')).view(np.uint8)
    return int.from_bytes(raw.tobytes(), 'little')


class Spec:
    """dswx_resample_spec_t: kind (KIND_F32 / KIND_I16 or a dtype), method ('bilinear' / 'cubic' or a code), shift 0 .. 8, the
    nodata value (None = none), `outside` (a uint32 whose low bytes are the element of an outside pixel) and the two strides."""

    def __init__(self, kind, method, shift, nodata=None, outside=0, src_tile_stride=0, mesh_tile_stride_nodes=0):
        self.kind = int(kind) if isinstance(kind, (int, np.integer)) else kind_of(kind)
        if self.kind not in DTYPES:
            raise ValueError(f'kind {kind!r}: not KIND_F32 or KIND_I16')
        self.dtype = DTYPES[self.kind]
        self.method, self.shift = method_of(method), int(shift)
        self.outside = int(outside) & 0xFFFFFFFF
        self.src_tile_stride, self.mesh_tile_stride_nodes = int(src_tile_stride), int(mesh_tile_stride_nodes)
        self.reserved = 0
        if not 0 <= self.shift <= warp.MAX_SHIFT:
            raise ValueError(f'shift {self.shift} outside 0 .. {warp.MAX_SHIFT}')
        self.has_nodata = 0 if nodata is None else 1
        self.nodata = nodata
        if nodata is None:
            self.nodata_word = 0
        elif self.kind == KIND_F32:
            self.nodata_word = int(np.array([nodata], dtype='<f4').view('<u4')[0])
        else:
            if int(nodata) != nodata or not warp.INT32_MIN <= int(nodata) <= warp.INT32_MAX:
                raise ValueError(f'the nodata value of an int16 plane is an integer, not {nodata!r}')
            self.nodata_word = int(nodata) & 0xFFFFFFFF


def weights():
    """int64 [256, 4]: Keys' cubic with a = -0.5 (Catmull-Rom) at f / 256 as integers over 2^25."""
    f = np.arange(256, dtype=np.int64)
    return np.stack([-65536 * f + 512 * f ** 2 - f ** 3, (1 << 25) - 1280 * f ** 2 + 3 * f ** 3,
                     65536 * f + 1024 * f ** 2 - 3 * f ** 3, -256 * f ** 2 + f ** 3], axis=1)


def _taps(tile, c, r, nodata):
    """(valid bool, value float64 -- 0.0 where not valid) of the source pixels (c, r) (int64 arrays, anywhere) of one tile."""
    H, W = tile.shape
    inside = (c >= 0) & (c < W) & (r >= 0) & (r < H)
    if not H * W:
        return inside, np.zeros(c.shape, dtype=np.float64)
    v = tile[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)]
    valid = inside & np.isfinite(v)
    if nodata is not None:
        valid &= (v != np.float32(nodata)) if tile.dtype == np.float32 else (v.astype(np.int64) != int(nodata))
    return valid, np.where(valid, v, 0).astype(np.float64)


def resample_tiles(tiles, mesh, shift, dst_shape, method, nodata=None, outside=0):
    """{'dst': [n, dst_h, dst_w] of the tiles' dtype, 'how': uint8 [n, dst_h, dst_w], 'head': uint64 [n, 8]} of tiles float32 or
    int16 [n_tiles, H, W] interpolated through `mesh` -- int32 [mesh_h, mesh_w, 2] for all tiles, or [n_tiles, mesh_h, mesh_w,
    2] -- by the module's definition, in float64 with its order of operations.  `outside` is a uint32 word (outside_word)."""
    tiles = np.asarray(tiles)
    kind_of(tiles.dtype)
    if tiles.ndim != 3:
        raise ValueError(f'the tiles are [n_tiles, H, W], not {tiles.shape}')
    cubic = method_of(method) == CUBIC
    n, H, W = tiles.shape
    dh, dw = (int(v) for v in dst_shape)
    if H * W > warp.MAX_PIXELS or dh * dw > warp.MAX_PIXELS:
        raise ValueError('more than 2^30 pixels')
    mesh = np.asarray(mesh)
    fill = np.array([int(outside) & ((1 << (8 * tiles.dtype.itemsize)) - 1)], dtype=f'<u{tiles.dtype.itemsize}').view(tiles.dtype)[0]
    dst = np.full((n, dh, dw), fill, dtype=tiles.dtype)
    how = np.zeros((n, dh, dw), dtype=np.uint8)
    head = np.zeros((n, HEAD_WORDS), dtype=np.uint64)
    table = weights().astype(np.float64)
    shared = warp.positions(mesh, shift, (dh, dw)) if mesh.ndim == 3 else None
    for t in range(n):
        sx, sy = shared if shared is not None else warp.positions(mesh[t], shift, (dh, dw))
        ux, uy = sx - 128, sy - 128
        c0, r0, fx, fy = ux >> 8, uy >> 8, ux & 255, uy & 255
        # bilinear, for every pixel
        S, Wt, count = np.zeros((dh, dw)), np.zeros((dh, dw), dtype=np.int64), np.zeros((dh, dw), dtype=np.int64)
        rlo, rhi = np.full((dh, dw), H, dtype=np.int64), np.zeros((dh, dw), dtype=np.int64)
        for k, w in enumerate(((256 - fx) * (256 - fy), fx * (256 - fy), (256 - fx) * fy, fx * fy)):
            row = r0 + (k >> 1)
            valid, p = _taps(tiles[t], c0 + (k & 1), row, nodata)
            S = np.where(valid, S + w.astype(np.float64) * p, S)
            Wt += np.where(valid, w, 0)
            count += valid
            rlo, rhi = np.where(valid, np.minimum(rlo, row), rlo), np.where(valid, np.maximum(rhi, row), rhi)
        result = np.where(Wt == 65536, S * 2.0 ** -16, S / np.maximum(Wt, 1).astype(np.float64))
        h = np.where(Wt == 0, HOW_OUTSIDE, np.where(count == 4, HOW_BILINEAR, HOW_RENORMALISED))
        if cubic:
            every = np.ones((dh, dw), dtype=bool)
            p = [[None] * 4 for _ in range(4)]
            for r in range(4):
                for c in range(4):
                    valid, p[r][c] = _taps(tiles[t], c0 - 1 + c, r0 - 1 + r, nodata)
                    every &= valid
            nx, ny = table[fx], table[fy]
            hr = [((nx[..., 0] * p[r][0] + nx[..., 1] * p[r][1]) + nx[..., 2] * p[r][2]) + nx[..., 3] * p[r][3] for r in range(4)]
            v = (((ny[..., 0] * hr[0] + ny[..., 1] * hr[1]) + ny[..., 2] * hr[2]) + ny[..., 3] * hr[3]) * 2.0 ** -50
            result, h = np.where(every, v, result), np.where(every, HOW_CUBIC, h)
            rlo, rhi = np.where(every, r0 - 1, rlo), np.where(every, r0 + 2, rhi)
        if tiles.dtype == np.float32:
            with np.errstate(over='ignore'):
                elem = result.astype(np.float32)
        else:
            elem = np.clip(np.rint(result), -32768, 32767).astype(np.int16)
        used = h != HOW_OUTSIDE
        dst[t][used] = elem[used]
        how[t] = h
        head[t] = [dh * dw, int((h == HOW_CUBIC).sum()), int((h == HOW_BILINEAR).sum()), int((h == HOW_RENORMALISED).sum()),
                   int((h == HOW_OUTSIDE).sum()), int(rlo[used].min()) if used.any() else H, int(rhi[used].max()) if used.any() else 0, 0]
    return {'dst': dst, 'how': how, 'head': head}
