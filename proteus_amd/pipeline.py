"""The product run on the device between the two codecs.

    band files --inflate (host threads, proteus_amd.codec)--> blocks in page-locked memory
        --copy engine--> HBM --dswx_untile_device--> planes
        --dswx_classify_device_2d--> layers (HBM)
        --dswx_cog_blocks_device (blocks + NEAREST overviews + predictor) / dswx_rgb_planes_device--> HBM
        --copy engine--> page-locked memory --deflate (host threads)--> GeoTIFF / COG

The host touches pixels only inside the DEFLATE codec; everything else the reference's GDAL calls do to a raster
(`ReadAsArray`, `save_as_cog`: core.py:7-91) is byte shuffling that runs in HBM.  One TileEngine per context; its
lock serialises the GPU part (milliseconds per tile), so that several tiles can be IN FLIGHT in one process -- tile
k + 1 inflating and tile k - 1 deflating on host threads while tile k is on the device (proteus_amd.batch) -- with one
HIP context per GPU.

No fallback hides here: a file layout the device kernels do not take (floating-point predictor, several samples per
pixel, big endian) is untiled by the host reader (geotiff.TiffDirectory.untile, the same bytes) and uploaded; the
classification itself has no host form anywhere.
"""
import threading
import time

import numpy as np

from . import _capi, geotiff, stages


class DevicePlane:
    """A raster in HBM: device pointer + shape + dtype.  The memory goes back to the engine's pool when the object dies."""

    def __init__(self, engine, buf, shape, dtype):
        self.engine, self.buf = engine, buf
        self.shape, self.dtype = tuple(int(v) for v in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self._host = None

    @property
    def ptr(self):
        return self.buf.ptr

    def numpy(self):
        """The raster on the host (copied once, then kept)."""
        if self._host is None:
            self._host = self.engine.download(self)
        return self._host

    def checksum(self):
        """The checksum of the raster as it lies in HBM (dswx_checksum_device; proteus_amd.checksum.checksum of the same
        array is the same number): eight bytes cross PCIe, not the raster.  A convenience -- nothing in the product run
        calls it."""
        if self.dtype.itemsize not in (1, 2, 4, 8):
            raise ValueError(f'no checksum for {self.dtype} planes')
        out = self.engine._take(8)
        try:
            with self.engine.lock, stages.span('gpu: checksum'):
                self.engine.ctx.checksum_device(self.ptr, self.dtype.itemsize, 1, self.nbytes // self.dtype.itemsize, out.ptr)
                self.engine.ctx.synchronize()
                return int(out.download(np.uint64, 1)[0])
        finally:
            self.engine._give(out)

    def histogram(self, kind=None, lo=0, shift=0):
        """How many elements of the raster fall into each of 256 bins, as it lies in HBM (dswx_histogram_device;
        proteus_amd.histogram.histogram of the same array is the same record): uint64 [256] -- a layer of a product run can be
        counted before it is written, and 2 KiB cross PCIe, not the raster.  The kind follows the dtype when None (uint8 by
        the byte, uint16 / int16 linearly with lo / shift); name HIST_DIAG for the DIAG layer."""
        from .histogram import BINS, check
        kind, lo, shift = check(self.dtype, kind, lo, shift)
        out = self.engine._take(8 * BINS)
        try:
            with self.engine.lock, stages.span('gpu: histogram'):
                self.engine.ctx.histogram_device(self.ptr, kind, 1, self.nbytes // self.dtype.itemsize, out.ptr, lo=lo, shift=shift)
                self.engine.ctx.synchronize()
                return out.download(np.uint64, BINS)
        finally:
            self.engine._give(out)

    def crosstab(self, other, spec, index=None):
        """How the classes of this raster fall into the classes of `other` (a uint8 DevicePlane of the same shape) as they lie
        in HBM (dswx_crosstab_device; proteus_amd.crosstab.crosstab_tiles of the two arrays gives the same records): uint64
        [n, 256], one record per leading index of a [n, H, W] stack, else one for the raster -- or [1, 256] for the leading
        index `index` alone; 2 KiB per record cross PCIe, not the rasters.  `spec` is a crosstab.Spec whose a_kind bins this
        raster's dtype."""
        from .crosstab import CELLS
        from .histogram import check
        check(self.dtype, spec.a_kind, spec.a_lo, spec.a_shift)
        if self.shape != other.shape or other.dtype != np.uint8:
            raise ValueError(f'{self.dtype} {self.shape} against {other.dtype} {other.shape}: the other plane is uint8 of the same shape')
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        n_elems = self.nbytes // self.dtype.itemsize // max(n_tiles, 1)
        first = 0
        if index is not None:
            if len(self.shape) != 3 or not 0 <= index < n_tiles:
                raise ValueError(f'index {index} of a raster of shape {self.shape}')
            first, n_tiles = int(index), 1
        out = self.engine._take(8 * CELLS * max(n_tiles, 1))
        try:
            with self.engine.lock, stages.span('gpu: crosstab'):
                self.engine.ctx.crosstab_device(self.ptr + first * n_elems * self.dtype.itemsize, other.ptr + first * n_elems,
                                                spec, n_tiles, n_elems, out.ptr)
                self.engine.ctx.synchronize()
                return out.download(np.uint64, CELLS * n_tiles).reshape(n_tiles, CELLS)
        finally:
            self.engine._give(out)

    def stack(self, spec, want=('count', 'last', 'last_index', 'share')):
        """The rasters of a [n, H, W] uint8 stack composited per pixel as they lie in HBM (dswx_stack_device;
        proteus_amd.stack.stack_tiles of the same array gives the same planes): a dict of [H, W] DevicePlanes for the outputs
        named in `want` -- 'count' gives 'count0' .. 'count<n_cats - 1>' (uint16), then 'last' (uint8), 'last_index' (uint16)
        and 'share' (uint8) -- which stay on the device, each to be checksummed, histogrammed or written.  `spec` is a
        stack.Spec (stack.wtr_spec for a WTR layer)."""
        if len(self.shape) != 3 or self.dtype != np.uint8:
            raise ValueError(f'a stack is a uint8 [n, H, W] plane, not {self.dtype} {self.shape}')
        n_tiles, shape = self.shape[0], self.shape[1:]
        made = _capi._stack_planes(want, spec, shape, lambda shp, dt: [self.engine.plane(shape, dt) for _ in range(shp[0])]
                                   if len(shp) == 3 else self.engine.plane(shp, dt))
        out = _capi.StackOut.of(count=[p.ptr for p in made.get('count', ())],
                                **{k: made[k].ptr for k in ('last', 'last_index', 'share') if k in made})
        with self.engine.lock, stages.span('gpu: stack'):
            self.engine.ctx.stack_device(self.ptr, spec, n_tiles, shape[0] * shape[1], out)
            self.engine.ctx.synchronize()
        res = {f'count{k}': p for k, p in enumerate(made.pop('count', ()))}
        res.update(made)
        return res

    def mosaic(self, place, canvas_shape, spec, want=('count', 'last', 'last_index', 'share')):
        """The rasters of a [n, H, W] uint8 plane placed on one canvas of canvas_shape = (canvas_h, canvas_w) by `place` (int
        [n, 2] = row0, col0 of every raster on the canvas; mosaic.layout makes one from geotransforms) and composited per
        canvas pixel as they lie in HBM (dswx_mosaic_device; proteus_amd.mosaic.mosaic_tiles of the same arrays gives the same
        planes): a dict of [canvas_h, canvas_w] DevicePlanes named as those of `stack`, which stay on the device -- 'last' can
        be labelled, measured, outlined, gridded or written across the seams of the rasters.  `spec` is a mosaic.Spec
        (mosaic.wtr_mosaic_spec for a WTR layer)."""
        if len(self.shape) != 3 or self.dtype != np.uint8:
            raise ValueError(f'a mosaic is made of a uint8 [n, H, W] plane, not {self.dtype} {self.shape}')
        n_tiles, height, width = self.shape
        place = np.ascontiguousarray(place, dtype=np.int32)
        if place.shape != (n_tiles, 2):
            raise ValueError(f'place has shape {place.shape}, not ({n_tiles}, 2)')
        shape = tuple(int(v) for v in canvas_shape)
        if len(shape) != 2 or min(shape) < 0 or max(shape) > _capi.MOSAIC_MAX_SIDE:
            raise ValueError(f'a canvas is (canvas_h, canvas_w) with sides 0 .. {_capi.MOSAIC_MAX_SIDE}, not {canvas_shape}')
        made = _capi._stack_planes(want, spec, shape, lambda shp, dt: [self.engine.plane(shape, dt) for _ in range(shp[0])]
                                   if len(shp) == 3 else self.engine.plane(shp, dt))
        out = _capi.StackOut.of(count=[p.ptr for p in made.get('count', ())],
                                **{k: made[k].ptr for k in ('last', 'last_index', 'share') if k in made})
        table = self.engine.upload(place if n_tiles else np.zeros((1, 2), dtype=np.int32))
        try:
            with self.engine.lock, stages.span('gpu: mosaic'):
                self.engine.ctx.mosaic_device(self.ptr, spec, n_tiles, height, width, table.ptr, shape[0], shape[1], out)
                self.engine.ctx.synchronize()
        finally:
            table.release()
        res = {f'count{k}': p for k, p in enumerate(made.pop('count', ()))}
        res.update(made)
        return res

    def warp(self, mesh, dst_shape, shift, outside=0, want=('dst',)):
        """The rasters of a [n, H, W] (or one [H, W]) plane of 1-, 2- or 4-byte elements resampled (nearest pixel) onto
        dst_shape = (dst_h, dst_w) through `mesh` as they lie in HBM (dswx_warp_device; proteus_amd.warp.warp_tiles of the same
        arrays gives the same arrays): int32 [mesh_h, mesh_w, 2] for all rasters or [n, mesh_h, mesh_w, 2], in 1/256 source
        pixel, a node every 1 << shift destination pixels (warp.affine_mesh and warp.utm_mesh make one from geotransforms).
        A dict of DevicePlanes for the outputs named in `want` -- 'dst' [n, dst_h, dst_w] of this plane's dtype ([dst_h, dst_w]
        for one raster), 'src_index' uint32 of the same shape, 'head' uint64 [n, 8] -- which stay on the device: 'dst' of a
        neighbour in another UTM zone can be mosaicked, labelled or written."""
        from . import warp as _warp
        if len(self.shape) not in (2, 3) or self.dtype.itemsize not in (1, 2, 4):
            raise ValueError(f'a warp is made of a [n, H, W] or [H, W] plane of 1-, 2- or 4-byte elements, not {self.dtype} {self.shape}')
        return self._through_mesh('warp', mesh, dst_shape, shift, want, _capi._warp_planes, _capi.WarpOut,
                                  lambda stride: _warp.Spec(self.dtype.itemsize, shift, outside, mesh_tile_stride_nodes=stride))

    def _through_mesh(self, what, mesh, dst_shape, shift, want, planes, out_type, make_spec):
        """What `warp` and `resample` share: the destination and the mesh validated, the spec made by make_spec(nodes between
        the meshes of consecutive tiles), the mesh uploaded for the one call of self.engine.ctx.<what>_device and released."""
        from .warp import mesh_shape
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        height, width = self.shape[-2:]
        shape = tuple(int(v) for v in dst_shape)
        if len(shape) != 2 or min(shape) < 0 or shape[0] * shape[1] > _capi.WARP_MAX_PIXELS:
            raise ValueError(f'a destination is (dst_h, dst_w) of at most {_capi.WARP_MAX_PIXELS} pixels, not {dst_shape}')
        mh, mw = mesh_shape(shape, shift)
        mesh = np.ascontiguousarray(mesh, dtype=np.int32)
        if mesh.shape not in ((mh, mw, 2), (n_tiles, mh, mw, 2)):
            raise ValueError(f'a mesh for {shape} at shift {shift} is [{mh}, {mw}, 2] or [{n_tiles}, {mh}, {mw}, 2], not {mesh.shape}')
        spec = make_spec(mh * mw if mesh.ndim == 4 else 0)
        lead = (n_tiles,) if len(self.shape) == 3 else ()
        made = planes(want, self.dtype, n_tiles, shape, lambda shp, dt: self.engine.plane(shp if len(shp) == 2 else lead + tuple(shp[1:]), dt))
        out = out_type.of(**{k: p.ptr for k, p in made.items()})
        table = self.engine.upload(mesh)
        try:
            with self.engine.lock, stages.span(f'gpu: {what}'):
                getattr(self.engine.ctx, f'{what}_device')(self.ptr, spec, n_tiles, height, width, table.ptr, shape[0], shape[1], out)
                self.engine.ctx.synchronize()
        finally:
            table.release()
        return made

    def resample(self, mesh, dst_shape, shift, method='cubic', nodata=None, outside=0, want=('dst',)):
        """The rasters of a float32 or int16 [n, H, W] (or one [H, W]) plane INTERPOLATED -- 'bilinear' or 'cubic' -- onto
        dst_shape = (dst_h, dst_w) through `mesh` (as for `warp`) as they lie in HBM (dswx_resample_device;
        proteus_amd.resample.resample_tiles of the same arrays gives the same arrays).  `nodata`: the value of a tap that is
        not valid (None: every finite value is); `outside`: a uint32 whose low bytes are the element of a pixel without a valid
        tap (resample.outside_word).  A dict of DevicePlanes for the outputs named in `want` -- 'dst' [n, dst_h, dst_w] of this
        plane's dtype ([dst_h, dst_w] for one raster), 'how' uint8 of the same shape, 'head' uint64 [n, 8] -- which stay on the
        device: the DEM of a product run goes on to the shadow kernel."""
        from . import resample as _resample
        if len(self.shape) not in (2, 3):
            raise ValueError(f'a resample is made of a [n, H, W] or [H, W] plane, not {self.shape}')
        return self._through_mesh('resample', mesh, dst_shape, shift, want, _capi._resample_planes, _capi.ResampleOut,
                                  lambda stride: _resample.Spec(self.dtype, method, shift, nodata, outside, mesh_tile_stride_nodes=stride))

    def land_mesh(self, copernicus, mesh_wc, mesh_cg, shape, spec, want=('land', 'head')):
        """This uint8 [wc_h, wc_w] plane as the WorldCover source window and `copernicus` (a DevicePlane uint8 [cg_h, cg_w]) as
        the CGLS one, read through the host meshes mesh_wc (of the lattice 3 H x 3 W) and mesh_cg (of shape = (H, W)) by `spec`
        (a landmesh.Spec) as they lie in HBM (dswx_land_mesh_device, ONE launch; proteus_amd.landmesh.land_tiles of the same
        arrays gives the same arrays): a dict of DevicePlanes for the outputs named in `want` -- 'land' uint8 [H, W], 'head'
        uint64 [1, 8] -- which stay on the device."""
        from .warp import mesh_shape
        H, W = (int(v) for v in shape)
        if len(self.shape) != 2 or len(copernicus.shape) != 2 or self.dtype != np.uint8 or copernicus.dtype != np.uint8:
            raise ValueError(f'the maps are uint8 [h, w] planes, not {self.dtype} {self.shape} and {copernicus.dtype} {copernicus.shape}')
        if spec.land_tile_stride or spec.wc_tile_stride or spec.cg_tile_stride:
            raise ValueError('one tile: the strides of the spec must be 0')
        meshes = []
        for name, mesh, dims, shift in (('mesh_wc', mesh_wc, (3 * H, 3 * W), spec.shift_wc), ('mesh_cg', mesh_cg, (H, W), spec.shift_cg)):
            mesh = np.ascontiguousarray(mesh, dtype=np.int32)
            if mesh.shape != mesh_shape(dims, shift) + (2,):
                raise ValueError(f'{name} for {dims} at shift {shift} is {mesh_shape(dims, shift) + (2,)}, not {mesh.shape}')
            meshes.append(mesh)
        want = _capi._wanted(want, {'land': 0, 'head': 0})
        made = {k: self.engine.plane(*{'land': ((H, W), np.uint8), 'head': ((1, _capi.LAND_MESH_HEAD_WORDS), np.uint64)}[k])
                for k in ('land', 'head') if k in want}
        tables = [self.engine.upload(m) for m in meshes]
        try:
            with self.engine.lock, stages.span('gpu: LAND through meshes'):
                self.engine.ctx.land_mesh_device(self.ptr, self.shape, copernicus.ptr, copernicus.shape, spec, 1, H, W, tables[0].ptr,
                                                 tables[1].ptr, made['land'].ptr if 'land' in made else None,
                                                 made['head'].ptr if 'head' in made else None)
                self.engine.ctx.synchronize()
        finally:
            for t in tables:
                t.release()
        return made

    def grid(self, spec, want=('count', 'share', 'coverage', 'major')):
        """The rasters of a [n, H, W] (or one [H, W]) uint8 plane aggregated onto cells as they lie in HBM (dswx_grid_device;
        proteus_amd.grid.grid_tiles of the same array gives the same planes): a dict of [n, GH, GW] DevicePlanes for the
        outputs named in `want` -- 'count' gives 'count0' .. 'count<n_cats - 1>' (uint32), then 'share', 'coverage' and
        'major' (uint8) -- which stay on the device, each to be histogrammed, stacked or written.  `spec` is a grid.Spec
        (grid.wtr_grid_spec for a WTR layer)."""
        from .grid import grid_shape
        if len(self.shape) not in (2, 3) or self.dtype != np.uint8:
            raise ValueError(f'a grid is made of a uint8 [n, H, W] or [H, W] plane, not {self.dtype} {self.shape}')
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        height, width = self.shape[-2:]
        shape = (n_tiles,) + grid_shape(height, width, spec)
        made = _capi._grid_planes(want, spec, shape, lambda shp, dt: [self.engine.plane(shape, dt) for _ in range(shp[0])]
                                  if len(shp) == 4 else self.engine.plane(shp, dt))
        out = _capi.GridOut.of(count=[p.ptr for p in made.get('count', ())],
                               **{k: made[k].ptr for k in ('share', 'coverage', 'major') if k in made})
        with self.engine.lock, stages.span('gpu: grid'):
            self.engine.ctx.grid_device(self.ptr, spec, n_tiles, height, width, out)
            self.engine.ctx.synchronize()
        res = {f'count{k}': p for k, p in enumerate(made.pop('count', ()))}
        res.update(made)
        return res

    def label(self, spec, want=('label', 'size', 'sieved', 'summary')):
        """The connected bodies of a [n, H, W] (or one [H, W]) uint8 plane as it lies in HBM (dswx_label_device;
        proteus_amd.label.label_tiles of the same array gives the same planes): a dict of DevicePlanes for the outputs named
        in `want` and the ones they need ('label' always, 'size' with 'sieved' or 'summary') -- 'label' and 'size' uint32
        [n, H, W], 'sieved' uint8 [n, H, W], 'summary' uint64 [n, 40] -- which stay on the device: 'sieved' can be
        histogrammed, gridded or written, every one checksummed.  `spec` is a label.Spec (label.wtr_label_spec for a WTR
        layer)."""
        if len(self.shape) not in (2, 3) or self.dtype != np.uint8:
            raise ValueError(f'bodies are labelled in a uint8 [n, H, W] or [H, W] plane, not {self.dtype} {self.shape}')
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        height, width = self.shape[-2:]
        made = {k: self.engine.plane((n_tiles, _capi.LABEL_SUMMARY_WORDS) if k == 'summary' else (n_tiles, height, width),
                                     _capi.LABEL_DTYPES[k]) for k in _capi._label_wanted(want)}
        out = _capi.LabelOut.of(**{k: p.ptr for k, p in made.items()})
        with self.engine.lock, stages.span('gpu: label'):
            self.engine.ctx.label_device(self.ptr, spec, n_tiles, height, width, out)
            self.engine.ctx.synchronize()
        return made

    def distance(self, spec, want=('dist2', 'nearest', 'summary')):
        """The squared distance of every pixel of a [n, H, W] (or one [H, W]) uint8 plane to the nearest target, as the plane
        lies in HBM (dswx_distance_device; proteus_amd.distance.distance_tiles of the same array gives the same planes): a
        dict of DevicePlanes for the outputs named in `want` and 'dist2' always -- 'dist2' and 'nearest' uint32 [n, H, W],
        'within' uint8 [n, H, W] (needs spec.max_radius > 0), 'summary' uint64 [n, 40] -- which stay on the device: 'within'
        can be histogrammed, gridded or written, every one checksummed.  `spec` is a distance.Spec
        (distance.wtr_distance_spec for a WTR layer)."""
        if len(self.shape) not in (2, 3) or self.dtype != np.uint8:
            raise ValueError(f'distances are measured in a uint8 [n, H, W] or [H, W] plane, not {self.dtype} {self.shape}')
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        height, width = self.shape[-2:]
        _capi._distance_refuse(height, width)
        made = {k: self.engine.plane((n_tiles, _capi.DISTANCE_SUMMARY_WORDS) if k == 'summary' else (n_tiles, height, width),
                                     _capi.DISTANCE_DTYPES[k]) for k in _capi._distance_wanted(want, spec)}
        out = _capi.DistanceOut.of(**{k: p.ptr for k, p in made.items()})
        with self.engine.lock, stages.span('gpu: distance'):
            self.engine.ctx.distance_device(self.ptr, spec, n_tiles, height, width, out)
            self.engine.ctx.synchronize()
        return made

    def outline(self, label_spec, spec):
        """The bodies of a [n, H, W] (or one [H, W]) uint8 plane labelled by `label_spec` (a label.Spec) and traced as rings
        by `spec` (an outline.Spec), label chained into outline as the plane lies in HBM (dswx_label_device, then
        dswx_outline_device; proteus_amd.outline.outline_tiles of the downloaded label plane gives the same): a dict of
        DevicePlanes 'chain' uint32 [n, max_edges], 'rings' uint32 [n, max_rings, 8] (only with spec.max_rings > 0;
        `.numpy().view(outline.ROW_DTYPE)[..., 0]` are the records), 'head' uint64 [n, 8] and 'label' uint32 [n, H, W], which
        stay on the device.  With label_spec None this plane is itself a uint32 id plane and is traced as it is (no 'label'
        then).  The working memory is taken for the call and given back."""
        if label_spec is None:
            if len(self.shape) not in (2, 3) or self.dtype != np.uint32:
                raise ValueError(f'outlines are traced in a uint32 [n, H, W] or [H, W] id plane, not {self.dtype} {self.shape}')
            made, ids = {}, self
        else:
            made = {'label': self.label(label_spec, want=('label',))['label']}
            ids = made['label']
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        height, width = self.shape[-2:]
        for k in _capi._outline_wanted(('chain', 'rings', 'head'), spec):
            made[k] = self.engine.plane(_capi._outline_shape(k, n_tiles, spec), _capi.OUTLINE_DTYPES[k])
        out = _capi.OutlineOut.of(**{k: p.ptr for k, p in made.items() if k != 'label'})
        work_bytes = _capi.outline_work_bytes(spec, n_tiles, height, width)
        work = self.engine._take(work_bytes)
        try:
            with self.engine.lock, stages.span('gpu: outline'):
                self.engine.ctx.outline_device(ids.ptr, spec, n_tiles, height, width, out, work.ptr, work_bytes)
                self.engine.ctx.synchronize()
        finally:
            self.engine._give(work)
        return made

    def burn(self, polygons_px, spec=None, words=None, want=('acc', 'head')):
        """Polygon rings burnt INTO this [n, H, W] (or one [H, W]) uint8 plane as it lies in HBM (dswx_burn_device with the
        plane as both `src` and `mask`; proteus_amd.burn.burn_tiles with src = the same array gives the same plane): the
        pixels whose centre is inside by the even-odd rule become spec.burn (a burn.Spec, default 1), every other pixel stays.
        `polygons_px` is a list of rings -- [k, 2] arrays of (x, y) in PIXEL coordinates, (0, 0) the top left corner of the
        raster, floats allowed, the closing point not repeated -- for an [H, W] plane, and a list of such lists, one per tile,
        for an [n, H, W] plane; ring j toggles words[j] (same nesting; default 1: rings that overlap cancel, so give every
        polygon a bit of its own, holes the bit of their polygon, where polygons may overlap).  Returns a dict of DevicePlanes
        'acc' uint32 [n, H, W] (always) and 'head' uint64 [n, 8], which stay on the device.  16 bytes per vertex cross PCIe,
        not a plane."""
        from . import burn as _burn
        return self._rings('burn', _burn.Spec() if spec is None else spec, polygons_px, words, want)

    def reach(self, polygons_px, spec, want=('acc', 'head')):
        """The pixels of this uint8 plane whose centre lies within spec.radius (a reach.Spec, 1/256 pixel) of an edge of the
        rings become spec.burn in place (dswx_reach_device with the plane as both `src` and `mask`;
        proteus_amd.reach.reach_tiles with src = the same array gives the same plane); every other pixel stays.  Rings and
        returned planes as for burn(), which it follows to give the polygons grown by the radius."""
        return self._rings('reach', spec, polygons_px, None, want)

    def _rings(self, entry, spec, polygons_px, words, want):
        from . import burn as _burn
        if len(self.shape) not in (2, 3) or self.dtype != np.uint8:
            raise ValueError(f'polygons are burnt into a uint8 [n, H, W] or [H, W] plane, not {self.dtype} {self.shape}')
        if spec.mask_tile_stride or spec.src_tile_stride:
            raise ValueError('the strides of the spec must be 0: the plane is dense')
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        height, width = self.shape[-2:]
        if len(self.shape) == 2:
            polygons_px, words = [polygons_px], [words]
        elif words is None:
            words = [None] * n_tiles
        if len(polygons_px) != n_tiles or len(words) != n_tiles:
            raise ValueError(f'{len(polygons_px)} lists of rings for {n_tiles} tiles')
        verts, first = _burn.tiles([_burn.records([_burn.quantise(np.asarray(p, dtype=np.float64).reshape(-1, 2)) for p in rings], w)
                                    for rings, w in zip(polygons_px, words)])
        made = {k: self.engine.plane((n_tiles, _capi.BURN_HEAD_WORDS) if k == 'head' else (n_tiles, height, width), _capi.BURN_DTYPES[k])
                for k in _capi._burn_wanted(tuple(want) + ('acc',)) if k != 'mask'}
        d_verts = self.engine.upload(verts.view(np.uint32).reshape(-1, 4) if len(verts) else np.zeros((1, 4), dtype=np.uint32))
        d_first = self.engine.upload(first)
        try:
            out = _capi.BurnOut.of(mask=self.ptr, **{k: p.ptr for k, p in made.items()})
            with self.engine.lock, stages.span('gpu: ' + entry):
                getattr(self.engine.ctx, entry + '_device')(d_verts.ptr, d_first.ptr, spec, n_tiles, height, width, self.ptr, out)
                self.engine.ctx.synchronize()
        finally:
            d_verts.release()
            d_first.release()
        self._host = None                                    # (the raster changed under a copy kept by numpy())
        return made

    def body_table(self, spec, value=None, want=('dense', 'rows', 'head')):
        """The bodies of this LABEL plane -- uint32 [n, H, W] (or one [H, W]) as label(...)['label'] leaves it in HBM --
        renumbered 1 .. K and tabulated (dswx_body_table_device; proteus_amd.bodies.body_table of the same arrays gives the
        same): a dict of DevicePlanes for the outputs named in `want` and 'dense' always -- 'dense' uint32 [n, H, W], 'rows'
        uint32 [n, max_rows, 16] (only with spec.max_rows > 0; `.numpy().view(bodies.ROW_DTYPE)[..., 0]` are the records),
        'head' uint64 [n, 8] -- which stay on the device, so plane.label(...)['label'].body_table(...) chains without a
        download.  `value` is a uint8 DevicePlane of the same raster (None with spec.n_cats == 0); `spec` a bodies.Spec
        (bodies.wtr_body_spec for a WTR layer as value)."""
        if len(self.shape) not in (2, 3) or self.dtype != np.uint32:
            raise ValueError(f'bodies are tabulated from a uint32 [n, H, W] or [H, W] label plane, not {self.dtype} {self.shape}')
        if (value is None) != (spec.n_cats == 0):
            raise ValueError('value is None if and only if n_cats is 0')
        if value is not None and (value.dtype != np.uint8 or tuple(value.shape) != tuple(self.shape)):
            raise ValueError(f'a value plane is uint8 {tuple(self.shape)}, not {value.dtype} {tuple(value.shape)}')
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        height, width = self.shape[-2:]
        made = {k: self.engine.plane(_capi._body_shape(k, n_tiles, height, width, spec), _capi.BODY_DTYPES[k])
                for k in _capi._body_wanted(want, spec)}
        out = _capi.BodyOut.of(**{k: p.ptr for k, p in made.items()})
        with self.engine.lock, stages.span('gpu: body table'):
            self.engine.ctx.body_table_device(self.ptr, value.ptr if value is not None else None, spec, n_tiles, height, width, out)
            self.engine.ctx.synchronize()
        return made

    def compare(self, other, atol=0.0, rtol=0.0, equal_nan=True):
        """This raster against `other` (a DevicePlane of the same shape and dtype) as they lie in HBM (dswx_compare_device;
        proteus_amd.compare.compare_tiles of the two arrays gives the same records): compare.RECORD [n], one record per
        leading index of a [n, H, W] stack, else one for the raster; 32 bytes per record cross PCIe, not the rasters."""
        from .compare import RECORD, kind_of
        if self.shape != other.shape or self.dtype != other.dtype:
            raise ValueError(f'{self.dtype} {self.shape} against {other.dtype} {other.shape}')
        n_tiles = self.shape[0] if len(self.shape) == 3 else 1
        n_elems = self.nbytes // self.dtype.itemsize // max(n_tiles, 1)
        out = self.engine._take(32 * max(n_tiles, 1))
        try:
            with self.engine.lock, stages.span('gpu: compare'):
                self.engine.ctx.compare_device(self.ptr, other.ptr, kind_of(self.dtype), n_tiles, n_elems, out.ptr,
                                               atol=atol, rtol=rtol, equal_nan=equal_nan)
                self.engine.ctx.synchronize()
                return out.download(RECORD, n_tiles)
        finally:
            self.engine._give(out)

    def element(self, index):
        """One element of the raster (flat index, C order) by an element-sized copy."""
        return self.buf.download(self.dtype, 1, int(index) * self.dtype.itemsize)[0]

    def release(self):
        if self.buf is not None:
            self.engine._give(self.buf)
            self.buf = None

    def __del__(self):
        try:
            self.release()
        except Exception:           # noqa: BLE001
            pass


class _PlaneView:
    """A raster inside another device buffer (no ownership): what the writer-side helpers need of a plane."""

    def __init__(self, ptr, shape, dtype, keep=None):
        self.ptr, self.shape, self.dtype, self._keep = int(ptr), tuple(shape), np.dtype(dtype), keep


class TileEngine:
    POOL_CAP = 6 << 30          # bytes of released device buffers kept for the next tile

    def __init__(self, ctx):
        self.ctx = ctx
        self.lock = threading.RLock()
        self._free = {}                     # nbytes -> [DeviceBuffer]
        self._free_bytes = 0
        self._weights = {}                  # (n_in, n_out) -> (first DeviceBuffer, weights DeviceBuffer, taps): CUBICSPLINE passes
        self._pool_lock = threading.RLock()   # re-entrant: a plane's finalizer (_give) may run -- cyclic GC -- on a thread that is inside _take

    # ---- device memory ------------------------------------------------------------------------------------
    @staticmethod
    def _round(nbytes):
        return max((int(nbytes) + 0xffff) & ~0xffff, 1 << 16)

    def _take(self, nbytes):
        n = self._round(nbytes)
        with self._pool_lock:
            spare = self._free.get(n)
            while spare:
                self._free_bytes -= n
                buf = spare.pop()
                # a plane that dies inside a reference cycle (the frames of a refused run, held by its traceback) is finalised
                # together with its buffer, in either order: the buffer may have been freed although it was given back
                if buf.ptr:
                    return buf
        with self.lock:
            return self.ctx.malloc(n)

    def _give(self, buf):
        if not buf.ptr:                      # freed already by its own finalizer (see _take)
            return
        with self._pool_lock:
            if self.ctx.handle and self._free_bytes + buf.nbytes <= self.POOL_CAP:
                self._free.setdefault(buf.nbytes, []).append(buf)
                self._free_bytes += buf.nbytes
                return
        buf.free()

    def close(self):
        with self._pool_lock:
            spare, self._free, self._free_bytes = self._free, {}, 0
            weights, self._weights = self._weights, {}
        for d_first, d_w, _ in weights.values():
            d_first.free()
            d_w.free()
        for bufs in spare.values():
            for b in bufs:
                b.free()

    def plane(self, shape, dtype):
        dtype = np.dtype(dtype)
        return DevicePlane(self, self._take(int(np.prod(shape, dtype=np.int64)) * dtype.itemsize), shape, dtype)

    def upload(self, arr):
        """numpy raster -> DevicePlane (through page-locked memory)."""
        arr = np.ascontiguousarray(arr)
        if arr.dtype == np.bool_:
            arr = arr.view(np.uint8)
        p = self.plane(arr.shape, arr.dtype)
        pinned = arr if self.ctx.is_pinned(arr) else None
        if pinned is None:
            pinned = self.ctx.pinned_empty(arr.shape, arr.dtype)
            np.copyto(pinned, arr)
        with self.lock, stages.span('gpu: upload'):
            self.ctx.h2d_async(p.ptr, pinned)
            self.ctx.synchronize()
        return p

    def download(self, plane):
        out = self.ctx.pinned_empty(plane.shape, plane.dtype)
        with self.lock, stages.span('gpu: download'):
            self.ctx.d2h_async(out, plane.ptr, plane.nbytes)
            self.ctx.synchronize()
        return out

    # ---- reader side ----------------------------------------------------------------------------------------
    def device_untile_ok(self, d):
        """Layouts dswx_untile_device takes: one sample per pixel, little endian; 1- / 2- / 4-byte integers with PREDICTOR
        1 / 2, Float32 with PREDICTOR 1 / 3 (a GDAL-written DEM)."""
        if d.spp != 1 or d.dt.byteorder not in ('=', '|', '<') or d.n_blocks * d.block_bytes >= (1 << 32):
            return False
        if d.dt.kind in 'iu':
            return d.dt.itemsize in (1, 2, 4) and d.predictor in (1, 2)
        return d.dt.kind == 'f' and d.dt.itemsize == 4 and d.predictor in (1, 3)

    def read_plane(self, path):
        return self.read_directory(geotiff.open_geotiff(path))

    def read_directory(self, d):
        """One single-band GeoTIFF (geotiff.TiffDirectory) -> (DevicePlane [H, W], GeoTiffInfo).  Inflate on host threads
        into page-locked memory; predictor + untile on the device when its kernel takes the layout, else by the host
        reader (same bytes)."""
        info = d.info
        if d.spp != 1:
            raise geotiff.GeoTiffError(f'{d.path}: {d.spp} samples per pixel, expected a single band')
        if not self.device_untile_ok(d):
            return self.upload(d.untile(d.inflate())[0]), info
        need = d.n_blocks * d.block_bytes
        staging = self.ctx.pinned_empty((need,), np.uint8)
        d.inflate(staging)
        dev_blocks = self._take(need)
        plane = self.plane((info.height, info.width), info.dtype)
        try:
            with self.lock, stages.span('gpu: blocks -> plane (h2d + untile)'):
                self.ctx.h2d_async(dev_blocks.ptr, staging, need)
                self.ctx.untile_device(dev_blocks.ptr, d.dt.itemsize, info.height, info.width, d.bw, d.bh, d.predictor, plane.ptr)
                self.ctx.synchronize()
        finally:
            self._give(dev_blocks)
        return plane, info

    def read_bands(self, path):
        """Every band of a GeoTIFF -> (DevicePlane [B, H, W], GeoTiffInfo): what compare_dswx_hls_products needs of a
        product file.  Band-planar files (what write_geotiff writes) in a layout dswx_untile_device takes are inflated on host
        threads and untiled band by band on the device; any other layout is untiled by the host reader (the same bytes) and
        uploaded."""
        d = geotiff.open_geotiff(path)
        info = d.info
        B, H, W = d.spp, info.height, info.width
        probe_spp, d.spp = d.spp, 1                      # device_untile_ok judges the layout of ONE band
        try:
            ok = (B == 1 or d.planar == 2) and self.device_untile_ok(d)
        finally:
            d.spp = probe_spp
        if not ok:
            return self.upload(d.untile(d.inflate())), info
        need = d.n_blocks * d.block_bytes
        staging = self.ctx.pinned_empty((need,), np.uint8)
        d.inflate(staging)
        dev_blocks = self._take(need)
        plane = self.plane((B, H, W), info.dtype)
        per_band = need // B
        try:
            with self.lock, stages.span('gpu: blocks -> plane (h2d + untile)'):
                self.ctx.h2d_async(dev_blocks.ptr, staging, need)
                for b in range(B):
                    self.ctx.untile_device(dev_blocks.ptr + b * per_band, d.dt.itemsize, H, W, d.bw, d.bh, d.predictor,
                                           plane.ptr + b * H * W * d.dt.itemsize)
                self.ctx.synchronize()
        finally:
            self._give(dev_blocks)
        return plane, info

    # ---- the classifier on resident planes --------------------------------------------------------------------
    def classify(self, bands, fmask, params, land=None, shad=None, ocean=None, layers=()):
        """bands: six DevicePlanes (int16 [H, W]); fmask / land / shad / ocean: DevicePlane or ndarray or None.
        Returns {layer: DevicePlane} + 'counters' (ndarray int64 [1, 3])."""
        H, W = bands[0].shape
        keep = []

        def dev(a, name):
            if a is None:
                return None
            if not isinstance(a, DevicePlane):
                a = np.ascontiguousarray(a, dtype=np.uint8)
                if a.shape != (H, W):
                    raise ValueError(f'{name} shape {a.shape} != bands shape {(H, W)}')
                a = self.upload(a)
            elif a.shape != (H, W):
                raise ValueError(f'{name} shape {a.shape} != bands shape {(H, W)}')
            keep.append(a)
            return a

        pin, pout = _capi.PlanesIn(), _capi.PlanesOut()
        for i, b in enumerate(bands):
            if b.shape != (H, W) or b.dtype != np.int16:
                raise ValueError('bands must be int16 planes of one shape')
            pin.band[i] = b.ptr
        pin.fmask = dev(fmask, 'fmask').ptr
        for name, a in (('land', land), ('shad', shad), ('ocean', ocean)):
            p = dev(a, name)
            setattr(pin, name, p.ptr if p is not None else None)
        res = {}
        for name in layers:
            if name != 'diag' and name not in _capi.U8_LAYERS:
                raise KeyError(name)
            res[name] = self.plane((H, W), np.uint16 if name == 'diag' else np.uint8)
            setattr(pout, name, res[name].ptr)
        d_cnt = self._take(256)
        cnt = self.ctx.pinned_empty((1, 3), np.int64)
        try:
            with self.lock:
                t0 = time.perf_counter()
                self.ctx.classify_device_2d(params, 1, H, W, pin, pout, d_cnt.ptr)
                self.ctx.d2h_async(cnt, d_cnt.ptr, 24)
                self.ctx.synchronize()
                stages.add('gpu: classify (resident planes)', t0, time.perf_counter())
                self.kernel_info = self.ctx.last_kernel_info()
        finally:
            self._give(d_cnt)
        res['counters'] = np.array(cnt, dtype=np.int64)
        del keep
        return res

    # ---- the layers next to the path, resident --------------------------------------------------------------------
    def crop(self, plane, margin):
        """_crop_2d_array_all_sides (dswx_hls.py:4320) on the device: plane[margin:-margin, margin:-margin]."""
        if margin == 0:
            return plane
        H, W = plane.shape
        out = self.plane((H - 2 * margin, W - 2 * margin), plane.dtype)
        es = plane.dtype.itemsize
        with self.lock, stages.span('gpu: crop'):
            self.ctx.copy_2d_device(out.ptr, out.shape[1] * es, plane.ptr + (margin * W + margin) * es, W * es,
                                    out.shape[1] * es, out.shape[0])
            self.ctx.synchronize()
        return out

    def shadow_layer(self, dem, sun_vector, sin_azimuth, cos_azimuth, min_slope_angle, max_sun_local_inc_angle, margin,
                     float32, pixel_spacing_x=30, pixel_spacing_y=30):
        """dem: DevicePlane float32 [H, W] (with its margin) -> SHAD DevicePlane u8 [H - 2 m, W - 2 m] (1 = not shadow)."""
        H, W = dem.shape
        out = self.plane((H - 2 * margin, W - 2 * margin), np.uint8)
        with self.lock, stages.span('gpu: shadow layer'):
            self.ctx.shadow_layer_device(dem.ptr, 1, H, W, margin, sun_vector, sin_azimuth, cos_azimuth, min_slope_angle,
                                         max_sun_local_inc_angle, out.ptr, pixel_spacing_x, pixel_spacing_y, float32=float32)
            self.ctx.synchronize()
        return out

    def landcover_mask(self, worldcover_up3, copernicus, forest_classes, thresholds, year_offset):
        """WorldCover [3H, 3W] + CGLS [H, W] (DevicePlanes, u8) -> LAND DevicePlane [H, W] (create_landcover_mask's
        per-pixel part, :994-1115)."""
        H, W = copernicus.shape
        if worldcover_up3.shape != (3 * H, 3 * W):
            raise ValueError(f'WorldCover raster {worldcover_up3.shape} is not three times the CGLS grid {(H, W)}')
        out = self.plane((H, W), np.uint8)
        with self.lock, stages.span('gpu: LAND aggregation'):
            self.ctx.landcover_mask_device(worldcover_up3.ptr, copernicus.ptr, 1, H, W, forest_classes, out.ptr,
                                           thresholds=thresholds, year_offset=year_offset)
            self.ctx.synchronize()
        return out

    def landcover_mask_mesh(self, worldcover, copernicus, mesh_wc, mesh_cg, shape, spec):
        """Source windows of the two maps (DevicePlanes, u8, NOT on the product grid) read through their meshes -> (LAND
        DevicePlane [H, W], head uint64 [8] on the host): create_landcover_mask's two warps and its per-pixel part in one
        launch (DevicePlane.land_mesh)."""
        made = worldcover.land_mesh(copernicus, mesh_wc, mesh_cg, shape, spec)
        try:
            head = made['head'].numpy().reshape(-1)
        finally:
            made['head'].release()
        return made['land'], head

    # ---- writer side ----------------------------------------------------------------------------------------
    WEIGHTS_CAP = 64            # (n_in, n_out) pairs kept: a worker sees one tile size, i.e. about ten pairs

    def _conv_weights(self, n_in, n_out):
        """Device copies of geotiff.convolve_weights(n_in, n_out), cached.  Called with the engine's lock HELD."""
        key = (int(n_in), int(n_out))
        hit = self._weights.get(key)
        if hit is None:
            first, w = geotiff.convolve_weights(*key)
            d_first, d_w = self.ctx.malloc(max(first.size * 4, 16)), self.ctx.malloc(max(w.nbytes, 16))
            d_first.upload(first.astype(np.int32))
            d_w.upload(np.ascontiguousarray(w.T))               # [taps][n_out]: the layout the device pass reads
            hit = self._weights[key] = (d_first, d_w, w.shape[1])
        return hit

    def cubicspline_overview(self, plane, factor):
        """One CUBICSPLINE overview level of a Float32 plane on the device (geotiff.overview_cubicspline: horizontal pass
        into float64, vertical pass, float32): what `save_as_cog` asks GDAL for on non-integer layers (core.py:41-46)."""
        H, W = plane.shape
        oh, ow = -(-H // factor), -(-W // factor)
        tmp = self._take(H * ow * 8)
        out = self.plane((oh, ow), np.float32)
        try:
            with self.lock, stages.span('gpu: CUBICSPLINE overview'):
                if len(self._weights) + 2 > self.WEIGHTS_CAP:   # rasters of ever-changing sizes: start over -- here, under the
                    for d_first, d_w, _ in self._weights.values():      # lock and before this call's own lookups, so that no
                        d_first.free()                                  # launch ever reads a freed entry
                        d_w.free()
                    self._weights.clear()
                fx, wx, tx = self._conv_weights(W, ow)
                fy, wy, ty = self._conv_weights(H, oh)
                self.ctx.convolve_axis_device(plane.ptr, False, H, W, W, 1, ow, tx, fx.ptr, wx.ptr, tmp.ptr, True, ow, 1)
                self.ctx.convolve_axis_device(tmp.ptr, True, ow, H, 1, ow, oh, ty, fy.ptr, wy.ptr, out.ptr, False, 1, ow)
                self.ctx.synchronize()
        finally:
            self._give(tmp)
        return out

    def _float_pyramid(self, plane, factors):
        """The levels write_geotiff builds for a floating-point layer: cascaded (each from the previous one when the factor
        divides, GDAL's GDALRegenerateCascadingOverviews), else from the full-resolution raster."""
        H, W = plane.shape
        rasters, prev_f = [plane], 1
        for f in factors:
            f = int(f)
            if f > 1 and (H > 1 or W > 1):
                lv = self.cubicspline_overview(rasters[-1], f // prev_f) if (prev_f > 1 and f % prev_f == 0) \
                    else self.cubicspline_overview(plane, f)
                if lv.shape != (-(-H // f), -(-W // f)):            # ceil of a ceil can differ by one: from the full image
                    lv = self.cubicspline_overview(plane, f)
                rasters.append(lv)
                prev_f = f
        return rasters

    def layer_levels(self, plane, factors=(), tile=512):
        """DevicePlane [H, W] -> [geotiff.BlockedLevel]: the blocks of the full-resolution image and of every overview,
        predictor-encoded, in page-locked memory.  Integer layers (u8 / u16 / i16): NEAREST overviews + PREDICTOR=2, one
        launch; Float32: CUBICSPLINE overviews (cascaded) + PREDICTOR=3 (core.py:37-46, :66-69)."""
        if plane.dtype.kind == 'f':
            return self.float_levels([plane], factors, tile)
        H, W = plane.shape
        dt = plane.dtype
        predictor = 2
        lay = _capi.cog_layout(H, W, dt.itemsize, factors, tile)
        total = lay['total_bytes']
        dev_blocks = self._take(total)
        host = self.ctx.pinned_empty((total,), np.uint8)
        try:
            with self.lock, stages.span('gpu: plane -> COG blocks (+ d2h)'):
                self.ctx.cog_blocks_device(plane.ptr, dt.itemsize, H, W, dev_blocks.ptr, factors, tile, predictor)
                self.ctx.d2h_async(host, dev_blocks.ptr, total)
                self.ctx.synchronize()
        finally:
            self._give(dev_blocks)
        out = []
        for k, lv in enumerate(lay['levels']):
            n = lv['blocks_down'] * lv['blocks_across'] * tile * tile * dt.itemsize
            out.append(geotiff.BlockedLevel(lv['height'], lv['width'], 1, dt, tile, predictor,
                                            host[lv['offset_bytes']: lv['offset_bytes'] + n]))
        return out

    def float_levels(self, bands, factors=(), tile=512):
        """Float32 planes of ONE file (1 band: the DEM layer; 3: an RGB composite) -> [geotiff.BlockedLevel] (planar:
        band-major inside every level), floating-point predictor, CUBICSPLINE overviews per band."""
        if any(b.dtype != np.float32 for b in bands):
            raise ValueError('float planes: float32 only')
        pyramids = [self._float_pyramid(b, factors) for b in bands]
        n_levels = len(pyramids[0])
        sizes = [_capi.cog_layout(pyramids[0][k].shape[0], pyramids[0][k].shape[1], 4, (), tile)['total_bytes'] for k in range(n_levels)]
        total = len(bands) * sum(sizes)
        dev_blocks = self._take(total)
        host = self.ctx.pinned_empty((total,), np.uint8)
        offs, cur = [], 0
        try:
            with self.lock, stages.span('gpu: Float32 planes -> blocks (+ d2h)'):
                for k in range(n_levels):
                    offs.append(cur)
                    for c in range(len(bands)):
                        lv = pyramids[c][k]
                        self.ctx.cog_blocks_device(lv.ptr, 4, lv.shape[0], lv.shape[1], dev_blocks.ptr + cur, (), tile, 3)
                        cur += sizes[k]
                self.ctx.d2h_async(host, dev_blocks.ptr, total)
                self.ctx.synchronize()
        finally:
            self._give(dev_blocks)
        return [geotiff.BlockedLevel(pyramids[0][k].shape[0], pyramids[0][k].shape[1], len(bands), np.float32, tile, 3,
                                     host[offs[k]: offs[k] + len(bands) * sizes[k]]) for k in range(n_levels)]

    def resample_nearest(self, plane, out_height, out_width):
        """geotiff.resample_nearest of a resident plane -> numpy [out_height, out_width] (the browse PNG's pixels): the gather
        runs in HBM, the small image is what crosses PCIe."""
        H, W = plane.shape
        ys, xs = geotiff.resample_nearest_indices(H, W, out_height, out_width)
        idx = np.concatenate([ys, xs]).astype(np.int32)
        n_out = int(out_height) * int(out_width) * plane.dtype.itemsize
        d_idx, d_out = self._take(max(idx.nbytes, 16)), self._take(max(n_out, 16))
        host = self.ctx.pinned_empty((int(out_height), int(out_width)), plane.dtype)
        pin_idx = self.ctx.pinned_empty(idx.shape, np.int32)
        np.copyto(pin_idx, idx)
        try:
            with self.lock, stages.span('gpu: resample (browse)'):
                self.ctx.h2d_async(d_idx.ptr, pin_idx)
                self.ctx.gather_2d_device(plane.ptr, plane.dtype.itemsize, H, W, d_idx.ptr, out_height, d_idx.ptr + 4 * int(out_height),
                                          out_width, d_out.ptr)
                if n_out:
                    self.ctx.d2h_async(host, d_out.ptr, n_out)
                self.ctx.synchronize()
        finally:
            self._give(d_idx)
            self._give(d_out)
        return host

    def byte_plane(self, plane):
        """A layer as GDAL stores it in a Byte band of the multi-band file (dswx_hls._gdal_byte; dswx_to_byte_device)."""
        if plane.dtype == np.uint8:
            return plane
        out = self.plane(plane.shape, np.uint8)
        with self.lock, stages.span('gpu: layer -> Byte band'):
            self.ctx.to_byte_device(plane.ptr, plane.dtype, plane.shape[0] * plane.shape[1], out.ptr)
            self.ctx.synchronize()
        return out

    def shoreline_mask(self, plan, shape):
        """The ocean mask of a shoreline.Plan as a resident uint8 plane of `shape`: a plane of zeros (ocean), the polygons burnt
        as 1 (32 colours per call, in place), then every pixel within plan.radius of an edge set to 1 (dswx_burn_device,
        dswx_reach_device).  The two record tables cross PCIe, not the plane."""
        from . import burn as _burn
        from . import reach as _reach
        height, width = shape
        mask = self.constant_plane(shape, 0)
        acc = self.plane((1, height, width), np.uint32)
        out = _capi.BurnOut.of(acc=acc.ptr, mask=mask.ptr)
        tables = [(t, 'burn_device', _burn.Spec(burn=1)) for t in plan.burn_calls] + [(plan.reach, 'reach_device', _reach.Spec(plan.radius, burn=1))]
        try:
            for (verts, first), entry, spec in tables:
                if not len(verts):
                    continue
                d_verts, d_first = self.upload(verts.view(np.uint32).reshape(-1, 4)), self.upload(first)
                try:
                    with self.lock, stages.span('gpu: ' + entry[:-7]):
                        getattr(self.ctx, entry)(d_verts.ptr, d_first.ptr, spec, 1, height, width, mask.ptr, out)
                        self.ctx.synchronize()
                finally:
                    d_verts.release()
                    d_first.release()
        finally:
            acc.release()
        return mask

    def constant_plane(self, shape, value):
        out = self.plane(shape, np.uint8)
        with self.lock:
            _capi._check(self.ctx.lib.dswx_memset_d(self.ctx.handle, out.ptr, int(value) & 0xff, out.nbytes))
        return out

    def band_stack_levels(self, bands, factors=(), tile=512):
        """Byte planes of ONE multi-band file (save_dswx_product: ten bands, planar) -> [geotiff.BlockedLevel] (band-major
        inside every level): blocks + NEAREST overviews + PREDICTOR=2 of every band on the device, each (band, level) piece
        copied to its place in page-locked memory."""
        H, W = bands[0].shape
        if any(b.dtype != np.uint8 or b.shape != (H, W) for b in bands):
            raise ValueError('band stack: uint8 planes of one shape')
        lay = _capi.cog_layout(H, W, 1, factors, tile)
        per_band = lay['total_bytes']
        sizes = [lv['blocks_down'] * lv['blocks_across'] * tile * tile for lv in lay['levels']]
        starts = np.concatenate([[0], np.cumsum([len(bands) * n for n in sizes])]).astype(np.int64)
        dev_blocks = self._take(per_band)
        host = self.ctx.pinned_empty((len(bands) * per_band,), np.uint8)
        try:
            with self.lock, stages.span('gpu: plane -> COG blocks (+ d2h)'):
                for c, b in enumerate(bands):
                    self.ctx.cog_blocks_device(b.ptr, 1, H, W, dev_blocks.ptr, factors, tile, 2)
                    for k, lv in enumerate(lay['levels']):
                        at = int(starts[k]) + c * sizes[k]
                        self.ctx.d2h_async(host[at: at + sizes[k]], dev_blocks.ptr + lv['offset_bytes'], sizes[k])
                self.ctx.synchronize()
        finally:
            self._give(dev_blocks)
        return [geotiff.BlockedLevel(lv['height'], lv['width'], len(bands), np.uint8, tile, 2,
                                     host[int(starts[k]): int(starts[k + 1])]) for k, lv in enumerate(lay['levels'])]

    def rgb_levels(self, red, green, blue, diag, scale, offset, clip, tile=512, factors=()):
        """The three-band Float32 composite of _save_output_rgb_file (dswx_hls.py:3013-3036) as planar BlockedLevels
        (floating-point predictor, CUBICSPLINE overviews for `factors`): scaling on the device, NaN where `diag` carries the
        fill code."""
        H, W = red.shape
        n = H * W
        rgb = self._take(3 * n * 4)
        try:
            with self.lock, stages.span('gpu: RGB planes'):
                self.ctx.rgb_planes_device(red.ptr, green.ptr, blue.ptr, diag.ptr if diag is not None else None, n,
                                           scale, offset, clip, rgb.ptr)
                self.ctx.synchronize()
            views = [_PlaneView(rgb.ptr + c * n * 4, (H, W), np.float32, keep=rgb) for c in range(3)]
            return self.float_levels(views, factors, tile)
        finally:
            self._give(rgb)


_engines = {}
_engines_lock = threading.Lock()


def engine_of(ctx):
    with _engines_lock:
        e = _engines.get(id(ctx))
        if e is None or e.ctx is not ctx:
            e = _engines[id(ctx)] = TileEngine(ctx)
        return e
