"""ctypes binding of include/dswx_hip.h (the C-ABI of the HIP classifier).

There is exactly one compute path: the HIP library.  If it is missing, or no
MI355X is visible, every entry point here raises -- nothing falls back to numpy.
"""
import contextlib
import ctypes
import threading
import weakref
import os

import numpy as np

from . import build as _build

DSWX_ABI_VERSION = 7
OK, ERR_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -3, -4, -5
ADJ_MODES = {'mask': 0, 'ignore': 1, 'cover': 2}
BAND_NAMES = ('blue', 'green', 'red', 'nir', 'swir1', 'swir2')
THRESHOLD_NAMES = ('wigt', 'awgt', 'pswt_1_mndwi', 'pswt_1_nir', 'pswt_1_swir1',
                   'pswt_1_ndvi', 'pswt_2_mndwi', 'pswt_2_blue', 'pswt_2_nir',
                   'pswt_2_swir1', 'pswt_2_swir2', 'lcmask_nir')
U8_LAYERS = ('wtr1', 'wtr1_aerosol', 'wtr2', 'wtr', 'bwtr', 'conf', 'cloud', 'browse')
F64_LAYERS = ('mndwi', 'ndvi', 'awesh')
# every symbol include/dswx_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTED_SYMBOLS = (
    'dswx_abi_version', 'dswx_last_error', 'dswx_device_count', 'dswx_ctx_create',
    'dswx_ctx_destroy', 'dswx_params_default', 'dswx_classify_host',
    'dswx_classify_device', 'dswx_classify_device_2d', 'dswx_classify_batch', 'dswx_synth_batch', 'dswx_interpret_layer_host', 'dswx_shadow_layer_host', 'dswx_shadow_layer_device', 'dswx_shadow_thresholds', 'dswx_shadow_layer_host_q', 'dswx_shadow_layer_device_q', 'dswx_shadow_layer_host_q32', 'dswx_shadow_layer_device_q32', 'dswx_landcover_mask_host', 'dswx_landcover_mask_device',
    'dswx_synth_fill', 'dswx_device_malloc',
    'dswx_device_free', 'dswx_host_alloc', 'dswx_host_free', 'dswx_memcpy_h2d', 'dswx_memcpy_d2h', 'dswx_memset_d',
    'dswx_stream_synchronize', 'dswx_event_create', 'dswx_event_destroy',
    'dswx_event_record', 'dswx_event_elapsed_ms', 'dswx_last_kernel_info',
    'dswx_batch_layout', 'dswx_batch_create', 'dswx_batch_destroy', 'dswx_batch_planes', 'dswx_batch_info',
    'dswx_batch_classify', 'dswx_batch_synth', 'dswx_batch_place_search', 'dswx_batch_place_slide',
    'dswx_batch_va_budget', 'dswx_batch_pool_trim',
    'dswx_shadow_layer_batch', 'dswx_landcover_mask_batch',
    'dswx_cog_layout', 'dswx_cog_blocks_device', 'dswx_untile_device', 'dswx_rgb_planes_device', 'dswx_copy_2d_device', 'dswx_convolve_axis_device',
    'dswx_to_byte_device', 'dswx_gather_2d_device',
    'dswx_memcpy_h2d_async', 'dswx_memcpy_d2h_async',
    'dswx_checksum_device', 'dswx_batch_checksum', 'dswx_checksum_host',
    'dswx_compare_device', 'dswx_batch_compare', 'dswx_compare_host',
    'dswx_histogram_device', 'dswx_batch_histogram', 'dswx_histogram_host',
    'dswx_crosstab_device', 'dswx_batch_crosstab', 'dswx_crosstab_host',
    'dswx_stack_device', 'dswx_batch_stack', 'dswx_stack_host',
    'dswx_grid_device', 'dswx_batch_grid', 'dswx_grid_host',
    'dswx_label_device', 'dswx_batch_label', 'dswx_label_host',
    'dswx_body_table_device', 'dswx_batch_body_table', 'dswx_body_table_host',
    'dswx_distance_device', 'dswx_batch_distance', 'dswx_distance_host',
    'dswx_outline_work_bytes', 'dswx_outline_device', 'dswx_outline_host',
    'dswx_burn_device', 'dswx_batch_burn', 'dswx_burn_host',
    'dswx_reach_device', 'dswx_batch_reach', 'dswx_reach_host',
    'dswx_mosaic_device', 'dswx_batch_mosaic', 'dswx_mosaic_host',
    'dswx_warp_device', 'dswx_batch_warp', 'dswx_warp_host',
    'dswx_resample_device', 'dswx_resample_host',
    'dswx_land_mesh_device', 'dswx_land_mesh_host')
HAS_COMPARE = 1                   # DSWX_HAS_COMPARE: additive to ABI v7
CMP_U8, CMP_U16, CMP_I16, CMP_F32, CMP_F64 = range(5)
HAS_HISTOGRAM = 1                 # DSWX_HAS_HISTOGRAM: additive to ABI v7
HIST_U8, HIST_U16, HIST_I16, HIST_DIAG = range(4)
HIST_BINS = 256
HAS_CROSSTAB = 1                  # DSWX_HAS_CROSSTAB: additive to ABI v7
CROSSTAB_CELLS, CROSSTAB_MAX_PAIRS = 256, 6
HAS_STACK = 1                     # DSWX_HAS_STACK: additive to ABI v7
STACK_MAX_CATS, STACK_MAX_TILES, STACK_NONE, STACK_NO_SHARE = 4, 65535, 65535, 255
HAS_GRID = 1                      # DSWX_HAS_GRID: additive to ABI v7
GRID_MAX_CATS, GRID_MAX_CELL_PIXELS, GRID_NO_SHARE, GRID_NONE = 4, 1 << 24, 255, 255
HAS_LABEL = 1                     # DSWX_HAS_LABEL: additive to ABI v7
LABEL_SUMMARY_WORDS = 40
LABEL_RECT_H, LABEL_RECT_W = 32, 128   # csrc/dswx_label_rule.h: the rectangle one workgroup labels in LDS (tests build shapes around its seams)
HAS_BODY_TABLE = 1                # DSWX_HAS_BODY_TABLE: additive to ABI v7
BODY_ROW_WORDS, BODY_HEAD_WORDS, BODY_MAX_CATS = 16, 8, 4
BODY_CHUNK, BODY_SCAN_STEP = 4096, 256   # csrc/dswx_body_rule.h: the elements one workgroup scans, the chunk counts per step of the scan launch (tests build shapes around the seams)
BODY_RECT_H, BODY_RECT_W = 32, 128       # csrc/dswx_body_rule.h: the rectangle whose contributions one workgroup combines in LDS
HAS_DISTANCE = 1                  # DSWX_HAS_DISTANCE: additive to ABI v7
DISTANCE_NONE, DISTANCE_SUMMARY_WORDS, DISTANCE_MAX_WIDTH, DISTANCE_MAX_SIDE = 0xFFFFFFFF, 40, 8192, 46340
# csrc/dswx_distance_rule.h: the rows and the columns of a column-pass thread, the columns of a block of the row pass and how far
# the row pass looks to either side before it turns to the blocks (tests build shapes around the seams)
DISTANCE_BAND_H, DISTANCE_COLS, DISTANCE_BLOCK_W, DISTANCE_NEAR = 64, 4, 64, 32
HAS_OUTLINE = 1                   # DSWX_HAS_OUTLINE: additive to ABI v7
OUTLINE_ROW_WORDS, OUTLINE_HEAD_WORDS = 8, 8
HAS_BURN = 1                      # DSWX_HAS_BURN: additive to ABI v7
BURN_HEAD_WORDS, BURN_MAX_COORD = 8, 1 << 30
# csrc/dswx_burn_rule.h: the rows of an edge that its own thread finishes (a longer edge is shared out over the wave) and the
# pixels of a row that a wave of the scan launch takes per step (tests build shapes around the seams)
BURN_THREAD_ROWS, BURN_SCAN_STEP = 4, 256
HAS_REACH = 1                     # DSWX_HAS_REACH: additive to ABI v7
REACH_HEAD_WORDS, REACH_MAX_RADIUS = 8, 1 << 20
# csrc/dswx_reach_rule.h: as for the burn (tests build shapes around the seams)
REACH_THREAD_ROWS, REACH_SCAN_STEP = 4, 256
HAS_MOSAIC = 1                    # DSWX_HAS_MOSAIC: additive to ABI v7
# csrc/dswx_mosaic.hip: the rows and the columns of the canvas rectangle of one workgroup, the tiles of the surviving-tile list
# in LDS, the placements tested per step and the loads in flight per thread (tests build shapes around the seams)
MOSAIC_RECT_H, MOSAIC_RECT_W, MOSAIC_LIST, MOSAIC_CHUNK, MOSAIC_ROUND = 4, 1024, 512, 256, 8
MOSAIC_MAX_SIDE = 1 << 30
HAS_WARP = 1                      # DSWX_HAS_WARP: additive to ABI v7
WARP_HEAD_WORDS, WARP_MAX_SHIFT, WARP_OUTSIDE, WARP_MAX_PIXELS = 8, 8, 0xFFFFFFFF, 1 << 30
# csrc/dswx_warp.hip: the rows and the columns of the destination rectangle of one workgroup, the pixels of a thread, and the
# shift below which a thread's pixels cross mesh cells (tests build shapes around the seams)
WARP_RECT_H, WARP_RECT_W, WARP_UNIT, WARP_FINE_BELOW = 4, 1024, 16, 4
HAS_RESAMPLE = 1                  # DSWX_HAS_RESAMPLE: additive to ABI v7
RESAMPLE_HEAD_WORDS, RESAMPLE_F32, RESAMPLE_I16, RESAMPLE_BILINEAR, RESAMPLE_CUBIC = 8, 0, 1, 1, 2
# csrc/dswx_resample_rule.h: the rows and the columns of the destination rectangle of one workgroup and the elements of the
# source window that it stages in LDS (a larger source box gathers from global memory; tests build shapes around the seams)
RESAMPLE_RECT_H, RESAMPLE_RECT_W, RESAMPLE_LDS_ELEMS = 8, 32, 4096
HAS_LAND_MESH = 1                 # DSWX_HAS_LAND_MESH: additive to ABI v7
LAND_MESH_HEAD_WORDS = 8
# csrc/dswx_land_mesh.hip: the rows and the columns of the rectangle of HLS pixels of one workgroup (tests build shapes around the seams)
LAND_MESH_RECT_H, LAND_MESH_RECT_W = 8, 32


class DswxError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f'dswx_hip error {code}: {message}')
        self.code = code


class Params(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_double) for n in THRESHOLD_NAMES] +
                [('band_fill', ctypes.c_double * 6),
                 ('fmask_fill', ctypes.c_double),
                 ('aerosol_max_nir', ctypes.c_double),
                 ('clip_negative_reflectance', ctypes.c_int32),
                 ('mask_adjacent_to_cloud_mode', ctypes.c_int32),
                 ('apply_aerosol_class_remapping', ctypes.c_int32),
                 ('collapse_wtr_classes', ctypes.c_int32),
                 ('browse_exclude_psw_aggressive', ctypes.c_int32),
                 ('browse_not_water_to_nodata', ctypes.c_int32),
                 ('browse_cloud_to_nodata', ctypes.c_int32),
                 ('browse_snow_to_nodata', ctypes.c_int32),
                 ('browse_ocean_masked_to_nodata', ctypes.c_int32),
                 ('offset_and_scale_inputs', ctypes.c_int32),
                 ('aerosol_fmask_lut', (ctypes.c_uint8 * 256) * 4),
                 ('band_scale', ctypes.c_double * 6),
                 ('band_offset', ctypes.c_double * 6)])


class BatchGeom(ctypes.Structure):
    _fields_ = [('n_tiles', ctypes.c_int64), ('height', ctypes.c_int64), ('width', ctypes.c_int64),
                ('tile_stride', ctypes.c_int64)]


class PlanesIn(ctypes.Structure):
    _fields_ = [('band', ctypes.c_void_p * 6), ('fmask', ctypes.c_void_p),
                ('land', ctypes.c_void_p), ('shad', ctypes.c_void_p),
                ('ocean', ctypes.c_void_p)]


class PlanesOut(ctypes.Structure):
    _fields_ = ([('diag', ctypes.c_void_p)] +
                [(n, ctypes.c_void_p) for n in U8_LAYERS] +
                [(n, ctypes.c_void_p) for n in F64_LAYERS])


# resident batches (include/dswx_hip.h, ABI v4; v5: address-space accounting, DSWX_BATCH_ALL_TILES)
BATCH_ALL_TILES = -1
BATCH_MASKS, BATCH_WTR1_AEROSOL, BATCH_BROWSE, BATCH_SEPARATE_OUTPUTS, BATCH_SLIDING_OUTPUTS = 1, 2, 4, 1 << 10, 1 << 11
BATCH_MAX_PLANES = 20
PLANE_INDEX = dict(blue=0, green=1, red=2, nir=3, swir1=4, swir2=5, fmask=6, land=7, shad=8, ocean=9, diag=10,
                   wtr1=11, wtr1_aerosol=12, wtr2=13, wtr=14, bwtr=15, conf=16, cloud=17, browse=18, counters=19)


class BatchLayout(ctypes.Structure):
    _fields_ = [('tile_stride', ctypes.c_int64), ('arena_bytes', ctypes.c_uint64),
                ('plane_bytes', ctypes.c_uint64 * BATCH_MAX_PLANES),
                ('plane_offset', ctypes.c_uint64 * BATCH_MAX_PLANES),
                ('write_span_bytes', ctypes.c_uint64)]


class BatchInfo(ctypes.Structure):
    _fields_ = [('geom', BatchGeom), ('flags', ctypes.c_uint32), ('n_allocations', ctypes.c_int32),
                ('bytes_allocated', ctypes.c_uint64), ('search_candidates', ctypes.c_int32),
                ('search_probes', ctypes.c_int32), ('first_come_launch_ms', ctypes.c_float),
                ('kept_launch_ms', ctypes.c_float), ('va_reserved_bytes', ctypes.c_uint64),
                ('va_retired_bytes', ctypes.c_uint64), ('va_budget_bytes', ctypes.c_uint64),
                ('va_pooled_bytes', ctypes.c_uint64), ('note', ctypes.c_char * 256)]


class CompareRecord(ctypes.Structure):
    """dswx_compare_t; proteus_amd.compare.RECORD is the same layout as a numpy dtype."""
    _fields_ = [('n_diff', ctypes.c_int64), ('first', ctypes.c_int64), ('max_abs_diff', ctypes.c_double),
                ('reserved', ctypes.c_uint64)]


class CrosstabSpec(ctypes.Structure):
    """dswx_crosstab_spec_t; proteus_amd.crosstab.Spec is the Python form."""
    _fields_ = [('a_kind', ctypes.c_int32), ('a_lo', ctypes.c_int32), ('a_shift', ctypes.c_int32), ('col_bits', ctypes.c_int32),
                ('row_of_bin', ctypes.c_uint8 * 256), ('col_of_byte', ctypes.c_uint8 * 256)]

    @classmethod
    def of(cls, spec):
        c = cls(spec.a_kind, spec.a_lo, spec.a_shift, spec.col_bits)
        ctypes.memmove(c.row_of_bin, spec.row_of_bin.ctypes.data, 256)
        ctypes.memmove(c.col_of_byte, spec.col_of_byte.ctypes.data, 256)
        return c


class CrosstabPair(ctypes.Structure):
    """dswx_crosstab_pair_t"""
    _fields_ = [('plane_a', ctypes.c_int32), ('plane_b', ctypes.c_int32), ('spec', CrosstabSpec)]


class StackSpec(ctypes.Structure):
    """dswx_stack_spec_t; proteus_amd.stack.Spec is the Python form."""
    _fields_ = [('n_cats', ctypes.c_int32), ('fill', ctypes.c_int32), ('cat_of_byte', ctypes.c_uint8 * 256)]

    @classmethod
    def of(cls, spec):
        c = cls(spec.n_cats, spec.fill)
        ctypes.memmove(c.cat_of_byte, spec.cat_of_byte.ctypes.data, 256)
        return c


class StackOut(ctypes.Structure):
    """dswx_stack_out_t: plane addresses, 0 / None = not wanted."""
    _fields_ = [('count', ctypes.c_void_p * STACK_MAX_CATS), ('last', ctypes.c_void_p), ('last_index', ctypes.c_void_p),
                ('share', ctypes.c_void_p)]

    @classmethod
    def of(cls, count=(), last=None, last_index=None, share=None):
        c = cls()
        for k, p in enumerate(count):
            c.count[k] = p or None
        c.last, c.last_index, c.share = last or None, last_index or None, share or None
        return c


class MosaicSpec(ctypes.Structure):
    """dswx_mosaic_spec_t; proteus_amd.mosaic.Spec is the Python form."""
    _fields_ = [('n_cats', ctypes.c_int32), ('fill', ctypes.c_int32), ('outside', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('cat_of_byte', ctypes.c_uint8 * 256)]

    @classmethod
    def of(cls, spec):
        c = cls(spec.n_cats, spec.fill, spec.outside, getattr(spec, 'reserved', 0))
        ctypes.memmove(c.cat_of_byte, spec.cat_of_byte.ctypes.data, 256)
        return c


class WarpSpec(ctypes.Structure):
    """dswx_warp_spec_t; proteus_amd.warp.Spec is the Python form."""
    _fields_ = [('elem_bytes', ctypes.c_int32), ('shift', ctypes.c_int32), ('outside', ctypes.c_uint32), ('reserved', ctypes.c_int32),
                ('src_tile_stride', ctypes.c_int64), ('mesh_tile_stride_nodes', ctypes.c_int64)]

    @classmethod
    def of(cls, spec):
        return cls(int(spec.elem_bytes), int(spec.shift), int(spec.outside) & 0xFFFFFFFF, int(getattr(spec, 'reserved', 0)),
                   int(spec.src_tile_stride), int(spec.mesh_tile_stride_nodes))


class WarpOut(ctypes.Structure):
    """dswx_warp_out_t: addresses, 0 / None = not wanted."""
    _fields_ = [('dst', ctypes.c_void_p), ('src_index', ctypes.c_void_p), ('head', ctypes.c_void_p)]

    @classmethod
    def of(cls, dst=None, src_index=None, head=None):
        return cls(dst or None, src_index or None, head or None)


class ResampleSpec(ctypes.Structure):
    """dswx_resample_spec_t; proteus_amd.resample.Spec is the Python form."""
    _fields_ = [('kind', ctypes.c_int32), ('method', ctypes.c_int32), ('shift', ctypes.c_int32), ('has_nodata', ctypes.c_int32),
                ('nodata', ctypes.c_uint32), ('outside', ctypes.c_uint32), ('reserved', ctypes.c_int32), ('reserved2', ctypes.c_int32),
                ('src_tile_stride', ctypes.c_int64), ('mesh_tile_stride_nodes', ctypes.c_int64)]

    @classmethod
    def of(cls, spec):
        return cls(int(spec.kind), int(spec.method), int(spec.shift), int(spec.has_nodata), int(spec.nodata_word) & 0xFFFFFFFF,
                   int(spec.outside) & 0xFFFFFFFF, int(getattr(spec, 'reserved', 0)), 0, int(spec.src_tile_stride),
                   int(spec.mesh_tile_stride_nodes))


class ResampleOut(ctypes.Structure):
    """dswx_resample_out_t: addresses, 0 / None = not wanted."""
    _fields_ = [('dst', ctypes.c_void_p), ('how', ctypes.c_void_p), ('head', ctypes.c_void_p)]

    @classmethod
    def of(cls, dst=None, how=None, head=None):
        return cls(dst or None, how or None, head or None)


class LandMeshSpec(ctypes.Structure):
    """dswx_land_mesh_spec_t; proteus_amd.landmesh.Spec is the Python form.  `forest` keeps the list that the pointer names."""
    _fields_ = [('shift_wc', ctypes.c_int32), ('shift_cg', ctypes.c_int32), ('outside_wc', ctypes.c_uint32), ('outside_cg', ctypes.c_uint32),
                ('thresholds', ctypes.c_int32 * 4), ('year_offset', ctypes.c_int32), ('n_forest_classes', ctypes.c_int32),
                ('reserved', ctypes.c_int32), ('reserved2', ctypes.c_int32), ('forest_classes', ctypes.c_void_p),
                ('wc_tile_stride', ctypes.c_int64), ('cg_tile_stride', ctypes.c_int64), ('mesh_wc_tile_stride_nodes', ctypes.c_int64),
                ('mesh_cg_tile_stride_nodes', ctypes.c_int64), ('land_tile_stride', ctypes.c_int64)]

    @classmethod
    def of(cls, spec):
        fc = np.ascontiguousarray(list(spec.forest_classes or []), dtype=np.int32)
        c = cls(int(spec.shift_wc), int(spec.shift_cg), int(spec.outside_wc) & 0xFFFFFFFF, int(spec.outside_cg) & 0xFFFFFFFF,
                (ctypes.c_int32 * 4)(*[int(v) for v in spec.thresholds]), int(spec.year_offset), int(fc.size),
                int(getattr(spec, 'reserved', 0)), int(getattr(spec, 'reserved2', 0)), fc.ctypes.data if fc.size else None,
                int(spec.wc_tile_stride), int(spec.cg_tile_stride), int(spec.mesh_wc_tile_stride_nodes),
                int(spec.mesh_cg_tile_stride_nodes), int(spec.land_tile_stride))
        c.forest = fc
        return c


class GridSpec(ctypes.Structure):
    """dswx_grid_spec_t; proteus_amd.grid.Spec is the Python form."""
    _fields_ = [('n_cats', ctypes.c_int32), ('cell_h', ctypes.c_int32), ('cell_w', ctypes.c_int32),
                ('cat_of_byte', ctypes.c_uint8 * 256)]

    @classmethod
    def of(cls, spec):
        c = cls(spec.n_cats, spec.cell_h, spec.cell_w)
        ctypes.memmove(c.cat_of_byte, spec.cat_of_byte.ctypes.data, 256)
        return c


class GridOut(ctypes.Structure):
    """dswx_grid_out_t: plane addresses, 0 / None = not wanted."""
    _fields_ = [('count', ctypes.c_void_p * GRID_MAX_CATS), ('share', ctypes.c_void_p), ('coverage', ctypes.c_void_p),
                ('major', ctypes.c_void_p)]

    @classmethod
    def of(cls, count=(), share=None, coverage=None, major=None):
        c = cls()
        for k, p in enumerate(count):
            c.count[k] = p or None
        c.share, c.coverage, c.major = share or None, coverage or None, major or None
        return c


class LabelSpec(ctypes.Structure):
    """dswx_label_spec_t; proteus_amd.label.Spec is the Python form."""
    _fields_ = [('connectivity', ctypes.c_int32), ('replace', ctypes.c_int32), ('min_size', ctypes.c_uint32),
                ('member_of_byte', ctypes.c_uint8 * 256)]

    @classmethod
    def of(cls, spec):
        c = cls(spec.connectivity, spec.replace, spec.min_size)
        ctypes.memmove(c.member_of_byte, spec.member_of_byte.ctypes.data, 256)
        return c


class LabelOut(ctypes.Structure):
    """dswx_label_out_t: plane addresses, 0 / None = not wanted."""
    _fields_ = [('label', ctypes.c_void_p), ('size', ctypes.c_void_p), ('sieved', ctypes.c_void_p), ('summary', ctypes.c_void_p)]

    @classmethod
    def of(cls, label=None, size=None, sieved=None, summary=None):
        return cls(label or None, size or None, sieved or None, summary or None)


class BodySpec(ctypes.Structure):
    """dswx_body_spec_t; proteus_amd.bodies.Spec is the Python form."""
    _fields_ = [('max_rows', ctypes.c_int64), ('n_cats', ctypes.c_int32), ('cat_of_byte', ctypes.c_uint8 * 256)]

    @classmethod
    def of(cls, spec):
        c = cls(spec.max_rows, spec.n_cats)
        ctypes.memmove(c.cat_of_byte, spec.cat_of_byte.ctypes.data, 256)
        return c


class BodyOut(ctypes.Structure):
    """dswx_body_out_t: addresses, 0 / None = not wanted."""
    _fields_ = [('dense', ctypes.c_void_p), ('rows', ctypes.c_void_p), ('head', ctypes.c_void_p)]

    @classmethod
    def of(cls, dense=None, rows=None, head=None):
        return cls(dense or None, rows or None, head or None)


class DistanceSpec(ctypes.Structure):
    """dswx_distance_spec_t; proteus_amd.distance.Spec is the Python form."""
    _fields_ = [('max_radius', ctypes.c_uint32), ('mark', ctypes.c_int32), ('target_of_byte', ctypes.c_uint8 * 256)]

    @classmethod
    def of(cls, spec):
        c = cls(spec.max_radius, spec.mark)
        ctypes.memmove(c.target_of_byte, spec.target_of_byte.ctypes.data, 256)
        return c


class DistanceOut(ctypes.Structure):
    """dswx_distance_out_t: plane addresses, 0 / None = not wanted."""
    _fields_ = [('dist2', ctypes.c_void_p), ('nearest', ctypes.c_void_p), ('within', ctypes.c_void_p), ('summary', ctypes.c_void_p)]

    @classmethod
    def of(cls, dist2=None, nearest=None, within=None, summary=None):
        return cls(dist2 or None, nearest or None, within or None, summary or None)


class OutlineSpec(ctypes.Structure):
    """dswx_outline_spec_t; proteus_amd.outline.Spec is the Python form."""
    _fields_ = [('max_edges', ctypes.c_int64), ('max_rings', ctypes.c_int64), ('connectivity', ctypes.c_int32),
                ('reserved', ctypes.c_int32)]

    @classmethod
    def of(cls, spec):
        return cls(spec.max_edges, spec.max_rings, spec.connectivity, 0)


class OutlineOut(ctypes.Structure):
    """dswx_outline_out_t: addresses, 0 / None = not wanted."""
    _fields_ = [('chain', ctypes.c_void_p), ('rings', ctypes.c_void_p), ('head', ctypes.c_void_p)]

    @classmethod
    def of(cls, chain=None, rings=None, head=None):
        return cls(chain or None, rings or None, head or None)


class BurnSpec(ctypes.Structure):
    """dswx_burn_spec_t; proteus_amd.burn.Spec is the Python form."""
    _fields_ = [('burn', ctypes.c_int32), ('background', ctypes.c_int32), ('mask_tile_stride', ctypes.c_int64),
                ('src_tile_stride', ctypes.c_int64)]

    @classmethod
    def of(cls, spec):
        return cls(spec.burn, spec.background, spec.mask_tile_stride, spec.src_tile_stride)


class ReachSpec(ctypes.Structure):
    """dswx_reach_spec_t; proteus_amd.reach.Spec is the Python form."""
    _fields_ = BurnSpec._fields_ + [('radius', ctypes.c_uint32), ('reserved', ctypes.c_uint32)]

    @classmethod
    def of(cls, spec):
        return cls(spec.burn, spec.background, spec.mask_tile_stride, spec.src_tile_stride, spec.radius, spec.reserved)


class BurnOut(ctypes.Structure):
    """dswx_burn_out_t: addresses, 0 / None = not wanted."""
    _fields_ = [('acc', ctypes.c_void_p), ('mask', ctypes.c_void_p), ('head', ctypes.c_void_p)]

    @classmethod
    def of(cls, acc=None, mask=None, head=None):
        return cls(acc or None, mask or None, head or None)


# the struct mirrors of the analytic entries by their C names (the offset tests compile the header against them)
ANALYTIC_STRUCTS = {'dswx_label_spec_t': LabelSpec, 'dswx_label_out_t': LabelOut, 'dswx_body_spec_t': BodySpec,
                    'dswx_body_out_t': BodyOut, 'dswx_distance_spec_t': DistanceSpec, 'dswx_distance_out_t': DistanceOut,
                    'dswx_outline_spec_t': OutlineSpec, 'dswx_outline_out_t': OutlineOut,
                    'dswx_burn_spec_t': BurnSpec, 'dswx_burn_out_t': BurnOut,
                    'dswx_reach_spec_t': ReachSpec}

COG_MAX_LEVELS = 8


class CogLayout(ctypes.Structure):
    _fields_ = [('n_levels', ctypes.c_int32), ('tile', ctypes.c_int32), ('factor', ctypes.c_int32 * COG_MAX_LEVELS),
                ('height', ctypes.c_int64 * COG_MAX_LEVELS), ('width', ctypes.c_int64 * COG_MAX_LEVELS),
                ('blocks_down', ctypes.c_int32 * COG_MAX_LEVELS), ('blocks_across', ctypes.c_int32 * COG_MAX_LEVELS),
                ('offset_bytes', ctypes.c_uint64 * COG_MAX_LEVELS), ('total_bytes', ctypes.c_uint64)]


_lib = None


def library_path():
    """The in-tree product library -- or another build of the same sources named by DSWX_HIP_LIB (tests: the build with
    the host code under UBSan, proteus_amd.build.build_ubsan)."""
    return os.environ.get('DSWX_HIP_LIB') or _build.LIB_PATH


_alt_libs = {}


def va_budget(new_budget_bytes=0):
    """dswx_batch_va_budget: the library's process-wide account of the address space its sliding ranges hold."""
    v = [ctypes.c_uint64() for _ in range(5)]
    _check(load_library().dswx_batch_va_budget(int(new_budget_bytes), *[ctypes.byref(x) for x in v]))
    return dict(zip(('budget_bytes', 'live_bytes', 'retired_bytes', 'loose_bytes', 'pooled_bytes'), (int(x.value) for x in v)))


def pool_trim():
    """dswx_batch_pool_trim: the pooled chunks of dropped sliding ranges back to the device (call when no other thread of
    the process allocates: the retired reservations are freed and re-reserved empty).  Returns the bytes released."""
    v = ctypes.c_uint64()
    _check(load_library().dswx_batch_pool_trim(ctypes.byref(v)))
    return int(v.value)


def load_library(path=None):
    """dlopen the in-tree HIP library; raises if it has not been built.  `path` loads another
    build of the same ABI next to it (tools/ab_variants.py: A/B of two builds in one process)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    if path is not None and path in _alt_libs:
        return _alt_libs[path]
    alt = path is not None
    if not alt and not os.environ.get('DSWX_HIP_LIB'):
        _build.build()        # no-op unless the sources changed since the library was built (never a stale binary)
    path = path or library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f'{path} is missing: the DSWx HIP extension has not been built '
            '(run `python -m proteus_amd.build`); there is no CPU fallback')
    lib = ctypes.CDLL(path)
    vp, i64, cp = ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p
    pp = ctypes.POINTER(ctypes.c_void_p)
    sig = {
        'dswx_abi_version': (ctypes.c_int, []),
        'dswx_last_error': (cp, []),
        'dswx_device_count': (ctypes.c_int, []),
        'dswx_ctx_create': (ctypes.c_int, [ctypes.c_int, pp]),
        'dswx_ctx_destroy': (ctypes.c_int, [vp]),
        'dswx_params_default': (ctypes.c_int, [ctypes.POINTER(Params)]),
        'dswx_classify_host': (ctypes.c_int, [vp, ctypes.POINTER(Params), i64, i64, i64,
                                              ctypes.POINTER(PlanesIn),
                                              ctypes.POINTER(PlanesOut), vp]),
        'dswx_classify_device': (ctypes.c_int, [vp, ctypes.POINTER(Params), i64, i64,
                                                ctypes.POINTER(PlanesIn),
                                                ctypes.POINTER(PlanesOut), vp, vp]),
        'dswx_classify_device_2d': (ctypes.c_int, [vp, ctypes.POINTER(Params), i64, i64, i64,
                                                   ctypes.POINTER(PlanesIn),
                                                   ctypes.POINTER(PlanesOut), vp, vp]),
        'dswx_classify_batch': (ctypes.c_int, [vp, ctypes.POINTER(Params), ctypes.POINTER(BatchGeom),
                                               ctypes.POINTER(PlanesIn), ctypes.POINTER(PlanesOut),
                                               vp, vp]),
        'dswx_synth_batch': (ctypes.c_int, [vp, ctypes.c_uint64, i64, ctypes.POINTER(BatchGeom),
                                            ctypes.POINTER(PlanesIn), vp]),
        'dswx_interpret_layer_host': (ctypes.c_int, [vp, vp, i64, vp]),
        'dswx_shadow_layer_host': (ctypes.c_int, [vp, vp, i64, i64, i64,
                                                  ctypes.POINTER(ctypes.c_double * 3)] +
                                   [ctypes.c_double] * 6 + [vp]),
        'dswx_shadow_layer_device': (ctypes.c_int, [vp, vp, i64, i64, i64, i64,
                                                    ctypes.POINTER(ctypes.c_double * 3)] +
                                     [ctypes.c_double] * 6 + [vp, vp]),
        'dswx_shadow_thresholds': (ctypes.c_int, [ctypes.c_double, ctypes.c_double,
                                                  ctypes.POINTER(ctypes.c_double),
                                                  ctypes.POINTER(ctypes.c_double)]),
        'dswx_shadow_layer_host_q': (ctypes.c_int, [vp, vp, i64, i64, i64,
                                                    ctypes.POINTER(ctypes.c_double * 3)] +
                                     [ctypes.c_double] * 6 + [vp]),
        'dswx_shadow_layer_device_q': (ctypes.c_int, [vp, vp, i64, i64, i64, i64,
                                                      ctypes.POINTER(ctypes.c_double * 3)] +
                                       [ctypes.c_double] * 6 + [vp, vp]),
        'dswx_shadow_layer_host_q32': (ctypes.c_int, [vp, vp, i64, i64, i64,
                                                      ctypes.POINTER(ctypes.c_double * 3),
                                                      ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                                      ctypes.c_float, ctypes.c_double, ctypes.c_double, vp]),
        'dswx_shadow_layer_device_q32': (ctypes.c_int, [vp, vp, i64, i64, i64, i64,
                                                        ctypes.POINTER(ctypes.c_double * 3),
                                                        ctypes.c_double, ctypes.c_double, ctypes.c_float,
                                                        ctypes.c_float, ctypes.c_double, ctypes.c_double,
                                                        vp, vp]),
        'dswx_landcover_mask_host': (ctypes.c_int, [vp, vp, vp, i64, i64, vp, ctypes.c_int32, vp,
                                                    ctypes.c_int32, vp]),
        'dswx_landcover_mask_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, ctypes.c_int32,
                                                      vp, ctypes.c_int32, vp, vp]),
        'dswx_shadow_layer_batch': (ctypes.c_int, [vp, vp, i64, i64, i64, i64, ctypes.POINTER(ctypes.c_double * 3)] +
                                    [ctypes.c_double] * 4 + [ctypes.c_int32, ctypes.c_double, ctypes.c_double, vp, i64, vp]),
        'dswx_landcover_mask_batch': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, ctypes.c_int32, vp,
                                                     ctypes.c_int32, vp, i64, vp]),
        'dswx_synth_fill': (ctypes.c_int, [vp, ctypes.c_uint64, i64, i64, i64, i64,
                                           ctypes.POINTER(PlanesIn), vp]),
        'dswx_device_malloc': (ctypes.c_int, [vp, ctypes.c_size_t, pp]),
        'dswx_device_free': (ctypes.c_int, [vp, vp]),
        'dswx_host_alloc': (ctypes.c_int, [vp, ctypes.c_size_t, pp]),
        'dswx_host_free': (ctypes.c_int, [vp, vp]),
        'dswx_memcpy_h2d': (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t]),
        'dswx_memcpy_d2h': (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t]),
        'dswx_memset_d': (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_size_t]),
        'dswx_stream_synchronize': (ctypes.c_int, [vp, vp]),
        'dswx_event_create': (ctypes.c_int, [vp, pp]),
        'dswx_event_destroy': (ctypes.c_int, [vp, vp]),
        'dswx_event_record': (ctypes.c_int, [vp, vp, vp]),
        'dswx_event_elapsed_ms': (ctypes.c_int, [vp, vp, vp,
                                                 ctypes.POINTER(ctypes.c_float)]),
        'dswx_last_kernel_info': (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.c_size_t]),
        'dswx_batch_layout': (ctypes.c_int, [ctypes.POINTER(BatchGeom), ctypes.c_uint32,
                                             ctypes.POINTER(BatchLayout)]),
        'dswx_batch_create': (ctypes.c_int, [vp, ctypes.POINTER(BatchGeom), ctypes.c_uint32, pp]),
        'dswx_batch_destroy': (ctypes.c_int, [vp]),
        'dswx_batch_planes': (ctypes.c_int, [vp, ctypes.POINTER(BatchGeom), ctypes.POINTER(PlanesIn),
                                             ctypes.POINTER(PlanesOut), pp]),
        'dswx_batch_info': (ctypes.c_int, [vp, ctypes.POINTER(BatchInfo)]),
        'dswx_batch_classify': (ctypes.c_int, [vp, ctypes.POINTER(Params), i64, vp]),
        'dswx_batch_synth': (ctypes.c_int, [vp, ctypes.c_uint64, i64, vp]),
        'dswx_batch_place_search': (ctypes.c_int, [vp, ctypes.POINTER(Params), ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_uint64]),
        'dswx_batch_place_slide': (ctypes.c_int, [vp, ctypes.POINTER(Params), ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64]),
        'dswx_batch_va_budget': (ctypes.c_int, [ctypes.c_uint64] + [ctypes.POINTER(ctypes.c_uint64)] * 5),
        'dswx_batch_pool_trim': (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64)]),
        'dswx_cog_layout': (ctypes.c_int, [i64, i64, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.c_int32, ctypes.POINTER(CogLayout)]),
        'dswx_cog_blocks_device': (ctypes.c_int, [vp, vp, ctypes.c_int32, i64, i64, ctypes.c_int32,
                                                  ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, vp, vp]),
        'dswx_untile_device': (ctypes.c_int, [vp, vp, ctypes.c_int32, i64, i64, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int32, vp, vp]),
        'dswx_rgb_planes_device': (ctypes.c_int, [vp, vp, vp, vp, vp, i64, ctypes.POINTER(ctypes.c_double * 3),
                                                  ctypes.POINTER(ctypes.c_double * 3), ctypes.c_int32, vp, vp]),
        'dswx_convolve_axis_device': (ctypes.c_int, [vp, vp, ctypes.c_int32, i64, i64, i64, i64, i64, ctypes.c_int32, vp, vp, vp,
                                                     ctypes.c_int32, i64, i64, vp]),
        'dswx_to_byte_device': (ctypes.c_int, [vp, vp, ctypes.c_int32, i64, vp, vp]),
        'dswx_gather_2d_device': (ctypes.c_int, [vp, vp, ctypes.c_int32, i64, i64, vp, ctypes.c_int32, vp, ctypes.c_int32, vp, vp]),
        'dswx_copy_2d_device': (ctypes.c_int, [vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, vp]),
        'dswx_memcpy_h2d_async': (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t, vp]),
        'dswx_memcpy_d2h_async': (ctypes.c_int, [vp, vp, vp, ctypes.c_size_t, vp]),
        'dswx_checksum_device': (ctypes.c_int, [vp, vp, ctypes.c_int32, i64, i64, i64, vp, vp]),
        'dswx_batch_checksum': (ctypes.c_int, [vp, ctypes.c_uint32, i64, i64, vp, vp]),
        'dswx_checksum_host': (ctypes.c_int, [vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]),
        'dswx_compare_device': (ctypes.c_int, [vp, vp, vp, ctypes.c_int32, i64, i64, i64, i64, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_int32, vp, vp]),
        'dswx_batch_compare': (ctypes.c_int, [vp, vp, ctypes.c_uint32, i64, i64, ctypes.c_double, ctypes.c_double,
                                              ctypes.c_int32, vp, vp]),
        'dswx_compare_host': (ctypes.c_int, [vp, vp, ctypes.c_int32, i64, ctypes.c_double, ctypes.c_double, ctypes.c_int32, vp]),
        'dswx_histogram_device': (ctypes.c_int, [vp, vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i64, i64, i64, vp, vp]),
        'dswx_batch_histogram': (ctypes.c_int, [vp, ctypes.c_uint32, i64, i64, ctypes.c_int32, ctypes.c_int32, vp, vp]),
        'dswx_histogram_host': (ctypes.c_int, [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i64, vp]),
        'dswx_crosstab_device': (ctypes.c_int, [vp, vp, vp, vp, i64, i64, i64, i64, vp, vp]),
        'dswx_batch_crosstab': (ctypes.c_int, [vp, vp, vp, ctypes.c_int32, i64, i64, vp, vp]),
        'dswx_crosstab_host': (ctypes.c_int, [vp, vp, vp, i64, vp]),
        'dswx_stack_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, vp]),
        'dswx_batch_stack': (ctypes.c_int, [vp, ctypes.c_int32, vp, i64, i64, vp, vp]),
        'dswx_stack_host': (ctypes.c_int, [vp, vp, i64, i64, i64, vp]),
        'dswx_mosaic_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, i64, vp, i64, i64, vp, vp]),
        'dswx_batch_mosaic': (ctypes.c_int, [vp, ctypes.c_int32, vp, i64, i64, vp, i64, i64, vp, vp]),
        'dswx_mosaic_host': (ctypes.c_int, [vp, vp, i64, i64, i64, i64, vp, i64, i64, vp]),
        'dswx_warp_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, i64, i64, vp, vp]),
        'dswx_batch_warp': (ctypes.c_int, [vp, ctypes.c_int32, vp, i64, i64, vp, i64, i64, vp, vp]),
        'dswx_warp_host': (ctypes.c_int, [vp, vp, i64, i64, i64, vp, i64, i64, vp]),
        'dswx_resample_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, i64, i64, vp, vp]),
        'dswx_resample_host': (ctypes.c_int, [vp, vp, i64, i64, i64, vp, i64, i64, vp]),
        'dswx_land_mesh_device': (ctypes.c_int, [vp, vp, i64, i64, vp, i64, i64, vp, i64, i64, i64, vp, vp, vp, vp, vp]),
        'dswx_land_mesh_host': (ctypes.c_int, [vp, i64, i64, vp, i64, i64, vp, i64, i64, i64, vp, vp, vp, vp]),
        'dswx_grid_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, i64, vp, vp]),
        'dswx_batch_grid': (ctypes.c_int, [vp, ctypes.c_int32, vp, i64, i64, vp, vp]),
        'dswx_grid_host': (ctypes.c_int, [vp, vp, i64, i64, i64, i64, vp]),
        'dswx_label_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, i64, vp, vp]),
        'dswx_batch_label': (ctypes.c_int, [vp, ctypes.c_int32, vp, i64, i64, vp, vp]),
        'dswx_label_host': (ctypes.c_int, [vp, vp, i64, i64, i64, i64, vp]),
        'dswx_distance_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, i64, vp, vp]),
        'dswx_batch_distance': (ctypes.c_int, [vp, ctypes.c_int32, vp, i64, i64, vp, vp]),
        'dswx_distance_host': (ctypes.c_int, [vp, vp, i64, i64, i64, i64, vp]),
        'dswx_body_table_device': (ctypes.c_int, [vp, vp, vp, vp, i64, i64, i64, i64, vp, vp]),
        'dswx_batch_body_table': (ctypes.c_int, [vp, ctypes.c_int32, vp, i64, i64, vp, vp, vp]),
        'dswx_body_table_host': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, i64, vp]),
        'dswx_outline_work_bytes': (ctypes.c_int, [vp, i64, i64, i64, vp]),
        'dswx_outline_device': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, vp, ctypes.c_uint64, vp]),
        'dswx_outline_host': (ctypes.c_int, [vp, vp, i64, i64, i64, vp]),
        'dswx_burn_device': (ctypes.c_int, [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp]),
        'dswx_batch_burn': (ctypes.c_int, [vp, ctypes.c_int32, vp, vp, vp, vp, vp, i64, i64, vp]),
        'dswx_burn_host': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, vp]),
        'dswx_reach_device': (ctypes.c_int, [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp]),
        'dswx_batch_reach': (ctypes.c_int, [vp, ctypes.c_int32, vp, vp, vp, vp, vp, i64, i64, vp]),
        'dswx_reach_host': (ctypes.c_int, [vp, vp, vp, i64, i64, i64, vp, vp]),
    }
    for name, (res, args) in sig.items():
        if alt and not hasattr(lib, name):
            continue                      # an older build of the same ABI version
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.dswx_abi_version() != DSWX_ABI_VERSION and not (alt and lib.dswx_abi_version() == DSWX_ABI_VERSION - 1):
        # (an A/B partner may be the previous ABI: tools/ab_variants.py drives it through the classify entries only,
        # whose signatures have not changed)
        raise RuntimeError('libdswx_hip.so ABI version mismatch; rebuild it')
    if alt:
        _alt_libs[path] = lib
    else:
        _lib = lib
    return lib


_lab = None
# every symbol tools/lab/csrc/dswx_lab.h declares
LAB_SYMBOLS = ('dswx_lab_attach', 'dswx_lab_configure', 'dswx_stream_probe')


def load_lab():
    """dlopen libdswx_lab.so (experiments: kernel structures that lost, roofline probes, A/B switches).
    Only tools/ and the variant tests call this; nothing in the product path does."""
    global _lab
    if _lab is not None:
        return _lab
    load_library()
    path = _build.build_lab()
    lab = ctypes.CDLL(path)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    lab.dswx_lab_attach.restype = ctypes.c_int
    lab.dswx_lab_attach.argtypes = [vp]
    lab.dswx_lab_configure.restype = ctypes.c_int
    lab.dswx_lab_configure.argtypes = [vp, ctypes.c_char_p, ctypes.c_int]
    lab.dswx_stream_probe.restype = ctypes.c_int
    lab.dswx_stream_probe.argtypes = [vp, i64, i64, i64, ctypes.POINTER(PlanesIn), ctypes.POINTER(PlanesOut),
                                      ctypes.c_int, vp]
    _lab = lab
    return lab


def _check(rc):
    if rc != OK:
        raise DswxError(rc, load_library().dswx_last_error().decode('utf-8', 'replace'))


def device_count():
    return load_library().dswx_device_count()


def default_params():
    p = Params()
    _check(load_library().dswx_params_default(ctypes.byref(p)))
    return p


def make_params(thresholds=None, *, band_fills=None, fmask_fill=255.0,
                clip_negative_reflectance=True, mask_adjacent_to_cloud_mode='mask',
                apply_aerosol_class_remapping=True, aerosol_fmask_values=None,
                collapse_wtr_classes=True, aerosol_max_nir=None,
                exclude_psw_aggressive_in_browse=True, not_water_in_browse='white',
                cloud_in_browse='gray', snow_in_browse='cyan',
                set_ocean_masked_to_nodata=True, offset_and_scale=None):
    """Build a dswx_params_t.

    thresholds: object with the HlsThresholds attributes, or dict, or None
    (defaults).  aerosol_fmask_values: {class: [fmask values]} for the WTR-1
    classes 0, 2, 3, 4, or None (defaults).  offset_and_scale: six (scale_factor, add_offset) pairs =
    flag_offset_and_scale_inputs (dswx_hls.py:2300-2302): the chain on float32 reflectances.  Unknown modes raise the same
    Exception text as the reference (dswx_hls.py:1977-1981).
    """
    p = default_params()
    if thresholds is not None:
        for name in THRESHOLD_NAMES:
            v = thresholds[name] if isinstance(thresholds, dict) else \
                getattr(thresholds, name)
            if v is None:
                raise ValueError(f'HLS threshold {name} is not set')
            setattr(p, name, float(v))
    if band_fills is not None:
        for i, f in enumerate(band_fills):
            p.band_fill[i] = float('nan') if f is None else float(f)
    p.fmask_fill = float('nan') if fmask_fill is None else float(fmask_fill)
    if mask_adjacent_to_cloud_mode not in ADJ_MODES:
        raise Exception('ERROR mask adjacent to cloud/cloud-shadow mode:'
                        f' {mask_adjacent_to_cloud_mode}')
    p.mask_adjacent_to_cloud_mode = ADJ_MODES[mask_adjacent_to_cloud_mode]
    p.clip_negative_reflectance = int(bool(clip_negative_reflectance))
    p.apply_aerosol_class_remapping = int(bool(apply_aerosol_class_remapping))
    p.collapse_wtr_classes = int(bool(collapse_wtr_classes))
    if aerosol_max_nir is not None:
        p.aerosol_max_nir = float(aerosol_max_nir)
    # browse options as generate_dswx_layers maps them (dswx_hls.py:5309-5316)
    p.browse_exclude_psw_aggressive = int(bool(exclude_psw_aggressive_in_browse))
    p.browse_not_water_to_nodata = int(not_water_in_browse == 'nodata')
    p.browse_cloud_to_nodata = int(cloud_in_browse == 'nodata')
    p.browse_snow_to_nodata = int(snow_in_browse == 'nodata')
    p.browse_ocean_masked_to_nodata = int(bool(set_ocean_masked_to_nodata))
    if offset_and_scale is not None:
        if len(offset_and_scale) != 6:
            raise ValueError('offset_and_scale needs six (scale_factor, add_offset) pairs')
        p.offset_and_scale_inputs = 1
        for i, (sf, off) in enumerate(offset_and_scale):
            p.band_scale[i], p.band_offset[i] = float(sf), float(off)
    if aerosol_fmask_values is not None:
        for row, cls in enumerate((0, 2, 3, 4)):
            for v in range(256):
                p.aerosol_fmask_lut[row][v] = 0
            for v in aerosol_fmask_values[cls]:
                if 0 <= int(v) <= 255 and int(v) == v:
                    p.aerosol_fmask_lut[row][int(v)] = 1
    return p


def _bisect_floats(pred, lo, hi, dtype=np.float64):
    """pred(lo) is False and pred(hi) True (or the reverse) for a predicate that is monotonic in
    the float `x` of `dtype`; returns the two adjacent floats (a, b), a < b, where it flips.
    `pred` is evaluated on ARRAYS (64 copies of the candidate) so that numpy takes the same SIMD
    loop it takes for a raster."""
    dtype = np.dtype(dtype)
    itype, sign = (np.int64, 0x7fffffffffffffff) if dtype == np.float64 else (np.int32, 0x7fffffff)

    def ordered(d):
        i = int(dtype.type(d).view(itype))
        return i if i >= 0 else -(i & sign)

    def value(k):
        return float(itype(k if k >= 0 else (-k) | (-sign - 1)).view(dtype))

    def test(d):
        with np.errstate(all='ignore'):
            return bool(pred(np.full(64, d, dtype=dtype))[17])
    a, b = ordered(lo), ordered(hi)
    fa = test(lo)
    while b - a > 1:
        m = a + (b - a) // 2
        if test(value(m)) == fa:
            a = m
        else:
            b = m
    return value(a), value(b)


_shadow_threshold_cache = {}


def shadow_thresholds(min_slope_angle, max_sun_local_inc_angle, float32=False):
    """(slope_arg_max, inc_q_min) for dswx_shadow_layer_*_q: the reference's two tests
    `degrees(arctan(t)) <= min_slope_angle` and `degrees(arccos(q)) <= max_sun_local_inc_angle`
    (dswx_hls.py:4264-4281) as bounds on t and q, located with numpy's own array functions.
    float32=True: the same in float32 arithmetic (numpy < 2 value-based casting) for the _q32 forms."""
    key = (float(min_slope_angle), float(max_sun_local_inc_angle), bool(float32))
    if key in _shadow_threshold_cache:
        return _shadow_threshold_cache[key]
    if np.isnan(key[0]) or np.isnan(key[1]):
        raise ValueError('shadow angle threshold is NaN')
    dt = np.float32 if float32 else np.float64
    # a Python-float threshold is a weak scalar: the comparison runs in the array's dtype
    inc_ok = lambda q: np.degrees(np.arccos(q)) <= key[1]          # noqa: E731
    slope_ok = lambda t: np.degrees(np.arctan(t)) <= key[0]        # noqa: E731
    one = lambda f, v: bool(f(np.full(64, v, dtype=dt))[17])       # noqa: E731
    with np.errstate(all='ignore'):
        if not one(inc_ok, 1.0):
            inc_q_min = 2.0                      # never
        elif one(inc_ok, -1.0):
            inc_q_min = -1.0                     # whenever arccos is defined
        else:
            inc_q_min = _bisect_floats(inc_ok, -1.0, 1.0, dt)[1]
        if one(slope_ok, np.inf):
            slope_arg_max = float('inf')
        elif not one(slope_ok, -np.inf):
            slope_arg_max = float('-inf')
        else:
            slope_arg_max = _bisect_floats(slope_ok, -np.inf, np.inf, dt)[0]
    _shadow_threshold_cache[key] = (slope_arg_max, inc_q_min)
    return slope_arg_max, inc_q_min


def _host_ptr(arr):
    return ctypes.c_void_p(arr.ctypes.data)


def _stream_arg(stream):
    """The `stream` argument of an entry: the caller's hipStream_t, NULL (the context's own stream) for None or 0."""
    return ctypes.c_void_p(stream) if stream else None


def _wanted(want, known):
    """`want` as a tuple: not empty, every name one of `known` (the outputs of an entry in the order of its struct)."""
    want = tuple(want)
    for k in want:
        if k not in known:
            raise ValueError(f'unknown output {k!r} ({", ".join(known)})')
    if not want:
        raise ValueError('no output wanted')
    return want


def _host_plane(tiles, raster):
    """(tiles, n_tiles, H, W, tile_stride) of a host plane: uint8 [n_tiles, H, W] (stride 0 = packed), or with raster=(H, W) a
    padded plane [n_tiles, tile_stride]."""
    tiles = np.ascontiguousarray(tiles)
    if tiles.dtype != np.uint8 or tiles.ndim != (3 if raster is None else 2):
        raise ValueError(f'a plane is uint8 [n_tiles, H, W] or, with raster=, [n_tiles, tile_stride], not {tiles.dtype} {tiles.shape}')
    if raster is None:
        (n, H, W), stride = tiles.shape, 0
    else:
        (n, stride), (H, W) = tiles.shape, raster
    return tiles, n, H, W, stride


def _malloc_planes(ctx, planes):
    """{name: DeviceBuffer} for {name: (shape, dtype)}; an empty plane still has an address."""
    return {k: ctx.malloc(max(int(np.prod(shape, dtype=np.int64)), 1) * np.dtype(dt).itemsize) for k, (shape, dt) in planes.items()}


@contextlib.contextmanager
def _owned(res, errors=None):
    """The device buffers of `res` were allocated for the call made inside: the caller's when it succeeds, freed when it raises."""
    try:
        yield res
    except errors or DswxError:
        for buf in res.values():
            buf.free()
        raise


class DeviceBuffer:
    """A hipMalloc'ed span owned by a Context."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        ptr = ctypes.c_void_p()
        _check(ctx.lib.dswx_device_malloc(ctx.handle, self.nbytes, ctypes.byref(ptr)))
        self.ptr = ptr.value

    def free(self):
        if self.ptr:
            self.ctx.lib.dswx_device_free(self.ctx.handle, ctypes.c_void_p(self.ptr))
            self.ptr = None

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        _check(self.ctx.lib.dswx_memcpy_h2d(self.ctx.handle,
                                            ctypes.c_void_p(self.ptr + offset),
                                            _host_ptr(arr), arr.nbytes))

    def download(self, dtype, count, offset=0):
        out = np.empty(count, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes
        _check(self.ctx.lib.dswx_memcpy_d2h(self.ctx.handle, _host_ptr(out),
                                            ctypes.c_void_p(self.ptr + offset),
                                            out.nbytes))
        return out

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One per process and device (dswx_ctx_t)."""

    def __init__(self, device=0, lib_path=None):
        self.lib = load_library(lib_path)
        h = ctypes.c_void_p()
        _check(self.lib.dswx_ctx_create(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)
        self._pinned = {}          # page-locked host spans: address -> bytes
        self._pinned_pool = {}     # released spans by size
        self._pinned_pool_bytes = 0
        self._pinned_lock = threading.RLock()  # reader threads allocate; finalizers release on ANY thread, also (cyclic GC) on
                                               # one that is inside the lock already: re-entrant

    def close(self):
        if self.handle:
            with self._pinned_lock:
                # the pool's spans belong to no array any more: hand them back before the context goes.  Spans of
                # arrays that are still alive are freed by their finalizers (dswx_host_free takes a NULL context).
                for nbytes, spans in self._pinned_pool.items():
                    for addr in spans:
                        self._pinned.pop(addr, None)
                        self.lib.dswx_host_free(self.handle, ctypes.c_void_p(addr))
                self._pinned_pool = {}
                self._pinned_pool_bytes = 0
                handle, self.handle = self.handle, None
            self.lib.dswx_ctx_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- page-locked host arrays -----------------------------------------------
    PINNED_POOL_CAP = 4 << 30      # bytes of released page-locked spans kept for reuse

    def pinned_empty(self, shape, dtype):
        """numpy array over page-locked memory (dswx_host_alloc).  When every plane handed to
        classify_host() is such an array the library works on them in place (zero copy: the kernels
        read and write the host planes across PCIe); outputs are then allocated page-locked as well.  Page-locking is
        slow (~0.1 ms per MB), so released spans go to a per-context pool and are reused."""
        dtype = np.dtype(dtype)
        nbytes = max(int(np.prod(shape, dtype=np.int64)) * dtype.itemsize, 1)
        addr = None
        with self._pinned_lock:
            spans = self._pinned_pool.get(nbytes)
            if spans:
                addr = spans.pop()
                self._pinned_pool_bytes -= nbytes
        if addr is None:
            ptr = ctypes.c_void_p()
            _check(self.lib.dswx_host_alloc(self.handle, nbytes, ctypes.byref(ptr)))
            addr = ptr.value
            with self._pinned_lock:
                self._pinned[addr] = nbytes
        raw = (ctypes.c_char * nbytes).from_address(addr)
        arr = np.frombuffer(raw, dtype=dtype, count=nbytes // dtype.itemsize).reshape(shape) \
            if int(np.prod(shape, dtype=np.int64)) else np.empty(shape, dtype)

        def release(ctx_ref=weakref.ref(self), lib=self.lib, addr=addr, nbytes=nbytes):
            ctx = ctx_ref()
            if ctx is None:
                lib.dswx_host_free(None, ctypes.c_void_p(addr))      # the context is gone: the span still is ours to free
                return
            with ctx._pinned_lock:
                keep = bool(ctx.handle) and ctx._pinned_pool_bytes + nbytes <= ctx.PINNED_POOL_CAP
                if keep:
                    ctx._pinned_pool.setdefault(nbytes, []).append(addr)
                    ctx._pinned_pool_bytes += nbytes
                else:
                    ctx._pinned.pop(addr, None)
                    lib.dswx_host_free(ctx.handle, ctypes.c_void_p(addr))
        weakref.finalize(raw, release)
        return arr

    def is_pinned(self, arr):
        a = arr.ctypes.data
        with self._pinned_lock:
            spans = list(self._pinned.items())
        return any(base <= a and a + arr.nbytes <= base + size for base, size in spans)

    # ---- host-pointer path ----------------------------------------------------
    def classify_host(self, bands, fmask, params, *, land=None, shad=None, ocean=None,
                      layers=('diag', 'wtr1', 'wtr1_aerosol', 'wtr2', 'wtr', 'bwtr',
                              'conf', 'cloud'),
                      counters=True):
        """bands: six int16 arrays of identical shape [H,W] or [T,H,W].

        Returns {layer: ndarray} (+ 'counters': int64 [T,3]) with the input's shape.
        """
        bands = [np.ascontiguousarray(b, dtype=np.int16) for b in bands]
        if len(bands) != 6:
            raise ValueError('need six reflectance bands')
        shape = bands[0].shape
        if len(shape) == 2:
            n_tiles, (h, w) = 1, shape
        elif len(shape) == 3:
            n_tiles, h, w = shape
        else:
            raise ValueError('bands must be [H,W] or [T,H,W]')

        def prep(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.uint8)   # bool SHAD -> 0/1 u8
            if a.shape != shape:
                raise ValueError(f'{name} shape {a.shape} != bands shape {shape}')
            return a

        for b in bands:
            if b.shape != shape:
                raise ValueError('band shapes differ')
        fmask = prep(fmask, 'fmask')
        land, shad, ocean = prep(land, 'land'), prep(shad, 'shad'), prep(ocean, 'ocean')
        pin = PlanesIn()
        for i, b in enumerate(bands):
            pin.band[i] = b.ctypes.data
        pin.fmask = fmask.ctypes.data
        pin.land = land.ctypes.data if land is not None else None
        pin.shad = shad.ctypes.data if shad is not None else None
        pin.ocean = ocean.ctypes.data if ocean is not None else None
        pinned_in = all(self.is_pinned(a) for a in bands + [fmask, land, shad, ocean] if a is not None)
        pout = PlanesOut()
        res = {}
        for name in layers:
            dt = np.uint16 if name == 'diag' else (np.float64 if name in F64_LAYERS
                                                   else np.uint8)
            if name != 'diag' and name not in U8_LAYERS and name not in F64_LAYERS:
                raise KeyError(name)
            res[name] = self.pinned_empty(shape, dt) if pinned_in else np.empty(shape, dtype=dt)
            setattr(pout, name, res[name].ctypes.data)
        cnt = np.zeros((n_tiles, 3), dtype=np.int64) if counters else None
        _check(self.lib.dswx_classify_host(
            self.handle, ctypes.byref(params), n_tiles, h, w, ctypes.byref(pin),
            ctypes.byref(pout), _host_ptr(cnt) if counters else None))
        if counters:
            res['counters'] = cnt
        return res

    # ---- device-pointer path --------------------------------------------------
    def classify_device(self, params, n_tiles, n_pixels, pin, pout, counters_ptr=None,
                        stream=None):
        _check(self.lib.dswx_classify_device(
            self.handle, ctypes.byref(params), int(n_tiles), int(n_pixels),
            ctypes.byref(pin), ctypes.byref(pout),
            ctypes.c_void_p(counters_ptr) if counters_ptr else None,
            _stream_arg(stream)))

    def interpret_layer(self, diag_decimal):
        """generate_interpreted_layer on the device; any integer array in, uint8 out."""
        d = np.ascontiguousarray(diag_decimal, dtype=np.int64)
        out = np.empty(d.shape, dtype=np.uint8)
        _check(self.lib.dswx_interpret_layer_host(self.handle, _host_ptr(d), d.size,
                                                  _host_ptr(out)))
        return out

    def shadow_layer(self, dem, sun_vector, sin_azimuth, cos_azimuth, min_slope_angle,
                     max_sun_local_inc_angle, pixel_spacing_x=30, pixel_spacing_y=30, margin=0,
                     float32=False):
        """Terrain shadow layer of one float32 DEM [H,W]; returns bool [H-2m, W-2m].  The two angle
        thresholds are pulled back through numpy's arccos / arctan (shadow_thresholds).
        float32=True reproduces numpy < 2 value-based casting (all-float32 arithmetic)."""
        dem = np.ascontiguousarray(dem, dtype=np.float32)
        if dem.ndim != 2:
            raise ValueError('dem must be 2-D')
        h, w = dem.shape
        out = np.empty((max(h - 2 * margin, 0), max(w - 2 * margin, 0)), dtype=np.uint8)
        vec = (ctypes.c_double * 3)(*[float(v) for v in sun_vector])
        slope_arg_max, inc_q_min = shadow_thresholds(min_slope_angle, max_sun_local_inc_angle, float32)
        fn = self.lib.dswx_shadow_layer_host_q32 if float32 else self.lib.dswx_shadow_layer_host_q
        _check(fn(self.handle, _host_ptr(dem), h, w, int(margin), ctypes.byref(vec),
                  float(sin_azimuth), float(cos_azimuth), slope_arg_max, inc_q_min,
                  float(pixel_spacing_x), float(pixel_spacing_y), _host_ptr(out)))
        return out.astype(bool)

    def landcover_mask(self, worldcover_up3, copernicus, forest_classes, thresholds=(6, 3, 7, 3),
                       year_offset=0):
        """LAND layer from the warped WorldCover (3x grid) and CGLS (HLS grid) maps."""
        wc = np.ascontiguousarray(worldcover_up3, dtype=np.uint8)
        cg = np.ascontiguousarray(copernicus, dtype=np.uint8)
        h, w = cg.shape
        if wc.shape != (3 * h, 3 * w):
            raise ValueError(f'worldcover_up3 shape {wc.shape} != {(3 * h, 3 * w)}')
        fc = np.ascontiguousarray(list(forest_classes or []), dtype=np.int32)
        thr = np.ascontiguousarray(thresholds, dtype=np.int32)
        out = np.empty((h, w), dtype=np.uint8)
        _check(self.lib.dswx_landcover_mask_host(
            self.handle, _host_ptr(wc), _host_ptr(cg), h, w,
            _host_ptr(fc) if fc.size else None, int(fc.size), _host_ptr(thr), int(year_offset),
            _host_ptr(out)))
        return out

    def landcover_mask_device(self, wc_ptr, cg_ptr, n_tiles, height, width, forest_classes, out_ptr,
                              thresholds=(6, 3, 7, 3), year_offset=0, stream=None, out_tile_stride=0):
        """Device-pointer form: [n_tiles][3H][3W] + [n_tiles][H][W] -> [n_tiles][H][W], asynchronous.
        out_tile_stride: pixels between the LAND rasters of consecutive tiles (dswx_landcover_mask_batch: the LAND plane
        of a resident batch); 0 = packed."""
        fc = np.ascontiguousarray(list(forest_classes or []), dtype=np.int32)
        thr = np.ascontiguousarray(thresholds, dtype=np.int32)
        _check(self.lib.dswx_landcover_mask_batch(
            self.handle, ctypes.c_void_p(wc_ptr), ctypes.c_void_p(cg_ptr), int(n_tiles), int(height),
            int(width), _host_ptr(fc) if fc.size else None, int(fc.size), _host_ptr(thr),
            int(year_offset), ctypes.c_void_p(out_ptr), int(out_tile_stride), _stream_arg(stream)))

    def shadow_layer_device(self, dem_ptr, n_tiles, height, width, margin, sun_vector, sin_azimuth,
                            cos_azimuth, min_slope_angle, max_sun_local_inc_angle, out_ptr,
                            pixel_spacing_x=30, pixel_spacing_y=30, stream=None, float32=False, out_tile_stride=0):
        """Device-pointer form: [n_tiles][H][W] float32 DEMs -> [n_tiles][H-2m][W-2m] u8, asynchronous.
        float32=True: numpy < 2 value-based casting (the _q32 entry point).  out_tile_stride != 0: the shadow rasters
        go that many pixels apart (dswx_shadow_layer_batch: the SHAD plane of a resident batch)."""
        vec = (ctypes.c_double * 3)(*[float(v) for v in sun_vector])
        slope_arg_max, inc_q_min = shadow_thresholds(min_slope_angle, max_sun_local_inc_angle, float32)
        if out_tile_stride:
            _check(self.lib.dswx_shadow_layer_batch(
                self.handle, ctypes.c_void_p(dem_ptr), int(n_tiles), int(height), int(width), int(margin), ctypes.byref(vec),
                float(sin_azimuth), float(cos_azimuth), float(slope_arg_max), float(inc_q_min), int(bool(float32)),
                float(pixel_spacing_x), float(pixel_spacing_y), ctypes.c_void_p(out_ptr), int(out_tile_stride),
                _stream_arg(stream)))
            return
        fn = self.lib.dswx_shadow_layer_device_q32 if float32 else self.lib.dswx_shadow_layer_device_q
        _check(fn(
            self.handle, ctypes.c_void_p(dem_ptr), int(n_tiles), int(height), int(width), int(margin),
            ctypes.byref(vec), float(sin_azimuth), float(cos_azimuth), slope_arg_max, inc_q_min,
            float(pixel_spacing_x), float(pixel_spacing_y),
            ctypes.c_void_p(out_ptr), _stream_arg(stream)))

    # ---- libdswx_lab.so (experiments; tools/ and the variant tests only) -----------
    def lab_configure(self, **settings):
        """A/B switches of this context, e.g. lab_configure(fused_variant=3) or (host_chunks=3);
        loads libdswx_lab.so and attaches its kernel structures on first use."""
        lab = load_lab()
        if not getattr(self, '_lab_attached', False):
            _check(lab.dswx_lab_attach(self.handle))
            self._lab_attached = True
        for key, value in settings.items():
            _check(lab.dswx_lab_configure(self.handle, key.encode(), int(value)))

    def stream_probe(self, n_tiles, n_pixels, pin, pout, variant=0, stream=None, tile_stride=0):
        _check(load_lab().dswx_stream_probe(
            self.handle, int(n_tiles), int(n_pixels), int(tile_stride), ctypes.byref(pin),
            ctypes.byref(pout), int(variant), _stream_arg(stream)))

    def classify_batch(self, params, geom, pin, pout, counters_ptr=None, stream=None):
        _check(self.lib.dswx_classify_batch(
            self.handle, ctypes.byref(params), ctypes.byref(geom), ctypes.byref(pin),
            ctypes.byref(pout), ctypes.c_void_p(counters_ptr) if counters_ptr else None,
            _stream_arg(stream)))

    def synth_batch(self, seed, tile0, geom, pin, stream=None):
        _check(self.lib.dswx_synth_batch(
            self.handle, int(seed), int(tile0), ctypes.byref(geom), ctypes.byref(pin),
            _stream_arg(stream)))

    def classify_device_2d(self, params, n_tiles, height, width, pin, pout, counters_ptr=None,
                           stream=None):
        _check(self.lib.dswx_classify_device_2d(
            self.handle, ctypes.byref(params), int(n_tiles), int(height), int(width),
            ctypes.byref(pin), ctypes.byref(pout),
            ctypes.c_void_p(counters_ptr) if counters_ptr else None,
            _stream_arg(stream)))

    def synth_fill(self, seed, tile0, n_tiles, height, width, pin, stream=None):
        _check(self.lib.dswx_synth_fill(
            self.handle, int(seed), int(tile0), int(n_tiles), int(height), int(width),
            ctypes.byref(pin), _stream_arg(stream)))

    def malloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    # ---- the raster formats either side of the path (ABI v6; device pointers) ---------------
    def cog_blocks_device(self, plane_ptr, elem_bytes, height, width, blocks_ptr, factors=(), tile=512, predictor=2,
                          stream=None):
        f = (ctypes.c_int32 * max(len(factors), 1))(*[int(x) for x in factors])
        _check(self.lib.dswx_cog_blocks_device(self.handle, ctypes.c_void_p(plane_ptr), int(elem_bytes), int(height), int(width),
                                               int(tile), f, len(factors), int(predictor), ctypes.c_void_p(blocks_ptr),
                                               _stream_arg(stream)))

    def untile_device(self, blocks_ptr, elem_bytes, height, width, block_width, block_height, predictor, plane_ptr, stream=None):
        _check(self.lib.dswx_untile_device(self.handle, ctypes.c_void_p(blocks_ptr), int(elem_bytes), int(height), int(width),
                                           int(block_width), int(block_height), int(predictor), ctypes.c_void_p(plane_ptr),
                                           _stream_arg(stream)))

    def rgb_planes_device(self, red_ptr, green_ptr, blue_ptr, diag_ptr, n_pixels, scale, offset, clip, out_ptr, stream=None):
        sc = (ctypes.c_double * 3)(*[float(v) for v in scale])
        of = (ctypes.c_double * 3)(*[float(v) for v in offset])
        _check(self.lib.dswx_rgb_planes_device(self.handle, ctypes.c_void_p(red_ptr), ctypes.c_void_p(green_ptr),
                                               ctypes.c_void_p(blue_ptr), ctypes.c_void_p(diag_ptr) if diag_ptr else None,
                                               int(n_pixels), ctypes.byref(sc), ctypes.byref(of), int(bool(clip)),
                                               ctypes.c_void_p(out_ptr), _stream_arg(stream)))

    def convolve_axis_device(self, src_ptr, src_is_f64, n_lines, n_in, src_line_stride, src_elem_stride, n_out, taps, first_ptr,
                             weights_ptr, dst_ptr, dst_is_f64, dst_line_stride, dst_elem_stride, stream=None):
        _check(self.lib.dswx_convolve_axis_device(
            self.handle, ctypes.c_void_p(src_ptr), int(bool(src_is_f64)), int(n_lines), int(n_in), int(src_line_stride),
            int(src_elem_stride), int(n_out), int(taps), ctypes.c_void_p(first_ptr), ctypes.c_void_p(weights_ptr),
            ctypes.c_void_p(dst_ptr), int(bool(dst_is_f64)), int(dst_line_stride), int(dst_elem_stride),
            _stream_arg(stream)))

    def to_byte_device(self, src_ptr, src_dtype, n, dst_ptr, stream=None):
        kind = {'uint16': 1, 'int16': 2, 'float32': 3}.get(np.dtype(src_dtype).name)
        if kind is None:
            raise ValueError(f'to_byte_device: {np.dtype(src_dtype)} planes are not taken')
        _check(self.lib.dswx_to_byte_device(self.handle, ctypes.c_void_p(src_ptr), kind, int(n), ctypes.c_void_p(dst_ptr),
                                            _stream_arg(stream)))

    def gather_2d_device(self, src_ptr, elem_bytes, src_height, src_width, rows_ptr, n_rows, cols_ptr, n_cols, dst_ptr, stream=None):
        _check(self.lib.dswx_gather_2d_device(self.handle, ctypes.c_void_p(src_ptr), int(elem_bytes), int(src_height), int(src_width),
                                              ctypes.c_void_p(rows_ptr), int(n_rows), ctypes.c_void_p(cols_ptr), int(n_cols),
                                              ctypes.c_void_p(dst_ptr), _stream_arg(stream)))

    def copy_2d_device(self, dst_ptr, dst_pitch, src_ptr, src_pitch, width_bytes, height, stream=None):
        _check(self.lib.dswx_copy_2d_device(self.handle, ctypes.c_void_p(dst_ptr), int(dst_pitch), ctypes.c_void_p(src_ptr),
                                            int(src_pitch), int(width_bytes), int(height),
                                            _stream_arg(stream)))

    def checksum_device(self, plane_ptr, elem_bytes, n_tiles, n_elems, out_ptr, tile_stride=0, stream=None):
        """dswx_checksum_device: the per-tile checksums (include/dswx_hip.h "checksums"; proteus_amd/checksum.py states the
        definition in numpy) of one device plane [n_tiles][tile_stride] -> device uint64 [n_tiles] at out_ptr; asynchronous."""
        _check(self.lib.dswx_checksum_device(self.handle, ctypes.c_void_p(plane_ptr), int(elem_bytes), int(n_tiles), int(n_elems),
                                             int(tile_stride), ctypes.c_void_p(out_ptr),
                                             _stream_arg(stream)))

    def compare_device(self, a_ptr, b_ptr, kind, n_tiles, n_elems, out_ptr, a_stride=0, b_stride=0, atol=0.0, rtol=0.0,
                       equal_nan=True, stream=None):
        """dswx_compare_device: two device planes [n_tiles][stride] of one kind (CMP_*; include/dswx_hip.h "compare",
        proteus_amd/compare.py states the definition in numpy) -> device records [n_tiles] (compare.RECORD) at out_ptr;
        asynchronous."""
        _check(self.lib.dswx_compare_device(self.handle, ctypes.c_void_p(a_ptr), ctypes.c_void_p(b_ptr), int(kind), int(n_tiles),
                                            int(n_elems), int(a_stride), int(b_stride), float(atol), float(rtol),
                                            int(bool(equal_nan)), ctypes.c_void_p(out_ptr),
                                            _stream_arg(stream)))

    def histogram_device(self, plane_ptr, kind, n_tiles, n_elems, out_ptr, lo=0, shift=0, tile_stride=0, stream=None):
        """dswx_histogram_device: one device plane [n_tiles][tile_stride] of one kind (HIST_*; include/dswx_hip.h "histogram",
        proteus_amd/histogram.py states the definition in numpy) -> device uint64 [n_tiles][256] at out_ptr; asynchronous."""
        _check(self.lib.dswx_histogram_device(self.handle, ctypes.c_void_p(plane_ptr), int(kind), int(lo), int(shift), int(n_tiles),
                                              int(n_elems), int(tile_stride), ctypes.c_void_p(out_ptr),
                                              _stream_arg(stream)))

    def crosstab_device(self, a_ptr, b_ptr, spec, n_tiles, n_elems, out_ptr, a_stride=0, b_stride=0, stream=None):
        """dswx_crosstab_device: device planes a [n_tiles][a_stride] (of spec.a_kind) and b [n_tiles][b_stride] (uint8)
        cross-tabulated by `spec` (a crosstab.Spec; include/dswx_hip.h "crosstab", proteus_amd/crosstab.py states the
        definition in numpy) -> device uint64 [n_tiles][256] at out_ptr; asynchronous."""
        _check(self.lib.dswx_crosstab_device(self.handle, ctypes.c_void_p(a_ptr), ctypes.c_void_p(b_ptr),
                                             ctypes.byref(CrosstabSpec.of(spec)), int(n_tiles), int(n_elems), int(a_stride),
                                             int(b_stride), ctypes.c_void_p(out_ptr), _stream_arg(stream)))

    def stack_device(self, stack_ptr, spec, n_tiles, n_elems, out, tile_stride=0, stream=None):
        """dswx_stack_device: one device stack uint8 [n_tiles][tile_stride] composited per pixel by `spec` (a stack.Spec;
        include/dswx_hip.h "stack", proteus_amd/stack.py states the definition in numpy) -> the planes `out` names (a StackOut
        of device addresses, n_elems elements each); one launch, asynchronous."""
        _check(self.lib.dswx_stack_device(self.handle, ctypes.c_void_p(stack_ptr), ctypes.byref(StackSpec.of(spec)), int(n_tiles),
                                          int(n_elems), int(tile_stride), ctypes.byref(out),
                                          _stream_arg(stream)))

    def mosaic_device(self, plane_ptr, spec, n_tiles, height, width, place_ptr, canvas_h, canvas_w, out, tile_stride=0, stream=None):
        """dswx_mosaic_device: one device plane uint8 [n_tiles][tile_stride], every tile a height x width raster, placed on a
        canvas_h x canvas_w canvas by the device table int32 [n_tiles][2] at place_ptr and composited per canvas pixel by `spec`
        (a mosaic.Spec; include/dswx_hip.h "mosaic", proteus_amd/mosaic.py states the definition in numpy) -> the planes `out`
        names (a StackOut of device addresses, canvas_h * canvas_w elements each); one launch, asynchronous."""
        _check(self.lib.dswx_mosaic_device(self.handle, ctypes.c_void_p(plane_ptr), ctypes.byref(MosaicSpec.of(spec)), int(n_tiles),
                                           int(height), int(width), int(tile_stride), ctypes.c_void_p(place_ptr), int(canvas_h),
                                           int(canvas_w), ctypes.byref(out), _stream_arg(stream)))

    def warp_device(self, plane_ptr, spec, n_tiles, height, width, mesh_ptr, dst_h, dst_w, out, stream=None):
        """dswx_warp_device: one device plane [n_tiles][spec.src_tile_stride] of elements of spec.elem_bytes, every tile a height
        x width raster, resampled (nearest pixel) onto dst_h x dst_w through the device mesh int32 [mesh_h][mesh_w][2] at
        mesh_ptr (a warp.Spec; include/dswx_hip.h "warp", proteus_amd/warp.py states the definition in numpy) -> the outputs
        `out` names (a WarpOut of device addresses); one memset of the head and one launch, asynchronous."""
        _check(self.lib.dswx_warp_device(self.handle, ctypes.c_void_p(plane_ptr), ctypes.byref(WarpSpec.of(spec)), int(n_tiles),
                                         int(height), int(width), ctypes.c_void_p(mesh_ptr), int(dst_h), int(dst_w),
                                         ctypes.byref(out), _stream_arg(stream)))

    def resample_device(self, plane_ptr, spec, n_tiles, height, width, mesh_ptr, dst_h, dst_w, out, stream=None):
        """dswx_resample_device: one device plane float32 or int16 [n_tiles][spec.src_tile_stride], every tile a height x width
        raster, interpolated (bilinear or cubic) onto dst_h x dst_w through the device mesh int32 [mesh_h][mesh_w][2] at mesh_ptr
        (a resample.Spec; include/dswx_hip.h "resample", proteus_amd/resample.py states the definition in numpy) -> the outputs
        `out` names (a ResampleOut of device addresses); one memset of the head and one launch, asynchronous."""
        _check(self.lib.dswx_resample_device(self.handle, ctypes.c_void_p(plane_ptr), ctypes.byref(ResampleSpec.of(spec)), int(n_tiles),
                                             int(height), int(width), ctypes.c_void_p(mesh_ptr), int(dst_h), int(dst_w),
                                             ctypes.byref(out), _stream_arg(stream)))

    def land_mesh_device(self, wc_ptr, wc_shape, cg_ptr, cg_shape, spec, n_tiles, height, width, mesh_wc_ptr, mesh_cg_ptr,
                         land_ptr=None, head_ptr=None, stream=None):
        """dswx_land_mesh_device: the LAND layer of n_tiles tiles of height x width HLS pixels from the device planes uint8
        [n_tiles][wc_shape] (WorldCover) and [n_tiles][cg_shape] (CGLS) read through the device meshes at mesh_wc_ptr (of the
        lattice 3 height x 3 width) and mesh_cg_ptr by `spec` (a landmesh.Spec; include/dswx_hip.h "land mesh",
        proteus_amd/landmesh.py states the definition in numpy) -> land uint8 [n_tiles][spec.land_tile_stride or height *
        width] and head uint64 [n_tiles][8], each wanted iff its address is given; one memset of the head and ONE launch,
        asynchronous."""
        _check(self.lib.dswx_land_mesh_device(self.handle, ctypes.c_void_p(wc_ptr), int(wc_shape[0]), int(wc_shape[1]),
                                              ctypes.c_void_p(cg_ptr), int(cg_shape[0]), int(cg_shape[1]),
                                              ctypes.byref(LandMeshSpec.of(spec)), int(n_tiles), int(height), int(width),
                                              ctypes.c_void_p(mesh_wc_ptr), ctypes.c_void_p(mesh_cg_ptr),
                                              ctypes.c_void_p(land_ptr or None), ctypes.c_void_p(head_ptr or None), _stream_arg(stream)))

    def land_mesh(self, worldcover, copernicus, mesh_wc, mesh_cg, shape, spec):
        """Host arrays in, host arrays out: the uint8 source windows [wc_h, wc_w] and [cg_h, cg_w] of ONE tile and their int32
        meshes uploaded, dswx_land_mesh_device, (land uint8 [H, W], head uint64 [8]) downloaded; complete on return."""
        H, W = (int(v) for v in shape)
        arrays = [np.ascontiguousarray(worldcover, dtype=np.uint8), np.ascontiguousarray(copernicus, dtype=np.uint8),
                  np.ascontiguousarray(mesh_wc, dtype=np.int32), np.ascontiguousarray(mesh_cg, dtype=np.int32)]
        bufs = []
        try:
            for a in arrays:
                bufs.append(self.malloc(max(a.nbytes, 8)))
                if a.nbytes:
                    bufs[-1].upload(a)
            out = self.malloc(max(H * W, 1) + 8 * LAND_MESH_HEAD_WORDS + 8)
            bufs.append(out)
            head_at = -(-max(H * W, 1) // 8) * 8
            self.land_mesh_device(bufs[0].ptr, arrays[0].shape, bufs[1].ptr, arrays[1].shape, spec, 1, H, W, bufs[2].ptr, bufs[3].ptr,
                                  out.ptr, out.ptr + head_at)
            self.synchronize()
            return out.download(np.uint8, H * W).reshape(H, W), out.download(np.uint64, LAND_MESH_HEAD_WORDS, offset=head_at)
        finally:
            for b in bufs:
                b.free()

    def grid_device(self, plane_ptr, spec, n_tiles, height, width, out, tile_stride=0, stream=None):
        """dswx_grid_device: one device plane uint8 [n_tiles][tile_stride], every tile a height x width raster, aggregated
        onto cells by `spec` (a grid.Spec; include/dswx_hip.h "grid", proteus_amd/grid.py states the definition in numpy) ->
        the planes `out` names (a GridOut of device addresses, n_tiles x GH x GW elements each); one launch, asynchronous."""
        _check(self.lib.dswx_grid_device(self.handle, ctypes.c_void_p(plane_ptr), ctypes.byref(GridSpec.of(spec)), int(n_tiles),
                                         int(height), int(width), int(tile_stride), ctypes.byref(out),
                                         _stream_arg(stream)))

    def label_device(self, plane_ptr, spec, n_tiles, height, width, out, tile_stride=0, stream=None):
        """dswx_label_device: the connected bodies of one device plane uint8 [n_tiles][tile_stride], every tile a height x
        width raster, by `spec` (a label.Spec; include/dswx_hip.h "label", proteus_amd/label.py states the definition in
        numpy) -> the planes `out` names (a LabelOut of device addresses); a fixed number of launches, asynchronous."""
        _check(self.lib.dswx_label_device(self.handle, ctypes.c_void_p(plane_ptr), ctypes.byref(LabelSpec.of(spec)), int(n_tiles),
                                          int(height), int(width), int(tile_stride), ctypes.byref(out),
                                          _stream_arg(stream)))

    def distance_device(self, plane_ptr, spec, n_tiles, height, width, out, tile_stride=0, stream=None):
        """dswx_distance_device: the squared distance of every pixel of one device plane uint8 [n_tiles][tile_stride], every
        tile a height x width raster, to the nearest target by `spec` (a distance.Spec; include/dswx_hip.h "distance",
        proteus_amd/distance.py states the definition in numpy) -> the planes `out` names (a DistanceOut of device addresses);
        a fixed number of launches, asynchronous."""
        _check(self.lib.dswx_distance_device(self.handle, ctypes.c_void_p(plane_ptr), ctypes.byref(DistanceSpec.of(spec)), int(n_tiles),
                                             int(height), int(width), int(tile_stride), ctypes.byref(out),
                                             _stream_arg(stream)))

    def body_table_device(self, label_ptr, value_ptr, spec, n_tiles, height, width, out, value_stride=0, stream=None):
        """dswx_body_table_device: the bodies of one device label plane uint32 [n_tiles][height * width] renumbered and
        tabulated against the device plane uint8 [n_tiles][value_stride] at `value_ptr` (0 / None with spec.n_cats == 0) by
        `spec` (a bodies.Spec; include/dswx_hip.h "body table", proteus_amd/bodies.py states the definition in numpy) -> the
        outputs `out` names (a BodyOut of device addresses); four launches and two memsets, asynchronous."""
        _check(self.lib.dswx_body_table_device(self.handle, ctypes.c_void_p(label_ptr), ctypes.c_void_p(value_ptr) if value_ptr else None,
                                               ctypes.byref(BodySpec.of(spec)), int(n_tiles), int(height), int(width),
                                               int(value_stride), ctypes.byref(out), _stream_arg(stream)))

    def outline_device(self, ids_ptr, spec, n_tiles, height, width, out, work_ptr, work_bytes, stream=None):
        """dswx_outline_device: the regions of one device id plane uint32 [n_tiles][height * width] traced as rings by `spec`
        (an outline.Spec; include/dswx_hip.h "outline", proteus_amd/outline.py states the definition in numpy) -> the outputs
        `out` names (an OutlineOut of device addresses), with the caller's working memory of outline_work_bytes(...) bytes at
        `work_ptr`; 9 + ceil(log2 capacity) launches and two memsets, asynchronous."""
        _check(self.lib.dswx_outline_device(self.handle, ctypes.c_void_p(ids_ptr) if ids_ptr else None, ctypes.byref(OutlineSpec.of(spec)),
                                            int(n_tiles), int(height), int(width), ctypes.byref(out),
                                            ctypes.c_void_p(work_ptr) if work_ptr else None, int(work_bytes),
                                            _stream_arg(stream)))

    def outline(self, ids, spec, n_tiles, height, width, want=('chain', 'rings', 'head'), stream=None):
        """The regions of the device id plane uint32 [n_tiles][height * width] at `ids` (an address or a DeviceBuffer)
        traced as rings: allocates the wanted outputs and the working memory (dswx_device_malloc), queues
        dswx_outline_device on `stream` and waits for it, since the working memory is freed on return.  Returns {output:
        DeviceBuffer}: 'chain' uint32 [n_tiles][max_edges], 'rings' uint32 [n_tiles][max_rings][8] (only with
        spec.max_rings > 0), 'head' uint64 [n_tiles][8] -- device buffers owned by the caller."""
        res = _malloc_planes(self, {k: (_outline_shape(k, n_tiles, spec), OUTLINE_DTYPES[k]) for k in _outline_wanted(want, spec)})
        work = None
        try:
            with _owned(res):
                work_bytes = outline_work_bytes(spec, n_tiles, height, width)
                work = self.malloc(work_bytes)
                self.outline_device(getattr(ids, 'ptr', ids), spec, n_tiles, height, width, OutlineOut.of(**{k: b.ptr for k, b in res.items()}),
                                    work.ptr, work_bytes, stream)
                self.synchronize(stream)
        finally:
            if work is not None:
                work.free()
        return res

    def burn_device(self, verts_ptr, tile_first_ptr, spec, n_tiles, height, width, src_ptr, out, stream=None):
        """dswx_burn_device: the records at `verts_ptr` (device, 16 bytes each) shared out by the device table int64
        [n_tiles + 1] at `tile_first_ptr`, burnt by `spec` (a burn.Spec; include/dswx_hip.h "burn", proteus_amd/burn.py states the
        definition in numpy) -> the outputs `out` names (a BurnOut of device addresses), with the optional device plane at
        `src_ptr` (which may be out.mask); two memsets and two launches, asynchronous."""
        _check(self.lib.dswx_burn_device(self.handle, ctypes.c_void_p(verts_ptr) if verts_ptr else None,
                                         ctypes.c_void_p(tile_first_ptr) if tile_first_ptr else None, ctypes.byref(BurnSpec.of(spec)),
                                         int(n_tiles), int(height), int(width), ctypes.c_void_p(src_ptr) if src_ptr else None,
                                         ctypes.byref(out), _stream_arg(stream)))

    def reach_device(self, verts_ptr, tile_first_ptr, spec, n_tiles, height, width, src_ptr, out, stream=None):
        """dswx_reach_device: as burn_device, for the pixels whose centre lies within spec.radius of an edge of the records
        (`spec` a reach.Spec; include/dswx_hip.h "reach", proteus_amd/reach.py states the definition in numpy); `src_ptr` may be
        out.mask: the reach ORed onto a burnt mask.  Two memsets and two launches, asynchronous."""
        _check(self.lib.dswx_reach_device(self.handle, ctypes.c_void_p(verts_ptr) if verts_ptr else None,
                                          ctypes.c_void_p(tile_first_ptr) if tile_first_ptr else None, ctypes.byref(ReachSpec.of(spec)),
                                          int(n_tiles), int(height), int(width), ctypes.c_void_p(src_ptr) if src_ptr else None,
                                          ctypes.byref(out), _stream_arg(stream)))

    def burn(self, verts, tile_first, height, width, spec, src=None, want=('acc', 'mask', 'head'), stream=None):
        """Rings burnt onto new device planes: uploads the host records `verts` (burn.VERTEX_DTYPE) and the table `tile_first`
        (int64 [n_tiles + 1]), allocates the wanted outputs and 'acc' always, queues dswx_burn_device on `stream` and waits
        for it, since the uploaded records are freed on return.  `src` (None, or a host plane uint8 [n_tiles, H, W], or
        [n_tiles, spec.mask_tile_stride]) is uploaded INTO 'mask' and burnt in place.  Returns {output: DeviceBuffer}: 'acc'
        uint32 [n_tiles][H*W], 'mask' uint8 [n_tiles][mask_tile_stride or H*W], 'head' uint64 [n_tiles][8] -- device buffers
        owned by the caller."""
        verts, tile_first, n = _burn_input(verts, tile_first)
        want = _burn_wanted(want)
        if src is not None and 'mask' not in want:
            raise ValueError("src without 'mask'")
        if src is not None and spec.src_tile_stride != spec.mask_tile_stride:
            raise ValueError('src is burnt in place here: src_tile_stride must equal mask_tile_stride')
        res = _malloc_planes(self, {k: (_burn_shape(k, n, height, width, spec), BURN_DTYPES[k]) for k in want})
        dv, df = self.malloc(max(verts.nbytes, 16)), self.malloc(tile_first.nbytes)
        try:
            with _owned(res):
                if verts.nbytes:
                    dv.upload(verts)
                df.upload(tile_first)
                if src is not None:
                    src = np.ascontiguousarray(src, dtype=np.uint8)
                    if src.size != int(np.prod(_burn_shape('mask', n, height, width, spec), dtype=np.int64)):
                        raise DswxError(ERR_ARG, f'src has {src.size} bytes, mask {_burn_shape("mask", n, height, width, spec)}')
                    if src.nbytes:
                        res['mask'].upload(src)
                self.burn_device(dv.ptr, df.ptr, spec, n, height, width, res['mask'].ptr if src is not None else None,
                                 BurnOut.of(**{k: b.ptr for k, b in res.items()}), stream)
                self.synchronize(stream)
        finally:
            dv.free()
            df.free()
        return res

    def h2d_async(self, dst_ptr, host_arr, nbytes=None, stream=None):
        _check(self.lib.dswx_memcpy_h2d_async(self.handle, ctypes.c_void_p(dst_ptr), _host_ptr(host_arr),
                                              int(host_arr.nbytes if nbytes is None else nbytes),
                                              _stream_arg(stream)))

    def d2h_async(self, host_arr, src_ptr, nbytes=None, stream=None):
        _check(self.lib.dswx_memcpy_d2h_async(self.handle, _host_ptr(host_arr), ctypes.c_void_p(src_ptr),
                                              int(host_arr.nbytes if nbytes is None else nbytes),
                                              _stream_arg(stream)))

    def synchronize(self, stream=None):
        _check(self.lib.dswx_stream_synchronize(
            self.handle, _stream_arg(stream)))

    def event(self):
        e = ctypes.c_void_p()
        _check(self.lib.dswx_event_create(self.handle, ctypes.byref(e)))
        return e

    def record(self, event, stream=None):
        _check(self.lib.dswx_event_record(
            self.handle, event, _stream_arg(stream)))

    def elapsed_ms(self, start, stop):
        ms = ctypes.c_float()
        _check(self.lib.dswx_event_elapsed_ms(self.handle, start, stop, ctypes.byref(ms)))
        return ms.value

    def destroy_event(self, event):
        self.lib.dswx_event_destroy(self.handle, event)

    def last_kernel_info(self):
        buf = ctypes.create_string_buffer(256)
        _check(self.lib.dswx_last_kernel_info(self.handle, buf, 256))
        return buf.value.decode()


def checksum_host(data):
    """dswx_checksum_host (no device needed): the checksum of a host buffer (bytes-like, or an array taken in C order)
    by the library's scalar statement of the definition."""
    a = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    v = ctypes.c_uint64()
    _check(load_library().dswx_checksum_host(_host_ptr(a) if a.size else None, a.size, ctypes.byref(v)))
    return int(v.value)


def compare_host(a, b, atol=0.0, rtol=0.0, equal_nan=True):
    """dswx_compare_host (no device needed): the record (compare.RECORD scalar) of two host arrays of one kind and size,
    taken in C order, by the library's scalar statement of the definition."""
    from .compare import RECORD, kind_of
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.size != b.size:
        raise ValueError(f'{a.dtype} x {a.size} against {b.dtype} x {b.size}')
    rec = np.zeros(1, dtype=RECORD)
    _check(load_library().dswx_compare_host(_host_ptr(a) if a.size else None, _host_ptr(b) if b.size else None, kind_of(a.dtype),
                                            a.size, float(atol), float(rtol), int(bool(equal_nan)), _host_ptr(rec)))
    return rec[0]


def histogram_host(a, kind=None, lo=0, shift=0):
    """dswx_histogram_host (no device needed): the record (uint64 [256]) of a host array, taken in C order, by the library's
    scalar statement of the definition; the kind follows the dtype when None (name HIST_DIAG for a DIAG plane)."""
    from .histogram import check
    a = np.ascontiguousarray(a)
    kind, lo, shift = check(a.dtype, kind, lo, shift)
    out = np.zeros(HIST_BINS, dtype=np.uint64)
    _check(load_library().dswx_histogram_host(_host_ptr(a) if a.size else None, kind, lo, shift, a.size, _host_ptr(out)))
    return out


def crosstab_host(a, b, spec):
    """dswx_crosstab_host (no device needed): the record (uint64 [256]) of two host arrays of one shape, taken in C order, by
    the library's scalar statement of the definition; a of spec.a_kind's dtype, b uint8."""
    from .histogram import check
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    check(a.dtype, spec.a_kind, spec.a_lo, spec.a_shift)
    if b.dtype != np.uint8 or a.shape != b.shape:
        raise ValueError(f'plane b is uint8 of the shape of a: {b.dtype} {b.shape} against {a.shape}')
    out = np.zeros(CROSSTAB_CELLS, dtype=np.uint64)
    _check(load_library().dswx_crosstab_host(_host_ptr(a) if a.size else None, _host_ptr(b) if b.size else None,
                                             ctypes.byref(CrosstabSpec.of(spec)), a.size, _host_ptr(out)))
    return out


def stack_host(tiles, spec, want=('count', 'last', 'last_index', 'share')):
    """dswx_stack_host (no device needed): the planes of proteus_amd.stack.stack_tiles -- those named in `want` -- of a host
    stack uint8 [n_tiles, ...], by the library's scalar statement of the definition."""
    tiles = np.ascontiguousarray(tiles)
    if tiles.dtype != np.uint8 or tiles.ndim < 1:
        raise ValueError(f'a stack is uint8 [n_tiles, ...], not {tiles.dtype} {tiles.shape}')
    T, shape = tiles.shape[0], tiles.shape[1:]
    n = int(np.prod(shape, dtype=np.int64))
    res = _stack_planes(want, spec, shape, lambda shp, dt: np.zeros(shp, dtype=dt))
    out = StackOut.of(count=[c.ctypes.data for c in res['count']] if 'count' in res else (),
                      **{k: res[k].ctypes.data for k in ('last', 'last_index', 'share') if k in res})
    _check(load_library().dswx_stack_host(_host_ptr(tiles) if tiles.size else None, ctypes.byref(StackSpec.of(spec)), T, n, 0,
                                          ctypes.byref(out)))
    return res


def mosaic_host(tiles, place, canvas_shape, spec, want=('count', 'last', 'last_index', 'share'), raster=None):
    """dswx_mosaic_host (no device needed): the planes of proteus_amd.mosaic.mosaic_tiles -- those named in `want` -- of a
    host plane uint8 [n_tiles, H, W] placed by `place` (int32 [n_tiles, 2] = row0, col0) on a canvas of canvas_shape, by the
    library's scalar statement of the definition.  With raster=(H, W), `tiles` is a padded plane uint8 [n_tiles, tile_stride],
    tile_stride >= H * W, whose padding is not read."""
    tiles, n, H, W, stride = _host_plane(tiles, raster)
    place = np.ascontiguousarray(place, dtype=np.int32).reshape(n, 2)
    ch, cw = (int(v) for v in canvas_shape)
    res = _stack_planes(want, spec, (max(ch, 0), max(cw, 0)), lambda shp, dt: np.zeros(shp, dtype=dt))
    out = StackOut.of(count=[c.ctypes.data for c in res['count']] if 'count' in res else (),
                      **{k: res[k].ctypes.data for k in ('last', 'last_index', 'share') if k in res})
    _check(load_library().dswx_mosaic_host(_host_ptr(tiles) if tiles.size else None, ctypes.byref(MosaicSpec.of(spec)), n, H, W,
                                           stride, _host_ptr(place) if n else None, ch, cw, ctypes.byref(out)))
    return res


def _mesh_planes(want, elem_dtype, n, dst_shape, make, second, head_words):
    """{name: plane} for the outputs of a warp or a resample named in `want`, each made by make(shape, dtype): 'dst', the
    per-pixel plane `second` = (name, dtype) and 'head'."""
    dh, dw = (max(int(v), 0) for v in dst_shape)
    shapes = {'dst': ((n, dh, dw), elem_dtype), second[0]: ((n, dh, dw), second[1]), 'head': ((n, head_words), np.uint64)}
    want = _wanted(want, shapes)
    return {k: make(*shapes[k]) for k in shapes if k in want}


def _mesh_host(entry, planes, spec_type, out_type, tiles, elem_ok, elems, mesh, spec, dst_shape, want, raster):
    """The host entry `entry` of a warp or a resample on a host plane and a host mesh: the shape checks, the node count that
    the entry itself cannot check (it has an address, not an array), the outputs and the call."""
    tiles = np.ascontiguousarray(tiles)
    if not elem_ok(tiles.dtype) or tiles.ndim != (3 if raster is None else 2):
        raise ValueError(f'a plane is [n_tiles, H, W] or, with raster=, [n_tiles, tile_stride] of {elems}, not {tiles.dtype} {tiles.shape}')
    n = tiles.shape[0]
    H, W = tiles.shape[1:] if raster is None else raster
    mesh = np.ascontiguousarray(mesh, dtype=np.int32)
    dh, dw = (int(v) for v in dst_shape)
    if n > 0 and dh > 0 and dw > 0 and 0 <= spec.shift <= WARP_MAX_SHIFT:            # (else the entry reads no node)
        step = 1 << spec.shift
        nodes = (((dh + step - 1) >> spec.shift) + 1) * (((dw + step - 1) >> spec.shift) + 1)
        if mesh.size < 2 * ((n - 1) * spec.mesh_tile_stride_nodes + nodes):
            raise ValueError(f'a mesh for {dh} x {dw} at shift {spec.shift} has {nodes} nodes per tile, {mesh.shape} is too small')
    res = planes(want, tiles.dtype, n, (dh, dw), lambda shp, dt: np.zeros(shp, dtype=dt))
    out = out_type.of(**{k: a.ctypes.data for k, a in res.items()})
    _check(getattr(load_library(), entry)(_host_ptr(tiles) if tiles.size else None, ctypes.byref(spec_type.of(spec)), n, int(H), int(W),
                                          _host_ptr(mesh) if mesh.size else None, dh, dw, ctypes.byref(out)))
    return res


def _warp_planes(want, elem_dtype, n, dst_shape, make):
    """{name: plane} for the outputs of a warp named in `want`, each made by make(shape, dtype)."""
    return _mesh_planes(want, elem_dtype, n, dst_shape, make, ('src_index', np.uint32), WARP_HEAD_WORDS)


def warp_host(tiles, mesh, spec, dst_shape, want=('dst', 'src_index', 'head'), raster=None):
    """dswx_warp_host (no device needed): the outputs of proteus_amd.warp.warp_tiles named in `want` -- 'dst' [n, dst_h, dst_w]
    of the plane's dtype, 'src_index' uint32 [n, dst_h, dst_w], 'head' uint64 [n, 8] -- of a host plane [n_tiles, H, W] of 1, 2
    or 4 bytes per element warped through the int32 mesh `mesh` ([mesh_h, mesh_w, 2], or per tile at
    spec.mesh_tile_stride_nodes) by `spec` (a warp.Spec), by the library's scalar statement of the definition.  With
    raster=(H, W), `tiles` is a padded plane [n_tiles, spec.src_tile_stride] whose padding is not read."""
    return _mesh_host('dswx_warp_host', _warp_planes, WarpSpec, WarpOut, tiles, lambda dt: dt.itemsize == spec.elem_bytes,
                      f'{spec.elem_bytes}-byte elements', mesh, spec, dst_shape, want, raster)


def _resample_planes(want, elem_dtype, n, dst_shape, make):
    """{name: plane} for the outputs of a resample named in `want`, each made by make(shape, dtype)."""
    return _mesh_planes(want, elem_dtype, n, dst_shape, make, ('how', np.uint8), RESAMPLE_HEAD_WORDS)


def resample_host(tiles, mesh, spec, dst_shape, want=('dst', 'how', 'head'), raster=None):
    """dswx_resample_host (no device needed): the outputs of proteus_amd.resample.resample_tiles named in `want` -- 'dst'
    [n, dst_h, dst_w] of the plane's dtype, 'how' uint8 [n, dst_h, dst_w], 'head' uint64 [n, 8] -- of a host plane float32 or
    int16 [n_tiles, H, W] interpolated through the int32 mesh `mesh` ([mesh_h, mesh_w, 2], or per tile at
    spec.mesh_tile_stride_nodes) by `spec` (a resample.Spec), by the library's scalar statement of the definition.  With
    raster=(H, W), `tiles` is a padded plane [n_tiles, spec.src_tile_stride] whose padding is not read."""
    return _mesh_host('dswx_resample_host', _resample_planes, ResampleSpec, ResampleOut, tiles, lambda dt: dt == spec.dtype,
                      spec.dtype, mesh, spec, dst_shape, want, raster)


def land_mesh_host(worldcover, copernicus, mesh_wc, mesh_cg, spec, shape, want=('land', 'head'), wc_raster=None, cg_raster=None,
                   land=None):
    """dswx_land_mesh_host (no device needed): the outputs of proteus_amd.landmesh.land_tiles named in `want` -- 'land' uint8
    [n, H, W] ([n, spec.land_tile_stride] with a stride), 'head' uint64 [n, 8] -- of the host planes uint8 `worldcover` [n, wc_h,
    wc_w] and `copernicus` [n, cg_h, cg_w] read through the int32 meshes mesh_wc (of the lattice 3 H x 3 W) and mesh_cg (of H x
    W) by `spec` (a landmesh.Spec), by the library's scalar statement of the definition.  With wc_raster=(wc_h, wc_w) /
    cg_raster=, the plane is padded, [n, spec.wc_tile_stride] / [n, spec.cg_tile_stride], and its padding is not read.  `land`:
    an array to write into (what the entry does not write stays)."""
    wc, n, wc_h, wc_w, _ = _host_plane(worldcover, wc_raster)
    cg, n_cg, cg_h, cg_w, _ = _host_plane(copernicus, cg_raster)
    if n_cg != n:
        raise ValueError(f'{n} WorldCover tiles but {n_cg} CGLS tiles')
    H, W = (int(v) for v in shape)
    mesh_wc, mesh_cg = np.ascontiguousarray(mesh_wc, dtype=np.int32), np.ascontiguousarray(mesh_cg, dtype=np.int32)
    if n > 0 and H > 0 and W > 0:            # the node counts that the entry itself cannot check (it has addresses, not arrays)
        for what, mesh, s, stride, dims in (('mesh_wc', mesh_wc, spec.shift_wc, spec.mesh_wc_tile_stride_nodes, (3 * H, 3 * W)),
                                            ('mesh_cg', mesh_cg, spec.shift_cg, spec.mesh_cg_tile_stride_nodes, (H, W))):
            if 0 <= s <= WARP_MAX_SHIFT:
                step = 1 << s
                nodes = (((dims[0] + step - 1) >> s) + 1) * (((dims[1] + step - 1) >> s) + 1)
                if mesh.size < 2 * ((n - 1) * stride + nodes):
                    raise ValueError(f'{what} for {dims[0]} x {dims[1]} at shift {s} has {nodes} nodes per tile, {mesh.shape} is too small')
    want = _wanted(want, {'land': 0, 'head': 0})
    res = {}
    if 'land' in want:
        res['land'] = land if land is not None else np.zeros((n, spec.land_tile_stride) if spec.land_tile_stride else (n, max(H, 0), max(W, 0)),
                                                             dtype=np.uint8)
    if 'head' in want:
        res['head'] = np.zeros((n, LAND_MESH_HEAD_WORDS), dtype=np.uint64)
    _check(load_library().dswx_land_mesh_host(_host_ptr(wc) if wc.size else None, int(wc_h), int(wc_w), _host_ptr(cg) if cg.size else None,
                                              int(cg_h), int(cg_w), ctypes.byref(LandMeshSpec.of(spec)), n, H, W,
                                              _host_ptr(mesh_wc) if mesh_wc.size else None, _host_ptr(mesh_cg) if mesh_cg.size else None,
                                              res['land'].ctypes.data if 'land' in res and res['land'].size else None,
                                              res['head'].ctypes.data if 'head' in res and res['head'].size else None))
    return res


def _stack_planes(want, spec, shape, make):
    """{name: plane} for the outputs named in `want` ('count' is [n_cats, ...]), each made by make(shape, dtype)."""
    dtypes = {'count': np.uint16, 'last': np.uint8, 'last_index': np.uint16, 'share': np.uint8}
    want = _wanted(want, dtypes)
    return {k: make(((spec.n_cats,) if k == 'count' else ()) + tuple(shape), dtypes[k]) for k in dtypes if k in want}


def grid_host(tiles, spec, want=('count', 'share', 'coverage', 'major'), raster=None):
    """dswx_grid_host (no device needed): the planes of proteus_amd.grid.grid_tiles -- those named in `want` -- of a host
    plane uint8 [n_tiles, H, W], by the library's scalar statement of the definition.  With raster=(H, W), `tiles` is a padded
    plane uint8 [n_tiles, tile_stride], tile_stride >= H * W, whose padding is not read."""
    tiles, n, H, W, stride = _host_plane(tiles, raster)
    from .grid import grid_shape
    res = _grid_planes(want, spec, (n,) + grid_shape(H, W, spec), lambda shp, dt: np.zeros(shp, dtype=dt))
    out = GridOut.of(count=[c.ctypes.data for c in res['count']] if 'count' in res else (),
                     **{k: res[k].ctypes.data for k in ('share', 'coverage', 'major') if k in res})
    _check(load_library().dswx_grid_host(_host_ptr(tiles) if tiles.size else None, ctypes.byref(GridSpec.of(spec)), n, H, W,
                                         stride, ctypes.byref(out)))
    return res


def _grid_planes(want, spec, shape, make):
    """{name: plane} for the outputs named in `want` ('count' is [n_cats, ...]), each made by make(shape, dtype)."""
    dtypes = {'count': np.uint32, 'share': np.uint8, 'coverage': np.uint8, 'major': np.uint8}
    want = _wanted(want, dtypes)
    return {k: make(((spec.n_cats,) if k == 'count' else ()) + tuple(shape), dtypes[k]) for k in dtypes if k in want}


LABEL_DTYPES = {'label': np.uint32, 'size': np.uint32, 'sieved': np.uint8, 'summary': np.uint64}


def _label_wanted(want):
    """`want` in the order of the struct; 'label' is always made (it is the working array), 'size' with sieved or summary."""
    want = _wanted(want, LABEL_DTYPES)
    made = {'label'} | set(want) | ({'size'} if 'sieved' in want or 'summary' in want else set())
    return tuple(k for k in LABEL_DTYPES if k in made)


def label_host(tiles, spec, want=('label', 'size', 'sieved', 'summary'), raster=None):
    """dswx_label_host (no device needed): the planes of proteus_amd.label.label_tiles -- those named in `want`, and the ones
    they need -- of a host plane uint8 [n_tiles, H, W], by the library's scalar union-find.  With raster=(H, W), `tiles` is a
    padded plane uint8 [n_tiles, tile_stride], tile_stride >= H * W, whose padding is not read."""
    tiles, n, H, W, stride = _host_plane(tiles, raster)
    res = {k: np.zeros((n, LABEL_SUMMARY_WORDS) if k == 'summary' else (n, H, W), dtype=LABEL_DTYPES[k]) for k in _label_wanted(want)}
    out = LabelOut.of(**{k: a.ctypes.data for k, a in res.items()})
    _check(load_library().dswx_label_host(_host_ptr(tiles) if tiles.size else None, ctypes.byref(LabelSpec.of(spec)), n, H, W,
                                          stride, ctypes.byref(out)))
    return res


DISTANCE_DTYPES = {'dist2': np.uint32, 'nearest': np.uint32, 'within': np.uint8, 'summary': np.uint64}


def _distance_wanted(want, spec):
    """`want` in the order of the struct; 'dist2' is always made (it is the working array); 'within' needs a radius."""
    want = _wanted(want, DISTANCE_DTYPES)
    if 'within' in want and spec.max_radius == 0:
        raise ValueError("'within' is wanted but max_radius is 0: the ring needs a radius")
    return tuple(k for k in DISTANCE_DTYPES if k == 'dist2' or k in want)


def _distance_refuse(H, W):
    """The limits of include/dswx_hip.h "distance" on a raster, refused here as the library would."""
    if H > DISTANCE_MAX_SIDE or W > DISTANCE_MAX_SIDE or H * W > 1 << 31:
        raise ValueError(f'{H} x {W} pixels: each side at most {DISTANCE_MAX_SIDE} and at most 2^31 pixels')
    if W > DISTANCE_MAX_WIDTH:
        raise ValueError(f'width {W} above DISTANCE_MAX_WIDTH ({DISTANCE_MAX_WIDTH})')


def distance_host(tiles, spec, want=('dist2', 'nearest', 'summary'), raster=None):
    """dswx_distance_host (no device needed): the planes of proteus_amd.distance.distance_tiles -- those named in `want`, and
    'dist2' always -- of a host plane uint8 [n_tiles, H, W], by the library's scalar transform.  With raster=(H, W), `tiles`
    is a padded plane uint8 [n_tiles, tile_stride], tile_stride >= H * W, whose padding is not read."""
    tiles, n, H, W, stride = _host_plane(tiles, raster)
    _distance_refuse(H, W)
    res = {k: np.zeros((n, DISTANCE_SUMMARY_WORDS) if k == 'summary' else (n, H, W), dtype=DISTANCE_DTYPES[k])
           for k in _distance_wanted(want, spec)}
    out = DistanceOut.of(**{k: a.ctypes.data for k, a in res.items()})
    _check(load_library().dswx_distance_host(_host_ptr(tiles) if tiles.size else None, ctypes.byref(DistanceSpec.of(spec)), n, H, W,
                                             stride, ctypes.byref(out)))
    return res


BODY_DTYPES = {'dense': np.uint32, 'rows': np.uint32, 'head': np.uint64}


def _body_wanted(want, spec):
    """`want` in the order of the struct; 'dense' is always made (it is the working array); 'rows' only with max_rows > 0."""
    want = _wanted(want, BODY_DTYPES)
    if spec.max_rows > 0 and 'rows' not in want:
        raise ValueError(f"max_rows {spec.max_rows} without 'rows': a table that is not wanted has max_rows 0")
    return tuple(k for k in BODY_DTYPES if k == 'dense' or (k in want and (k != 'rows' or spec.max_rows > 0)))


def _body_shape(k, n, H, W, spec):
    return {'dense': (n, H, W), 'rows': (n, spec.max_rows, BODY_ROW_WORDS), 'head': (n, BODY_HEAD_WORDS)}[k]


def body_table_host(label, value, spec, want=('dense', 'rows', 'head'), raster=None):
    """dswx_body_table_host (no device needed): the outputs of proteus_amd.bodies.body_table -- those named in `want`, and
    'dense' always; 'rows' as uint32 [n_tiles, max_rows, 16], which `.view(bodies.ROW_DTYPE)[..., 0]` turns into records -- of
    a host label plane uint32 [n_tiles, H, W] and a value plane uint8 [n_tiles, H, W] (None with spec.n_cats == 0), by the
    library's scalar statement.  With raster=(H, W), `value` is a padded plane uint8 [n_tiles, value_stride], value_stride >=
    H * W, whose padding is not read."""
    label = np.ascontiguousarray(label)
    if label.dtype != np.uint32 or label.ndim != 3:
        raise ValueError(f'a label plane is uint32 [n_tiles, H, W], not {label.dtype} {label.shape}')
    n, H, W = label.shape
    stride = 0
    if value is not None:
        value = np.ascontiguousarray(value)
        if value.dtype != np.uint8 or (value.shape != label.shape if raster is None else value.ndim != 2 or value.shape[0] != n or tuple(raster) != (H, W)):
            raise ValueError(f'a value plane is uint8 {label.shape} or, with raster=, [n_tiles, value_stride], not {value.dtype} {value.shape}')
        if raster is not None:
            stride = value.shape[1]
    res = {k: np.zeros(_body_shape(k, n, H, W, spec), dtype=BODY_DTYPES[k]) for k in _body_wanted(want, spec)}
    out = BodyOut.of(**{k: a.ctypes.data for k, a in res.items()})
    _check(load_library().dswx_body_table_host(_host_ptr(label) if label.size else None,
                                               _host_ptr(value) if value is not None else None,
                                               ctypes.byref(BodySpec.of(spec)), n, H, W, stride, ctypes.byref(out)))
    return res


OUTLINE_DTYPES = {'chain': np.uint32, 'rings': np.uint32, 'head': np.uint64}


def _outline_wanted(want, spec):
    """`want` in the order of the struct; 'rings' only with max_rings > 0, and only with 'chain'."""
    want = _wanted(want, OUTLINE_DTYPES)
    if spec.max_rings > 0 and 'rings' not in want:
        raise ValueError(f"max_rings {spec.max_rings} without 'rings': a table that is not wanted has max_rings 0")
    if 'rings' in want and spec.max_rings > 0 and 'chain' not in want:
        raise ValueError("'rings' without 'chain': a row names a place in the chain")
    return tuple(k for k in OUTLINE_DTYPES if k in want and (k != 'rings' or spec.max_rings > 0))


def _outline_shape(k, n, spec):
    return {'chain': (n, spec.max_edges), 'rings': (n, spec.max_rings, OUTLINE_ROW_WORDS), 'head': (n, OUTLINE_HEAD_WORDS)}[k]


def outline_work_bytes(spec, n_tiles, height, width):
    """dswx_outline_work_bytes (no device needed): the bytes of working memory dswx_outline_device needs."""
    v = ctypes.c_uint64()
    _check(load_library().dswx_outline_work_bytes(ctypes.byref(OutlineSpec.of(spec)), int(n_tiles), int(height), int(width), ctypes.byref(v)))
    return int(v.value)


def outline_host(ids, spec, want=('chain', 'rings', 'head')):
    """dswx_outline_host (no device needed): the outputs of proteus_amd.outline.outline_tiles named in `want` -- 'rings' as
    uint32 [n_tiles, max_rings, 8], which `.view(outline.ROW_DTYPE)[..., 0]` turns into records -- of a host id plane uint32
    [n_tiles, H, W], by the library's scalar walk."""
    ids = np.ascontiguousarray(ids)
    if ids.dtype != np.uint32 or ids.ndim != 3:
        raise ValueError(f'an id plane is uint32 [n_tiles, H, W], not {ids.dtype} {ids.shape}')
    n, H, W = ids.shape
    res = {k: np.zeros(_outline_shape(k, n, spec), dtype=OUTLINE_DTYPES[k]) for k in _outline_wanted(want, spec)}
    out = OutlineOut.of(**{k: a.ctypes.data for k, a in res.items()})
    _check(load_library().dswx_outline_host(_host_ptr(ids) if ids.size else None, ctypes.byref(OutlineSpec.of(spec)), n, H, W,
                                            ctypes.byref(out)))
    return res


BURN_DTYPES = {'acc': np.uint32, 'mask': np.uint8, 'head': np.uint64}


def _burn_wanted(want):
    """`want` in the order of the struct; 'acc' is always made (it is the working array)."""
    want = _wanted(want, BURN_DTYPES)
    return tuple(k for k in BURN_DTYPES if k == 'acc' or k in want)


def _burn_shape(k, n, H, W, spec):
    return {'acc': (n, H, W), 'mask': (n, spec.mask_tile_stride) if spec.mask_tile_stride else (n, H, W), 'head': (n, BURN_HEAD_WORDS)}[k]


def _burn_input(verts, tile_first):
    """(records as contiguous burn.VERTEX_DTYPE, table as contiguous int64, n_tiles)."""
    from .burn import VERTEX_DTYPE
    verts = np.ascontiguousarray(verts)
    if verts.dtype != VERTEX_DTYPE or verts.ndim != 1:
        raise ValueError(f'records are burn.VERTEX_DTYPE [k], not {verts.dtype} {verts.shape}')
    tile_first = np.ascontiguousarray(tile_first, dtype=np.int64)
    if tile_first.ndim != 1 or len(tile_first) < 1:
        raise ValueError(f'tile_first is int64 [n_tiles + 1], not {tile_first.shape}')
    return verts, tile_first, len(tile_first) - 1


def burn_host(verts, tile_first, height, width, spec, src=None, want=('acc', 'mask', 'head'), mask=None):
    """dswx_burn_host (no device needed): the outputs of proteus_amd.burn.burn_tiles named in `want`, and 'acc' always, of the
    host records `verts` (burn.VERTEX_DTYPE) shared out by `tile_first` (int64 [n_tiles + 1]), by the library's scalar
    statement.  'mask' is uint8 [n_tiles, H, W], or [n_tiles, spec.mask_tile_stride] with a stride; `mask` names an array of
    that size to write into instead of a new one (the bytes between the rasters are left as they are), and `src` (uint8, of
    the size the spec's src stride implies) may be that very array: burnt in place."""
    return _rings_host('dswx_burn_host', BurnSpec, verts, tile_first, height, width, spec, src, want, mask)


def reach_host(verts, tile_first, height, width, spec, src=None, want=('acc', 'mask', 'head'), mask=None):
    """dswx_reach_host (no device needed): the outputs of proteus_amd.reach.reach_tiles, with the arguments of burn_host and
    `spec` a reach.Spec."""
    return _rings_host('dswx_reach_host', ReachSpec, verts, tile_first, height, width, spec, src, want, mask)


def _rings_host(entry, spec_struct, verts, tile_first, height, width, spec, src, want, mask):
    verts, tile_first, n = _burn_input(verts, tile_first)
    want = _burn_wanted(want)
    res = {k: np.zeros(_burn_shape(k, n, height, width, spec), dtype=BURN_DTYPES[k]) for k in want if not (k == 'mask' and mask is not None)}
    if mask is not None:
        if 'mask' not in want or mask.dtype != np.uint8 or not mask.flags.c_contiguous or \
                mask.size != int(np.prod(_burn_shape('mask', n, height, width, spec), dtype=np.int64)):
            raise ValueError("mask= is a contiguous uint8 array of the size of the 'mask' output, and 'mask' is wanted")
        res['mask'] = mask
    if src is not None:
        if src is not mask:
            src = np.ascontiguousarray(src, dtype=np.uint8)
        if src.size != n * (spec.src_tile_stride or height * width):
            raise ValueError(f'src has {src.size} bytes, not {n} tiles of {spec.src_tile_stride or height * width}')
    dummy = np.zeros(1, dtype=verts.dtype)
    out = BurnOut.of(**{k: a.ctypes.data for k, a in res.items()})
    _check(getattr(load_library(), entry)(_host_ptr(verts if verts.size else dummy), _host_ptr(tile_first), ctypes.byref(spec_struct.of(spec)),
                                          n, int(height), int(width), _host_ptr(src) if src is not None else None, ctypes.byref(out)))
    return res


def cog_layout(height, width, elem_bytes, factors=(), tile=512):
    """dswx_cog_layout (no device needed): {'n_levels', 'total_bytes', 'levels': [{'factor', 'height', 'width',
    'blocks_down', 'blocks_across', 'offset_bytes'}]}."""
    lay = CogLayout()
    f = (ctypes.c_int32 * max(len(factors), 1))(*[int(x) for x in factors])
    _check(load_library().dswx_cog_layout(int(height), int(width), int(elem_bytes), int(tile), f, len(factors), ctypes.byref(lay)))
    return {'n_levels': lay.n_levels, 'total_bytes': int(lay.total_bytes), 'tile': lay.tile,
            'levels': [{'factor': lay.factor[k], 'height': int(lay.height[k]), 'width': int(lay.width[k]),
                        'blocks_down': lay.blocks_down[k], 'blocks_across': lay.blocks_across[k],
                        'offset_bytes': int(lay.offset_bytes[k])} for k in range(lay.n_levels)]}


def batch_layout(n_tiles, height, width, masks=False, extra_layers=(), tile_stride=0, separate_outputs=False,
                 sliding_outputs=False):
    """dswx_batch_layout: where dswx_batch_create puts every plane (pure function, no device).  Returns
    {'tile_stride', 'arena_bytes', 'write_span_bytes', 'planes': {name: (offset, nbytes)}}."""
    flags = _batch_flags(masks, extra_layers, separate_outputs, sliding_outputs)
    lay = BatchLayout()
    geom = BatchGeom(n_tiles, height, width, tile_stride)
    _check(load_library().dswx_batch_layout(ctypes.byref(geom), flags, ctypes.byref(lay)))
    planes = {name: (int(lay.plane_offset[k]), int(lay.plane_bytes[k])) for name, k in PLANE_INDEX.items()
              if lay.plane_bytes[k]}
    return {'tile_stride': int(lay.tile_stride), 'arena_bytes': int(lay.arena_bytes),
            'write_span_bytes': int(lay.write_span_bytes), 'planes': planes}


def _batch_flags(masks, extra_layers, separate_outputs, sliding_outputs=False):
    unknown = [x for x in extra_layers if x not in ('wtr1_aerosol', 'browse')]
    if unknown:
        raise ValueError(f'a resident batch has no plane {unknown[0]!r}')
    return ((BATCH_MASKS if masks else 0) | (BATCH_WTR1_AEROSOL if 'wtr1_aerosol' in extra_layers else 0)
            | (BATCH_BROWSE if 'browse' in extra_layers else 0) | (BATCH_SEPARATE_OUTPUTS if separate_outputs else 0)
            | (BATCH_SLIDING_OUTPUTS if sliding_outputs else 0))


def _plane_index(name):
    """DSWX_PLANE_* of a plane by its name."""
    if name not in PLANE_INDEX:
        raise ValueError(f'unknown plane {name!r}')
    return PLANE_INDEX[name]


class DeviceBatch:
    """Band-planar batch resident in HBM (dswx_batch_t of include/dswx_hip.h): every plane is [n_tiles][tile_stride].

    The LIBRARY allocates and lays out the planes (dswx_batch_create: one allocation, 256-byte aligned plane
    offsets; with separate_outputs one for the inputs and one per output plane, which is what `place_search`
    needs).  By default the tile stride is H*W rounded up to a multiple of 256 pixels, so every tile starts on a
    256-byte boundary in every plane (contiguous tiles of 3660 x 3660 do not: 13,395,600 = 144 mod 256, which
    costs ~20 % of the HBM rate); `tile_align=1` gives contiguous tiles.
    Used by bench.py, the multi-GPU driver and the device-path parity tests.
    """

    def __init__(self, ctx, n_tiles, height, width, masks=False, extra_layers=(), tile_align=256,
                 separate_outputs=False, sliding_outputs=False):
        self.ctx, self.n_tiles, self.height, self.width = ctx, n_tiles, height, width
        self.n_pixels = height * width
        self.masks = masks
        stride = -(-self.n_pixels // tile_align) * tile_align
        flags = _batch_flags(masks, extra_layers, separate_outputs, sliding_outputs)
        h = ctypes.c_void_p()
        geom = BatchGeom(n_tiles, height, width, stride)
        if stride == 0:                 # an empty tile: let the library resolve the stride (0 stays 0)
            geom.tile_stride = 0
        self._lib = ctx.lib             # kept for free(): the batch may outlive ctx.handle
        self.handle = None
        _check(ctx.lib.dswx_batch_create(ctx.handle, ctypes.byref(geom), flags, ctypes.byref(h)))
        self.handle = h
        self.out_layers = ['wtr1'] + (['wtr1_aerosol'] if 'wtr1_aerosol' in extra_layers else []) + \
            ['wtr2', 'wtr', 'bwtr', 'conf', 'cloud'] + (['browse'] if 'browse' in extra_layers else [])
        self._rebind()

    def _rebind(self):
        """Fetch the plane pointers (they change when place_search re-binds output planes)."""
        self.geom, self.pin, self.pout = BatchGeom(), PlanesIn(), PlanesOut()
        cnt = ctypes.c_void_p()
        _check(self.ctx.lib.dswx_batch_planes(self.handle, ctypes.byref(self.geom), ctypes.byref(self.pin),
                                              ctypes.byref(self.pout), ctypes.byref(cnt)))
        self.tile_stride = int(self.geom.tile_stride)
        self.counters_ptr = cnt.value
        info = self.info()
        self.nbytes = info['bytes_allocated']

    def info(self):
        bi = BatchInfo()
        _check(self.ctx.lib.dswx_batch_info(self.handle, ctypes.byref(bi)))
        return {'bytes_allocated': int(bi.bytes_allocated), 'n_allocations': int(bi.n_allocations),
                'flags': int(bi.flags), 'search_candidates': int(bi.search_candidates),
                'search_probes': int(bi.search_probes),
                'first_come_launch_ms': float(bi.first_come_launch_ms), 'kept_launch_ms': float(bi.kept_launch_ms),
                'va_reserved_bytes': int(bi.va_reserved_bytes), 'va_retired_bytes': int(bi.va_retired_bytes),
                'va_budget_bytes': int(bi.va_budget_bytes), 'va_pooled_bytes': int(bi.va_pooled_bytes),
                'note': bi.note.decode()}

    def place_search(self, params, candidates=6, launches=3, keep_free_bytes=8 << 30):
        """dswx_batch_place_search: measured placement of the output planes (separate_outputs batches whose inputs
        are resident).  On MI355X the fused kernel's rate depends on the ranges its seven write streams land in --
        a stable property of the allocation -- so a long-lived batch is worth placing.
        Returns the record of the search."""
        _check(self.ctx.lib.dswx_batch_place_search(self.handle, ctypes.byref(params), int(candidates),
                                                    int(launches), int(keep_free_bytes)))
        self._rebind()
        i = self.info()
        return {'trials': i['search_candidates'], 'probes': i['search_probes'],
                'first_come_launch_ms': round(i['first_come_launch_ms'], 4),
                'kept_launch_ms': round(i['kept_launch_ms'], 4)}

    def place_slide(self, params, slack_bytes=48 << 30, step_bytes=2 << 30, spread_gaps=4, refine_passes=1,
                    launches=3, keep_free_bytes=8 << 30):
        """dswx_batch_place_slide: the output region (sliding_outputs batches) timed at offsets 0, step, 2 step, ...
        of a range `slack_bytes` longer than itself; the best position is kept and the rest of the range returned to the
        device.  Returns the record of the search."""
        _check(self.ctx.lib.dswx_batch_place_slide(self.handle, ctypes.byref(params), int(slack_bytes), int(step_bytes),
                                                   int(spread_gaps), int(refine_passes), int(launches),
                                                   int(keep_free_bytes)))
        self._rebind()
        i = self.info()
        rec = {'positions': i['search_candidates'], 'probes': i['search_probes'],
               'first_come_launch_ms': round(i['first_come_launch_ms'], 4),
               'kept_launch_ms': round(i['kept_launch_ms'], 4), 'va_retired_gib': round(i['va_retired_bytes'] / 2 ** 30, 2)}
        if i['note']:
            rec['note'] = i['note']
        return rec

    def synth(self, seed, tile0=0, stream=None):
        _check(self.ctx.lib.dswx_batch_synth(self.handle, int(seed), int(tile0),
                                             _stream_arg(stream)))

    def classify(self, params, stream=None, counters=True, n_tiles=None):
        """The first `n_tiles` resident tiles (None = all, DSWX_BATCH_ALL_TILES; 0 = none: an empty chunk is no work).
        counters=False goes through dswx_classify_batch with a NULL counters pointer (dswx_batch_classify always counts)."""
        if n_tiles is None:
            n_tiles = BATCH_ALL_TILES
        if counters:
            _check(self.ctx.lib.dswx_batch_classify(self.handle, ctypes.byref(params), int(n_tiles),
                                                    _stream_arg(stream)))
        elif n_tiles != 0:
            geom = BatchGeom(self.n_tiles if n_tiles == BATCH_ALL_TILES else n_tiles, self.height, self.width,
                             self.tile_stride)
            self.ctx.classify_batch(params, geom, self.pin, self.pout, None, stream)

    def _plane(self, name):
        if name in BAND_NAMES:
            ptr, dt = self.pin.band[BAND_NAMES.index(name)], np.int16
        elif name in ('fmask', 'land', 'shad', 'ocean'):
            ptr, dt = getattr(self.pin, name), np.uint8
        elif name == 'diag' or name in U8_LAYERS:
            ptr, dt = getattr(self.pout, name), (np.uint16 if name == 'diag' else np.uint8)
        else:
            raise ValueError(f'unknown plane {name!r}')
        if not ptr:
            raise ValueError(f'plane {name!r} is not part of this batch (masks / extra_layers of DeviceBatch)')
        return ptr, dt

    def plane_names(self):
        """The planes this batch has (inputs, layers, extra layers), in the order of PLANE_INDEX."""
        return [n for n in PLANE_INDEX if n != 'counters' and (
            getattr(self.pout, n) if n == 'diag' or n in U8_LAYERS else
            self.pin.band[BAND_NAMES.index(n)] if n in BAND_NAMES else getattr(self.pin, n))]

    def _mask(self, names):
        """(plane mask, the names in the order of its bits: row i of a mask entry's output is plane order[i]) of `names`
        (None: every plane the batch has)."""
        names = self.plane_names() if names is None else list(names)
        mask = 0
        for n in names:
            mask |= 1 << _plane_index(n)
        return mask, sorted(set(names), key=PLANE_INDEX.get)

    def _tiles(self, tile0, n_tiles):
        """(the n_tiles an entry is given, the tiles its outputs are sized for) for tiles tile0 .. tile0 + n_tiles - 1; None
        is DSWX_BATCH_ALL_TILES: every tile from tile0, which the library resolves."""
        if n_tiles is None or n_tiles == BATCH_ALL_TILES:
            return BATCH_ALL_TILES, max(self.n_tiles - tile0, 0)
        return int(n_tiles), max(int(n_tiles), 0)

    def checksums(self, names=None, tile0=0, n_tiles=None, stream=None):
        """dswx_batch_checksum: {name: uint64 [n_tiles]}, the checksum of every selected plane of tiles tile0 .. tile0 +
        n_tiles - 1 (default: every plane the batch has -- 'counters' only when named -- and every tile from tile0), by ONE
        kernel launch; complete on return.  proteus_amd.checksum.checksum(read_tile(name, t)) is the same number."""
        mask, order = self._mask(names)
        n_tiles, count = self._tiles(tile0, n_tiles)
        out = np.zeros((len(order), count), dtype=np.uint64)
        _check(self.ctx.lib.dswx_batch_checksum(self.handle, mask, int(tile0), n_tiles, _host_ptr(out), _stream_arg(stream)))
        return dict(zip(order, out))

    def compare(self, other, names=None, tile0=0, n_tiles=None, atol=0.0, rtol=0.0, equal_nan=True, stream=None):
        """dswx_batch_compare: {name: compare.RECORD [n_tiles]}, this batch's selected planes against `other`'s (default:
        every plane this batch has), tiles tile0 .. tile0 + n_tiles - 1 of both, by ONE kernel launch; complete on return.
        proteus_amd.compare.compare(self.read_tile(name, t), other.read_tile(name, t), ...) is the same record."""
        from .compare import RECORD
        mask, order = self._mask(names)
        n_tiles, count = self._tiles(tile0, n_tiles)
        out = np.zeros((len(order), count), dtype=RECORD)
        _check(self.ctx.lib.dswx_batch_compare(self.handle, other.handle, mask, int(tile0), n_tiles, float(atol), float(rtol),
                                               int(bool(equal_nan)), _host_ptr(out), _stream_arg(stream)))
        return dict(zip(order, out))

    def histogram(self, names=None, tile0=0, n_tiles=None, band_lo=0, band_shift=6, stream=None):
        """dswx_batch_histogram: {name: uint64 [n_tiles, 256]}, the counts of every selected plane of tiles tile0 .. tile0 +
        n_tiles - 1 (default: every plane the batch has and every tile from tile0), by ONE kernel launch; complete on return.
        The bands are binned linearly with band_lo / band_shift (the defaults: reflectances 0 .. 16383 in bins of 64), 'diag' by
        its five test bits, every other plane by its byte: proteus_amd.histogram.histogram(read_tile(name, t), kind, lo, shift)
        is the same record."""
        mask, order = self._mask(names)
        n_tiles, count = self._tiles(tile0, n_tiles)
        out = np.zeros((len(order), count, HIST_BINS), dtype=np.uint64)
        _check(self.ctx.lib.dswx_batch_histogram(self.handle, mask, int(tile0), n_tiles, int(band_lo), int(band_shift),
                                                 _host_ptr(out), _stream_arg(stream)))
        return dict(zip(order, out))

    def crosstab(self, pairs, other=None, tile0=0, n_tiles=None, stream=None):
        """dswx_batch_crosstab: uint64 [n_pairs, n_tiles, 256], for every pair (name_a, name_b, spec) plane name_a of this
        batch against plane name_b of `other` (default: of this batch) by spec (a crosstab.Spec), tiles tile0 .. tile0 +
        n_tiles - 1 of both (default: every tile from tile0), by ONE kernel launch for at most CROSSTAB_MAX_PAIRS pairs; complete
        on return.  proteus_amd.crosstab.crosstab(self.read_tile(name_a, t), other.read_tile(name_b, t), spec) is the same record."""
        other = self if other is None else other
        pairs = list(pairs)
        arr = (CrosstabPair * max(len(pairs), 1))()
        for k, (name_a, name_b, spec) in enumerate(pairs):
            arr[k].plane_a, arr[k].plane_b, arr[k].spec = _plane_index(name_a), _plane_index(name_b), CrosstabSpec.of(spec)
        n_tiles, count = self._tiles(tile0, n_tiles)
        out = np.zeros((len(pairs), count, CROSSTAB_CELLS), dtype=np.uint64)
        _check(self.ctx.lib.dswx_batch_crosstab(self.handle, other.handle, arr, len(pairs), int(tile0), n_tiles,
                                                _host_ptr(out), _stream_arg(stream)))
        return out

    def stack(self, name, spec, tile0=0, n_tiles=None, want=('count', 'last', 'last_index', 'share'), stream=None):
        """dswx_batch_stack: tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0) of the uint8 plane `name`
        composited per pixel by `spec` (a stack.Spec), by ONE kernel launch, asynchronous on `stream`.  Returns {output:
        DeviceBuffer} for the outputs named in `want`: 'count' uint16 [n_cats][H*W], 'last' uint8 [H*W], 'last_index' uint16
        [H*W], 'share' uint8 [H*W] -- device planes owned by the caller.  proteus_amd.stack.stack_tiles of the downloaded
        tiles gives the same planes."""
        plane = _plane_index(name)
        n = max(self.n_pixels, 1)
        res = _malloc_planes(self.ctx, _stack_planes(want, spec, (n,), lambda shp, dt: (shp, dt)))
        out = StackOut.of(count=[res['count'].ptr + 2 * n * k for k in range(spec.n_cats)] if 'count' in res else (),
                          **{k: res[k].ptr for k in ('last', 'last_index', 'share') if k in res})
        with _owned(res):
            _check(self.ctx.lib.dswx_batch_stack(self.handle, plane, ctypes.byref(StackSpec.of(spec)), int(tile0),
                                                 self._tiles(tile0, n_tiles)[0], ctypes.byref(out), _stream_arg(stream)))
        return res

    def mosaic(self, name, place_ptr, canvas_shape, spec, tile0=0, n_tiles=None, want=('count', 'last', 'last_index', 'share'),
               stream=None):
        """dswx_batch_mosaic: tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0) of the uint8 plane `name`
        placed on a canvas of canvas_shape = (canvas_h, canvas_w) by the DEVICE table int32 [n_tiles][2] at place_ptr (entry 0
        belongs to tile0) and composited per canvas pixel by `spec` (a mosaic.Spec), by ONE kernel launch, asynchronous on
        `stream`.  Returns {output: DeviceBuffer} for the outputs named in `want`: 'count' uint16 [n_cats][canvas_h * canvas_w],
        'last' uint8, 'last_index' uint16 (counted from tile0) and 'share' uint8 [canvas_h * canvas_w] -- device planes owned by
        the caller.  proteus_amd.mosaic.mosaic_tiles of the downloaded tiles gives the same planes."""
        plane = _plane_index(name)
        ch, cw = (int(v) for v in canvas_shape)
        n = max(ch * cw, 1)
        res = _malloc_planes(self.ctx, _stack_planes(want, spec, (n,), lambda shp, dt: (shp, dt)))
        out = StackOut.of(count=[res['count'].ptr + 2 * n * k for k in range(spec.n_cats)] if 'count' in res else (),
                          **{k: res[k].ptr for k in ('last', 'last_index', 'share') if k in res})
        with _owned(res):
            _check(self.ctx.lib.dswx_batch_mosaic(self.handle, plane, ctypes.byref(MosaicSpec.of(spec)), int(tile0),
                                                  self._tiles(tile0, n_tiles)[0], ctypes.c_void_p(place_ptr), ch, cw,
                                                  ctypes.byref(out), _stream_arg(stream)))
        return res

    def warp(self, name, mesh_ptr, dst_shape, spec, tile0=0, n_tiles=None, want=('dst', 'src_index', 'head'), stream=None):
        """dswx_batch_warp: tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0) of ANY plane `name` but the
        counters resampled (nearest pixel) onto dst_shape = (dst_h, dst_w) through the DEVICE mesh int32 [mesh_h][mesh_w][2] at
        mesh_ptr (mesh 0 belongs to tile0) by `spec` (a warp.Spec whose elem_bytes is the plane's), by one memset and ONE kernel
        launch, asynchronous on `stream`.  Returns {output: DeviceBuffer} for the outputs named in `want`: 'dst' [n_tiles][dst_h *
        dst_w] elements, 'src_index' uint32 of the same shape, 'head' uint64 [n_tiles][8] -- device memory owned by the caller.
        proteus_amd.warp.warp_tiles of the downloaded tiles gives the same arrays."""
        plane = _plane_index(name)
        n_tiles, nt = self._tiles(tile0, n_tiles)
        elem = {1: np.uint8, 2: np.uint16, 4: np.uint32}.get(int(spec.elem_bytes), np.uint8)
        res = _malloc_planes(self.ctx, _warp_planes(want, elem, nt, dst_shape, lambda shp, dt: (shp, dt)))
        out = WarpOut.of(**{k: b.ptr for k, b in res.items()})
        with _owned(res):
            _check(self.ctx.lib.dswx_batch_warp(self.handle, plane, ctypes.byref(WarpSpec.of(spec)), int(tile0), n_tiles,
                                                ctypes.c_void_p(mesh_ptr), int(dst_shape[0]), int(dst_shape[1]), ctypes.byref(out),
                                                _stream_arg(stream)))
        return res

    def land_mesh(self, wc_ptr, wc_shape, cg_ptr, cg_shape, spec, mesh_wc_ptr, mesh_cg_ptr, tile0=0, n_tiles=None, head_ptr=None,
                  stream=None):
        """dswx_land_mesh_device straight into the LAND plane of tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from
        tile0) of this batch, with the batch's tile stride: source tile 0 and mesh 0 belong to tile0.  `spec` is a landmesh.Spec
        whose land_tile_stride is 0 (the batch has its own).  head_ptr: device uint64 [n_tiles][8], or None."""
        import copy
        if spec.land_tile_stride:
            raise ValueError('the LAND plane has the stride of the batch: spec.land_tile_stride must be 0')
        land = self._plane('land')[0]
        nt = self._tiles(tile0, n_tiles)[1]
        if tile0 < 0 or tile0 + nt > self.n_tiles:
            raise ValueError(f'tiles {tile0} .. {tile0 + nt - 1} are not tiles of this batch of {self.n_tiles}')
        spec = copy.copy(spec)
        spec.land_tile_stride = self.tile_stride
        self.ctx.land_mesh_device(wc_ptr, wc_shape, cg_ptr, cg_shape, spec, nt, self.height, self.width, mesh_wc_ptr, mesh_cg_ptr,
                                  land + int(tile0) * self.tile_stride, head_ptr, stream)

    def grid(self, name, spec, tile0=0, n_tiles=None, want=('count', 'share', 'coverage', 'major'), stream=None):
        """dswx_batch_grid: tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0) of the uint8 plane `name`
        aggregated onto cells by `spec` (a grid.Spec), by ONE kernel launch, asynchronous on `stream`.  Returns {output:
        DeviceBuffer} for the outputs named in `want`: 'count' uint32 [n_cats][n_tiles][GH*GW], 'share', 'coverage' and
        'major' uint8 [n_tiles][GH*GW] -- device planes owned by the caller.  proteus_amd.grid.grid_tiles of the downloaded
        tiles gives the same planes."""
        plane = _plane_index(name)
        from .grid import grid_shape
        n_tiles, nt = self._tiles(tile0, n_tiles)
        gh, gw = grid_shape(self.height, self.width, spec)
        n = max(nt * gh * gw, 1)
        res = _malloc_planes(self.ctx, _grid_planes(want, spec, (n,), lambda shp, dt: (shp, dt)))
        out = GridOut.of(count=[res['count'].ptr + 4 * n * k for k in range(spec.n_cats)] if 'count' in res else (),
                         **{k: res[k].ptr for k in ('share', 'coverage', 'major') if k in res})
        with _owned(res):
            _check(self.ctx.lib.dswx_batch_grid(self.handle, plane, ctypes.byref(GridSpec.of(spec)), int(tile0), n_tiles,
                                                ctypes.byref(out), _stream_arg(stream)))
        return res

    def label(self, name, spec, tile0=0, n_tiles=None, want=('label', 'size', 'sieved', 'summary'), stream=None):
        """dswx_batch_label: the connected bodies of tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0) of
        the uint8 plane `name` by `spec` (a label.Spec), asynchronous on `stream`.  Returns {output: DeviceBuffer} for the
        outputs named in `want` and the ones they need ('label' always, 'size' with 'sieved' or 'summary'): 'label' and
        'size' uint32 [n_tiles][H*W], 'sieved' uint8 [n_tiles][H*W], 'summary' uint64 [n_tiles][40] -- device planes owned by
        the caller.  proteus_amd.label.label_tiles of the downloaded tiles gives the same planes."""
        plane = _plane_index(name)
        n_tiles, nt = self._tiles(tile0, n_tiles)
        res = _malloc_planes(self.ctx, {k: ((nt, LABEL_SUMMARY_WORDS if k == 'summary' else self.n_pixels), LABEL_DTYPES[k])
                                        for k in _label_wanted(want)})
        out = LabelOut.of(**{k: b.ptr for k, b in res.items()})
        with _owned(res):
            _check(self.ctx.lib.dswx_batch_label(self.handle, plane, ctypes.byref(LabelSpec.of(spec)), int(tile0), n_tiles,
                                                 ctypes.byref(out), _stream_arg(stream)))
        return res

    def distance(self, name, spec, tile0=0, n_tiles=None, want=('dist2', 'nearest', 'summary'), stream=None):
        """dswx_batch_distance: the squared distance to the nearest target, by `spec` (a distance.Spec), of every pixel of tiles
        tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0) of the uint8 plane `name`, asynchronous on `stream`.
        Returns {output: DeviceBuffer} for the outputs named in `want` and 'dist2' always: 'dist2' and 'nearest' uint32
        [n_tiles][H*W], 'within' uint8 [n_tiles][H*W] (needs spec.max_radius > 0), 'summary' uint64 [n_tiles][40] -- device
        planes owned by the caller.  proteus_amd.distance.distance_tiles of the downloaded tiles gives the same planes."""
        plane = _plane_index(name)
        n_tiles, nt = self._tiles(tile0, n_tiles)
        res = _malloc_planes(self.ctx, {k: ((nt, DISTANCE_SUMMARY_WORDS if k == 'summary' else self.n_pixels), DISTANCE_DTYPES[k])
                                        for k in _distance_wanted(want, spec)})
        out = DistanceOut.of(**{k: b.ptr for k, b in res.items()})
        with _owned(res):
            _check(self.ctx.lib.dswx_batch_distance(self.handle, plane, ctypes.byref(DistanceSpec.of(spec)), int(tile0), n_tiles,
                                                    ctypes.byref(out), _stream_arg(stream)))
        return res

    def body_table(self, value_name, spec, label, tile0=0, n_tiles=None, want=('dense', 'rows', 'head'), stream=None):
        """dswx_batch_body_table: the bodies of `label` -- the device address (or a DeviceBuffer) of the dense label plane
        uint32 [n_tiles][H*W] of tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0), for instance
        label(...)['label'] of the same range -- renumbered and tabulated against the uint8 plane `value_name` (None with
        spec.n_cats == 0) by `spec` (a bodies.Spec), asynchronous on `stream`.  Returns {output: DeviceBuffer} for the outputs
        named in `want` and 'dense' always: 'dense' uint32 [n_tiles][H*W], 'rows' uint32 [n_tiles][max_rows][16] (only with
        max_rows > 0), 'head' uint64 [n_tiles][8] -- device planes owned by the caller.  proteus_amd.bodies.body_table of
        the downloaded planes gives the same."""
        plane = -1 if value_name is None else _plane_index(value_name)
        n_tiles, nt = self._tiles(tile0, n_tiles)
        res = _malloc_planes(self.ctx, {k: (_body_shape(k, nt, self.height, self.width, spec), BODY_DTYPES[k])
                                        for k in _body_wanted(want, spec)})
        out = BodyOut.of(**{k: b.ptr for k, b in res.items()})
        with _owned(res):
            _check(self.ctx.lib.dswx_batch_body_table(self.handle, plane, ctypes.byref(BodySpec.of(spec)), int(tile0), n_tiles,
                                                      ctypes.c_void_p(getattr(label, 'ptr', label)), ctypes.byref(out),
                                                      _stream_arg(stream)))
        return res

    def outline(self, name, label_spec, spec, tile0=0, n_tiles=None, stream=None):
        """dswx_batch_label chained into dswx_outline_device: the bodies of tiles tile0 .. tile0 + n_tiles - 1 (default: every
        tile from tile0) of the uint8 plane `name`, labelled by `label_spec` (a label.Spec) and traced as rings by `spec` (an
        outline.Spec), on `stream`; complete on return.  Returns {output: DeviceBuffer}: 'chain' uint32
        [n_tiles][max_edges], 'rings' uint32 [n_tiles][max_rings][8] (only with spec.max_rings > 0), 'head' uint64
        [n_tiles][8] and 'label' uint32 [n_tiles][H*W] -- device planes owned by the caller.  (The library has no
        dswx_batch_outline: the input of the outline is the caller's label plane, not a plane of the batch.)"""
        res = self.label(name, label_spec, tile0, n_tiles, want=('label',), stream=stream)
        with _owned(res, (DswxError, ValueError)):
            res.update(self.ctx.outline(res['label'], spec, self._tiles(tile0, n_tiles)[1], self.height, self.width, stream=stream))
        return res

    def burn(self, name, verts, tile_first, spec, tile0=0, n_tiles=None, want=('acc', 'head'), stream=None):
        """dswx_batch_burn: the records `verts` shared out by `tile_first` (int64 [n_tiles + 1], entry 0 = tile0) burnt INTO
        the uint8 plane `name` of tiles tile0 .. tile0 + n_tiles - 1 (default: every tile from tile0) by `spec` (a burn.Spec
        with both strides 0) -- the one entry that writes a plane of the batch; 'ocean' in front of classify() is the natural
        use.  `verts` and `tile_first` are host arrays (uploaded, the call then waits for `stream` before it frees them) or
        DeviceBuffers / device addresses (asynchronous).  Returns {output: DeviceBuffer}: 'acc' uint32 [n_tiles][H*W] always
        (the working array), 'head' uint64 [n_tiles][8] when wanted -- device planes owned by the caller.
        proteus_amd.burn.burn_tiles with src = the downloaded plane gives the same plane and the same outputs."""
        return self._rings('dswx_batch_burn', BurnSpec, name, verts, tile_first, spec, tile0, n_tiles, want, stream)

    def reach(self, name, verts, tile_first, spec, tile0=0, n_tiles=None, want=('acc', 'head'), stream=None):
        """dswx_batch_reach: the pixels of the uint8 plane `name` whose centre lies within spec.radius of an edge of the records
        become spec.burn in place (`spec` a reach.Spec with both strides 0); everything else as for burn().  burn() then
        reach() on 'ocean' is the buffered polygon.  proteus_amd.reach.reach_tiles with src = the downloaded plane gives the
        same plane and the same outputs."""
        return self._rings('dswx_batch_reach', ReachSpec, name, verts, tile_first, spec, tile0, n_tiles, want, stream)

    def _rings(self, entry, spec_struct, name, verts, tile_first, spec, tile0, n_tiles, want, stream):
        plane = _plane_index(name)
        n_tiles, nt = self._tiles(tile0, n_tiles)
        want = _burn_wanted(tuple(want) + ('acc',))
        if 'mask' in want:
            raise ValueError("'mask' is the plane of the batch here")
        res = _malloc_planes(self.ctx, {k: ((nt, BURN_HEAD_WORDS if k == 'head' else self.n_pixels), BURN_DTYPES[k]) for k in want})
        temps = []
        try:
            with _owned(res):
                if isinstance(verts, np.ndarray) or isinstance(tile_first, np.ndarray):
                    verts, tile_first, _ = _burn_input(verts, tile_first)
                    temps = [self.ctx.malloc(max(verts.nbytes, 16)), self.ctx.malloc(tile_first.nbytes)]
                    if verts.nbytes:
                        temps[0].upload(verts)
                    temps[1].upload(tile_first)
                    verts, tile_first = temps
                _check(getattr(self.ctx.lib, entry)(self.handle, plane, ctypes.c_void_p(getattr(verts, 'ptr', verts)),
                                                    ctypes.c_void_p(getattr(tile_first, 'ptr', tile_first)), ctypes.byref(spec_struct.of(spec)),
                                                    ctypes.c_void_p(res['acc'].ptr), ctypes.c_void_p(res['head'].ptr) if 'head' in res else None,
                                                    int(tile0), n_tiles, _stream_arg(stream)))
                if temps:
                    self.ctx.synchronize(stream)
        finally:
            for b in temps:
                b.free()
        return res

    def read_tile(self, name, tile):
        """Download one plane of one tile as [H,W]."""
        ptr, dt = self._plane(name)
        out = np.empty(self.n_pixels, dtype=dt)
        if out.nbytes:
            _check(self.ctx.lib.dswx_memcpy_d2h(
                self.ctx.handle, _host_ptr(out),
                ctypes.c_void_p(ptr + tile * self.tile_stride * out.itemsize), out.nbytes))
        return out.reshape(self.height, self.width)

    def write_tile(self, name, tile, arr):
        ptr, dt = self._plane(name)
        arr = np.ascontiguousarray(arr, dtype=dt).ravel()
        assert arr.size == self.n_pixels
        if arr.nbytes:
            _check(self.ctx.lib.dswx_memcpy_h2d(
                self.ctx.handle, ctypes.c_void_p(ptr + tile * self.tile_stride * arr.itemsize), _host_ptr(arr),
                arr.nbytes))

    def read_counters(self):
        out = np.empty((self.n_tiles, 3), dtype=np.int64)
        if out.nbytes:
            _check(self.ctx.lib.dswx_memcpy_d2h(self.ctx.handle, _host_ptr(out),
                                                ctypes.c_void_p(self.counters_ptr), out.nbytes))
        return out

    def write_counters_sentinel(self, value):
        """Fill the counters plane with `value` (tests: which tiles did a launch write?)."""
        arr = np.full((self.n_tiles, 3), value, dtype=np.int64)
        if arr.nbytes:
            _check(self.ctx.lib.dswx_memcpy_h2d(self.ctx.handle, ctypes.c_void_p(self.counters_ptr), _host_ptr(arr),
                                                arr.nbytes))

    def free(self):
        """dswx_batch_destroy: allowed after the context is gone (the batch remembers its device), so the HBM of a
        batch that outlives its Context is still returned."""
        if self.handle:
            self._lib.dswx_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
