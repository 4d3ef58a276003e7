/*
 * dswx_hip.h -- C ABI of the MI355X (gfx950) DSWx-HLS per-pixel classifier.
 *
 * This is the drop-in boundary for the per-pixel hot path of NASA PROTEUS
 * `src/proteus/dswx_hls.py` (reference file:line given per entry point).  The
 * reference has no FFI: its seam is the run of numpy calls inside
 * generate_dswx_layers (:5088-5112, :5225-5286, :5358-5369).  A maintainer binds
 * this library from Python with ctypes (INTEGRATION.md shows the stub) and
 * replaces that run of calls with ONE call to dswx_classify_host().
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer; no
 * allocation crosses the ABI except through dswx_device_malloc/free; every
 * function returns DSWX_OK (0) or a negative status and records a message
 * retrievable with dswx_last_error() (thread-local).  There is no CPU fallback:
 * without a HIP device dswx_ctx_create() fails with DSWX_ERR_NO_DEVICE.
 *
 * Plane layout ("band-planar batch"): every plane is [n_tiles][tile_stride] with
 * the tile's H*W pixels row-major at the start of its slot.  tile_stride defaults
 * to H*W (contiguous tiles, what the reference's seam holds).  For the full HBM rate
 * make every plane BASE 256-byte aligned (a hipMalloc pointer is) and the tile stride
 * a multiple of 8 pixels: the table-driven kernel then keeps every wave access on a
 * 128-byte line boundary on any such stride -- a 3660 x 3660 tile is 13,395,600
 * pixels = 144 mod 256, and a fixed thread -> pixel mapping would put every 1 KiB wave
 * store of tiles 1.. across partial lines (5.1 - 5.6 vs 5.7 - 6.3 TB/s, DESIGN.md
 * section 5); since ABI v5 the kernel shifts the mapping per tile instead, and a
 * stride padded to 256 pixels (dswx_batch_create's default) is no longer needed
 * for speed.  Strides that are not multiples of 8 pixels run the same kernel too (it starts every tile at its first
 * 8-pixel boundary; ABI unchanged, round 5).  Planes at ANY address (int16 planes 2-byte aligned) and, in 'cover' mode, any
 * stride take the same kernel since round 6, through unaligned 16-byte accesses: 0.59 - 0.72 of the HBM peak instead of the
 * aligned layouts' 0.75 - 0.80.
 */
#ifndef DSWX_HIP_H
#define DSWX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSWX_ABI_VERSION 7

enum {
    DSWX_OK = 0,
    DSWX_ERR_ARG = -1,          /* bad argument (NULL, size, non-finite threshold) */
    DSWX_ERR_HIP = -2,          /* a HIP runtime call failed                        */
    DSWX_ERR_NO_DEVICE = -3,    /* no usable gfx950 device                          */
    DSWX_ERR_UNSUPPORTED = -4,  /* e.g. adjacent-to-cloud mode outside 0..2          */
    DSWX_ERR_ALIGN = -5         /* device pointer not aligned for its element type  */
};

/* mask_adjacent_to_cloud_mode, dswx_hls.py:1919-1993 / :1996-2086 */
enum { DSWX_ADJ_MASK = 0, DSWX_ADJ_IGNORE = 1, DSWX_ADJ_COVER = 2 };

/* index of the counters a tile produces, dswx_hls.py:5104-5112 */
enum { DSWX_N_VALID = 0, DSWX_N_CLOUD_AND_VALID = 1, DSWX_N_NOT_OCEAN = 2,
       DSWX_N_COUNTERS = 3 };

/*
 * Everything that parameterises the chain.
 *  - the twelve doubles are HlsThresholds (dswx_hls.py:274-318, defaults
 *    defaults/dswx_hls.yaml:176-212); they must be finite.
 *  - band_fill / fmask_fill: the `image == fill_value` test of
 *    _load_hls_band_from_file (:2195-2209); NaN disables the test for a plane.
 *  - clip_negative_reflectance: FLAG_CLIP_NEGATIVE_REFLECTANCE (:31, :2298).
 *  - aerosol_fmask_lut[k][v] != 0  <=>  Fmask value v is in the runconfig list
 *    for WTR-1 class {0,2,3,4}[k] (:1249-1302, defaults yaml :77-89).
 *  - aerosol_max_nir: AEROSOL_REMAPPING_MAX_NIR (:45-46) = 1000.0.
 *  - collapse_wtr_classes: FLAG_COLLAPSE_WTR_CLASSES (:26); when set, WTR, WTR-1,
 *    WTR-1-AEROSOL and WTR-2 leave in the collapsed form the reference SAVES
 *    (_collapse_wtr_classes :2578-2598, applied at :2688-2689).
 *  - offset_and_scale_inputs: flag_offset_and_scale_inputs (CLI --offset-and-scale-inputs, :2300-2302).  When set,
 *    every clipped reflectance becomes band_scale[k] * (float32(value) - band_offset[k]) -- the `scale_factor` and
 *    `add_offset` of the band's metadata (:2295-2298) -- and the whole chain (indices, five tests, `nir <=
 *    aerosol_max_nir`, `nir > lcmask_nir`) is evaluated in float32 as numpy does on float32 arrays (thresholds rounded
 *    to float32 first: a Python float is a weak scalar against a float32 array).  The fill test stays on the raw
 *    integers.  Same kernels, the five tests in float32 (since round 5: 0.77 of the HBM peak; the production
 *    configuration leaves this off).
 *  - browse_*: the keyword arguments of _compute_browse_array (:3057-3064); the browse
 *    layer is derived from the UNCOLLAPSED WTR (PSW-aggressive is dropped before the
 *    collapse, :3112-3119), which only exists inside the kernel.
 */
typedef struct dswx_params {
    double wigt, awgt, pswt_1_mndwi, pswt_1_nir, pswt_1_swir1, pswt_1_ndvi,
           pswt_2_mndwi, pswt_2_blue, pswt_2_nir, pswt_2_swir1, pswt_2_swir2,
           lcmask_nir;
    double band_fill[6];
    double fmask_fill;
    double aerosol_max_nir;
    int32_t clip_negative_reflectance;
    int32_t mask_adjacent_to_cloud_mode;
    int32_t apply_aerosol_class_remapping;
    int32_t collapse_wtr_classes;
    /* browse layer, _compute_browse_array :3057-3129 (only read when out->browse != NULL) */
    int32_t browse_exclude_psw_aggressive;
    int32_t browse_not_water_to_nodata;
    int32_t browse_cloud_to_nodata;
    int32_t browse_snow_to_nodata;
    int32_t browse_ocean_masked_to_nodata;
    int32_t offset_and_scale_inputs;       /* ABI <= 3: reserved, zero */
    uint8_t aerosol_fmask_lut[4][256];
    double band_scale[6];                  /* only read when offset_and_scale_inputs != 0 */
    double band_offset[6];
} dswx_params_t;

/* Inputs.  band[] order: blue, green, red, nir, swir1, swir2 (raw int16 as read
 * from the HLS files, fill values still in place).  land / shad / ocean are
 * optional (NULL = layer not given): LAND codes :252-264, SHAD 0 = masked
 * (:168-169), OCEAN 0 = ocean (:5243-5245). */
typedef struct dswx_planes_in {
    const int16_t* band[6];
    const uint8_t* fmask;
    const uint8_t* land;
    const uint8_t* shad;
    const uint8_t* ocean;
} dswx_planes_in_t;

/* Outputs; any pointer may be NULL (that layer is then not produced).
 *   diag          UInt16 decimal-digit rendering, nodata 65535  (:4286-4317, :5227)
 *   wtr1          WTR-1 as SAVED, i.e. before aerosol remapping (:5229-5258)
 *   wtr1_aerosol  WTR-1 after _apply_aerosol_class_remapping    (:5260-5266)
 *   wtr2          _apply_landcover_and_shadow_masks             (:5268)
 *   wtr           _apply_cloud_masking                          (:5286)
 *   bwtr          _get_binary_water_layer                       (:5358)
 *   conf          _get_confidence_layer                         (:5368)
 *   cloud         _add_snow_to_cloud_layer                      (:5282)
 *   browse        _compute_browse_array on WTR                  (:5309-5316)
 *   mndwi/ndvi/awesh  float64 spectral indices (:1872-1887); debug planes, they
 *                 select a slower kernel variant.                                   */
typedef struct dswx_planes_out {
    uint16_t* diag;
    uint8_t* wtr1;
    uint8_t* wtr1_aerosol;
    uint8_t* wtr2;
    uint8_t* wtr;
    uint8_t* bwtr;
    uint8_t* conf;
    uint8_t* cloud;
    uint8_t* browse;
    double* mndwi;
    double* ndvi;
    double* awesh;
} dswx_planes_out_t;

/* Geometry of a device-resident batch; tile_stride in pixels, 0 = height*width. */
typedef struct dswx_batch_geom {
    int64_t n_tiles;
    int64_t height;
    int64_t width;
    int64_t tile_stride;
} dswx_batch_geom_t;

typedef struct dswx_ctx dswx_ctx_t;

/* ---- library / context ------------------------------------------------------ */
int dswx_abi_version(void);
const char* dswx_last_error(void);
int dswx_device_count(void);
int dswx_ctx_create(int device, dswx_ctx_t** out);
int dswx_ctx_destroy(dswx_ctx_t* ctx);
/* fills `p` with defaults/dswx_hls.yaml:73-101,176-212 and the constants above */
int dswx_params_default(dswx_params_t* p);

/* ---- the hot path ------------------------------------------------------------ */
/* Host-pointer entry: replaces dswx_hls.py:5089, :5110-5112, :5225-5231,
 * :5245-5249, :5261, :5268, :5282, :5286, :5358, :5368 for a batch of tiles.
 * Stages H2D, runs the fused kernel, stages D2H.  counters: [n_tiles][3] or NULL. */
int dswx_classify_host(dswx_ctx_t* ctx, const dswx_params_t* params,
                       int64_t n_tiles, int64_t height, int64_t width,
                       const dswx_planes_in_t* in, const dswx_planes_out_t* out,
                       int64_t* counters);

/* Device-pointer entry (inputs already resident in HBM): asynchronous on
 * `stream` (a hipStream_t, NULL = the context's stream).  counters: device
 * int64 [n_tiles][3] or NULL; they are zeroed on the stream first.  Mode 'cover'
 * returns DSWX_ERR_UNSUPPORTED here (no geometry): use dswx_classify_device_2d. */
int dswx_classify_device(dswx_ctx_t* ctx, const dswx_params_t* params,
                         int64_t n_tiles, int64_t n_pixels,
                         const dswx_planes_in_t* in, const dswx_planes_out_t* out,
                         int64_t* counters, void* stream);

/* Same, with the tile geometry (n_pixels = height * width).  Required for
 * mask_adjacent_to_cloud_mode 'cover' (_add_snow_to_cloud_layer :2055-2078), whose
 * masked dilations are a 2-D neighbourhood operation: the fused kernel then stops
 * before the snow step and a second, LDS-tiled kernel dilates and finishes CLOUD,
 * WTR, BWTR and CONF.  For 'mask' / 'ignore' it is identical to dswx_classify_device. */
int dswx_classify_device_2d(dswx_ctx_t* ctx, const dswx_params_t* params,
                            int64_t n_tiles, int64_t height, int64_t width,
                            const dswx_planes_in_t* in, const dswx_planes_out_t* out,
                            int64_t* counters, void* stream);

/* The general device entry: dswx_classify_device_2d plus an explicit tile stride. */
int dswx_classify_batch(dswx_ctx_t* ctx, const dswx_params_t* params,
                        const dswx_batch_geom_t* geom, const dswx_planes_in_t* in,
                        const dswx_planes_out_t* out, int64_t* counters, void* stream);

/* generate_interpreted_layer (dswx_hls.py:1687-1707) alone: `n` DIAG values in
 * decimal (0..31 -> class 0..4 per interpreted_dswx_band_dict :97-143; 32 and any
 * other value -> 255), host pointers.  This is the function the reference's unit
 * test exercises (tests/test_dswx_hls_units.py:7-28). */
int dswx_interpret_layer_host(dswx_ctx_t* ctx, const int64_t* diag_decimal, int64_t n,
                              uint8_t* out);

/* Terrain shadow layer: _compute_opera_shadow_layer (dswx_hls.py:4215-4283) followed
 * by the DEM-margin crop (_crop_2d_array_all_sides :4320, used at :5170).
 *   dem       float32 [height][width] including the margin (DEM_MARGIN_IN_PIXELS = 50, :58)
 *   shadow    uint8 [height-2*margin][width-2*margin]; 1 = not shadow, 0 = shadow
 *   sun_vector, sin_azimuth, cos_azimuth: the float64 scalars the reference derives from
 *             the sun angles (:4246-4253, :4276-4277); the caller computes them (the Python
 *             host does it with numpy exactly as the reference), so that they are
 *             bit-identical to the reference's whatever libm is in use
 *   thresholds in degrees (:4279-4281); pixel spacings as :4217 (default 30, 30).
 * float32 / float64 split of the arithmetic: see the kernel comment (numpy >= 2 promotion). */
int dswx_shadow_layer_host(dswx_ctx_t* ctx, const float* dem, int64_t height, int64_t width,
                           int64_t margin, const double sun_vector[3], double sin_azimuth,
                           double cos_azimuth, double min_slope_angle,
                           double max_sun_local_inc_angle, double pixel_spacing_x,
                           double pixel_spacing_y, uint8_t* shadow);
/* The two angle tests pulled back onto the arguments of arccos / arctan (both monotonic):
 *   degrees(arccos(q)) <= max_sun_local_inc_angle  <=>  *inc_q_min <= q <= 1
 *   degrees(arctan(t)) <= min_slope_angle          <=>  t <= *slope_arg_max
 * found by bisection over the doubles with libm.  dswx_shadow_layer_host/_device call this;
 * a caller that wants the boundary of ITS math library (the Python host uses numpy's own
 * arccos / arctan, as the reference does) computes the pair itself and calls the _q forms. */
int dswx_shadow_thresholds(double min_slope_angle, double max_sun_local_inc_angle,
                           double* slope_arg_max, double* inc_q_min);
int dswx_shadow_layer_host_q(dswx_ctx_t* ctx, const float* dem, int64_t height, int64_t width,
                             int64_t margin, const double sun_vector[3], double sin_azimuth,
                             double cos_azimuth, double slope_arg_max, double inc_q_min,
                             double pixel_spacing_x, double pixel_spacing_y, uint8_t* shadow);
int dswx_shadow_layer_device_q(dswx_ctx_t* ctx, const float* dem, int64_t n_tiles,
                               int64_t height, int64_t width, int64_t margin,
                               const double sun_vector[3], double sin_azimuth, double cos_azimuth,
                               double slope_arg_max, double inc_q_min, double pixel_spacing_x,
                               double pixel_spacing_y, uint8_t* shadow, void* stream);
/* float32 variants: the value-based casting of numpy < 2 (the reference pins numpy 1.23.5), under
 * which the float64 sun scalars do not upcast the float32 DEM arrays, so every product, sum,
 * quotient, arccos / arctan / degrees and comparison of dswx_hls.py:4264-4281 is float32 (scalars
 * rounded to float32 first).  Thresholds are float32 values located with float32 arccos / arctan
 * (proteus_amd._capi.shadow_thresholds(..., float32=True)).  The _q forms above reproduce numpy >= 2
 * (NEP 50), where those steps are float64. */
int dswx_shadow_layer_host_q32(dswx_ctx_t* ctx, const float* dem, int64_t height, int64_t width,
                               int64_t margin, const double sun_vector[3], double sin_azimuth,
                               double cos_azimuth, float slope_arg_max, float inc_q_min,
                               double pixel_spacing_x, double pixel_spacing_y, uint8_t* shadow);
int dswx_shadow_layer_device_q32(dswx_ctx_t* ctx, const float* dem, int64_t n_tiles,
                                 int64_t height, int64_t width, int64_t margin,
                                 const double sun_vector[3], double sin_azimuth, double cos_azimuth,
                                 float slope_arg_max, float inc_q_min, double pixel_spacing_x,
                                 double pixel_spacing_y, uint8_t* shadow, void* stream);
/* Device-pointer form for `n_tiles` DEMs of equal size, asynchronous on `stream`. */
int dswx_shadow_layer_device(dswx_ctx_t* ctx, const float* dem, int64_t n_tiles,
                             int64_t height, int64_t width, int64_t margin,
                             const double sun_vector[3], double sin_azimuth, double cos_azimuth,
                             double min_slope_angle, double max_sun_local_inc_angle,
                             double pixel_spacing_x, double pixel_spacing_y, uint8_t* shadow,
                             void* stream);

/* LAND layer, the per-pixel part of create_landcover_mask (dswx_hls.py:994-1115) after
 * the two GDAL warps: `worldcover_up3` is the ESA WorldCover map on the 3x finer grid
 * (uint8 [3*height][3*width]), `copernicus` the CGLS-100m map on the HLS grid (uint8
 * [height][width]).  3x3 sums of WorldCover {80,90,95} (water), 50 (urban), 10 (tree,
 * only where the CGLS class is one of `forest_classes`) -- decimate_by_summation
 * :874-904 -- then the hierarchy of :1058-1103 with `thresholds` = [evergreen,
 * low-intensity developed, high-intensity developed, water] (landcover_threshold_dict
 * :270-271) and year_offset = WorldCover year - 2000.  land: uint8 [height][width]. */
int dswx_landcover_mask_host(dswx_ctx_t* ctx, const uint8_t* worldcover_up3,
                             const uint8_t* copernicus, int64_t height, int64_t width,
                             const int32_t* forest_classes, int32_t n_forest_classes,
                             const int32_t thresholds[4], int32_t year_offset, uint8_t* land);

/* Device-pointer form for `n_tiles` map pairs of equal size ([n_tiles][3H][3W] and
 * [n_tiles][H][W]), asynchronous on `stream`. */
int dswx_landcover_mask_device(dswx_ctx_t* ctx, const uint8_t* worldcover_up3,
                               const uint8_t* copernicus, int64_t n_tiles, int64_t height,
                               int64_t width, const int32_t* forest_classes,
                               int32_t n_forest_classes, const int32_t thresholds[4],
                               int32_t year_offset, uint8_t* land, void* stream);

/* The two layer kernels writing straight into the SHAD / LAND planes of a resident batch: as the _device forms, with the
 * distance between the output rasters of consecutive tiles given explicitly (bytes = pixels; 0 = packed rasters;
 * dswx_batch_geom_t.tile_stride of the batch whose plane `shadow` / `land` is).  dswx_shadow_layer_batch takes the
 * pulled-back thresholds like the _q / _q32 forms (float32_arithmetic != 0: slope_arg_max and inc_q_min hold float32
 * values, numpy < 2 promotion). */
int dswx_shadow_layer_batch(dswx_ctx_t* ctx, const float* dem, int64_t n_tiles, int64_t height,
                            int64_t width, int64_t margin, const double sun_vector[3], double sin_azimuth,
                            double cos_azimuth, double slope_arg_max, double inc_q_min,
                            int32_t float32_arithmetic, double pixel_spacing_x, double pixel_spacing_y,
                            uint8_t* shadow, int64_t shadow_tile_stride, void* stream);
int dswx_landcover_mask_batch(dswx_ctx_t* ctx, const uint8_t* worldcover_up3, const uint8_t* copernicus,
                              int64_t n_tiles, int64_t height, int64_t width,
                              const int32_t* forest_classes, int32_t n_forest_classes,
                              const int32_t thresholds[4], int32_t year_offset, uint8_t* land,
                              int64_t land_tile_stride, void* stream);

/* Deterministic synthetic HLS tiles written straight into HBM (SURVEY.md §8d;
 * same integer recipe as proteus_amd/synth.py).  Fills in->band[0..5], in->fmask
 * and whichever of land/shad/ocean is non-NULL for tiles tile0..tile0+n_tiles-1. */
int dswx_synth_fill(dswx_ctx_t* ctx, uint64_t seed, int64_t tile0, int64_t n_tiles,
                    int64_t height, int64_t width, const dswx_planes_in_t* in,
                    void* stream);

/* dswx_synth_fill with an explicit tile stride. */
int dswx_synth_batch(dswx_ctx_t* ctx, uint64_t seed, int64_t tile0,
                     const dswx_batch_geom_t* geom, const dswx_planes_in_t* in, void* stream);

/* ---- resident batches: allocation and placement of the planes (ABI v4) ---------
 * The seam at dswx_hls.py:5225-5286 works on arrays the caller already holds; a service that keeps a
 * batch of tiles resident in HBM (bench.py, proteus_amd/batch.py) needs them allocated -- and on MI355X
 * WHERE the seven output planes lie decides between 0.71 and 0.80 of the HBM peak for the same launch
 * (the rate follows the position of the write streams in the address space, with
 * a 32-GiB structure; round 3 looked for a layout RULE and found none that holds from one process to
 * the next -- profiles/r03_placement_rule_trials.json).  dswx_batch_create allocates the planes of a
 * batch (one hipMalloc, packed, unless a flag says otherwise); dswx_batch_place_slide (what bench.py uses)
 * and dswx_batch_place_search are the opt-in measured placements, so the placed rate is available to
 * every caller of this ABI, not to a Python helper only. */
typedef struct dswx_batch dswx_batch_t;

/* plane indices of dswx_batch_layout_t */
enum {
    DSWX_PLANE_BAND0 = 0,      /* blue, green, red, nir, swir1, swir2 = 0..5 (int16) */
    DSWX_PLANE_FMASK = 6,
    DSWX_PLANE_LAND = 7, DSWX_PLANE_SHAD = 8, DSWX_PLANE_OCEAN = 9,          /* DSWX_BATCH_MASKS */
    DSWX_PLANE_DIAG = 10,      /* uint16 */
    DSWX_PLANE_WTR1 = 11, DSWX_PLANE_WTR1_AEROSOL = 12, DSWX_PLANE_WTR2 = 13, DSWX_PLANE_WTR = 14,
    DSWX_PLANE_BWTR = 15, DSWX_PLANE_CONF = 16, DSWX_PLANE_CLOUD = 17, DSWX_PLANE_BROWSE = 18,
    DSWX_PLANE_COUNTERS = 19,  /* int64 [n_tiles][3] */
    DSWX_BATCH_MAX_PLANES = 20
};

/* flags of dswx_batch_create / dswx_batch_layout */
enum {
    DSWX_BATCH_MASKS = 1 << 0,            /* LAND, SHAD, OCEAN input planes (BASELINE config 5) */
    DSWX_BATCH_WTR1_AEROSOL = 1 << 1,     /* optional output planes */
    DSWX_BATCH_BROWSE = 1 << 2,
    /* layout: default = ONE allocation, inputs then outputs back to back (what a plain caller does) */
    DSWX_BATCH_SEPARATE_OUTPUTS = 1 << 10, /* one allocation for the inputs, one per output plane: what
                                              dswx_batch_place_search needs */
    DSWX_BATCH_SLIDING_OUTPUTS = 1 << 11   /* the output planes packed in a range of the virtual address space that
                                              is backed chunk by chunk (HIP virtual memory management): what
                                              dswx_batch_place_slide needs */
};

typedef struct dswx_batch_layout {
    int64_t tile_stride;                              /* pixels, as resolved (see dswx_batch_create) */
    uint64_t arena_bytes;                             /* the single allocation (SEPARATE_OUTPUTS: the inputs') */
    uint64_t plane_bytes[DSWX_BATCH_MAX_PLANES];      /* 0 = plane absent */
    uint64_t plane_offset[DSWX_BATCH_MAX_PLANES];     /* inside the arena (SEPARATE_OUTPUTS: 0 for outputs;
                                                         SLIDING_OUTPUTS: inside the output region) */
    uint64_t write_span_bytes;                        /* first byte of the first to last byte of the last
                                                         output plane (0 with SEPARATE_OUTPUTS) */
} dswx_batch_layout_t;

typedef struct dswx_batch_info {
    dswx_batch_geom_t geom;           /* tile_stride resolved */
    uint32_t flags;
    int32_t n_allocations;
    uint64_t bytes_allocated;         /* HBM the batch holds */
    /* record of the last dswx_batch_place_search (zeros if none ran) */
    int32_t search_candidates;
    int32_t search_probes;            /* probe measurements taken (each `launches` launches) */
    float first_come_launch_ms;       /* the planes as first allocated ... */
    float kept_launch_ms;             /* ... and as kept, timed back to back at the end of the search */
    /* ABI v5: address space (DSWX_BATCH_SLIDING_OUTPUTS; see dswx_batch_va_budget) */
    uint64_t va_reserved_bytes;       /* the reservation this batch's output range lives in (0: no range) */
    uint64_t va_retired_bytes;        /* process-wide: address space of dropped ranges, reserved and empty for good */
    uint64_t va_budget_bytes;         /* process-wide limit on reserved + retired address space */
    uint64_t va_pooled_bytes;         /* process-wide: physical chunks of dropped ranges kept for later ranges */
    char note[256];                   /* "" or why a sliding batch was allocated packed / why the last
                                         dswx_batch_place_slide left the planes where they were */
} dswx_batch_info_t;

/* n_tiles of dswx_batch_classify: every resident tile (ABI v5; up to v4 this was spelled 0, which made an empty last
 * chunk of a walk re-classify the whole batch -- 0 is now what it says: no tiles, no work) */
#define DSWX_BATCH_ALL_TILES (-1)

/* The layout rule alone (pure function, no device needed): where dswx_batch_create would put every
 * plane.  geom->tile_stride 0 = height*width rounded up to a multiple of 256 pixels (every tile of
 * every plane then starts on a 256-byte boundary: the fast kernel, see the top of this file); any
 * other value is taken as given (>= height*width).  Plane offsets are 256-byte aligned. */
int dswx_batch_layout(const dswx_batch_geom_t* geom, uint32_t flags, dswx_batch_layout_t* out);

/* DSWX_BATCH_SLIDING_OUTPUTS on a device without HIP virtual memory management: DSWX_ERR_UNSUPPORTED.  If the address
 * range cannot be had -- hipMemAddressReserve refuses, or the library's address-space budget is spent
 * (dswx_batch_va_budget) -- the batch is allocated PACKED (as without the flag) and dswx_batch_info_t.note says why;
 * dswx_batch_info_t.flags shows the layout in effect.  dswx_batch_place_slide on such a batch times the planes where they
 * are and succeeds (search_probes 0). */
int dswx_batch_create(dswx_ctx_t* ctx, const dswx_batch_geom_t* geom, uint32_t flags,
                      dswx_batch_t** out);
/* Frees every allocation of the batch.  A batch must not be USED after its context is destroyed; destroying it
 * afterwards is allowed. */
int dswx_batch_destroy(dswx_batch_t* batch);
/* Address space and memory of the sliding ranges (ABI v5).  Two properties of HIP virtual memory management on ROCm 7.2 /
 * gfx950 (plain-HIP reproducers: tools/vmm_reuse_repro.hip, tools/lab/vmm_meminfo.hip):
 *   (1) an address that a kernel has accessed through one mapping must never be mapped onto other physical memory -- the
 *       kernel's translation stays stale and its stores go to the released memory;
 *   (2) the physical memory of a chunk that was ever mapped returns to the device only when the address RESERVATION it was
 *       mapped in is freed.
 * By default the library therefore RETIRES every sliding range it drops: the addresses stay reserved, empty, for the life
 * of the process (`retired_bytes`; `live_bytes` = reserved by ranges in use), and the physical chunks go into a process-wide
 * POOL (`pooled_bytes`) from which later batches and placements of the same chunk size are built before new memory is
 * created -- nothing is ever exposed to reuse, and a service that re-creates or re-places batches reuses its own memory.
 * dswx_batch_pool_trim() gives the pooled memory back to the device: it releases the chunks, frees every retired
 * reservation -- which is what returns the memory -- and reserves the same addresses again at once, empty.  Between those
 * two calls the addresses are up for grabs by other threads of the process: call it when none of them allocates (a range
 * lost that way is counted in `loose_bytes` and is out of the library's control).  Batches may be LIVE during a trim,
 * placed ones included: a kept placement's chunks were once mapped in the (now retired) wide range whose reservation the trim
 * frees, and that was measured to be harmless (tests/test_gpu_parity.py::test_pool_trim_while_a_placed_batch_is_live;
 * profiles/r05_trim_live_probe.json).  The library never trims by itself, not even when an allocation fails: the error
 * text of dswx_batch_create then says how many bytes the pool holds.  Chunk sizes are powers of two (2 MiB ... 1 GiB), so
 * batches of different geometry share the pool.
 * Address space is consumed for good: 100 - 160 GiB per placed batch at 256 tiles of 3660 x 3660 (the first-come range, the
 * wide range and, when the batch goes, the range of the kept chunks), so the default BUDGET of 64 TiB (half of the 47-bit
 * space) lasts 400 - 650 placements.  When live + retired + a new request would pass the budget the library reserves no
 * more: sliding batches fall back as described at dswx_batch_create.
 * new_budget_bytes 0 = leave the budget as it is; any output pointer may be NULL.  Process-wide, thread-safe. */
int dswx_batch_va_budget(uint64_t new_budget_bytes, uint64_t* budget_bytes, uint64_t* live_bytes,
                         uint64_t* retired_bytes, uint64_t* loose_bytes, uint64_t* pooled_bytes);
int dswx_batch_pool_trim(uint64_t* released_bytes);
/* Device pointers of the planes (absent planes NULL), the resolved geometry and the counters array
 * ([n_tiles][3] int64); any output argument may be NULL.  Hand them to dswx_classify_batch /
 * dswx_synth_batch, or use the two conveniences below. */
int dswx_batch_planes(const dswx_batch_t* batch, dswx_batch_geom_t* geom, dswx_planes_in_t* in,
                      dswx_planes_out_t* out, int64_t** counters);
int dswx_batch_info(const dswx_batch_t* batch, dswx_batch_info_t* info);
/* dswx_classify_batch over the first `n_tiles` resident tiles (DSWX_BATCH_ALL_TILES = all, 0 = none), counters
 * included. */
int dswx_batch_classify(dswx_batch_t* batch, const dswx_params_t* params, int64_t n_tiles,
                        void* stream);
/* dswx_synth_batch into the resident input planes: tiles tile0 .. tile0 + n_tiles - 1. */
int dswx_batch_synth(dswx_batch_t* batch, uint64_t seed, int64_t tile0, void* stream);
/* Opt-in, measured placement (DSWX_BATCH_SEPARATE_OUTPUTS batches whose inputs are resident): beside
 * every output plane `candidates - 1` spare allocations are made (as many sets as fit while
 * `keep_free_bytes` of device memory stay free), and one pass of coordinate descent binds each plane in
 * turn (DIAG first) to the candidate under which `launches` launches of the real kernel run fastest;
 * the chosen and the first-come planes are then timed back to back and the better set is kept.  The
 * spares are freed.  Output pointers change: call dswx_batch_planes again.  Synchronous. */
int dswx_batch_place_search(dswx_batch_t* batch, const dswx_params_t* params, int32_t candidates,
                            int32_t launches, uint64_t keep_free_bytes);
/* The cheaper measured placement (DSWX_BATCH_SLIDING_OUTPUTS batches whose inputs are resident).  The rate follows
 * the POSITION of the packed output region in the address space with a structure of ~32 GiB, so
 * one dimension is enough: a range `slack_bytes` longer than the output planes is mapped beside the current one
 * (bounded so that `keep_free_bytes` of device memory stay free), the kernel is timed (`launches` launches) with the
 * output region at offsets 0, step_bytes, 2 step_bytes, ... of it, the best position and the first-come range are
 * then timed back to back, and the better one is kept: the chunks (physical memory) under the chosen position move into a
 * fresh address range of their own, the wide range is dropped (its other chunks go to the library's pool, see
 * dswx_batch_va_budget / dswx_batch_pool_trim); the moved planes are timed once more and kept only if they still beat the
 * first-come range.  After the packed positions `spread_gaps` more
 * candidates are tried: the planes spread over the range with equal gaps of 1/spread_gaps ... 1 x the largest gap that
 * fits (0 = packed positions only).  `refine_passes` passes of refinement follow: from the best candidate, every
 * plane in turn (DIAG first) tries the other free places of the range on a grid of 2 step_bytes and keeps the best
 * (the per-plane freedom of dswx_batch_place_search without its spare allocations; ~12 probes per plane and pass).
 * slack / step + 1 + spread_gaps probes without refinement (25 + 4 at 48 GiB / 2 GiB:
 * about 1 s for 256 tiles) and slack_bytes of transient memory, against 185 probes and five spare sets of planes
 * for dswx_batch_place_search.  Output pointers change: call dswx_batch_planes again.  Synchronous.
 * (Every placement retires the address ranges it drops: see dswx_batch_va_budget.  When the
 * wide range cannot be reserved or mapped the planes stay where they are, the call succeeds and dswx_batch_info_t.note
 * says why.) */
int dswx_batch_place_slide(dswx_batch_t* batch, const dswx_params_t* params, uint64_t slack_bytes,
                           uint64_t step_bytes, int32_t spread_gaps, int32_t refine_passes,
                           int32_t launches, uint64_t keep_free_bytes);

/* ---- the raster formats either side of the path (ABI v6) --------------------------------
 * The reference reads and saves every raster through GDAL.  Reading a band file is inflate -> inverse predictor ->
 * blocks into the raster (`ReadAsArray` in _load_hls_band_from_file, dswx_hls.py:2136-2302); saving a layer is
 * `save_as_cog` (core.py:7-91): NEAREST overviews 4 / 16 / 64 / 128 for the integer layers (:37-46), 512 x 512 blocks,
 * PREDICTOR=2 (integers) / 3 (floating point), DEFLATE (:60-75); the RGB composites are
 * scale * (float32(band) - offset) with NaN on invalid pixels (_save_output_rgb_file, dswx_hls.py:3013-3036).
 * Compression stays on the host (include/dswx_codec.h); the byte shuffling between an inflated block and the
 * classifier's planes, and between its layers and the blocks to deflate, runs on the device with these entries.
 * All pointers are DEVICE pointers; asynchronous on `stream` (NULL = the context's stream).  Every plane and index array is
 * aligned to its samples (any such address: no larger alignment is asked for), `blocks` of dswx_cog_blocks_device to 16
 * bytes; a pointer that is not is refused with DSWX_ERR_ALIGN before anything is launched (dswx_copy_2d_device moves
 * bytes and takes any address). */
#define DSWX_COG_MAX_LEVELS 8
typedef struct dswx_cog_layout {
    int32_t n_levels;                                /* the full-resolution image + the overview levels */
    int32_t tile;
    int32_t factor[DSWX_COG_MAX_LEVELS];             /* 1, then the factors that produce a level */
    int64_t height[DSWX_COG_MAX_LEVELS];             /* ceil(N / factor), what GDAL makes an overview */
    int64_t width[DSWX_COG_MAX_LEVELS];
    int32_t blocks_down[DSWX_COG_MAX_LEVELS];
    int32_t blocks_across[DSWX_COG_MAX_LEVELS];
    uint64_t offset_bytes[DSWX_COG_MAX_LEVELS];      /* of the level's first block in the blocked buffer */
    uint64_t total_bytes;
} dswx_cog_layout_t;
/* Where dswx_cog_blocks_device puts what (pure function, no device needed).  A factor of 1, or any factor on a 1 x 1
 * raster, produces no level (the host writer's rule). */
int dswx_cog_layout(int64_t height, int64_t width, int32_t elem_bytes, int32_t tile, const int32_t* factors,
                    int32_t n_factors, dswx_cog_layout_t* out);
/* One plane [height][width] -> `blocks`: for every level of dswx_cog_layout, its tile x tile blocks in row-major block
 * order, edge blocks zero-padded, each block row predictor-encoded and little endian -- exactly the bytes the TIFF writer
 * hands to DEFLATE.  elem_bytes 1 / 2: integer samples, predictor 1 (none) or 2 (horizontal differencing in the sample's
 * width), overview levels by GDAL's NEAREST rule (src = min(int(0.5 + dst * N / N_ovr), N - 1), restated from
 * GDALResampleChunk_Near: GDAL is not in the reference tree, parity of the rule itself is unpinned).  elem_bytes 4:
 * Float32 with predictor 3 (TIFF Technical Note 3), one level per call: the reference's overviews of a Float32 layer are
 * CUBICSPLINE -- build each level with dswx_convolve_axis_device (two passes) and pass it here on its own. */
int dswx_cog_blocks_device(dswx_ctx_t* ctx, const void* plane, int32_t elem_bytes, int64_t height, int64_t width,
                           int32_t tile, const int32_t* factors, int32_t n_factors, int32_t predictor, void* blocks,
                           void* stream);
/* The inverse for a file being read: `blocks` = every block of one plane of an image, inflated, in block order, each
 * block_height x block_width samples (tiles; or strips: block_width = width, the short last strip's slot padded), native
 * byte order; elem_bytes 1 / 2 / 4 with predictor 1 (none) or 2 (running sum in the sample's width), or elem_bytes 4 with
 * predictor 3 (Float32, TIFF Technical Note 3: what GDAL writes for a Float32 DEM with PREDICTOR=3).  -> plane [height][width].
 * Predictor 3 goes through a scratch of the context: such calls of one context are ordered across streams (a call on
 * another stream than the previous one waits for it, as the classifier's launches do); predictors 1 and 2 are not. */
int dswx_untile_device(dswx_ctx_t* ctx, const void* blocks, int32_t elem_bytes, int64_t height, int64_t width,
                       int32_t block_width, int32_t block_height, int32_t predictor, void* plane, void* stream);
/* One separable pass of the CUBICSPLINE overview convolution `save_as_cog` asks GDAL for on non-integer layers
 * (core.py:41-46; restated from GDAL's GDALResampleChunk_Convolution in proteus_amd/geotiff.py: _convolve_axis -- GDAL is not
 * in the reference tree, last-ulp agreement of the float results is unpinned): for every line r < n_lines and output
 * position j < n_out, dst = sum_k src[r, clamp(first[j] + k, 0, n_in - 1)] * weights[k * n_out + j], normalised over the taps whose
 * sample is not NaN; NaN if none is left.  Accumulation in float64 in tap order.  Strides in elements, so that the same entry
 * does the horizontal pass (lines = rows) and the vertical one (lines = columns); src / dst float32 or float64; `first`
 * (int32 [n_out]) and `weights` (float64 [taps][n_out]) are DEVICE arrays the host prepares. */
int dswx_convolve_axis_device(dswx_ctx_t* ctx, const void* src, int32_t src_is_f64, int64_t n_lines, int64_t n_in,
                              int64_t src_line_stride, int64_t src_elem_stride, int64_t n_out, int32_t taps,
                              const int32_t* first, const double* weights, void* dst, int32_t dst_is_f64,
                              int64_t dst_line_stride, int64_t dst_elem_stride, void* stream);
/* Rows of `width_bytes` bytes from one device raster to another (hipMemcpy2DAsync, device to device): the crop of a DEM
 * with its margin to the product grid (_crop_2d_array_all_sides, dswx_hls.py:4320) without a trip to the host. */
int dswx_copy_2d_device(dswx_ctx_t* ctx, void* dst, size_t dst_pitch_bytes, const void* src, size_t src_pitch_bytes,
                        size_t width_bytes, size_t height, void* stream);
/* out[c][i] = scale[c] * (float32(band_c[i], clipped to >= 1 if clip_negative_reflectance) - offset[c]) in float32, NaN
 * where diag[i] == 65535 (diag may be NULL: no masking); out = float [3][n_pixels]. */
int dswx_rgb_planes_device(dswx_ctx_t* ctx, const int16_t* red, const int16_t* green, const int16_t* blue,
                           const uint16_t* diag, int64_t n_pixels, const double scale[3], const double offset[3],
                           int32_t clip_negative_reflectance, float* out, void* stream);
/* A plane as GDAL stores it in a Byte band (save_dswx_product creates all ten bands of the multi-band file as GDT_Byte,
 * dswx_hls.py:2663-2666, so DIAG and DEM saturate there): src_kind 1 uint16 / 2 int16: clamped to 0 .. 255; 3 float32:
 * NaN -> 0, clamped, rounded half up (GDALCopyWords; GDAL is not in the reference tree: the rule is GDAL's documented
 * conversion, unpinned by execution). */
int dswx_to_byte_device(dswx_ctx_t* ctx, const void* src, int32_t src_kind, int64_t n, uint8_t* dst, void* stream);
/* dst[i][j] = src[rows[i]][cols[j]] (rows / cols: DEVICE int32 arrays of source indices, which the caller guarantees to lie
 * inside src_height x src_width): the nearest-neighbour resampling of the browse image (geotiff2png after
 * _compute_browse_array, dswx_hls.py:5335-5349; GDAL RasterIO's pick src = floor((dst + 0.5) * N_src / N_dst), which the host
 * evaluates -- proteus_amd/geotiff.py: resample_nearest) on a plane that stays in HBM; only the small image crosses PCIe. */
int dswx_gather_2d_device(dswx_ctx_t* ctx, const void* src, int32_t elem_bytes, int64_t src_height, int64_t src_width,
                          const int32_t* rows, int32_t n_rows, const int32_t* cols, int32_t n_cols, void* dst, void* stream);

/* ---- checksums: what a plane contains, one 64-bit word per tile (ABI v7) ------------------------------------------
 * A resident batch holds tens of gigabytes of layers in HBM; these entries say what is in them without the planes
 * crossing PCIe: compare a resident tile with a file, a host array, an earlier run or another rank's copy by comparing
 * eight bytes.  THE DEFINITION (independent of address, alignment, tile stride, launch geometry and device) -- for one
 * tile of n elements of b bytes (b = 1, 2, 4 or 8):
 *   take the n b bytes of the tile in memory order and split them into m = ceil(n b / 8) little-endian 64-bit words
 *   w_0 .. w_(m-1); word 0 starts at element 0 of the tile whatever its address, the last word is zero-padded;
 *       C = mix(n b) + sum over g of mix(w_g + (g + 1) K)        (mod 2^64)
 *   K = DSWX_CHECKSUM_K (odd), and mix is the splitmix64 finaliser
 *       x ^= x >> 30;  x *= DSWX_CHECKSUM_M1;  x ^= x >> 27;  x *= DSWX_CHECKSUM_M2;  x ^= x >> 31      (mod 2^64)
 *   n = 0 is legal: C = mix(0) = 0.
 * Properties (tests/test_checksum.py):
 *   - the sum is commutative: any order of blocks and of their atomic adds gives the same value -- the device entries are
 *     deterministic;
 *   - mix is a bijection of the 64-bit words (xor-shifts and odd multiplies are): a change confined to ONE 8-byte word
 *     ALWAYS changes C;
 *   - the position key sits INSIDE the non-linear mix: transposed, shifted or row-swapped data is not cancelled linearly
 *     (a linear form sum of w_g odd(g) misses a swap of the top bytes of two words 128 apart).
 * Changes that touch several words are detected with probability 1 - 2^-64 under the usual heuristic; this is an
 * integrity check against mistakes, not a cryptographic hash. */
#define DSWX_CHECKSUM_K 0x9E3779B97F4A7C15ULL
#define DSWX_CHECKSUM_M1 0xBF58476D1CE4E5B9ULL
#define DSWX_CHECKSUM_M2 0x94D049BB133111EBULL
/* One plane [n_tiles][tile_stride_elems] of elem_bytes-wide elements in DEVICE memory -> out[n_tiles] (device uint64: the
 * checksum of the first n_elems elements of every tile; the bytes between n_elems and the stride are not read).
 * Asynchronous on `stream` (NULL = the context's stream), no synchronisation inside: out is zeroed on the stream, then one
 * kernel adds into it.  tile_stride_elems 0 = n_elems.  `plane` off its element alignment (or `out` off 8 bytes):
 * DSWX_ERR_ALIGN, as the raster-format entries; elem_bytes not 1 / 2 / 4 / 8, a negative size or tile count, a stride below
 * n_elems, or a NULL pointer with n_tiles > 0: DSWX_ERR_ARG.  (The arguments are checked before the context is.) */
int dswx_checksum_device(dswx_ctx_t* ctx, const void* plane, int32_t elem_bytes, int64_t n_tiles, int64_t n_elems,
                         int64_t tile_stride_elems, uint64_t* out_device_u64, void* stream);
/* The planes of a resident batch selected by `plane_mask` (bit k = plane DSWX_PLANE_k: inputs, layers, extra layers, and
 * DSWX_PLANE_COUNTERS as [n_tiles][3] int64), tiles tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the
 * last), the height x width pixels of every tile -> out[popcount(plane_mask)][n_tiles] in HOST memory, planes in ascending
 * index order, complete on return.  ONE kernel launch for all selected planes, on `stream`; the addresses are those of
 * dswx_batch_planes, so packed, separate-output and placed batches are alike.  A plane the batch does not have:
 * DSWX_ERR_ARG, and dswx_last_error() names it.  (The device words live in an allocation made and freed by the call.) */
int dswx_batch_checksum(dswx_batch_t* batch, uint32_t plane_mask, int64_t tile0, int64_t n_tiles, uint64_t* out_host_u64,
                        void* stream);
/* The same definition on a HOST buffer in plain scalar C++: needs no device and no context.  The other half of a
 * comparison -- the expected value of a host array or a decoded file -- not a fallback of the two entries above. */
int dswx_checksum_host(const void* data, size_t n_bytes, uint64_t* out_u64);

/* ---- compare: where two planes differ, in how many elements and by how much (additive to ABI v7) ---------------------
 * A checksum says THAT a resident tile differs; these entries say where, in how many elements and by how much, again
 * without a plane crossing PCIe: 32 bytes per tile come back.  A C caller tests for them with DSWX_HAS_COMPARE.
 * THE DEFINITION.  Two planes a, b of the same element kind (DSWX_CMP_*), each [n_tiles][tile_stride] with its OWN stride
 * and address; only the first n_elems elements of a tile are read, the padding up to the stride never is.  An element pair
 * (x, y) = (a[i], b[i]) is CLOSE when numpy's isclose(a, b, rtol, atol, equal_nan) says so -- operation by operation:
 *   integer kinds   |x - y| <= atol + rtol |y| evaluated in double (both values convert exactly);
 *   DSWX_CMP_F64    the same test in double;
 *   DSWX_CMP_F32    all in float32, as numpy evaluates it for float32 arrays against Python-float tolerances: atol and rtol
 *                   are rounded to float32 first, d = |x - y| is ONE float32 subtraction, tol = atol32 + rtol32 |y| a float32
 *                   multiply, then a float32 add (no contraction into a fused multiply-add); close iff d <= tol and y is finite;
 *   float kinds, in addition: x == y is close (equal infinities, -0 against +0), and a pair of NaNs is close iff equal_nan.
 *   rtol = atol = 0 is value equality.
 * Per tile the result is one record:
 *   n_diff        the number of pairs that are not close;
 *   first         the smallest flat element index within the tile that is not close, -1 if there is none;
 *   max_abs_diff  the maximum of |double(x) - double(y)| over the not-close pairs in which neither value is NaN: 0.0 when
 *                 there is no such pair, +inf when an infinity is involved;
 *   reserved      zero.
 * The three are a sum, a minimum and a maximum of non-negative doubles (which are ordered as their bit patterns): all
 * order-independent, so the device entries are deterministic whatever the order of the blocks and of their atomics. */
#define DSWX_HAS_COMPARE 1
enum { DSWX_CMP_U8 = 0, DSWX_CMP_U16 = 1, DSWX_CMP_I16 = 2, DSWX_CMP_F32 = 3, DSWX_CMP_F64 = 4, DSWX_CMP_KINDS = 5 };
typedef struct dswx_compare {
    int64_t n_diff;
    int64_t first;
    double max_abs_diff;
    uint64_t reserved;
} dswx_compare_t;
/* Two planes in DEVICE memory -> out[n_tiles] (device records).  Asynchronous on `stream` (NULL = the context's stream), no
 * synchronisation inside: the records are initialised on the stream, then one kernel fills them.  A stride of 0 = n_elems;
 * a == b is legal.  `kind` not a DSWX_CMP_* value, a negative size or tile count, a stride below n_elems, a NULL pointer
 * with n_tiles > 0, atol or rtol negative or not finite: DSWX_ERR_ARG; a plane off its element alignment, or `out` off 8
 * bytes: DSWX_ERR_ALIGN.  (The arguments are checked before the context is.) */
int dswx_compare_device(dswx_ctx_t* ctx, const void* a, const void* b, int32_t kind, int64_t n_tiles, int64_t n_elems,
                        int64_t a_stride_elems, int64_t b_stride_elems, double atol, double rtol, int32_t equal_nan,
                        dswx_compare_t* out_device_records, void* stream);
/* The planes selected by `plane_mask` (bit k = plane DSWX_PLANE_k: inputs, layers, extra layers) of TWO resident batches,
 * tiles tile0 .. tile0 + n_tiles - 1 of both (n_tiles DSWX_BATCH_ALL_TILES = up to the last tile of batch_a), the height x
 * width pixels of every tile -> out[popcount(plane_mask)][n_tiles] records in HOST memory, planes in ascending index order,
 * complete on return.  ONE kernel launch for all selected planes, on `stream` (NULL = the stream of batch_a's context); the
 * kinds come from the library's plane table (bands int16, DIAG uint16, the rest uint8), the addresses are those of
 * dswx_batch_planes, so packed, separate-output, placed, padded and contiguous batches mix freely.  The batches must be on
 * the same device and have equal height and width (their strides may differ): otherwise DSWX_ERR_ARG.  A plane that either
 * batch lacks: DSWX_ERR_ARG, and dswx_last_error() names it.  DSWX_PLANE_COUNTERS in the mask: DSWX_ERR_ARG (twenty-four
 * bytes per tile: compare their checksums, or the counters themselves).  batch_a == batch_b is legal. */
int dswx_batch_compare(dswx_batch_t* batch_a, dswx_batch_t* batch_b, uint32_t plane_mask, int64_t tile0, int64_t n_tiles,
                       double atol, double rtol, int32_t equal_nan, dswx_compare_t* out_host_records, void* stream);
/* The same definition on two HOST buffers in plain scalar C++: needs no device and no context.  The other half of a
 * comparison -- what the record of a host array against a decoded file is -- not a fallback of the two entries above. */
int dswx_compare_host(const void* a, const void* b, int32_t kind, int64_t n_elems, double atol, double rtol,
                      int32_t equal_nan, dswx_compare_t* out_record);

/* ---- histogram: how much of each value a plane holds, 256 counts per tile (additive to ABI v7) ------------------------
 * A checksum says that a resident tile is what it should be, a comparison where two differ; these entries say what is IN a
 * tile -- how many pixels are open water, partial water, snow, cloud, ocean-masked or fill, how often each of the five
 * diagnostic tests fired, how the reflectances of a band are distributed -- again without the plane crossing PCIe: 2 KiB per
 * tile and plane come back.  A C caller tests for them with DSWX_HAS_HISTOGRAM.
 * THE DEFINITION.  One record per tile and plane is uint64_t bins[DSWX_HIST_BINS].  Only the first n_elems elements of a tile
 * are counted, the padding up to the tile stride is never read.  The bin of an element v follows the plane's `kind`:
 *   DSWX_HIST_U8                    (uint8 planes)  bin = the byte;
 *   DSWX_HIST_U16, DSWX_HIST_I16    (uint16 / int16 planes)  linear, with `lo` (int32) and `shift` (0 .. 8): d = (int32)v - lo
 *                                   as an integer; if 0 <= d < (256 << shift) the element is counted in bin d >> shift,
 *                                   otherwise it is NOT COUNTED -- the bins sum to the number of elements in range;
 *   DSWX_HIST_DIAG                  (uint16 planes in the saved DIAG form: the decimal digits of v are the five test bits,
 *                                   _get_binary_representation, dswx_hls.py:4286-4317)  if every decimal digit of v is 0 or 1
 *                                   and v <= 11111: bin = d0 + 2 d1 + 4 d2 + 8 d3 + 16 d4 (0 .. 31, d0 the units digit);
 *                                   v == 65535 (nodata): bin 32; any other value: bin 33.  Bins 34 .. 255 stay zero.
 * `lo` and `shift` are ignored for DSWX_HIST_U8 and DSWX_HIST_DIAG (a shift outside 0 .. 8 is refused for every kind).
 * The counts are integer sums: they do not depend on the order of the blocks or of their atomic adds, so the device entries
 * are deterministic. */
#define DSWX_HAS_HISTOGRAM 1
#define DSWX_HIST_BINS 256
enum { DSWX_HIST_U8 = 0, DSWX_HIST_U16 = 1, DSWX_HIST_I16 = 2, DSWX_HIST_DIAG = 3, DSWX_HIST_KINDS = 4 };
/* One plane [n_tiles][tile_stride_elems] in DEVICE memory -> out[n_tiles][DSWX_HIST_BINS] (device uint64).  Asynchronous on
 * `stream` (NULL = the context's stream), no synchronisation inside: out is zeroed on the stream, then one kernel adds into
 * it.  tile_stride_elems 0 = n_elems.  `kind` not a DSWX_HIST_* value, `shift` outside 0 .. 8, a negative size, tile count or
 * stride, a stride below n_elems, or a NULL pointer with n_tiles > 0: DSWX_ERR_ARG; a plane off its element alignment, or
 * `out` off 8 bytes: DSWX_ERR_ALIGN.  (The arguments are checked before the context is; the limits on the size of a plane
 * are those of dswx_compare_device.) */
int dswx_histogram_device(dswx_ctx_t* ctx, const void* plane, int32_t kind, int32_t lo, int32_t shift, int64_t n_tiles,
                          int64_t n_elems, int64_t tile_stride_elems, uint64_t* out_device_u64, void* stream);
/* The planes of a resident batch selected by `plane_mask` (bit k = plane DSWX_PLANE_k: inputs, layers, extra layers), tiles
 * tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last), the height x width pixels of every tile ->
 * out[popcount(plane_mask)][n_tiles][DSWX_HIST_BINS] in HOST memory, planes in ascending index order, complete on return.
 * ONE kernel launch for all selected planes, on `stream`; the addresses are those of dswx_batch_planes, so packed,
 * separate-output and placed batches are alike.  The kinds come from the library's plane table: the six bands are
 * DSWX_HIST_I16 with band_lo / band_shift (0 and 6: reflectances 0 .. 16383 in bins of 64), DIAG is DSWX_HIST_DIAG, every
 * other plane DSWX_HIST_U8.  DSWX_PLANE_COUNTERS in the mask: DSWX_ERR_ARG.  A plane the batch does not have: DSWX_ERR_ARG,
 * and dswx_last_error() names it.  (The device words live in an allocation made and freed by the call.) */
int dswx_batch_histogram(dswx_batch_t* batch, uint32_t plane_mask, int64_t tile0, int64_t n_tiles, int32_t band_lo,
                         int32_t band_shift, uint64_t* out_host_u64, void* stream);
/* The same definition on a HOST buffer (any address) in plain scalar C++: needs no device and no context.  The other half
 * of a comparison -- the counts of a host array or a decoded file -- not a fallback of the two entries above.
 * out_u64_256 = uint64_t [DSWX_HIST_BINS], 8-byte aligned. */
int dswx_histogram_host(const void* data, int32_t kind, int32_t lo, int32_t shift, int64_t n_elems, uint64_t* out_u64_256);

/* ---- crosstab: how the classes of one plane fall into the classes of another, 256 cells per tile (additive to ABI v7) ---
 * A histogram says how much of each class ONE plane holds; marginals do not determine a joint table, so these entries read
 * TWO planes in step and count their joint classes -- which WTR-2 classes cloud masking turned into snow or cloud, what a
 * changed threshold moved between "not water" and "partial surface water", how a band is distributed inside open water and
 * outside it, the confusion matrix of a product against a validation map -- again without a plane crossing PCIe: 2 KiB per
 * tile and pair come back.  A C caller tests for them with DSWX_HAS_CROSSTAB.
 * THE DEFINITION.  A and B are two planes, each [n_tiles][its own tile stride] at its own address; only the first n_elems
 * elements of a tile are read, the padding up to the stride never.  Plane A is of any histogram kind (a_kind = DSWX_HIST_U8 /
 * U16 / I16 / DIAG, with a_lo and a_shift as in the histogram section); plane B is always uint8.  col_bits is 0 .. 8: there
 * are C = 1 << col_bits columns and R = 256 >> col_bits rows.  For the element pair (x, y) = (A[i], B[i]):
 *   bin = the histogram bin of x exactly as the histogram section defines it (bin < 0: not counted);
 *   row = row_of_bin[bin], col = col_of_byte[y];
 *   the pair is counted in cells[row * C + col] iff bin >= 0, row < R and col < C; otherwise it is NOT COUNTED.
 * One record per tile (and pair) is uint64_t cells[DSWX_CROSSTAB_CELLS]: the 2-KiB record of a histogram.  The counts are
 * integer sums, so the device entries are deterministic.  It follows that
 *   - col_bits 0, col_of_byte all zero, row_of_bin the identity: the record IS dswx_histogram's record of A;
 *   - col_bits 8, row_of_bin all zero, col_of_byte the identity: the U8 histogram of B over the pairs whose A element is counted;
 *   - where nothing is excluded the row sums are the histogram of row_of_bin[bin(A)], the column sums that of col_of_byte[B]. */
#define DSWX_HAS_CROSSTAB 1
#define DSWX_CROSSTAB_CELLS 256
#define DSWX_CROSSTAB_MAX_PAIRS 6 /* per dswx_batch_crosstab call: the tables ride in the 4 KiB of kernel arguments */
typedef struct dswx_crosstab_spec {
    int32_t a_kind;           /* DSWX_HIST_* of plane A */
    int32_t a_lo, a_shift;    /* DSWX_HIST_U16 / DSWX_HIST_I16 (a shift outside 0 .. 8 is refused for every kind) */
    int32_t col_bits;         /* 0 .. 8 */
    uint8_t row_of_bin[256];  /* a value >= 256 >> col_bits: the bin is not counted */
    uint8_t col_of_byte[256]; /* a value >= 1 << col_bits: the byte is not counted */
} dswx_crosstab_spec_t;       /* 528 bytes */
typedef struct dswx_crosstab_pair {
    int32_t plane_a;          /* DSWX_PLANE_* of batch_a */
    int32_t plane_b;          /* DSWX_PLANE_* of batch_b: a uint8 plane */
    dswx_crosstab_spec_t spec;
} dswx_crosstab_pair_t;       /* 536 bytes */
/* Planes a [n_tiles][a_stride_elems] and b [n_tiles][b_stride_elems] in DEVICE memory -> out[n_tiles][DSWX_CROSSTAB_CELLS]
 * (device uint64).  Asynchronous on `stream` (NULL = the context's stream), no synchronisation inside: out is zeroed on the
 * stream, then one kernel adds into it; the spec's tables travel in the kernel arguments.  A stride of 0 = n_elems; a == b
 * is legal.  a_kind not a DSWX_HIST_* value, a_shift outside 0 .. 8, col_bits outside 0 .. 8, a NULL spec, a negative size,
 * tile count or stride, a stride below n_elems, or a NULL plane with n_tiles > 0: DSWX_ERR_ARG; plane a off its element
 * alignment, or `out` off 8 bytes: DSWX_ERR_ALIGN.  (The arguments are checked before the context is; the limits on the
 * size of a plane are those of dswx_compare_device.) */
int dswx_crosstab_device(dswx_ctx_t* ctx, const void* a, const uint8_t* b, const dswx_crosstab_spec_t* spec, int64_t n_tiles,
                         int64_t n_elems, int64_t a_stride_elems, int64_t b_stride_elems, uint64_t* out_device_u64,
                         void* stream);
/* pairs[k].plane_a of batch_a against pairs[k].plane_b of batch_b (batch_a == batch_b is legal: WTR-1 against WTR-2 of one
 * batch), tiles tile0 .. tile0 + n_tiles - 1 of both (n_tiles DSWX_BATCH_ALL_TILES = up to the last of batch_a), the height x
 * width pixels of every tile -> out[n_pairs][n_tiles][DSWX_CROSSTAB_CELLS] in HOST memory, complete on return.  ONE kernel
 * launch for all pairs, on `stream`; at most DSWX_CROSSTAB_MAX_PAIRS pairs, more: DSWX_ERR_ARG.  spec.a_kind must agree with
 * the library's plane table -- a band takes DSWX_HIST_I16, DIAG takes DSWX_HIST_DIAG or DSWX_HIST_U16, every other plane
 * DSWX_HIST_U8 -- and plane_b must be a uint8 plane: otherwise DSWX_ERR_ARG, and dswx_last_error() names the plane.  Devices,
 * tile sizes, tile ranges, missing planes and DSWX_PLANE_COUNTERS: the rules of dswx_batch_compare.  (The device words live
 * in an allocation made and freed by the call.) */
int dswx_batch_crosstab(dswx_batch_t* batch_a, dswx_batch_t* batch_b, const dswx_crosstab_pair_t* pairs, int32_t n_pairs,
                        int64_t tile0, int64_t n_tiles, uint64_t* out_host_u64, void* stream);
/* The same definition on HOST buffers (any address) in plain scalar C++: needs no device and no context.
 * out_u64_256 = uint64_t [DSWX_CROSSTAB_CELLS], 8-byte aligned. */
int dswx_crosstab_host(const void* a, const uint8_t* b, const dswx_crosstab_spec_t* spec, int64_t n_elems,
                       uint64_t* out_u64_256);

/* ---- stack: the tiles of a plane composited per pixel -- counts, latest observation, share (additive to ABI v7) ----------
 * Checksum, compare, histogram and crosstab reduce WITHIN a tile; these entries reduce ACROSS the tiles of a plane, pixel by
 * pixel.  When the tiles are the dates of one MGRS tile that is how often a pixel was water out of the times it was observed
 * at all, its latest clear observation with the clouds filled from earlier dates, and the date that observation came from --
 * without a WTR plane crossing PCIe: the results are planes in device memory, to be checksummed, histogrammed or written.  A C
 * caller tests for the entries with DSWX_HAS_STACK.
 * THE DEFINITION.  A stack is one uint8 plane [n_tiles][tile_stride] at any address; only the first n_elems bytes of a tile
 * are read, the padding up to the stride never.  The tile index t is time order.  For pixel i, with
 * c(t) = cat_of_byte[stack[t][i]]:
 *   count[k][i]    the number of tiles t with c(t) == k, for k < n_cats (a count[k] pointer with k >= n_cats must be NULL);
 *   n_obs          the sum of count[k][i] over k; t* the largest t with c(t) < n_cats;
 *   last[i]        stack[t*][i], and last_index[i] = t*; where n_obs == 0 they are `fill` and DSWX_STACK_NONE;
 *   share[i]       (100 * count[0][i]) / n_obs in integer division (category 0 is the category of interest); where
 *                  n_obs == 0 it is DSWX_STACK_NO_SHARE.
 * n_tiles <= DSWX_STACK_MAX_TILES, so a count fits its uint16 and a real index never equals DSWX_STACK_NONE.  n_tiles == 0 is
 * legal and writes the no-observation values; n_elems == 0 writes nothing.  All of it is integer arithmetic per pixel: the
 * result is deterministic and independent of the launch geometry. */
#define DSWX_HAS_STACK 1
#define DSWX_STACK_MAX_CATS 4
#define DSWX_STACK_MAX_TILES 65535
#define DSWX_STACK_NONE 65535          /* last_index of a pixel no tile observed */
#define DSWX_STACK_NO_SHARE 255        /* share of a pixel no tile observed */
typedef struct dswx_stack_spec {
    int32_t n_cats;                    /* 1 .. DSWX_STACK_MAX_CATS */
    int32_t fill;                      /* 0 .. 255: `last` of a pixel no tile observed */
    uint8_t cat_of_byte[256];          /* category of a byte; a value >= n_cats: the byte is NOT AN OBSERVATION */
} dswx_stack_spec_t;                   /* 264 bytes */
typedef struct dswx_stack_out {        /* planes of n_elems elements each; any pointer may be NULL = not wanted */
    uint16_t* count[DSWX_STACK_MAX_CATS];
    uint8_t*  last;
    uint16_t* last_index;
    uint8_t*  share;
} dswx_stack_out_t;
/* One stack [n_tiles][tile_stride_elems] in DEVICE memory -> the wanted planes of *out_device (device memory, n_elems
 * elements each).  Asynchronous on `stream` (NULL = the context's stream): ONE kernel launch, no synchronisation, no scratch
 * of the context.  tile_stride_elems 0 = n_elems.  A NULL spec or out struct, n_cats outside 1 .. 4, fill outside 0 .. 255, a
 * negative size, tile count or stride, a stride below n_elems, n_tiles > DSWX_STACK_MAX_TILES, a NULL stack with n_tiles > 0
 * and n_elems > 0, a count[k] pointer with k >= n_cats, or every output NULL: DSWX_ERR_ARG; a count[k] or last_index pointer
 * off 2 bytes: DSWX_ERR_ALIGN.  The stack and the byte outputs take any address.  (The arguments are checked before the
 * context is, and a refused call writes nothing; the limits on the size of a plane are those of dswx_compare_device.)
 * The output planes MUST NOT OVERLAP the stack or each other: that is NOT CHECKED. */
int dswx_stack_device(dswx_ctx_t* ctx, const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems,
                      int64_t tile_stride_elems, const dswx_stack_out_t* out_device, void* stream);
/* Plane `plane` (a uint8 DSWX_PLANE_* of the library's plane table: Fmask, the masks, every layer but DIAG) of a resident
 * batch, tiles tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last) as the stack -> the wanted planes
 * of *out_device: device planes of height x width elements owned by the caller.  Asynchronous on `stream` (NULL = the stream
 * of the batch's context) like dswx_stack_device.  The address and the stride are those of dswx_batch_planes, so packed,
 * separate-output, placed, padded and contiguous batches are alike.  A plane that is not uint8 (the bands, DIAG), a plane the
 * batch does not have, or DSWX_PLANE_COUNTERS: DSWX_ERR_ARG, and dswx_last_error() names the plane.  Tile ranges: the rules
 * of dswx_batch_compare. */
int dswx_batch_stack(dswx_batch_t* batch, int32_t plane, const dswx_stack_spec_t* spec, int64_t tile0, int64_t n_tiles,
                     const dswx_stack_out_t* out_device, void* stream);
/* The same definition on HOST buffers in plain scalar C++: needs no device and no context.  The other half of a comparison,
 * not a fallback of the two entries above.  The refusals of dswx_stack_device, except that every buffer, the uint16 ones
 * included, may sit at any address. */
int dswx_stack_host(const uint8_t* stack, const dswx_stack_spec_t* spec, int64_t n_tiles, int64_t n_elems,
                    int64_t tile_stride_elems, const dswx_stack_out_t* out_host);

/* ---- grid: a plane aggregated onto a coarse grid -- per-cell category counts, share, coverage, majority (additive to ABI v7)
 * Checksum, compare, histogram and crosstab reduce a tile as a flat run of elements and stack reduces across tiles; none of
 * them knows that a tile is a height x width raster.  These entries do: they aggregate every tile onto cells of cell_h x
 * cell_w pixels -- the water fraction of 900 m cells of a 30 m WTR layer, the fraction of each cell that was observed at all,
 * and a majority overview that keeps class bytes legal without throwing pixels away -- without the plane crossing PCIe.  The
 * results are small planes in device memory, [n_tiles][GH * GW], to be histogrammed, cross-tabulated, stacked or written.  A C
 * caller tests for the entries with DSWX_HAS_GRID.
 * THE DEFINITION.  A plane is uint8 [n_tiles][tile_stride] at any address.  The first height * width bytes of a tile are its
 * raster, rows contiguous with a row pitch of `width`; the padding up to the stride is never read.  The grid has
 * GH = ceil(height / cell_h) rows and GW = ceil(width / cell_w) columns of cells; cell (gy, gx) covers the rows gy * cell_h ..
 * min(height, (gy + 1) * cell_h) - 1 and the columns gx * cell_w .. min(width, (gx + 1) * cell_w) - 1, so the last row and the
 * last column of cells are ragged, and n_pix is the number of pixels a cell really covers.  For every tile and cell, with
 * c(p) = cat_of_byte[byte at pixel p] (the table of a stack spec, unchanged):
 *   count[k]   the number of pixels p of the cell with c(p) == k, for k < n_cats (a count[k] pointer with k >= n_cats must be
 *              NULL);
 *   n_obs      the sum of count[k] over k;
 *   share      (100 * count[0]) / n_obs in integer division (category 0 is the category of interest); DSWX_GRID_NO_SHARE
 *              where n_obs == 0;
 *   coverage   (100 * n_obs) / n_pix in integer division: 0 .. 100;
 *   major      the smallest k whose count is the largest; DSWX_GRID_NONE where n_obs == 0.
 * min(cell_h, height) * min(cell_w, width) <= DSWX_GRID_MAX_CELL_PIXELS, so 100 * count fits 32 bits and a whole 3660 x 3660
 * tile may be ONE cell (for one cell per tile dswx_batch_histogram gives the same counts faster: a cell belongs to one
 * workgroup here).  n_tiles == 0 or an empty raster writes nothing.  All of it is integer arithmetic: the result is
 * deterministic and independent of the launch geometry. */
#define DSWX_HAS_GRID 1
#define DSWX_GRID_MAX_CATS 4
#define DSWX_GRID_MAX_CELL_PIXELS (1 << 24)
#define DSWX_GRID_NO_SHARE 255         /* share of a cell without an observation */
#define DSWX_GRID_NONE 255             /* major of a cell without an observation */
typedef struct dswx_grid_spec {
    int32_t n_cats;                    /* 1 .. DSWX_GRID_MAX_CATS */
    int32_t cell_h, cell_w;            /* >= 1 */
    uint8_t cat_of_byte[256];          /* category of a byte; a value >= n_cats: the byte is NOT AN OBSERVATION */
} dswx_grid_spec_t;                    /* 268 bytes */
typedef struct dswx_grid_out {         /* planes [n_tiles][GH * GW], dense; any pointer may be NULL = not wanted */
    uint32_t* count[DSWX_GRID_MAX_CATS];
    uint8_t*  share;
    uint8_t*  coverage;
    uint8_t*  major;
} dswx_grid_out_t;
/* One plane [n_tiles][tile_stride_elems] in DEVICE memory -> the wanted planes of *out_device (device memory, n_tiles x GH x
 * GW elements each).  Asynchronous on `stream` (NULL = the context's stream): ONE kernel launch, no synchronisation, no scratch
 * of the context, nothing zeroed in front.  tile_stride_elems 0 = height * width.  A NULL spec or out struct, n_cats outside
 * 1 .. 4, a cell size below 1, a cell of more than DSWX_GRID_MAX_CELL_PIXELS pixels, a negative size, tile count or stride, a
 * stride below height * width, a NULL plane with something to read, a count[k] pointer with k >= n_cats, or every output
 * NULL: DSWX_ERR_ARG; a count[k] pointer off 4 bytes: DSWX_ERR_ALIGN.  The plane and the byte outputs take any address.  (The
 * arguments are checked before the context is, and a refused call writes nothing; height and width are at most 2^30, the
 * limits on the size of a plane are those of dswx_compare_device.)  The output planes MUST NOT OVERLAP the plane or each
 * other: that is NOT CHECKED. */
int dswx_grid_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height,
                     int64_t width, int64_t tile_stride_elems, const dswx_grid_out_t* out_device, void* stream);
/* Plane `plane` (a uint8 DSWX_PLANE_* of the library's plane table: Fmask, the masks, every layer but DIAG) of a resident
 * batch, tiles tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last) -> the wanted planes of
 * *out_device: device planes of n_tiles x GH x GW elements owned by the caller, output tile 0 = tile0.  Asynchronous on
 * `stream` (NULL = the stream of the batch's context) like dswx_grid_device.  The address and the stride are those of
 * dswx_batch_planes, so packed, separate-output, placed, padded and contiguous batches are alike.  A plane that is not uint8
 * (the bands, DIAG), a plane the batch does not have, or DSWX_PLANE_COUNTERS: DSWX_ERR_ARG, and dswx_last_error() names the
 * plane.  Tile ranges: the rules of dswx_batch_compare. */
int dswx_batch_grid(dswx_batch_t* batch, int32_t plane, const dswx_grid_spec_t* spec, int64_t tile0, int64_t n_tiles,
                    const dswx_grid_out_t* out_device, void* stream);
/* The same definition on HOST buffers in plain scalar C++: needs no device and no context.  The other half of a comparison,
 * not a fallback of the two entries above.  The refusals of dswx_grid_device, except that every buffer, the uint32 ones
 * included, may sit at any address. */
int dswx_grid_host(const uint8_t* plane, const dswx_grid_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                   int64_t tile_stride_elems, const dswx_grid_out_t* out_host);

/* ---- label: the connected bodies of a plane -- per-pixel label and body size, a sieved copy, a summary (additive to ABI v7)
 * Every entry above treats a pixel on its own or in a fixed rectangle.  A surface-water product is about water BODIES: how
 * many lakes a tile holds, how large each is, which one-pixel specks are noise.  These entries label the connected bodies of
 * every tile of a plane without the plane crossing PCIe; the results are planes in device memory that dswx_histogram_device,
 * dswx_checksum_device and dswx_grid_device accept.  A C caller tests for the entries with DSWX_HAS_LABEL.
 * THE DEFINITION.  A plane is uint8 [n_tiles][tile_stride] at any address.  The first height * width bytes of a tile are its
 * raster, rows contiguous with a row pitch of `width`; the padding up to the stride is never read.  Pixel p is a MEMBER iff
 * member_of_byte[byte at p] != 0.  Two members are ADJACENT when they are neighbours in the 4-neighbourhood (connectivity 4)
 * or the 8-neighbourhood (connectivity 8) of the same tile; rows do not wrap -- (y, width - 1) and (y + 1, 0) are not
 * neighbours -- and tiles never connect.  A BODY is a maximal set of members connected through adjacency.  Per tile, with
 * idx(p) = y * width + x:
 *   label[p]    uint32: 0 for a non-member, else 1 + the smallest idx(q) over the body of p.  This is the order in which
 *               scipy.ndimage.label numbers bodies WITHOUT the renumbering to 1 .. K: renumbering is deliberately not done
 *               here (the labels of a tile are distinct and ordered, not dense);
 *   size[p]     uint32: 0 for a non-member, else the number of pixels of the body of p;
 *   sieved[p]   uint8: the input byte, except that a member whose body has fewer than min_size pixels becomes `replace`;
 *               min_size == 1 copies.  (GDAL's sieve lets a removed body adopt the value of its largest neighbour; this rule
 *               is simpler: one replacement byte);
 *   summary     uint64 [DSWX_LABEL_SUMMARY_WORDS] per tile: word 0 bodies; 1 member pixels; 2 the largest size; 3 the label of
 *               the largest body (the smallest label on a tie, 0 when there is none); 4 bodies with size >= min_size; 5 the
 *               pixels in those bodies; 6, 7 zero; 8 + b, b = 0 .. 31, the bodies with floor(log2(size)) == b.
 * height * width <= 2^31, so that a label fits 32 bits.  n_tiles == 0 or an empty raster writes nothing.  All of it is
 * integer arithmetic: the result is deterministic and independent of the launch geometry and of the order in which atomics
 * arrive. */
#define DSWX_HAS_LABEL 1
#define DSWX_LABEL_SUMMARY_WORDS 40
typedef struct dswx_label_spec {
    int32_t connectivity;              /* 4 or 8 */
    int32_t replace;                   /* 0 .. 255: the byte of a sieved-out member */
    uint32_t min_size;                 /* >= 1 */
    uint8_t member_of_byte[256];       /* != 0: a pixel with this byte is a member */
} dswx_label_spec_t;                   /* 268 bytes */
typedef struct dswx_label_out {        /* planes [n_tiles][height * width], dense; summary [n_tiles][40] */
    uint32_t* label;                   /* REQUIRED: it is the working array of the union-find */
    uint32_t* size;                    /* required whenever sieved or summary is wanted; else NULL = not wanted */
    uint8_t*  sieved;                  /* NULL = not wanted */
    uint64_t* summary;                 /* NULL = not wanted */
} dswx_label_out_t;
/* One plane [n_tiles][tile_stride_elems] in DEVICE memory -> the wanted planes of *out_device (device memory).  Asynchronous
 * on `stream` (NULL = the context's stream): at most five kernel launches (label a rectangle in LDS; unite across the seams of
 * the rectangles; flatten and count; broadcast the sizes, sieve and summarise; unpack the summary's largest-body key) plus one
 * hipMemsetAsync of `summary`; no synchronisation, no scratch of the context, no allocation, and nothing the caller has to
 * zero in front: a second call on the same outputs gives the same result.  No workgroup ever waits for another.
 * tile_stride_elems 0 = height * width.  A NULL spec or out struct, a connectivity that is not 4 or 8, `replace` outside
 * 0 .. 255, min_size == 0, a negative size, tile count or stride, a stride below height * width, height * width above 2^31, a
 * NULL plane with something to read, a NULL label, or a NULL size with sieved or summary wanted: DSWX_ERR_ARG; label or size
 * off 4 bytes or summary off 8: DSWX_ERR_ALIGN.  The plane and `sieved` take any address.  (The arguments are checked before
 * the context is, and a refused call writes nothing; the limits on the size of a plane are those of dswx_compare_device.)
 * The outputs MUST NOT OVERLAP the plane or each other: that is NOT CHECKED. */
int dswx_label_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height,
                      int64_t width, int64_t tile_stride_elems, const dswx_label_out_t* out_device, void* stream);
/* Plane `plane` (a uint8 DSWX_PLANE_* of the library's plane table: Fmask, the masks, every layer but DIAG) of a resident
 * batch, tiles tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last) -> the wanted planes of
 * *out_device: device planes owned by the caller, output tile 0 = tile0.  Asynchronous on `stream` (NULL = the stream of the
 * batch's context) like dswx_label_device.  The address and the stride are those of dswx_batch_planes, so packed,
 * separate-output, placed, padded and contiguous batches are alike.  A plane that is not uint8 (the bands, DIAG), a plane the
 * batch does not have, or DSWX_PLANE_COUNTERS: DSWX_ERR_ARG, and dswx_last_error() names the plane.  Tile ranges: the rules
 * of dswx_batch_compare. */
int dswx_batch_label(dswx_batch_t* batch, int32_t plane, const dswx_label_spec_t* spec, int64_t tile0, int64_t n_tiles,
                     const dswx_label_out_t* out_device, void* stream);
/* The same definition on HOST buffers: a plain scalar union-find in C++, needs no device and no context.  The other half of
 * a comparison, not a fallback of the two entries above.  The refusals of dswx_label_device, except that every buffer, the
 * uint32 and uint64 ones included, may sit at any address. */
int dswx_label_host(const uint8_t* plane, const dswx_label_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                    int64_t tile_stride_elems, const dswx_label_out_t* out_host);

/* ---- body table: the labelled bodies of a plane renumbered 1 .. K and tabulated, one 64-byte row per body (additive to ABI v7)
 * The label entries above leave per-pixel planes and a 40-word summary; the question after labelling is per BODY: how many
 * lakes, and for each where it is, how large, how long its shoreline, how much of it open or partial water -- or cloud on
 * another date.  These entries answer it without the 4-byte label plane crossing PCIe, and give the dense renumbering that
 * the label entries deliberately left out, so that per-body arrays can be indexed on the device.  The first entries here
 * whose output size depends on the data.  A C caller tests for them with DSWX_HAS_BODY_TABLE.
 * THE DEFINITION.  Per tile, `label` is a uint32 plane [n_tiles][height * width], dense, as dswx_label_device leaves it: 0 for
 * a non-member, else 1 + the smallest pixel index of the body; `value` an optional uint8 plane [n_tiles][value_stride] at any
 * address whose padding is never read.  The spec: n_cats 0 .. DSWX_BODY_MAX_CATS; cat_of_byte[256] in the convention of
 * dswx_stack_spec_t (an entry >= n_cats: the byte is not counted); value == NULL if and only if n_cats == 0; max_rows >= 0
 * is the capacity of the table per tile.  With idx(p) = y * width + x, a pixel with L = label[p] != 0 is WELL-FORMED iff
 * L <= idx(p) + 1 and label[L - 1] == L.  Every other non-zero pixel is MALFORMED: it belongs to no body, gets dense 0 and is
 * only counted in the head.  The entries never read outside the tile for ANY content of `label`: the bound on L is checked
 * before the dependent load, so a label plane taken before its last launch, or a caller's garbage, is legal input.  The ROOTS
 * are the pixels with label[p] == idx(p) + 1, K is their number, rank(r) the number of roots with a smaller index.
 *   dense[p]   uint32: 0 for label 0 or a malformed pixel, else 1 + rank(label[p] - 1).  For a plane from dswx_label_* this is
 *              exactly the array that scipy.ndimage.label returns.  REQUIRED: it is the working array of the prefix sum;
 *   rows       [n_tiles][max_rows] rows of DSWX_BODY_ROW_WORDS uint32 (64 bytes; the 64-bit fields at even words); row k is
 *              the body with dense == k + 1, for k < min(K, max_rows):
 *                word 0 label; 1 area (pixels); 2, 3 x_min, x_max; 4, 5 y_min, y_max; 6-7 perimeter (uint64); 8-9 sum_x
 *                (uint64); 10-11 sum_y (uint64); 12 .. 15 count[c]: the pixels of the body with cat_of_byte[value at p] == c
 *                for c < n_cats, else 0.
 *              The perimeter counts the pairs (pixel of the body, one of its four edge directions) whose neighbour is outside
 *              the tile or holds a different label VALUE; rows do not wrap; uint64 because a checkerboard body of 2^30 pixels
 *              has 2^32 edges.  The centroid is sum / area, left to the caller so that everything stays integer.  Rows
 *              min(K, max_rows) .. max_rows - 1 are all zero.  Bodies of rank >= max_rows have no row, but their dense
 *              values and their share of the head are complete: a table that is too small is truncated, never wrong (and K
 *              is known beforehand from word 0 of the label summary);
 *   head       uint64 [n_tiles][DSWX_BODY_HEAD_WORDS]: word 0 K; 1 min(K, max_rows); 2 well-formed member pixels; 3 malformed
 *              pixels; 4 the sum of the perimeters of all K bodies; 5 .. 7 zero.
 * rows and head may each be NULL = not wanted; rows NULL requires max_rows == 0.  height * width <= 2^31.  n_tiles == 0 or an
 * empty raster writes nothing.  All of it is integer arithmetic: the result is deterministic and independent of the launch
 * geometry and of the order in which atomics arrive. */
#define DSWX_HAS_BODY_TABLE 1
#define DSWX_BODY_ROW_WORDS 16
#define DSWX_BODY_HEAD_WORDS 8
#define DSWX_BODY_MAX_CATS 4
typedef struct dswx_body_spec {
    int64_t max_rows;                  /* 0 .. 2^31: rows of the table per tile */
    int32_t n_cats;                    /* 0 .. DSWX_BODY_MAX_CATS */
    uint8_t cat_of_byte[256];          /* category of a value byte; >= n_cats: not counted */
} dswx_body_spec_t;                    /* 272 bytes */
typedef struct dswx_body_out {
    uint32_t* dense;                   /* [n_tiles][height * width]; REQUIRED: it is the working array of the prefix sum */
    uint32_t* rows;                    /* [n_tiles][max_rows][16]; NULL = not wanted (max_rows must be 0 then) */
    uint64_t* head;                    /* [n_tiles][8]; NULL = not wanted */
} dswx_body_out_t;
/* One label plane and an optional value plane [n_tiles][value_stride_elems] in DEVICE memory -> the wanted outputs of
 * *out_device (device memory).  Asynchronous on `stream` (NULL = the context's stream): four kernel launches (count the roots
 * of every chunk of 4096 elements into dense itself; scan those counts per tile; rank the roots and begin their rows;
 * tabulate a rectangle per workgroup, equal bodies combined per thread, wave and workgroup before any atomic) plus one hipMemsetAsync each of `rows` and
 * `head`; no synchronisation, no scratch of the context, no allocation, and nothing the caller has to zero in front: a second
 * call on the same outputs gives the same bytes.  No workgroup ever waits for another: the prefix sum is reduce, scan of the
 * partials, apply, as successive launches.  value_stride_elems 0 = height * width.  A NULL spec or out struct, n_cats outside
 * 0 .. 4, a value plane with n_cats == 0 or none with n_cats > 0, a negative size, tile count, stride or max_rows, a stride
 * below height * width, height * width above 2^31, a NULL dense, a NULL label with something to read, NULL rows with
 * max_rows > 0, or max_rows above 2^31: DSWX_ERR_ARG; label or dense off 4 bytes or rows or head off 8: DSWX_ERR_ALIGN.  The
 * value plane takes any address.  (The arguments are checked before the context is, and a refused call writes nothing; the
 * limits on the size of a plane are those of dswx_compare_device.)  The outputs MUST NOT OVERLAP the inputs or each other:
 * that is NOT CHECKED. */
int dswx_body_table_device(dswx_ctx_t* ctx, const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec,
                           int64_t n_tiles, int64_t height, int64_t width, int64_t value_stride_elems,
                           const dswx_body_out_t* out_device, void* stream);
/* The same for tiles tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last) of a resident batch:
 * `value_plane` is a uint8 DSWX_PLANE_* of the library's plane table, or -1 for none (n_cats == 0); `label_device` is the
 * dense label plane [n_tiles][height * width] of the SAME tile range in device memory owned by the caller, for instance the
 * `label` of dswx_batch_label; output tile 0 = tile0.  The address and the stride of the value plane are those of
 * dswx_batch_planes.  A plane that is not uint8 (the bands, DIAG), a plane the batch does not have, or DSWX_PLANE_COUNTERS:
 * DSWX_ERR_ARG, and dswx_last_error() names the plane.  Tile ranges: the rules of dswx_batch_compare. */
int dswx_batch_body_table(dswx_batch_t* batch, int32_t value_plane, const dswx_body_spec_t* spec, int64_t tile0, int64_t n_tiles,
                          const uint32_t* label_device, const dswx_body_out_t* out_device, void* stream);
/* The same definition on HOST buffers in plain scalar C++: needs no device and no context.  The other half of a comparison,
 * not a fallback of the two entries above.  The refusals of dswx_body_table_device, except that every buffer, the uint32 and
 * uint64 ones included, may sit at any address. */
int dswx_body_table_host(const uint32_t* label, const uint8_t* value, const dswx_body_spec_t* spec, int64_t n_tiles,
                         int64_t height, int64_t width, int64_t value_stride_elems, const dswx_body_out_t* out_host);

/* ---- distance: the exact Euclidean distance of every pixel to the nearest target of a plane (additive to ABI v7)
 * The entries above say what a plane holds, per pixel, per cell and per body.  These say HOW FAR: for every pixel the squared
 * distance to the nearest water (or cloud, or any set of bytes), which target that is, the ring of pixels within a radius of
 * a shoreline, and a per-tile summary -- without the plane crossing PCIe; the results are planes in device memory that
 * dswx_histogram_device and dswx_checksum_device accept, and `nearest` looked up in a `label` plane of dswx_label_device says
 * which body a pixel is nearest to.  A C caller tests for the entries with DSWX_HAS_DISTANCE.
 * THE DEFINITION.  A plane is uint8 [n_tiles][tile_stride] at any address.  The first height * width bytes of a tile are its
 * raster, rows contiguous with a row pitch of `width`; the padding up to the stride is never read.  Rows do not wrap and tiles
 * never see each other.  Pixel q is a TARGET iff target_of_byte[byte at q] != 0.  With idx(p) = y * width + x,
 * d2(p, q) = (yp - yq)^2 + (xp - xq)^2 and R = max_radius (0 = unbounded), a target q REACHES p when R == 0 or
 * d2(p, q) <= R * R.  Per tile:
 *   dist2[p]    uint32: the minimum of d2(p, q) over the targets that reach p; 0 on a target; DSWX_DISTANCE_NONE when no
 *               target reaches p, which includes a tile without targets.  For R == 0 and a tile with a target this is the
 *               square of scipy.ndimage.distance_transform_edt of the non-targets, exactly.  REQUIRED: it is the working
 *               array between the launches;
 *   nearest[p]  uint32: idx(q) of the target that attains it; ties go to the smallest column, then the smallest row, that is,
 *               lexicographic in (d2, xq, yq) -- the tie a separable transform produces naturally: the column pass ties
 *               upward, the row pass ties leftward.  DSWX_DISTANCE_NONE where dist2 is;
 *   within[p]   uint8: the input byte, except that a non-target p with dist2[p] != DSWX_DISTANCE_NONE becomes `mark`: the
 *               buffer ring.  Only meaningful with R > 0: wanted with R == 0 is refused;
 *   summary     uint64 [DSWX_DISTANCE_SUMMARY_WORDS] per tile: word 0 targets; 1 reached non-target pixels; 2 pixels not
 *               reached; 3 the largest dist2 among reached pixels (0 when none); 4 idx of the pixel holding it (the smallest
 *               idx on a tie, 0 when none); 5 the sum of dist2 over reached pixels; 6, 7 zero; 8 + b, b = 0 .. 31, the reached
 *               non-target pixels with floor(log2(dist2)) == b.
 * height and width are each at most 46340, so that (height - 1)^2 + (width - 1)^2 stays below DSWX_DISTANCE_NONE;
 * height * width <= 2^31; width <= DSWX_DISTANCE_MAX_WIDTH: the row pass keeps one whole row of the working array in LDS,
 * 4 bytes a pixel plus three words per 64 columns, which at 8192 columns is 34 KiB a workgroup -- four workgroups (sixteen
 * waves) stay resident in the 160 KiB of a compute unit.  n_tiles == 0 or an empty raster writes nothing.  All of it is
 * integer arithmetic: the result is deterministic and independent of the launch geometry and of the order in which atomics
 * arrive. */
#define DSWX_HAS_DISTANCE 1
#define DSWX_DISTANCE_NONE 0xFFFFFFFFu
#define DSWX_DISTANCE_SUMMARY_WORDS 40
#define DSWX_DISTANCE_MAX_WIDTH 8192
#define DSWX_DISTANCE_MAX_SIDE 46340
typedef struct dswx_distance_spec {
    uint32_t max_radius;               /* R in pixels; 0 = unbounded */
    int32_t mark;                      /* 0 .. 255: the byte of a reached non-target in `within` */
    uint8_t target_of_byte[256];       /* != 0: a pixel with this byte is a target */
} dswx_distance_spec_t;                /* 264 bytes */
typedef struct dswx_distance_out {     /* planes [n_tiles][height * width], dense; summary [n_tiles][40] */
    uint32_t* dist2;                   /* REQUIRED: it is the working array between the column pass and the row pass */
    uint32_t* nearest;                 /* NULL = not wanted */
    uint8_t*  within;                  /* NULL = not wanted; requires max_radius > 0 */
    uint64_t* summary;                 /* NULL = not wanted */
} dswx_distance_out_t;
/* One plane [n_tiles][tile_stride_elems] in DEVICE memory -> the wanted planes of *out_device (device memory).  Asynchronous
 * on `stream` (NULL = the context's stream): at most four kernel launches (note the targets of every band of 64 rows; the
 * vertical offset to the nearest target of the column for every pixel, with the carry across bands read from those notes; the
 * row pass, which finishes dist2 in place and writes nearest, within and the summary; unpack the summary's largest-distance
 * key) plus one hipMemsetAsync of `summary`; no synchronisation, no scratch of the context, no allocation, and nothing the
 * caller has to zero in front: a second call on the same outputs gives the same result.  No workgroup ever waits for another.
 * tile_stride_elems 0 = height * width.  A NULL spec or out struct, `mark` outside 0 .. 255, a negative size, tile count or
 * stride, a stride below height * width, height or width above 46340, height * width above 2^31, width above
 * DSWX_DISTANCE_MAX_WIDTH, a NULL plane with something to read, a NULL dist2, or `within` wanted with max_radius == 0:
 * DSWX_ERR_ARG; dist2 or nearest off 4 bytes or summary off 8: DSWX_ERR_ALIGN.  The plane and `within` take any address.
 * (The arguments are checked before the context is, and a refused call writes nothing; the limits on the size of a plane are
 * those of dswx_compare_device.)  The outputs MUST NOT OVERLAP the plane or each other: that is NOT CHECKED. */
int dswx_distance_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height,
                         int64_t width, int64_t tile_stride_elems, const dswx_distance_out_t* out_device, void* stream);
/* Plane `plane` (a uint8 DSWX_PLANE_* of the library's plane table: Fmask, the masks, every layer but DIAG) of a resident
 * batch, tiles tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last) -> the wanted planes of
 * *out_device: device planes owned by the caller, output tile 0 = tile0.  Asynchronous on `stream` (NULL = the stream of the
 * batch's context) like dswx_distance_device.  The address and the stride are those of dswx_batch_planes, so packed,
 * separate-output, placed, padded and contiguous batches are alike.  A plane that is not uint8 (the bands, DIAG), a plane the
 * batch does not have, or DSWX_PLANE_COUNTERS: DSWX_ERR_ARG, and dswx_last_error() names the plane.  Tile ranges: the rules
 * of dswx_batch_compare. */
int dswx_batch_distance(dswx_batch_t* batch, int32_t plane, const dswx_distance_spec_t* spec, int64_t tile0, int64_t n_tiles,
                        const dswx_distance_out_t* out_device, void* stream);
/* The same definition on HOST buffers in plain scalar C++: needs no device and no context.  The other half of a comparison,
 * not a fallback of the two entries above.  The refusals of dswx_distance_device, except that every buffer, the uint32 and
 * uint64 ones included, may sit at any address. */
int dswx_distance_host(const uint8_t* plane, const dswx_distance_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                       int64_t tile_stride_elems, const dswx_distance_out_t* out_host);

/* ---- outline: the regions of an id plane traced as ordered rings of pixel edges (additive to ABI v7)
 * The body table above says how long a shoreline is; users of a water-extent product then ask for the lake POLYGONS.  These
 * entries put the edges that the body table's perimeter counts in order, ring after ring, without the 4-byte label plane
 * crossing PCIe: what comes back is 4 bytes per edge and 32 bytes per ring.  A C caller tests for them with DSWX_HAS_OUTLINE.
 * THE DEFINITION.  `ids` is a uint32 plane [n_tiles][height * width], dense, typically the `label` of dswx_label_device or
 * the `dense` of dswx_body_table_device: 0 is background, any other value the id of the region the pixel belongs to.  ANY
 * CONTENT IS LEGAL: ids are only compared for equality and never used as an index.  idx(p) = y * width + x; rows do not wrap,
 * tiles never see each other, outside the tile counts as 0.
 *   EDGES      a boundary edge is a pair (pixel p with ids[p] = v != 0, direction d) whose neighbour across d is outside the
 *              tile or holds a different value: exactly the pair that the body table's perimeter counts.  Its KEY is
 *              4 * idx(p) + d, a uint32, hence height * width <= 2^30.  On pixel corners, x right and y down: d = 0 the top
 *              edge from (x, y) to (x+1, y); 1 the right edge from (x+1, y) to (x+1, y+1); 2 the bottom edge from (x+1, y+1)
 *              to (x, y+1); 3 the left edge from (x, y+1) to (x, y).  The region lies on the right of the direction of
 *              travel: outer rings run clockwise on screen, holes the other way.
 *   SUCCESSOR  with T[d] = (1,0), (0,1), (-1,0), (0,-1) the travel of edge d and O[d] = (0,-1), (1,0), (0,1), (-1,0) the step
 *              across it: A = p + T[d] is the pixel ahead on the region's side, B = A + O[d] the one ahead on the other side,
 *              a = (ids[A] == v), b = (ids[B] == v), both false outside the tile.  connectivity 4: if !a the successor is
 *              4 * idx(p) + (d+1)%4 (turn right), else if !b 4 * idx(A) + d (straight), else 4 * idx(B) + (d+3)%4 (turn left).
 *              connectivity 8: if b 4 * idx(B) + (d+3)%4, else if a 4 * idx(A) + d, else 4 * idx(p) + (d+1)%4.  The two differ
 *              only where two pixels of one id touch at a corner.  The successor is always a boundary edge and the map a
 *              bijection, so the edges fall into cycles: the RINGS.  A ring STARTS at its smallest key; the rings of a tile
 *              are ORDERED by their start keys; E is the number of edges of the tile and R the number of its rings.  Every
 *              body of a dswx_label_* plane outlined with the connectivity it was labelled with has exactly one ring of
 *              positive area, whose start key is 4 * (label - 1); its holes are the enclosed components of its complement.
 *   chain      uint32 [n_tiles][max_edges]: the keys of all E edges, ring after ring in ring order, each ring from its start
 *              along the successor map; entries E .. max_edges - 1 are zero;
 *   rings      [n_tiles][max_rings] rows of DSWX_OUTLINE_ROW_WORDS uint32 (32 bytes; the 64-bit field at an even word): word 0
 *              the id v; 1 the start key; 2 the offset of the ring in `chain`; 3 its length in edges; 4 its corners: the edges
 *              whose direction differs from their predecessor's, which are the vertices of the polygon once collinear points
 *              are dropped (a single pixel has 4); 5 zero; 6-7 area2 (int64): the sum over the ring's edges of
 *              x1 * y2 - x2 * y1, start corner 1 and end corner 2, twice the signed area, positive for an outer ring and
 *              negative for a hole.  Rows min(R, max_rings) .. max_rings - 1 are zero.  The chain of a tile is complete even
 *              when R > max_rings: a ring table that is too small is truncated, never wrong;
 *   head       uint64 [n_tiles][DSWX_OUTLINE_HEAD_WORDS]: word 0 E; 1 R; 2 min(R, max_rings); 3 the edges written, which is E
 *              when the tile fits; 4 the rings with area2 > 0; 5 those with area2 < 0; 6 the sum of the corners; 7 1 when
 *              E > max_edges.  When E > max_edges, words 1 .. 6 are 0 and the tile's chain and rings are all zero: the caller
 *              learns E and calls again.
 * chain, rings and head may each be NULL = not wanted; rings NULL requires max_rings == 0, chain NULL requires rings NULL; a
 * call with only head is the counting call.  All of it is integer arithmetic: the result is deterministic and independent of
 * the launch geometry and of the order in which atomics arrive.
 * NO dswx_batch_* FORM: the input is a label plane owned by the caller, not a plane of the batch; the `label` that
 * dswx_batch_label left is passed to dswx_outline_device as it is. */
#define DSWX_HAS_OUTLINE 1
#define DSWX_OUTLINE_ROW_WORDS 8
#define DSWX_OUTLINE_HEAD_WORDS 8
typedef struct dswx_outline_spec {
    int64_t max_edges;                 /* 0 .. 2^31: entries of `chain` per tile */
    int64_t max_rings;                 /* 0 .. 2^31: rows of `rings` per tile */
    int32_t connectivity;              /* 4 or 8 */
    int32_t reserved;                  /* zero */
} dswx_outline_spec_t;                 /* 24 bytes */
typedef struct dswx_outline_out {
    uint32_t* chain;                   /* [n_tiles][max_edges]; NULL = not wanted (rings must be NULL then) */
    uint32_t* rings;                   /* [n_tiles][max_rings][8]; NULL = not wanted (max_rings must be 0 then) */
    uint64_t* head;                    /* [n_tiles][8]; NULL = not wanted */
} dswx_outline_out_t;
/* The bytes of working memory that dswx_outline_device needs for these arguments, at least 16.  THE FIRST ENTRY THAT NEEDS
 * WORKING MEMORY OF THE CALLER: the earlier entries work inside their own outputs, but here the working set is 36 bytes per
 * edge of capacity and 5 per pixel (two copies of a 16-byte state per edge, between which the rounds alternate, 16 bytes per
 * four edges for the sums of a ring, the number of the first edge and the edge mask of every pixel), several times all the
 * outputs together, sized by a capacity only the caller knows, and the entry may neither allocate nor touch the context's
 * scratch.  The capacity that counts is min(max_edges, 4 * height * width).  A NULL spec or `bytes`, a negative size, a
 * raster above 2^30 pixels or max_edges above 2^31: DSWX_ERR_ARG. */
int dswx_outline_work_bytes(const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width, uint64_t* bytes);
/* One id plane in DEVICE memory -> the wanted outputs of *out_device (device memory), with `work_device` (device memory of
 * at least dswx_outline_work_bytes bytes, whose content before and after the call means nothing) as the working memory.
 * Asynchronous on `stream` (NULL = the context's stream): 9 + N kernel launches, N = ceil(log2(min(max_edges, 4 * height *
 * width))) <= 31 -- count the edges of every chunk of 4096 pixels; scan those counts per tile; number the first edge of every
 * pixel; emit for every edge its key and the number of its successor; N rounds of pointer jumping, one launch each, after
 * which every edge knows the start of its ring and its distance to it (the number of rounds is fixed by the capacity, so that
 * nothing is read back; the workgroups of a tile return at once when a flag in the working memory says that the round before
 * changed nothing for that tile); count, scan and rank the ring starts, carrying count and length together; scatter the keys
 * into the chain, the sums of a ring combined per wave before any atomic; finish the rows and the head -- plus one
 * hipMemsetAsync each of `chain` and `rings`; no synchronisation, no scratch of the context, no allocation, and nothing the
 * caller has to zero in front: a second call on the same outputs gives the same bytes.  No workgroup ever waits for another.
 * A NULL spec or out struct, a connectivity that is neither 4 nor 8, reserved != 0, a negative size, tile count or capacity,
 * height * width above 2^30, max_edges or max_rings above 2^31, a NULL ids with something to read, NULL rings with
 * max_rings > 0, NULL chain with rings wanted, a NULL work_device, or work_bytes below what dswx_outline_work_bytes returns:
 * DSWX_ERR_ARG; ids, chain or rings off 4 bytes, or head or work_device off 8: DSWX_ERR_ALIGN.  (The arguments are checked
 * before the context is, and a refused call writes nothing.)  The outputs and the working memory MUST NOT OVERLAP the input or
 * each other: that is NOT CHECKED. */
int dswx_outline_device(dswx_ctx_t* ctx, const uint32_t* ids, const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height,
                        int64_t width, const dswx_outline_out_t* out_device, void* work_device, uint64_t work_bytes, void* stream);
/* The same definition on HOST buffers as a plain scalar walk in C++: needs no device, no context and no working memory of the
 * caller.  The other half of a comparison, not a fallback of the entry above.  The refusals of dswx_outline_device, except
 * that every buffer may sit at any address. */
int dswx_outline_host(const uint32_t* ids, const dswx_outline_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                      const dswx_outline_out_t* out_host);

/* ---- burn: polygon rings rasterised onto planes -- the opposite direction of the outline (additive to ABI v7)
 * label, body table and outline go from a resident plane to vectors.  These entries go back: the edges of polygon rings
 * become pixels, without a plane crossing PCIe -- a coastline, an area of interest or an edited lake polygon becomes a plane
 * on the device, or is burnt straight into the OCEAN plane of a resident batch in front of dswx_batch_classify.  What the
 * reference does with gdal.RasterizeLayer(burn_values=[1]) in _create_ocean_mask (dswx_hls.py:3464-3572).  A C caller tests
 * for the entries with DSWX_HAS_BURN.  The metric Buffer(margin_m) of the VECTOR is the "reach" block below (the distance
 * entry's `within` buffers the RASTER afterwards).  STILL REFUSED by this library: reading .shp files and reprojecting from
 * the SRS of a shapefile -- host work, which proteus_amd/shoreline.py does for WGS 84 geographic and WGS 84 / UTM.
 * UNPINNED: GDAL is not part of this project's environment, so GDAL's handling of a pixel centre that lies exactly on an edge
 * is not pinned by any test.  The definition below is this project's own; it agrees with GDAL's documented default (a pixel
 * is burnt when its CENTRE is inside) wherever no centre lies exactly on an edge.
 * THE DEFINITION.  Coordinates are int32 in units of 1/256 pixel, x right and y down: pixel (c, r) has its centre at
 * (256 c + 128, 256 r + 128).  A coordinate v is LEGAL iff |v| <= 2^30 (DSWX_BURN_MAX_COORD).  Rows do not wrap and tiles never
 * see each other.
 *   INPUT      `verts`: records of 16 bytes {int32 x, y; uint32 word; uint32 next}.  `tile_first`: int64 [n_tiles + 1]; tile t
 *              owns the records tile_first[t] .. tile_first[t + 1] - 1 of `verts`: its count is tile_first[t + 1] -
 *              tile_first[t], and ZERO when that is negative or tile_first[t] is: a decreasing table means that the affected
 *              tiles have no records.  Record i of a tile (counted from the tile's first) is the directed edge from its
 *              (x, y) to the (x, y) of record `next` of the same tile.  A closed ring is a cycle of `next`; the rasterisation
 *              needs only the multiset of edges, so nothing checks that the cycles close.  ANY CONTENT OF A RECORD IS LEGAL: a
 *              record is MALFORMED when its `next` is >= the count of its tile, or when one of the four coordinates of its
 *              two endpoints is not legal.  A malformed record contributes nothing and is counted; `next` is compared with
 *              the count before the record it names is read.
 *   CROSSING   orient the edge so that y0 < y1; an edge with y0 == y1 contributes nothing.  The edge CROSSES row r iff
 *              y0 <= 256 r + 128 < y1 and 0 <= r < height.  For such a row, with yc = 256 r + 128,
 *                  col = max(0, ceil(((x1 - x0) * (yc - y0) + (x0 - 128) * (y1 - y0)) / (256 * (y1 - y0))))
 *              in exact integer arithmetic: the first pixel of the row whose centre is at or to the right of the crossing
 *              (with legal coordinates every intermediate stays below 2^63).  If col < width the crossing TOGGLES:
 *              acc[r][col] ^= word; otherwise it is dropped.
 *   RESULT     acc[r][c] is the XOR of all toggles of row r at columns <= c: the XOR of the words of all edges that cross row
 *              r at or to the left of the centre of (c, r).  Rows are half-open at the bottom end of an edge, columns closed
 *              on the left.  For one ring with word w, acc is w exactly on the pixels whose centre is inside by the even-odd
 *              rule; if every polygon of a set has a bit of its own, acc != 0 is their union; and if every ring that
 *              dswx_outline_* returns for an id plane gets its id as word, acc IS that id plane, whatever the plane holds and
 *              with either connectivity.
 *   acc        uint32 [n_tiles][height * width], dense.  REQUIRED: it is the working array;
 *   mask       uint8 [n_tiles][mask_tile_stride] (0 = height * width): mask[p] = acc[p] != 0 ? burn : (src ? src[p] :
 *              background); the bytes between height * width and the stride are not touched.  NULL = not wanted.  `src` is an
 *              optional uint8 plane [n_tiles][src_tile_stride] (0 = height * width) and MAY BE `mask` ITSELF, with the same
 *              stride: burn in place, several calls OR together.  Any other overlap is NOT CHECKED;
 *   head       uint64 [n_tiles][DSWX_BURN_HEAD_WORDS]: word 0 the records of the tile; 1 the malformed ones; 2 the edges that
 *              cross at least one row of the tile; 3 the toggles applied; 4 the crossings dropped at col >= width; 5 the
 *              crossings whose column was negative before the clamp to 0 (applied or dropped, they count in 3 or 4 too); 6 the
 *              pixels with acc != 0; 7 zero.  NULL = not wanted.
 * height * width <= 2^30, as for the outline.  n_tiles == 0 writes nothing.  All of it is integer arithmetic: the result is
 * deterministic and independent of the launch geometry and of the order in which atomics arrive (XOR and integer addition
 * commute). */
#define DSWX_HAS_BURN 1
#define DSWX_BURN_HEAD_WORDS 8
#define DSWX_BURN_MAX_COORD (1 << 30)
typedef struct dswx_burn_vertex {
    int32_t x, y;                      /* 1/256 pixel */
    uint32_t word;                     /* what a crossing of the edge that starts here toggles */
    uint32_t next;                     /* the record at which that edge ends, counted from the tile's first record */
} dswx_burn_vertex_t;                  /* 16 bytes */
typedef struct dswx_burn_spec {
    int32_t burn;                      /* 0 .. 255: the byte of a pixel with acc != 0 in `mask` */
    int32_t background;                /* 0 .. 255: the byte of every other pixel when there is no `src` */
    int64_t mask_tile_stride;          /* elements between the tiles of `mask`; 0 = height * width */
    int64_t src_tile_stride;           /* elements between the tiles of `src`; 0 = height * width */
} dswx_burn_spec_t;                    /* 24 bytes */
typedef struct dswx_burn_out {
    uint32_t* acc;                     /* [n_tiles][height * width]; REQUIRED: the working array */
    uint8_t*  mask;                    /* [n_tiles][mask_tile_stride]; NULL = not wanted */
    uint64_t* head;                    /* [n_tiles][8]; NULL = not wanted */
} dswx_burn_out_t;
/* Records and table in DEVICE memory -> the wanted outputs of *out_device (device memory).  Asynchronous on `stream` (NULL =
 * the context's stream): one hipMemsetAsync each of `acc` and `head` and two kernel launches -- every record computes its
 * first crossing with one 64-bit division and steps it exactly down the rows (an edge of more than a few rows is shared out
 * over the lanes of its wave), each crossing one atomic XOR on `acc`, the counts summed per workgroup before one set of
 * 64-bit atomics; then an XOR prefix along every row of `acc` in place, which also writes `mask` and counts the pixels.  No
 * synchronisation, no scratch of the context, no allocation, no working memory and nothing the caller has to zero in front: a
 * second call on the same outputs gives the same bytes (with `src` == `mask` the second call burns into the first one's
 * result, which leaves it as it is).  No workgroup ever waits for another.  `tile_first` is read ON THE DEVICE ONLY: its
 * content is not validated on the host, the records it names must lie inside `verts` (NOT CHECKED), and a decreasing table
 * gives the affected tiles zero records as stated above.  A NULL spec or out struct, `burn` or `background` outside 0 .. 255,
 * a negative size, tile count or stride, a stride that is neither 0 nor at least height * width, height * width above 2^30,
 * more than 2^32 tiles, NULL verts or tile_first with n_tiles > 0, a NULL acc with something to write, or `src` without
 * `mask`: DSWX_ERR_ARG; verts off 16 bytes, acc off 4, or tile_first or head off 8: DSWX_ERR_ALIGN.  `mask` and `src` take
 * any address.  (The arguments are checked before the context is, and a refused call writes nothing.) */
int dswx_burn_device(dswx_ctx_t* ctx, const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec,
                     int64_t n_tiles, int64_t height, int64_t width, const uint8_t* src, const dswx_burn_out_t* out_device,
                     void* stream);
/* Plane `plane` (a uint8 DSWX_PLANE_* of the library's plane table: Fmask, the masks, every layer but DIAG;
 * DSWX_PLANE_OCEAN is the natural target) of a resident batch is BOTH `mask` and `src`, at the batch's tile stride, for tiles
 * tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last): the polygons are burnt into the plane in
 * place, tile_first[0] belongs to tile0, and acc_device (required) and head_device (NULL = not wanted) are the caller's device
 * memory with tile 0 = tile0.  THE FIRST dswx_batch_* ENTRY THAT WRITES A PLANE OF THE BATCH: every earlier one only reads
 * them.  Asynchronous on `stream` (NULL = the stream of the batch's context) like dswx_burn_device.  The two strides of
 * `spec` must be 0: DSWX_ERR_ARG otherwise.  A plane that is not uint8 (the bands, DIAG), a plane the batch does not have, or
 * DSWX_PLANE_COUNTERS: DSWX_ERR_ARG, and dswx_last_error() names the plane.  Tile ranges: the rules of dswx_batch_compare. */
int dswx_batch_burn(dswx_batch_t* batch, int32_t plane, const dswx_burn_vertex_t* verts_device, const int64_t* tile_first_device,
                    const dswx_burn_spec_t* spec, uint32_t* acc_device, uint64_t* head_device, int64_t tile0, int64_t n_tiles,
                    void* stream);
/* The same definition on HOST buffers in plain scalar C++, one division per crossing: needs no device and no context.  The
 * other half of a comparison, not a fallback of the two entries above.  The refusals of dswx_burn_device, except that every
 * buffer may sit at any address. */
int dswx_burn_host(const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_burn_spec_t* spec, int64_t n_tiles,
                   int64_t height, int64_t width, const uint8_t* src, const dswx_burn_out_t* out_host);

/* ---- reach: every pixel whose centre lies within a radius of a polygon edge -- the exact buffer (additive to ABI v7) --------
 * The burn entries give the inside of polygons.  These give the pixels NEAR their edges, measured from pixel centres to the
 * vector itself: burn, then reach onto the same mask (`src` == `mask`), is the polygon grown by the radius -- what the
 * reference does with Buffer(margin_m) in front of gdal.RasterizeLayer in _create_ocean_mask (dswx_hls.py:3464-3572).  A C
 * caller tests for the entries with DSWX_HAS_REACH.
 * UNPINNED: GDAL and GEOS are not part of this project's environment.  OGR's Buffer replaces the circle at a convex vertex by
 * chords (30 segments per quadrant by default) that lie inside it by at most r (1 - cos 1.5 deg) = 3.4e-4 r; an exact buffer
 * differs from it only in centres inside that sliver.  No test pins the two to each other.
 * THE DEFINITION.  Records, `tile_first`, the count of a tile, legality (|v| <= 2^30) and MALFORMED are those of the burn block
 * above, to the letter -- `next` is compared with the count before the record it names is read -- and so are the coordinates:
 * int32 in 1/256 pixel, the centre of pixel (c, r) at P = (256 c + 128, 256 r + 128).  `word` is ignored.  NOTHING IS DROPPED:
 * a horizontal edge takes part, and an edge whose two endpoints coincide is a point and takes part.
 *   RADIUS     `radius`: uint32 in 1/256 pixel, 0 <= radius <= DSWX_REACH_MAX_RADIUS = 2^20 (4096 pixels).
 *   REACHED    pixel (c, r) is REACHED by the well-formed edge A -> B iff the squared Euclidean distance from P to the closed
 *              segment is <= radius^2, in exact integers: with d = B - A, u = P - A, D = d.d, t = u.d and R = radius,
 *                  D == 0 or t <= 0:   u.u <= R^2
 *                  t >= D:             |P - B|^2 <= R^2
 *                  otherwise:          (u x d)^2 <= R^2 D
 *              stated in unbounded integers: at the extreme coordinates u x d and t pass 2^63 and R^2 D reaches 2^103.
 *   acc        uint32 [n_tiles][height * width], dense.  REQUIRED: it is the working array.  acc[r][c] is the number of
 *              well-formed edges of the tile that reach (c, r), modulo 2^32;
 *   mask       uint8 [n_tiles][mask_tile_stride] (0 = height * width): mask[p] = acc[p] != 0 ? burn : (src ? src[p] :
 *              background), strides, `src` and `src` == `mask` as for the burn entries: reach ORed onto a burnt mask;
 *   head       uint64 [n_tiles][DSWX_REACH_HEAD_WORDS]: word 0 the records of the tile; 1 the malformed ones; 2 the edges that
 *              reach at least one pixel of the tile; 3 the (edge, row) intervals applied -- the capsule of an edge is convex, so
 *              the pixels of a row that it reaches are one interval of columns; 4 the applied intervals cut at column 0 (the
 *              edge also reaches the centre of column -1 of that row); 5 those cut at column width - 1 (it also reaches the
 *              centre of column `width`); 6 the pixels with acc != 0; 7 zero.  NULL = not wanted.
 * height * width <= 2^30.  n_tiles == 0 writes nothing.  All of it is integer arithmetic (floating point only proposes where
 * an interval ends; the exact predicate decides): deterministic and independent of the launch geometry and of the order in
 * which atomics arrive. */
#define DSWX_HAS_REACH 1
#define DSWX_REACH_HEAD_WORDS 8
#define DSWX_REACH_MAX_RADIUS (1 << 20)
typedef struct dswx_reach_spec {
    int32_t burn;                      /* 0 .. 255: the byte of a pixel with acc != 0 in `mask` */
    int32_t background;                /* 0 .. 255: the byte of every other pixel when there is no `src` */
    int64_t mask_tile_stride;          /* elements between the tiles of `mask`; 0 = height * width */
    int64_t src_tile_stride;           /* elements between the tiles of `src`; 0 = height * width */
    uint32_t radius;                   /* 1/256 pixel, 0 .. DSWX_REACH_MAX_RADIUS */
    uint32_t reserved;                 /* must be 0 */
} dswx_reach_spec_t;                   /* 32 bytes */
typedef dswx_burn_out_t dswx_reach_out_t;      /* acc (REQUIRED), mask, head: as for the burn entries */
/* Records and table in DEVICE memory -> the wanted outputs of *out_device (device memory).  Asynchronous on `stream` (NULL =
 * the context's stream): one hipMemsetAsync each of `acc` and `head` and two kernel launches -- every (edge, row) adds +1 at
 * the first reached column and -1 behind the last one with two atomic adds on `acc` (the rows of an edge are shared out over
 * the lanes of its wave); then a prefix sum along every row of `acc` in place, which also writes `mask` and counts the pixels.
 * No synchronisation, no scratch of the context, no allocation, no working memory and nothing the caller has to zero in
 * front: a second call on the same outputs gives the same bytes.  No workgroup ever waits for another.  `tile_first` is read ON
 * THE DEVICE ONLY, as for dswx_burn_device.  The refusals and alignments of dswx_burn_device, and a radius above
 * DSWX_REACH_MAX_RADIUS or a `reserved` that is not 0: DSWX_ERR_ARG.  (The arguments are checked before the context is, and a
 * refused call writes nothing.) */
int dswx_reach_device(dswx_ctx_t* ctx, const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec,
                      int64_t n_tiles, int64_t height, int64_t width, const uint8_t* src, const dswx_reach_out_t* out_device,
                      void* stream);
/* The twin of dswx_batch_burn: plane `plane` (a uint8 DSWX_PLANE_*; DSWX_PLANE_OCEAN is the natural target) of a resident batch
 * is BOTH `mask` and `src`, at the batch's tile stride, for tiles tile0 .. tile0 + n_tiles - 1: the pixels within the radius of
 * an edge become `burn` in place, every other pixel stays.  acc_device (required) and head_device (NULL = not wanted) are the
 * caller's device memory with tile 0 = tile0.  Asynchronous like dswx_reach_device.  The two strides of `spec` must be 0.  The
 * refusals of dswx_batch_burn. */
int dswx_batch_reach(dswx_batch_t* batch, int32_t plane, const dswx_burn_vertex_t* verts_device, const int64_t* tile_first_device,
                     const dswx_reach_spec_t* spec, uint32_t* acc_device, uint64_t* head_device, int64_t tile0, int64_t n_tiles,
                     void* stream);
/* The same definition on HOST buffers in plain scalar C++: needs no device and no context.  The other half of a comparison,
 * not a fallback of the two entries above.  The refusals of dswx_reach_device, except that every buffer may sit at any
 * address. */
int dswx_reach_host(const dswx_burn_vertex_t* verts, const int64_t* tile_first, const dswx_reach_spec_t* spec, int64_t n_tiles,
                    int64_t height, int64_t width, const uint8_t* src, const dswx_reach_out_t* out_host);

/* ---- mosaic: tiles placed on one canvas and composited per canvas pixel -- a stack with placements (additive to ABI v7) ---
 * Every entry above treats a tile on its own, and a stack requires every tile to cover the same pixels.  Neighbouring MGRS
 * tiles of one UTM zone share the 30 m lattice and overlap by about 326 pixels: a lake on a seam is two bodies until the tiles
 * are placed relative to each other.  These entries do that without a plane crossing PCIe.  The result is a canvas plane in
 * device memory, and the entries that take a caller's plane of any height x width (label, body table, distance, outline, grid,
 * histogram) work across the seams unchanged.  Several dates of several neighbours give the latest clear observation and the
 * surface-water occurrence per canvas pixel.  A C caller tests for the entries with DSWX_HAS_MOSAIC.
 * THE DEFINITION.  The input is one uint8 plane [n_tiles][tile_stride] at any address; every tile is a raster of height x
 * width with row pitch `width`, and the padding up to the stride is never read.  place = int32 [n_tiles][2] = (row0, col0),
 * the canvas position of pixel (0, 0) of the tile; ANY content is legal.  The canvas is canvas_h x canvas_w, dense, row pitch
 * canvas_w.  Tile t COVERS canvas pixel (Y, X) iff 0 <= Y - row0[t] < height and 0 <= X - col0[t] < width, evaluated in 64
 * bits (INT32_MIN and INT32_MAX are ordinary values).  Tiles may overlap, coincide, hang over any edge of the canvas, lie
 * wholly outside it (ignored) or be larger than it.  Per canvas pixel the rule of a stack (above) is applied, unchanged, over
 * the COVERING tiles in increasing t: count[k], last, last_index (the index t in the plane, not a rank among the covering
 * tiles) and share.  A pixel that is covered but never observed gets `fill`, DSWX_STACK_NONE, DSWX_STACK_NO_SHARE and counts
 * 0, as in a stack; a pixel that NO tile covers gets the same values except last = `outside`.  n_tiles <=
 * DSWX_STACK_MAX_TILES; n_tiles == 0 writes the outside values; an empty canvas writes nothing; an empty tile raster covers
 * nothing.  canvas_h, canvas_w <= 2^30.  All of it is integer arithmetic per pixel: the result is deterministic and
 * independent of the launch geometry.
 * THE LIMITS THAT REMAIN.  The tiles of one plane share a size, and placement is in whole pixels of ONE lattice: these entries
 * resample and reproject nothing.  A neighbour in another UTM zone goes through the warp entries below first (bin/dswx_mosaic.py
 * --reproject); without that it is refused by the tools as before. */
#define DSWX_HAS_MOSAIC 1
typedef struct dswx_mosaic_spec {
    int32_t n_cats;                    /* 1 .. DSWX_STACK_MAX_CATS */
    int32_t fill;                      /* 0 .. 255: `last` of a pixel that is covered but that no tile observed */
    int32_t outside;                   /* 0 .. 255: `last` of a pixel that no tile covers */
    int32_t reserved;                  /* must be 0 */
    uint8_t cat_of_byte[256];          /* as in dswx_stack_spec_t */
} dswx_mosaic_spec_t;                  /* 272 bytes */
/* One plane [n_tiles][tile_stride_elems] in DEVICE memory, placed by place_device (DEVICE memory, read by the device only) ->
 * the wanted planes of *out_device (device memory, canvas_h * canvas_w elements each).  Asynchronous on `stream` (NULL = the
 * context's stream): ONE kernel launch, no synchronisation, no scratch of the context, no allocation, no memset; every wanted
 * output element is written exactly once and nothing else is written.  tile_stride_elems 0 = height * width.  The refusals of
 * dswx_stack_device (with height * width for n_elems), and: `outside` outside 0 .. 255, reserved != 0, a negative height,
 * width or canvas size, a tile side or a canvas side above 2^30, a canvas above 2^46 pixels or above what one launch covers
 * (2^36 pixels), a NULL place_device with n_tiles > 0: DSWX_ERR_ARG; place_device off 4 bytes: DSWX_ERR_ALIGN.  (The
 * arguments are checked before the context is, and a refused call writes nothing; the limits on the size of the plane are
 * those of dswx_compare_device.)  The output planes MUST NOT OVERLAP the plane, the table or each other: NOT CHECKED. */
int dswx_mosaic_device(dswx_ctx_t* ctx, const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height,
                       int64_t width, int64_t tile_stride_elems, const int32_t* place_device, int64_t canvas_h, int64_t canvas_w,
                       const dswx_stack_out_t* out_device, void* stream);
/* Plane `plane` (a uint8 DSWX_PLANE_* of the library's plane table) of a resident batch, tiles tile0 .. tile0 + n_tiles - 1
 * (n_tiles DSWX_BATCH_ALL_TILES = up to the last) placed by place_device, whose entry 0 belongs to tile0 -> the wanted planes
 * of *out_device: device planes of canvas_h x canvas_w elements owned by the caller.  last_index counts from tile0, as that of
 * dswx_batch_stack does.  Asynchronous on `stream` (NULL = the stream of the batch's context) like dswx_mosaic_device.
 * Planes and tile ranges: the rules of dswx_batch_stack. */
int dswx_batch_mosaic(dswx_batch_t* batch, int32_t plane, const dswx_mosaic_spec_t* spec, int64_t tile0, int64_t n_tiles,
                      const int32_t* place_device, int64_t canvas_h, int64_t canvas_w, const dswx_stack_out_t* out_device,
                      void* stream);
/* The same definition on HOST buffers in plain scalar C++, with a HOST place table: needs no device and no context.  The
 * other half of a comparison, not a fallback of the two entries above.  The refusals of dswx_mosaic_device, except that every
 * buffer, the table and the uint16 planes included, may sit at any address. */
int dswx_mosaic_host(const uint8_t* plane, const dswx_mosaic_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                     int64_t tile_stride_elems, const int32_t* place_host, int64_t canvas_h, int64_t canvas_w,
                     const dswx_stack_out_t* out_host);

/* ---- warp: planes resampled onto another lattice through a coordinate mesh, nearest pixel (additive to ABI v7) -------------
 * Every entry above leaves a pixel where it is or moves it by whole pixels of one lattice.  These entries move the pixels of a
 * plane to the positions that a MESH of source coordinates names, without the plane crossing PCIe: a neighbour in another UTM
 * zone onto the lattice of this tile (then dswx_mosaic_*), a product on a shifted or coarser lattice over another one, a
 * caller's land cover that is not on the HLS grid.  The split is that of dswx_burn_*: coordinates are int32 in 1/256 pixel, the
 * device sees numbers and never a projection (proteus_amd/warp.py computes meshes for north-up geotransforms and for pairs of
 * WGS 84 / UTM zones on the host).  A C caller tests for the entries with DSWX_HAS_WARP.
 * Bilinear / cubic resampling of float32 and int16 planes (the DEM's `cubic`) is the "resample" section below.
 * STILL REFUSED: mode or average resampling onto coarser lattices (dswx_grid_* aggregates); SRSs other than EPSG:4326 and
 * WGS 84 / UTM; antimeridian handling; reading .shp.
 * UNPINNED: GDAL and PROJ are not part of this project's environment, so gdal.Warp's own choice of the nearest pixel, its
 * approximate transformer (0.125 pixel error threshold) and its handling of a centre exactly on a pixel boundary are not
 * pinned by any test.  The definition below is this project's own.
 * THE DEFINITION.
 *   SOURCE     a plane [n_tiles][src_tile_stride] of elements of elem_bytes in {1, 2, 4} (class planes, int16 bands, DIAG,
 *              uint32 label / dense / acc planes, float32 planes as bit patterns): elements are copied, never interpreted.
 *              Every tile is a raster of height x width with row pitch `width`; the padding up to the stride is never read;
 *              stride 0 = height * width.
 *   DST        dst_h x dst_w per tile, dense.
 *   MESH       int32 [mesh_h][mesh_w][2] = (x, y) in 1/256 SOURCE pixel, x right and y down as for the burn entries: source
 *              pixel (c, r) has its centre at (256 c + 128, 256 r + 128).  step = 1 << shift, shift 0 .. 8; mesh_h = ((dst_h +
 *              step - 1) >> shift) + 1, mesh_w likewise.  Node (i, j) is the source position of the CENTRE of destination pixel
 *              (X, Y) = (j * step, i * step), which may lie past the destination's edge.  mesh_tile_stride_nodes 0 = one mesh
 *              for all tiles (the dates of one MGRS tile), else the nodes between the meshes of consecutive tiles.  ANY
 *              CONTENT IS LEGAL: INT32_MIN and INT32_MAX are ordinary values, garbage maps to garbage positions.
 *   POSITION   of destination pixel (X, Y): i = Y >> shift, fy = Y & (step - 1), j = X >> shift, fx = X & (step - 1); in
 *              64-bit integers, for x and in the same way for y,
 *                  num = (step - fy) * ((step - fx) * x[i][j]     + fx * x[i][j + 1])
 *                      +  fy         * ((step - fx) * x[i + 1][j] + fx * x[i + 1][j + 1])
 *                  sx  = (num + (1 << (2 * shift - 1))) >> (2 * shift)      (arithmetic shift; shift == 0: sx = x[i][j])
 *              |num| < 2^48.  The nearest source pixel is c = sx >> 8, r = sy >> 8 (floor); it is INSIDE iff 0 <= c < width and
 *              0 <= r < height.
 *   dst        [n_tiles][dst_h * dst_w] elements: the element of source pixel (c, r) of the same tile where inside, else the
 *              low elem_bytes bytes of spec.outside.  NULL = not wanted.
 *   src_index  uint32 [n_tiles][dst_h * dst_w]: r * width + c where inside, else DSWX_WARP_OUTSIDE (0xFFFFFFFF): a caller
 *              warps further planes by a plain gather, and a label plane stays meaningful.  NULL = not wanted.
 *   head       uint64 [n_tiles][DSWX_WARP_HEAD_WORDS]: word 0 the destination pixels, 1 those inside, 2 those outside, 3 and 4
 *              the smallest and the largest source row used (height and 0 if none), 5 and 6 the same for columns (width and
 *              0), 7 zero.  NULL = not wanted.
 * height * width <= 2^30 and dst_h * dst_w <= 2^30 (so every side is <= 2^30).  n_tiles == 0 or an empty destination writes
 * nothing; an empty source raster makes every pixel outside.  All of it is integer arithmetic per pixel: the result is
 * deterministic and independent of the launch geometry; no atomics touch the planes, and the atomics of `head` (add, min,
 * max) commute. */
#define DSWX_HAS_WARP 1
#define DSWX_WARP_HEAD_WORDS 8
#define DSWX_WARP_MAX_SHIFT 8
#define DSWX_WARP_OUTSIDE 0xFFFFFFFFu
typedef struct dswx_warp_spec {
    int32_t  elem_bytes;               /* 1, 2 or 4 */
    int32_t  shift;                    /* 0 .. DSWX_WARP_MAX_SHIFT: a mesh node every 1 << shift destination pixels */
    uint32_t outside;                  /* its low elem_bytes bytes are the element of a pixel that is not inside */
    int32_t  reserved;                 /* must be 0 */
    int64_t  src_tile_stride;          /* elements between the tiles of the plane; 0 = height * width */
    int64_t  mesh_tile_stride_nodes;   /* nodes between the meshes of consecutive tiles; 0 = one mesh for all tiles */
} dswx_warp_spec_t;                    /* 32 bytes */
typedef struct dswx_warp_out {
    void*     dst;                     /* [n_tiles][dst_h * dst_w] elements of elem_bytes; NULL = not wanted */
    uint32_t* src_index;               /* [n_tiles][dst_h * dst_w]; NULL = not wanted */
    uint64_t* head;                    /* [n_tiles][8]; NULL = not wanted */
} dswx_warp_out_t;
/* One plane in DEVICE memory, warped through mesh_device (DEVICE memory, read by the device only) -> the wanted outputs of
 * *out_device (device memory).  Asynchronous on `stream` (NULL = the context's stream): one hipMemsetAsync of `head` (only if
 * wanted) and ONE kernel launch, whatever the tile count (past the 65535 tiles of grid.y the workgroups walk the tiles); no
 * synchronisation, no scratch of the context, no allocation, and nothing the caller has to zero in front: a second call on
 * the same outputs gives the same bytes.  No workgroup ever waits for another.  A NULL spec or out struct, elem_bytes not 1 /
 * 2 / 4, shift outside 0 .. 8, reserved != 0, a negative size, tile count or stride, a stride that is neither 0 nor large
 * enough (src: height * width, mesh: mesh_h * mesh_w), height * width or dst_h * dst_w above 2^30, more than 2^32 tiles or a
 * plane above 2^46 elements, a NULL mesh or a NULL plane (of rasters that are not empty) with something to write:
 * DSWX_ERR_ARG; mesh or src_index off 4 bytes, head off 8, plane or dst off elem_bytes: DSWX_ERR_ALIGN.  (The arguments are
 * checked before the context is, and a refused call writes nothing.)  Every output NULL is no work, not an error.  Overlap of
 * the outputs with the plane, the mesh or each other is NOT CHECKED. */
int dswx_warp_device(dswx_ctx_t* ctx, const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height,
                     int64_t width, const int32_t* mesh_device, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out_device,
                     void* stream);
/* Plane `plane` of a resident batch -- ANY DSWX_PLANE_* but DSWX_PLANE_COUNTERS: the bands, Fmask, the masks, DIAG, every
 * layer -- tiles tile0 .. tile0 + n_tiles - 1 (n_tiles DSWX_BATCH_ALL_TILES = up to the last), warped through mesh_device,
 * whose mesh 0 belongs to tile0 -> the wanted outputs of *out_device: the caller's device memory, tile 0 = tile0.  The element
 * size is the plane table's: a spec->elem_bytes that disagrees is DSWX_ERR_ARG, and so is a spec->src_tile_stride that is not 0
 * (the plane has the stride of the batch).  Asynchronous on `stream` (NULL = the stream of the batch's context) like
 * dswx_warp_device.  A plane the batch does not have or DSWX_PLANE_COUNTERS: DSWX_ERR_ARG, and dswx_last_error() names the
 * plane.  Tile ranges: the rules of dswx_batch_compare. */
int dswx_batch_warp(dswx_batch_t* batch, int32_t plane, const dswx_warp_spec_t* spec, int64_t tile0, int64_t n_tiles,
                    const int32_t* mesh_device, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out_device, void* stream);
/* The same definition on HOST buffers in plain scalar C++, with a HOST mesh: needs no device and no context.  The other half of
 * a comparison, not a fallback of the two entries above.  The refusals of dswx_warp_device, except that every buffer may sit
 * at any address. */
int dswx_warp_host(const void* plane, const dswx_warp_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                   const int32_t* mesh_host, int64_t dst_h, int64_t dst_w, const dswx_warp_out_t* out_host);

/* ---- resample: float32 and int16 planes interpolated through the coordinate mesh, bilinear and cubic (additive to ABI v7) ---
 * The entries above copy the NEAREST pixel.  These INTERPOLATE: the DEM, which the reference warps with GDAL's `cubic` for
 * every product that has one, or an int16 band.  Byte class planes have no business here.  A C caller tests for the entries
 * with DSWX_HAS_RESAMPLE.
 * STILL REFUSED: element kinds other than float32 and int16; mode, average or lanczos resampling; a projection on the device.
 * UNPINNED: GDAL is not part of this project's environment, so gdal.Warp's double-precision positions (ours are quantised to
 * 1/256 source pixel), its weighting at the raster's border and at nodata taps, and its rounding of integer results are not
 * pinned by execution.  The definition below is this project's own.
 * THE DEFINITION.
 *   SOURCE, DST, MESH and the POSITION (sx, sy) of a destination pixel are EXACTLY those of the section above, in the same
 *              64-bit integers; the same size limits hold and any mesh content is legal.
 *   KIND       DSWX_RESAMPLE_F32 (float32) or DSWX_RESAMPLE_I16 (int16).
 *   METHOD     DSWX_RESAMPLE_BILINEAR or DSWX_RESAMPLE_CUBIC (nearest stays with dswx_warp_*).
 *   BASE       ux = sx - 128, c0 = ux >> 8, fx = ux & 255, and uy, r0, fy likewise (arithmetic shifts in 64 bits): a sample at
 *              a pixel centre has f = 0.
 *   VALID TAP  source pixel (c, r) is valid iff 0 <= c < width and 0 <= r < height (compared in 64 bits BEFORE the load), its
 *              value is finite (float32 NaN and +-Inf are not) and, if spec.has_nodata, it is != the nodata value: float32
 *              compared as a value with the float32 whose bits spec.nodata holds, int16 as an integer with (int32_t)
 *              spec.nodata.  A tap's value is converted to double, exactly.
 *   WEIGHTS    Keys' cubic with a = -0.5 (Catmull-Rom, GDAL's `cubic`) as INTEGERS over 2^25, f = 0 .. 255:
 *                  N0 = -65536 f + 512 f^2 - f^3          N1 = 2^25 - 1280 f^2 + 3 f^3
 *                  N2 =  65536 f + 1024 f^2 - 3 f^3       N3 = -256 f^2 + f^3
 *              They sum to 2^25, |N| <= 2^25 (exact in a double), and reproduce every polynomial of degree <= 2.
 *   CUBIC      if all 16 taps (c0 - 1 .. c0 + 2) x (r0 - 1 .. r0 + 2) are valid, with p[r][k] the tap of row r0 - 1 + r and
 *              column c0 - 1 + k:
 *                  h_r = ((Nx0 * p[r][0] + Nx1 * p[r][1]) + Nx2 * p[r][2]) + Nx3 * p[r][3]
 *                  v   = ((Ny0 * h_0 + Ny1 * h_1) + Ny2 * h_2) + Ny3 * h_3            result = v * 2^-50
 *              every product and every sum ONE IEEE double operation rounded on its own (no fused multiply-add).  Otherwise
 *              the pixel takes the BILINEAR rule, as GDAL does at borders and masked taps.
 *   BILINEAR   taps (c0, r0), (c0 + 1, r0), (c0, r0 + 1), (c0 + 1, r0 + 1) in that order with the integer weights
 *              (256 - fx)(256 - fy), fx (256 - fy), (256 - fx) fy, fx fy.  From S = 0.0 and Wt = 0, over the VALID taps only,
 *              in that order: S = S + w * p (the product is exact, the sum rounded), Wt += w.  Wt == 0: the pixel is OUTSIDE.
 *              Wt == 65536: result = S * 2^-16.  Otherwise result = S / (double)Wt.
 *   ELEMENT    float32: the double rounded to float32, to nearest even; float32 subnormals are kept, a cubic overshoot past
 *              FLT_MAX becomes an infinity.  int16: rint (half to even), then clamped to -32768 .. 32767.  An OUTSIDE pixel
 *              gets the low bytes of spec.outside, as in the warp spec.  No NaN is ever produced by arithmetic, so device and
 *              host agree on every bit.
 *   dst        [n_tiles][dst_h * dst_w] elements.  NULL = not wanted.
 *   how        uint8 [n_tiles][dst_h * dst_w]: 0 = outside, 1 = bilinear with all four taps valid, 2 = bilinear with fewer
 *              (renormalised by Wt), 3 = cubic.  NULL = not wanted.
 *   head       uint64 [n_tiles][DSWX_RESAMPLE_HEAD_WORDS]: word 0 the destination pixels, 1 those of how 3, 2 of how 1, 3 of
 *              how 2, 4 of how 0; 5 and 6 the smallest and the largest source ROW among the valid taps of the window used
 *              (4 x 4 for a cubic pixel, 2 x 2 for a bilinear one, nothing for an outside one; height and 0 if none); 7 zero.
 *              Column ranges are not reported: a host computes its source window from the mesh.  NULL = not wanted.
 * There is NO dswx_batch_resample: no plane of a batch is float32, and interpolating class planes is meaningless. */
#define DSWX_HAS_RESAMPLE 1
#define DSWX_RESAMPLE_HEAD_WORDS 8
#define DSWX_RESAMPLE_F32 0
#define DSWX_RESAMPLE_I16 1
#define DSWX_RESAMPLE_BILINEAR 1
#define DSWX_RESAMPLE_CUBIC 2
typedef struct dswx_resample_spec {
    int32_t  kind;                     /* DSWX_RESAMPLE_F32 or DSWX_RESAMPLE_I16 */
    int32_t  method;                   /* DSWX_RESAMPLE_BILINEAR or DSWX_RESAMPLE_CUBIC */
    int32_t  shift;                    /* 0 .. DSWX_WARP_MAX_SHIFT: a mesh node every 1 << shift destination pixels */
    int32_t  has_nodata;               /* 0: every finite value is valid */
    uint32_t nodata;                   /* float32: the bits of the value; int16: the value as int32 */
    uint32_t outside;                  /* its low bytes are the element of an OUTSIDE pixel */
    int32_t  reserved;                 /* must be 0 */
    int32_t  reserved2;                /* must be 0 (padding in front of the 64-bit strides) */
    int64_t  src_tile_stride;          /* elements between the tiles of the plane; 0 = height * width */
    int64_t  mesh_tile_stride_nodes;   /* nodes between the meshes of consecutive tiles; 0 = one mesh for all tiles */
} dswx_resample_spec_t;                /* 48 bytes */
typedef struct dswx_resample_out {
    void*     dst;                     /* [n_tiles][dst_h * dst_w] float32 or int16; NULL = not wanted */
    uint8_t*  how;                     /* [n_tiles][dst_h * dst_w]; NULL = not wanted */
    uint64_t* head;                    /* [n_tiles][8]; NULL = not wanted */
} dswx_resample_out_t;
/* One plane in DEVICE memory, resampled through mesh_device (DEVICE memory) -> the wanted outputs of *out_device (device
 * memory).  Asynchronous on `stream` (NULL = the context's stream): one hipMemsetAsync of `head` (only if wanted) and ONE
 * kernel launch, whatever the tile count (past the 65535 tiles of grid.y the workgroups walk the tiles); no synchronisation,
 * no scratch of the context, no allocation, nothing the caller has to zero in front: a second call on the same outputs gives
 * the same bytes, and no workgroup ever waits for another.  The refusals are those of dswx_warp_device with `kind` (not
 * DSWX_RESAMPLE_F32 / _I16) and `method` (not _BILINEAR / _CUBIC) in the place of elem_bytes and `how` in the place of
 * src_index: DSWX_ERR_ARG; mesh off 4 bytes, head off 8, plane or dst off the element size: DSWX_ERR_ALIGN.  The arguments
 * are checked before the context is, and a refused call writes nothing.  Overlap of the outputs with the plane, the mesh or
 * each other is NOT CHECKED. */
int dswx_resample_device(dswx_ctx_t* ctx, const void* plane, const dswx_resample_spec_t* spec, int64_t n_tiles, int64_t height,
                         int64_t width, const int32_t* mesh_device, int64_t dst_h, int64_t dst_w,
                         const dswx_resample_out_t* out_device, void* stream);
/* The same definition on HOST buffers in plain scalar C++, with a HOST mesh: needs no device and no context.  The other half of
 * a comparison, not a fallback.  The refusals of dswx_resample_device, except that every buffer may sit at any address. */
int dswx_resample_host(const void* plane, const dswx_resample_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                       const int32_t* mesh_host, int64_t dst_h, int64_t dst_w, const dswx_resample_out_t* out_host);

/* ---- land mesh: the LAND layer from land-cover maps that are NOT on the HLS grid, read through two meshes (additive to ABI v7)
 * dswx_landcover_mask_* wants the ESA WorldCover map on the grid three times finer than the HLS grid and the Copernicus
 * CGLS-100 m map on the HLS grid.  Both ship in EPSG:4326.  Chaining dswx_warp_device twice and dswx_landcover_mask_device
 * needs a [3 height][3 width] and a [height][width] intermediate per tile and writes 10 bytes per HLS pixel only to read them
 * again.  These entries read the two SOURCE windows through their meshes and write LAND, and are defined as exactly that chain.
 * A C caller tests for them with DSWX_HAS_LAND_MESH.
 * STILL REFUSED: mode or average resampling; a projection on the device (proteus_amd/landmesh.py plans the windows and makes
 * the meshes on the host); the antimeridian; mosaics of several files per map.
 * UNPINNED: GDAL and PROJ are not part of this project's environment, so gdal.Warp's own choice of the nearest pixel, its
 * approximate transformer (0.125 pixel error threshold) and its handling of a centre exactly on a pixel boundary are not
 * pinned by any test.  The definition below is this project's own.
 * THE DEFINITION, by reference to the two sections it joins.  For every tile
 *                  land == dswx_landcover_mask(W3, CG, forest_classes, thresholds, year_offset)
 *   W3         uint8 [3 height][3 width]: the `dst` of dswx_warp_* (elem_bytes 1) of the WorldCover plane -- tiles of wc_h x wc_w,
 *              wc_tile_stride apart -- through mesh_wc with shift_wc and outside_wc onto a destination of 3 height x 3 width.
 *   CG         uint8 [height][width]: the `dst` of dswx_warp_* of the CGLS plane -- tiles of cg_h x cg_w, cg_tile_stride apart --
 *              through mesh_cg with shift_cg and outside_cg onto a destination of height x width.
 *   MESHES     as in the "warp" section, one per map: mesh_wc has ((3 height + step - 1) >> shift_wc) + 1 rows of nodes,
 *              mesh_cg ((height + step - 1) >> shift_cg) + 1, columns likewise.  ANY CONTENT IS LEGAL, INT32_MIN and INT32_MAX
 *              included.  The POSITION of a pixel is the one of that section and no other.
 *   land       uint8 [n_tiles][land_tile_stride], the first height * width bytes of every tile written, the rest untouched:
 *              the 3 x 3 counts of W3, the forest test of CG, the hierarchy and the uint8 wrap of the two developed classes
 *              exactly as dswx_landcover_mask_* state them.  NULL = not wanted.
 *   head       uint64 [n_tiles][DSWX_LAND_MESH_HEAD_WORDS]: word 0 the HLS pixels, 1 the fine pixels whose WorldCover tap was
 *              inside, 2 those whose tap was outside, 3 the HLS pixels whose CGLS tap was inside, 4 those whose tap was outside,
 *              5 the HLS pixels whose nine WorldCover taps were ALL outside, 6 the LAND pixels equal to 255, 7 zero.  NULL =
 *              not wanted.  (Words 2 and 4 not zero: a map does not cover the tile.)
 * height * width <= 2^30 / 9 (the fine lattice stays within the warp's limit) and wc_h * wc_w, cg_h * cg_w <= 2^30.  n_tiles ==
 * 0 or an empty lattice writes nothing; an empty source raster makes every tap `outside`.  Integer arithmetic only: the result
 * does not depend on the launch geometry, and the atomics of `head` (additions) commute. */
#define DSWX_HAS_LAND_MESH 1
#define DSWX_LAND_MESH_HEAD_WORDS 8
typedef struct dswx_land_mesh_spec {
    int32_t  shift_wc;                     /* 0 .. DSWX_WARP_MAX_SHIFT: a node of mesh_wc every 1 << shift_wc FINE pixels */
    int32_t  shift_cg;                     /* 0 .. DSWX_WARP_MAX_SHIFT: a node of mesh_cg every 1 << shift_cg HLS pixels */
    uint32_t outside_wc;                   /* 0 .. 255: the WorldCover byte of a tap that is not inside */
    uint32_t outside_cg;                   /* 0 .. 255: the CGLS byte of a tap that is not inside */
    int32_t  thresholds[4];                /* as dswx_landcover_mask_*: evergreen, low- and high-intensity developed, water */
    int32_t  year_offset;                  /* as dswx_landcover_mask_* */
    int32_t  n_forest_classes;             /* >= 0 */
    int32_t  reserved;                     /* must be 0 */
    int32_t  reserved2;                    /* must be 0 (padding in front of the pointer) */
    const int32_t* forest_classes;         /* HOST memory, read before the call returns; NULL only with n_forest_classes 0 */
    int64_t  wc_tile_stride;               /* bytes between the tiles of the WorldCover plane; 0 = wc_h * wc_w */
    int64_t  cg_tile_stride;               /* bytes between the tiles of the CGLS plane; 0 = cg_h * cg_w */
    int64_t  mesh_wc_tile_stride_nodes;    /* nodes between the meshes of consecutive tiles; 0 = one mesh for all tiles */
    int64_t  mesh_cg_tile_stride_nodes;    /* likewise */
    int64_t  land_tile_stride;             /* bytes between the LAND rasters of consecutive tiles; 0 = height * width (the
                                              LAND plane of a resident batch: dswx_batch_geom_t.tile_stride) */
} dswx_land_mesh_spec_t;                   /* 96 bytes */
/* The two planes and the two meshes in DEVICE memory -> land and head (device memory).  Asynchronous on `stream` (NULL = the
 * context's stream): one hipMemsetAsync of `head` (only if wanted) and ONE kernel launch, whatever the tile count (past the
 * 65535 tiles of grid.y the workgroups walk the tiles); no synchronisation, no scratch of the context, no allocation, nothing
 * the caller has to zero in front: a second call on the same outputs gives the same bytes, and no workgroup ever waits for
 * another.  Refusals, in the order and with the texts of dswx_warp_device and dswx_landcover_mask_*: a NULL spec, a shift
 * outside 0 .. 8, reserved or reserved2 != 0, outside_wc or outside_cg above 255, a negative forest count or a NULL list with a
 * positive one (the thresholds are part of the spec and cannot be NULL), height * width above 2^30 / 9; per map (WorldCover
 * first) a negative size, tile count or stride, a source above 2^30 pixels, a stride that is neither 0 nor large enough, more
 * than 2^32 tiles or a plane above 2^46 bytes; a land_tile_stride that is neither 0 nor at least height * width; with something
 * to write (land or head), a NULL mesh or a NULL plane whose raster is not empty: DSWX_ERR_ARG.  A mesh off 4 bytes or
 * head off 8: DSWX_ERR_ALIGN (the planes and land are bytes).  The arguments are checked before the context is, and a refused
 * call writes nothing.  land and head both NULL is no work, not an error.  Overlap is NOT CHECKED. */
int dswx_land_mesh_device(dswx_ctx_t* ctx, const uint8_t* worldcover, int64_t wc_h, int64_t wc_w, const uint8_t* copernicus,
                          int64_t cg_h, int64_t cg_w, const dswx_land_mesh_spec_t* spec, int64_t n_tiles, int64_t height,
                          int64_t width, const int32_t* mesh_wc_device, const int32_t* mesh_cg_device, uint8_t* land,
                          uint64_t* head, void* stream);
/* The same definition on HOST buffers in plain scalar C++, with HOST meshes: needs no device and no context.  The other half of
 * a comparison, not a fallback.  The refusals of dswx_land_mesh_device, except that every buffer may sit at any address. */
int dswx_land_mesh_host(const uint8_t* worldcover, int64_t wc_h, int64_t wc_w, const uint8_t* copernicus, int64_t cg_h,
                        int64_t cg_w, const dswx_land_mesh_spec_t* spec, int64_t n_tiles, int64_t height, int64_t width,
                        const int32_t* mesh_wc_host, const int32_t* mesh_cg_host, uint8_t* land, uint64_t* head);

/* ---- device plumbing for hosts without another HIP binding ------------------- */
int dswx_device_malloc(dswx_ctx_t* ctx, size_t bytes, void** out);
int dswx_device_free(dswx_ctx_t* ctx, void* ptr);
/* Page-locked host memory.  dswx_classify_host() recognises buffers allocated HERE and, when
 * EVERY plane lies inside such a buffer, works on them in place: the host planes are mapped into
 * the device's address space and the kernels read the inputs and write the layers across PCIe
 * themselves (zero copy, both directions at once, every mode) instead of the synchronous
 * copy-compute-copy sequence.  Any other memory -- pageable, or page-locked by the caller with
 * hipHostRegister, whose pages need not be resident -- is copied.  There is no reference
 * counterpart (numpy arrays are pageable); results are identical. */
int dswx_host_alloc(dswx_ctx_t* ctx, size_t bytes, void** out);
/* ctx may be NULL here (a span may outlive the context it was allocated through). */
int dswx_host_free(dswx_ctx_t* ctx, void* ptr);
int dswx_memcpy_h2d(dswx_ctx_t* ctx, void* dst, const void* src, size_t bytes);
int dswx_memcpy_d2h(dswx_ctx_t* ctx, void* dst, const void* src, size_t bytes);
int dswx_memset_d(dswx_ctx_t* ctx, void* dst, int value, size_t bytes);      /* complete on return, like the two copies above */
/* asynchronous on `stream` (NULL = the context's stream); the host side must be page-locked (dswx_host_alloc) for the
 * copy to overlap with anything */
int dswx_memcpy_h2d_async(dswx_ctx_t* ctx, void* dst, const void* src, size_t bytes, void* stream);
int dswx_memcpy_d2h_async(dswx_ctx_t* ctx, void* dst, const void* src, size_t bytes, void* stream);
int dswx_stream_synchronize(dswx_ctx_t* ctx, void* stream);
/* HIP events on the stream the kernels run on (timing for bench.py) */
int dswx_event_create(dswx_ctx_t* ctx, void** out);
int dswx_event_destroy(dswx_ctx_t* ctx, void* event);
int dswx_event_record(dswx_ctx_t* ctx, void* event, void* stream);
int dswx_event_elapsed_ms(dswx_ctx_t* ctx, void* start, void* stop, float* ms);

/* Name and launch geometry of the kernel the last dswx_classify_* / dswx_*checksum* / dswx_*compare* / dswx_*histogram* /
 * dswx_*crosstab* / dswx_*stack* / dswx_*grid* / dswx_*label* / dswx_*body_table* / dswx_*distance* / dswx_*outline* / dswx_*burn* / dswx_*mosaic* / dswx_*warp* / dswx_*resample* / dswx_land_mesh_device call on this context selected (for profiles / DESIGN.md; the
 * histogram's, the crosstab's, the stack's and the grid's also name their replica count): writes a NUL-terminated string. */
int dswx_last_kernel_info(dswx_ctx_t* ctx, char* buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* DSWX_HIP_H */
