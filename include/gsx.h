/*
 * gsx.h — C ABI of libgsx.so: MI355X (gfx950) Gaussian-splat majority-vote labeler + rasterizer.
 *
 * Plain C types only (pointers, sizes, PODs); no C++ or torch types cross this boundary.
 * The reference (GloireLINVANI/3D_Gaussian_Splatting_Project) has no FFI: its hot path lives
 * behind Python functions.  Each entry point names the reference lines it replaces
 * (dls.py = deep_learning_segmentation.py, gs.js = Web_Viewer_Gaussians_Selection/gaussians_selection.js).
 *
 * Conventions
 *   - every function returns GSX_OK (0) or a negative gsx_status; gsx_last_error() has the text.
 *   - "not visible" / "no vote" are ordinary results, never errors (dls.py:73,82,306).
 *   - host pointers are read/written during the call only; the library never keeps them.
 *   - device pointers returned by *_device() accessors stay valid until the next gsx_vote_begin /
 *     gsx_upload_* on the same ctx, and belong to the ctx.
 *   - one ctx = one GPU = one HIP stream (gsx_render_views and the early vote add internal ones); a ctx is used from one host
 *     thread at a time; the library runs its own worker threads for host-side packing and the second render stream.
 *   - there is NO CPU fallback: without a gfx950 device gsx_create fails with GSX_E_HIP.
 */
#ifndef GSX_H
#define GSX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSX_ABI_VERSION 2

typedef enum gsx_status {
    GSX_OK = 0,
    GSX_E_INVALID = -1,     /* bad argument (NULL, negative size, unknown enum)            */
    GSX_E_HIP = -2,         /* a HIP runtime call failed / no usable device               */
    GSX_E_STATE = -3,       /* call order violated (e.g. vote_view before vote_begin)     */
    GSX_E_RANGE = -4,       /* a seg-map label outside [-1, n_classes-1], too many views  */
    GSX_E_UNSUPPORTED = -5, /* configuration outside what the kernels are built for       */
    GSX_E_IO = -6           /* PLY file could not be read / written                       */
} gsx_status;

typedef struct gsx_ctx gsx_ctx;

/* One entry of cameras.json (dls.py:17-22, 54-63; gs.js:81-107).  All fp64, as JSON gives. */
typedef struct gsx_camera {
    double fx, fy;
    int32_t width, height;
    double R[9]; /* "rotation", row-major 3x3 */
    double p[3]; /* "position" */
} gsx_camera;

/* element type of a segmentation map handed to gsx_vote_view* (dls.py:124,142,158) */
typedef enum gsx_seg_dtype {
    GSX_SEG_I32 = 0, /* int32, values in [-1, n_classes-1]  (YOLO / Mask2Former maps)      */
    GSX_SEG_I64 = 1, /* int64, same range                    (SegFormer argmax)             */
    GSX_SEG_U8 = 2,  /* uint8 holding label+1 (0 = label -1): the compact on-device form   */
    GSX_SEG_U8_LABELS = 3 /* uint8 holding the label itself, 0 .. n_classes-1 (a class map stored
                        * as an 8-bit image; it cannot express -1)                          */
} gsx_seg_dtype;

/* element type of a binary mask handed to gsx_iou_masks* / gsx_masks_top_index (ev.py = Image_Segmentation/evaluation.py).
 * A pixel is SET iff value != 0 (ev.py:29-30), compared on the whole element: NaN, infinities, denormals, 256 and 2^32 are
 * set, -0.0 is not. */
typedef enum gsx_mask_dtype {
    GSX_MASK_U8 = 0,  /* uint8, also numpy / torch bool */
    GSX_MASK_I32 = 1,
    GSX_MASK_I64 = 2,
    GSX_MASK_F32 = 3,
    GSX_MASK_F64 = 4
} gsx_mask_dtype;

/* element type of a network output handed to gsx_segmap_from_logits / gsx_segmap_from_masks.  fp16 and bf16 are compared by
 * value, with no rounding step: every one of their values is an fp32 value. */
typedef enum gsx_float_dtype {
    GSX_F32 = 0,
    GSX_F16 = 1,
    GSX_BF16 = 2
} gsx_float_dtype;

/* ---------------------------------------------------------------------------------------------
 * context
 * ------------------------------------------------------------------------------------------- */
int gsx_abi_version(void);
/* number of HIP devices visible to this process (0 if none / no driver) */
int gsx_device_count(void);
/* device_id: HIP device ordinal of this process's GPU.  Fails (GSX_E_HIP) if the device is
 * missing or is not gfx950. */
int gsx_create(int device_id, gsx_ctx** out);
void gsx_destroy(gsx_ctx* ctx);
/* ctx may be NULL: returns the calling thread's last error raised without a ctx */
const char* gsx_last_error(const gsx_ctx* ctx);
/* the ctx's hipStream_t (as void*) on which every kernel of this ctx is launched */
void* gsx_stream(gsx_ctx* ctx);
int gsx_synchronize(gsx_ctx* ctx);
/* tuning knobs; none of them changes any result.
 *   "spatial_sort" (default 1)  Morton-order the Gaussians on the GPU at upload: a wave's 64 Gaussians
 *                               then project to neighbouring pixels (seg-map gathers hit few lines)
 *   "xcd_swizzle"  (default 32) which workgroups of the vote kernels share an XCD and its L2: 0 = hardware order,
 *                               1 = XCD x takes the x-th contiguous eighth of the Morton curve, C >= 2 = the curve
 *                               is cut into chunks of C workgroups dealt round-robin to the XCDs (compact pieces
 *                               of space per L2, and all XCDs finish together)
 *   "vote_unroll"  (default 8)  views whose seg-map gathers are in flight together: 2, 4, 8
 *   "flat_project" (default 1)  the projection as one straight-line block (all rows, both divisions, one predicate at
 *                               the end, one wave-uniform depth early-out) instead of the reference's three early
 *                               returns as divergent branches; same operations on the same operands
 *   "wave_cull"    (default 1)  skip a view for a whole wave when the bounding sphere of its 64 Gaussians lies
 *                               outside the view's frustum by a safety margin (see gsx_debug_cull_planes).  Skips
 *                               33 % of the (wave, view) pairs of the benchmark scene, bit-identical results.  On its
 *                               own it measured 3-5 % slower (the kernel waited on seg-map gathers, which invisible
 *                               pairs never issued); together with "seg_coarse" it is worth 12 %
 *   "filter_project" (default 1) the two IEEE divisions of the projection are preceded by an fp32 filter (one v_rcp_f32, two
 *                               v_fma_f32) with a proven error bound: a wave whose lanes are all farther than the bound from
 *                               every pixel boundary takes floor() of the filter's result, any other wave the exact
 *                               divisions for that view (about one wave and view in ten at 1080p).  Bit-identical by
 *                               construction (csrc/vote_device.hpp: project_filtered; gsx_debug_filter_check)
 *   "host_compact" (default 1)  host maps (gsx_vote_view) cross PCIe as their coarse level plus the 16-byte blocks of the
 *                               mixed 4x4 cells only, and a kernel behind the DMA rebuilds the pool form (the link, not
 *                               the host pass, is what the hand-over of 200 1080p maps waits for); 0 = the pool form
 *                               itself crosses the link.  Same pool bytes, same labels
 *   "early_vote"   (default 1)  a run whose views all arrive on this context through gsx_vote_view (first_view 0, at most
 *                               255 announced, >= 32 of them, >= 2^18 Gaussians) votes its first views on a second stream
 *                               while the host is still handing over the rest; gsx_vote_finalize then walks only the views
 *                               behind them on top of the early counts (with more than 255 announced views: every batch of
 *                               <= 255 views but the last starts its count kernel when it is staged).  Same labels, bit for bit.  0 = off, 2 = whatever
 *                               the run's size (tests).  "early_vote_at": the stage starts when this many permille of the
 *                               announced views are staged; 0 (default): chosen from the run's own hand-over rate so
 *                               that the stage ends as the last map arrives (between 50 and 88 %)
 *   "early_replay" (default 1)  the form of the early vote: 1 = the early stage only RECORDS every vote (no histogram, no LDS:
 *                               0.73 ms of GPU time for 160 of 200 views at 3 M Gaussians), the last stage replays the record
 *                               behind its own walk in the one-piece kernel's order; 0 = the early stage keeps count and
 *                               first-view planes (1.85 ms, 0.9 GB more memory) and the last stage folds them in.  Same
 *                               labels, same span within the run-to-run spread (round 3 made the cheaper one the default)
 *   "labels_u8"    (default 1)  labels leave the device as one byte each (label + 1) and are widened on the host
 *                               (gsx_vote_finalize); 0 = int32 over the link
 *   "exchange_slabs" / "exchange_local"  plane layout of exchange protocol v2, see gsx_vote_slab_reduce
 *   "blend_pk2"    (default 2)  rasterizer: 0 = one pixel per thread, 1 = two (packed fp32), 2 = four (one wave per tile,
 *                               staging chunks of 64 records, the "tile opaque" vote every 16)
 *   "render_phases" (default 2) rasterizer: a frame is binned, sorted and blended front to back in this many DEPTH
 *                               PHASES (1..8); a phase skips the tiles the earlier ones left opaque (1 - alpha <
 *                               1e-5 on every pixel), so a dense scene sorts a few times the (tile, splat) pairs the
 *                               blend consumes instead of all of them (3 M splats @1080p: 23.3 M pairs -> 7.2 M with 2
 *                               phases, 2.2 M consumed; with "render_bin32" and "render_compact": 2.75 M (bin, splat) pairs for
 *                               1.2 M records evaluated).  What is skipped could not have moved a channel by 1e-5
 *   "render_phase_ratio" (default 6)  phase p ends after nvis / ratio^(K-1-p) splats of the depth order (2..64), nvis = the
 *                               splats the level-1 sort keeps ("render_compact")
 *   "render_compact" (default 1) rasterizer: the splats without a tile rectangle in the view (behind the camera, off the frame,
 *                               between the pixel centres, dropped by the JS sort's quirk) get a key that the FIRST pass of
 *                               the level-1 radix sort leaves out - a stable LSD pass is an order-preserving partition
 *                               anyway - so the second pass, the bin kernels and their scans see only the others; the
 *                               depth phases are cut on the device from their count.  0 = every splat is sorted (the
 *                               phases are then cut from n: the best ratio was 4)
 *   "render_frames" (default 4) gsx_render_views: frames in flight, each on a HIP stream of its own (1..6; 935 / 1252 /
 *                               1359 / 1396 / 1296 / 1349 views/s with 1..6 at 3 M splats @1080p SH 3: four streams for the
 *                               four hardware queues)
 *   "render_multi_pre" (default 1)  gsx_render_views: ONE pre pass (depth keys, vertex shader, colours, tile rectangles) per
 *                               group of frames in flight instead of one per frame: a splat's texel pair and SH coefficients
 *                               are read once for all views of the group (168 MB per view instead of 816 at 3 M splats, SH
 *                               3).  Bit-identical frames
 *   "render_bin32" (default 1)  rasterizer: the (list, splat) pairs are binned, sorted and ranged by 32x32-pixel BINS (2x2 tiles);
 *                               a pair's value carries the mask of the bin's tiles the splat's rectangle covers (and that
 *                               are not opaque yet), and a tile's blend wave takes the entries of its bin's list that name
 *                               it, in list order: 7.45 M -> 2.87 M pairs per view at 3 M splats @1080p, 1610-1650 ->
 *                               1910-1960 views/s, frames bit-identical.  Needs "blend_pk2" = 2, "exact_cull" = 0 and
 *                               fewer than 2^28 splats; otherwise (or with 0) the lists are per 16x16 tile
 *   "render_wide_sort" (default 1) rasterizer: with at most 2048 lists (32x32-pixel bins up to about 1440p) the pair sort is ONE radix
 *                               pass over the whole 11-bit key whose digit bases are the lists' ranges (no second pass, no ranges
 *                               kernel, no keys written): 1 = for a frame on its own (gsx_render_view: 6 % less kernel time), 2 =
 *                               also with several frames in flight (measured 1 % slower there: its stores are scattered), 0 = never.
 *                               The same lists, bit-identical frames
 *   "render_share_stream" (default 1)  gsx_render_views: the first extra frame runs on the context's second stream (the
 *                               early vote's) instead of one more stream - a context that has labelled before would
 *                               otherwise hold five streams for four hardware queues (1120 instead of 1340 views/s)
 *   "exact_cull"   (default 0)  rasterizer: bin a splat only into the tiles its |vPosition| <= 2 ellipse reaches
 *                               (minimum of the quadratic over the tile), not its whole bounding box.  The binning
 *                               is wave-cooperative (no lane walks a rectangle on its own), yet on the 3 M-splat
 *                               scene the test still costs more (+0.18 ms) than the 23 % fewer pairs save (-0.07)
 *   "tile_lpt"     (default 0)  rasterizer: blend the tiles with the longest splat lists first (measured:
 *                               blend -3 %, paid back by the extra ordering launches; per-tile lists only: ignored
 *                               while "render_bin32" is in effect)
 *   "seg_tiled"    (default 1)  keep the u8 seg maps as strips of 16 pixel columns (16x8 pixels per 128-B line;
 *                               applies to the views staged after the call)
 *   "batched_counts" (default 1) more than 255 views on one GPU: one fast u8-histogram launch per batch of <= 255 views
 *                               into its own count plane, then the sparse tie pass of exchange protocol v3 across
 *                               the batches (0: accumulate 16-bit count and first-view planes instead)
 *   "seg_coarse"   (default 1)  keep a second, 4x4-coarsened level of every strip-stored map (a cell holds the label
 *                               its 16 pixels share, or 255) and look a vote up there first; only lanes that hit a
 *                               mixed cell read the full-resolution map.  Same labels; a wave then touches ~3 cache
 *                               lines per view instead of ~16 (HBM traffic per launch 5.2 GB -> 0.5 GB).  Needs
 *                               n_classes <= 254, unit scale and "seg_tiled"; otherwise the one-level path runs
 *   "iou_table_lds" (default 1) gsx_iou_label_maps*: a table of up to 40000 entries is counted in a u32 copy in LDS per
 *                               workgroup and flushed once; 0 = every add goes to the global u64 table (the path of larger
 *                               tables).  Same tables
 *   "smooth_search" (default 0) gsx_smooth_labels: 1 = the search form (no stored lists, a class table in LDS) for k <= 64 too,
 *                               where the default runs over lists.  Same labels, support and changed counts */
int gsx_set_option(gsx_ctx* ctx, const char* name, int64_t value);
/* the current value of an option that other code overrides for a while and has to put back: "early_vote", "early_vote_at",
 * "early_replay", "seg_tiled", "seg_coarse"; GSX_E_INVALID for any other name */
int gsx_get_option(gsx_ctx* ctx, const char* name, int64_t* value);

/* ---------------------------------------------------------------------------------------------
 * scene upload — replaces load_gaussians (dls.py:25-40), which keeps only x,y,z
 * ------------------------------------------------------------------------------------------- */
/* SoA host arrays of n floats each */
int gsx_upload_positions(gsx_ctx* ctx, int64_t n, const float* x, const float* y, const float* z);
/* AoS rows (e.g. the vertex rows of a 3DGS PLY): float at base + i*stride_bytes + off_{x,y,z} */
int gsx_upload_positions_strided(gsx_ctx* ctx, int64_t n, const void* base, int64_t stride_bytes,
                                 int64_t off_x, int64_t off_y, int64_t off_z);
int64_t gsx_num_gaussians(const gsx_ctx* ctx);

/* ---------------------------------------------------------------------------------------------
 * parity probe for project_gaussian (dls.py:43-82): one position through the device kernel.
 * *visible = 0 where the reference returns None; then *x = *y = -1.
 * ------------------------------------------------------------------------------------------- */
int gsx_project_one(gsx_ctx* ctx, const float pos[3], const gsx_camera* cam, int32_t* x, int32_t* y,
                    int32_t* visible);
/* batch form over the uploaded positions: x,y are host arrays of n int32 (-1 = not visible) */
int gsx_project_all(gsx_ctx* ctx, const gsx_camera* cam, int32_t* x, int32_t* y);

/* ---------------------------------------------------------------------------------------------
 * majority vote — replaces the loop body and arg-max of assign_labels (dls.py:252-308)
 *
 *   gsx_vote_begin        gaussian_votes = {}                                   dls.py:252
 *   gsx_vote_view*        one iteration of `for camera in cameras` whose PNG exists.  The caller
 *                         keeps the skip of missing images (dls.py:256-259): views are numbered
 *                         by the caller in processing order.                    dls.py:255-295
 *   gsx_vote_finalize     arg-max, first-inserted label wins ties, -1 if never visible
 *                                                                               dls.py:297-308
 * Views are staged in device memory (compact u8 maps) and consumed by ONE fused kernel launch at
 * flush/finalize time; they stay resident until the next gsx_vote_begin so that a run can be
 * repeated (gsx_vote_rewind) without re-uploading.
 * ------------------------------------------------------------------------------------------- */
/* n_classes: labels are -1 .. n_classes-1 (1 <= n_classes <= 255: the on-device maps are u8).
 * first_view / total_views: this ctx will receive the global view indices
 * [first_view, first_view + k); total_views is the number of views over ALL ranks (sizes the
 * counters: <= 65535).  Single GPU: first_view = 0, total_views = number of views (upper bound ok). */
int gsx_vote_begin(gsx_ctx* ctx, int32_t n_classes, int32_t first_view, int32_t total_views);
/* seg: HOST pointer, seg_h x seg_w row-major.  img_w,img_h: the PIL image size (dls.py:261-263).
 * The map is read during the call (worker threads narrow it to u8 bins and check the label range: GSX_E_RANGE fails THIS
 * call and stages nothing) and written into pinned memory in a compact transfer form - the 4x4-coarsened level plus one
 * 16-byte block per cell whose pixels differ (option "host_compact"); one asynchronous DMA per group of up to 16 maps moves
 * the records and a kernel queued behind it rebuilds the two-level on-device map.  Nothing is synchronised: 200 calls
 * cost the host pass over the maps (the link carries ~0.3 MB per 1080p map of an ordinary segmentation, 2.2 MB at worst).
 * Option "host_threads" sizes the worker pool; default 0 = gsx_default_host_threads(): min(16, usable CPUs), where the usable
 * CPUs are the affinity mask capped by the cgroup's CPU quota and divided by LOCAL_WORLD_SIZE (the ranks torch.distributed.run
 * started on this node: one process per GPU share the node's CPUs); env GSX_HOST_THREADS overrides it.
 * Option "host_pack" = 0 selects the alternative hand-over: the workers only copy the raw map into pinned memory, the raw
 * bytes cross PCIe (4x as many for int32) and the fused kernel of gsx_vote_view_device packs them; the range check is
 * then the deferred device-side one.  Measured slower on the GPU box; for hosts short of cores. */
int gsx_vote_view(gsx_ctx* ctx, const gsx_camera* cam, const void* seg, int32_t seg_dtype, int32_t seg_w,
                  int32_t seg_h, int32_t img_w, int32_t img_h);
/* same, seg is a DEVICE pointer (e.g. the segmentation model's output tensor on this GPU): one fused kernel on
 * the ctx stream (gsx_stream) reads it once and writes both map levels; the caller orders that stream after the
 * producer of the map and keeps the map alive until the stream has passed (gsx_synchronize, an event, ...).
 * Nothing is read back here: a label outside [-1, n_classes-1] is recorded on the device and fails the call that
 * hands out the labels (gsx_vote_finalize, gsx_vote_labels_from_*) with GSX_E_RANGE, naming the view. */
int gsx_vote_view_device(gsx_ctx* ctx, const gsx_camera* cam, const void* seg_dev, int32_t seg_dtype,
                         int32_t seg_w, int32_t seg_h, int32_t img_w, int32_t img_h);
/* n device maps of one geometry and dtype, views in array order: 16 maps per kernel launch (a 1080p map is ~2 us
 * of HBM time, less than a launch).  cams[n], segs_dev[n]. */
int gsx_vote_views_device(gsx_ctx* ctx, int32_t n, const gsx_camera* cams, const void* const* segs_dev, int32_t seg_dtype,
                          int32_t seg_w, int32_t seg_h, int32_t img_w, int32_t img_h);
int32_t gsx_vote_num_views(const gsx_ctx* ctx);
/* forget accumulated votes but keep the staged views: the next flush/finalize votes them again */
int gsx_vote_rewind(gsx_ctx* ctx);
/* single-GPU end: runs the fused kernel (+ arg-max) and leaves int32 labels on the device.
 * labels_out: host array of n int32, or NULL to skip the device-to-host copy.  A label is -1 .. 254, so the copy moves
 * ONE byte per Gaussian (label + 1) into pinned memory and the worker threads widen it into labels_out (option
 * "labels_u8" = 0: int32 over the link, the A/B of DESIGN.md section 3). */
int gsx_vote_finalize(gsx_ctx* ctx, int32_t* labels_out);
/* device pointer of the n int32 labels written by gsx_vote_finalize / gsx_vote_labels_from_keys */
void* gsx_vote_labels_device(gsx_ctx* ctx);

/* ---- multi-GPU exchange (views sharded over ranks; one process per GPU) ----------------------
 * rank-local:  gsx_vote_flush            fused kernel -> per-Gaussian vote histogram planes
 * exchange 1:  all-reduce SUM (int32 words) over gsx_vote_counts_device()   [the histogram]
 * rank-local:  gsx_vote_tiebreak_keys    per Gaussian: max-count bins -> (earliest view, bin) key
 * exchange 2:  all-reduce MAX (int32) over gsx_vote_keys_device()           [n words]
 * rank-local:  gsx_vote_labels_from_keys
 * The counts plane packs 8- or 16-bit counters into int32 words so that an int32 SUM is exact
 * (total votes per bin <= total_views, which fits the counter). */
int gsx_vote_flush(gsx_ctx* ctx);
void* gsx_vote_counts_device(gsx_ctx* ctx, int64_t* n_int32_words);
int gsx_vote_tiebreak_keys(gsx_ctx* ctx);
void* gsx_vote_keys_device(gsx_ctx* ctx, int64_t* n_int32_words);
int gsx_vote_labels_from_keys(gsx_ctx* ctx, int32_t* labels_out);
/* ---- multi-GPU exchange, protocol v2: all-to-all instead of all-reduce (SURVEY.md section 5's preferred shape)
 * Set the options "exchange_slabs" = world size and "exchange_local" = 1 BEFORE gsx_vote_begin: the planes
 * become u8 [slab][bins][sn] with per-rank counters (<= 255 views per rank) and LOCAL first-view codes.
 *   rank-local:  gsx_vote_flush
 *   exchange 1:  all_to_all (equal splits) over gsx_vote_counts_device() and over gsx_vote_first_device():
 *                rank j receives slab j of every rank, [src rank][bins][sn]           -- 2 x bins*n/world bytes/peer
 *   rank-local:  gsx_vote_slab_reduce(recv_counts, recv_first): sums the counters and resolves ties by
 *                (lowest rank, earliest local view) = globally earliest view, since ranks own contiguous
 *                rank-ordered view blocks -> sn int32 labels of this rank's slab at gsx_vote_keys_device()
 *   exchange 2:  all_gather of the slab labels -> slabs*sn int32 in Morton (upload) order
 *   rank-local:  gsx_vote_labels_from_sorted(all_labels_dev, labels_out): back to the caller's order */
void* gsx_vote_first_device(gsx_ctx* ctx, int64_t* n_int32_words);
/* ---- protocol v3: counts-only all-to-all + a sparse tie pass (same options as v2) -------------------------
 * Only the COUNT plane crosses the fabric (half of v2's bytes) and it comes out of the fast u8-histogram
 * kernel; first-view information is computed afterwards, for the tied Gaussians only.
 *   rank-local:  gsx_vote_flush_counts        u8 count plane [slab][bins][sn] at gsx_vote_counts_device()
 *   exchange 1:  all_to_all over the count plane
 *   rank-local:  gsx_vote_slab_totals(recv)   unique maximum -> label; otherwise label -2 and the set of
 *                                             max-count bins as a bit mask, u32 [8][sn] at gsx_vote_cand_device()
 *   exchange 2:  all_gather of the masks -> [slab][8][sn]
 *   rank-local:  gsx_vote_tie_codes(masks)    tied Gaussians only: walk this rank's views in forward order, stop
 *                                             at the first one voting a candidate -> u16 codes [slab][sn]
 *                                             ((255 - local view) << 8 | bin) at gsx_vote_codes_device()
 *   exchange 3:  all_to_all over the codes (2 bytes per Gaussian)
 *   rank-local:  gsx_vote_tie_resolve(recv)   lowest rank with a code wins = globally earliest view
 *   exchange 4:  all_gather of the slab labels (gsx_vote_keys_device), then gsx_vote_labels_from_sorted */
int gsx_vote_flush_counts(gsx_ctx* ctx);
int gsx_vote_slab_totals(gsx_ctx* ctx, const void* recv_counts_dev);
void* gsx_vote_cand_device(gsx_ctx* ctx, int64_t* n_int32_words);
int gsx_vote_tie_codes(gsx_ctx* ctx, const void* cand_all_dev);
void* gsx_vote_codes_device(gsx_ctx* ctx, int64_t* n_int32_words);
int gsx_vote_tie_resolve(gsx_ctx* ctx, const void* recv_codes_dev);
int64_t gsx_vote_slab_size(const gsx_ctx* ctx);
int gsx_vote_slab_reduce(gsx_ctx* ctx, const void* recv_counts_dev, const void* recv_first_dev);
int gsx_vote_labels_from_sorted(gsx_ctx* ctx, const void* sorted_labels_dev, int32_t* labels_out);
/* ---- protocol v4: views sharded for the hand-over, GAUSSIANS sharded for the vote (bench.py's default for N > 1) ----
 * The packed maps of 200 1080p views are 0.44 GB in total; the dense vote histogram of 3 M Gaussians is 0.45 GB PER
 * RANK.  So the maps cross the fabric, not the votes; no option is needed and the tie rule is the single-GPU one.
 *   rank-local:  gsx_vote_view* for this rank's contiguous, rank-ordered block of views
 *   exchange 0:  every rank learns all (view count, pool bytes) pairs and all view blobs  [tiny; see gsx_vote_export]
 *   rank-local:  gsx_vote_export(chunk): chunk = the largest rank's pool bytes; the rank's pool now spans >= chunk
 *   exchange 1:  all_gather of the pools, chunk bytes per rank, into one caller-owned device buffer
 *   rank-local:  gsx_vote_import: the ctx now holds ALL views, their maps read from the gathered buffer
 *                gsx_vote_slab_labels(rank, world): the fused single-GPU kernel over this rank's slab of the Gaussians
 *                (Morton order) -> slab_size int32 labels at gsx_vote_keys_device()
 *   exchange 2:  all_gather of the slab labels, then gsx_vote_labels_from_sorted
 * A view blob is GSX_VIEW_BLOB_BYTES opaque bytes (the library's view descriptor: camera, map geometry, offset inside
 * the exporting rank's pool); it is only meaningful to another instance of the same library build. */
#define GSX_VIEW_BLOB_BYTES 256
/* reserve_bytes: grow this rank's pool to at least that many bytes (the all-gather reads `chunk` bytes from it).
 * blobs_out (may be NULL): gsx_vote_num_views() * GSX_VIEW_BLOB_BYTES bytes on the host.  *pool_dev: the pool,
 * valid until the next gsx_vote_view* / gsx_vote_begin; *pool_bytes: bytes in use (a multiple of 256). */
int gsx_vote_export(gsx_ctx* ctx, int64_t reserve_bytes, void* blobs_out, void** pool_dev, int64_t* pool_bytes);
/* bytes of this rank's pool in use (what gsx_vote_export reports), without touching the stream: host maps that are packed
 * but whose grouped DMA has not been queued yet are counted; gsx_vote_export queues them */
int64_t gsx_vote_pool_bytes(const gsx_ctx* ctx);
/* statistics: bytes of HOST maps (gsx_vote_view) sent over PCIe since gsx_vote_begin - compact records (option
 * "host_compact") or maps in pool form */
int64_t gsx_vote_link_bytes(const gsx_ctx* ctx);
/* statistics: the run's first views that were voted on a second stream while the rest was still being handed over
 * (option "early_vote"; 0: none, the run is voted in one piece by gsx_vote_finalize) */
int64_t gsx_vote_early_views(const gsx_ctx* ctx);
/* part r contributed part_views[r] views (blobs in part order) whose maps start at byte part_offsets[r] of
 * pool_all_dev (pool_all_bytes long; caller-owned, must stay alive and unchanged until the labels have been fetched).
 * Replaces the views staged so far; global view order = part order.  Blobs are validated against the pool size. */
int gsx_vote_import(gsx_ctx* ctx, int32_t n_parts, const int32_t* part_views, const int64_t* part_offsets, const void* blobs,
                    const void* pool_all_dev, int64_t pool_all_bytes);
/* gsx_vote_import for a run whose maps all share ONE geometry (seg_w x seg_h, images img_w x img_h: a capture from one
 * camera model), without the blobs: every rank holds the whole camera list (load_cameras, dls.py:17-22) and derives the
 * descriptors itself, exactly as gsx_vote_view does - cams[k] is the camera of global view k (part order), view v of part r
 * lies at part_offsets[r] + v * (the pool stride gsx_vote_view gives a map of this geometry under this context's options:
 * all ranks must run the same build with the same options).  No exchange of view blobs is needed then.
 * GSX_E_INVALID, and nothing imported, when the sizes cannot be those of the run: a view of a part would end outside the pool
 * or inside the next part (the caller laid the parts out with another stride than gsx_vote_map_stride(seg_w, seg_h)), or a view
 * this context staged itself has another map size, scale (seg / img), strip size or coarse offset than the derived descriptors
 * (a swapped (h, w), a map_size of another resolution, a wrong image size). */
int gsx_vote_import_uniform(gsx_ctx* ctx, int32_t n_parts, const int32_t* part_views, const int64_t* part_offsets, const gsx_camera* cams,
                            int32_t seg_w, int32_t seg_h, int32_t img_w, int32_t img_h, const void* pool_all_dev, int64_t pool_all_bytes);
/* *stride = bytes from one staged map to the next in the pool for maps of seg_w x seg_h under this context's options and class
 * count (after gsx_vote_begin): the packed size (u8 strips of 16 columns, rows padded to 8, + the 4x4-coarsened level; one byte
 * per pixel stands for the int labels of logits.argmax, dls.py:142) rounded up to 256.  What gsx_vote_view advances by and
 * gsx_vote_import_uniform steps by: a multi-rank run sizes its all-gathers from this, never from a rank's own pool. */
int gsx_vote_map_stride(gsx_ctx* ctx, int32_t seg_w, int32_t seg_h, int64_t* stride);
/* *match = 1 when the views this context staged itself are exactly n views of a uniform run as gsx_vote_import_uniform derives
 * them - n of them, view i from cams[i] (camera frame, dls.py:60-66, and seg / img scales, dls.py:267-271) with a seg_w x seg_h
 * map of img_w x img_h images, at byte i * gsx_vote_map_stride of the pool - else 0.  A rank of a run without header exchange asks
 * before it trusts a schedule built on (cameras, map size, image size) alone.  GSX_E_STATE while imported views are in place. */
int gsx_vote_views_match_uniform(gsx_ctx* ctx, int32_t n, const gsx_camera* cams, int32_t seg_w, int32_t seg_h, int32_t img_w,
                                 int32_t img_h, int32_t* match);
/* takes the last gsx_vote_import / gsx_vote_import_uniform back: the context holds this rank's own views in its own pool again
 * (a protocol that imports before it knows whether every rank's pool was what the schedule assumed can fall back) */
int gsx_vote_import_undo(gsx_ctx* ctx);
/* votes the Gaussians [slab * S, min(n, (slab+1) * S)) of the Morton order over all staged views, S = *slab_size =
 * ceil(n / slabs) rounded up to 256; labels (int32, Morton order) at gsx_vote_keys_device()[0 .. S). */
int gsx_vote_slab_labels(gsx_ctx* ctx, int32_t slab, int32_t slabs, int64_t* slab_size);
/* copies of the rank-local planes for tests: counts[bins][n] and first-view codes, widened to u16 */
int gsx_vote_debug_planes(gsx_ctx* ctx, uint16_t* counts_out, uint16_t* first_out);

/* ---------------------------------------------------------------------------------------------
 * rasterizer — the viewer's GPU/worker path (gs.js) as tile-based HIP kernels
 *
 *   gsx_upload_splats    processPlyBuffer gs.js:464-585 (importance order, u8 quantisation, 32-byte
 *                        .splat rows) + generateTexture gs.js:286-357 (4*Sigma as truncated fp16)
 *   gsx_render_view      getViewMatrix/calculateProjectionMatrix gs.js:66-107, runSort gs.js:417-462
 *                        (front-to-back 16-bit depth buckets, stable), vertex shader gs.js:696-750,
 *                        fragment shader + blend gs.js:782-799, 1033-1038
 * Inputs are the 3DGS PLY attributes as float arrays (AoS per attribute, row i = vertex i):
 *   xyz n x 3, scale n x 3 (log), rot n x 4 (w first), opacity n (logit), f_dc n x 3, labels n (or NULL).
 *   scale == NULL selects the viewer's fallback (scale 0.01, identity rotation, gs.js:559-563);
 *   opacity == NULL -> alpha 255 (gs.js:576).
 * Where a splat's importance exp(s0) * exp(s1) * exp(s2) * sigmoid(opacity) is NaN (Infinity * 0) the importance order is
 * unspecified: the reference's sort comparator returns NaN there (gs.js:527).
 * rgba_out: height x width x 4 floats, row 0 = top row, premultiplied colour exactly as the fragment
 * shader emits it (float, not the canvas's 8-bit quantisation); NULL leaves the image on the device.
 * ------------------------------------------------------------------------------------------- */
int gsx_upload_splats(gsx_ctx* ctx, int64_t n, const float* xyz, const float* scale, const float* rot,
                      const float* opacity, const float* f_dc, const int32_t* labels);
/* Optional view-dependent colour: spherical harmonics of degree 0..3 (standard 3DGS real-SH basis,
 * dir = normalize(position - camera position), rgb = clamp(0.5 + SH, 0, 1) in float).  NOT part of the
 * reference (gs.js:565-569 reads only f_dc and quantises it to 8 bits): once this is called the float
 * SH colour replaces rgba8/255; geometry, alpha and depth fade stay the reference's.  f_rest: n x
 * 3*((d+1)^2-1) floats in 3DGS PLY order (f_rest_[c*K1 + k-1]); NULL for degree 0.  Call after
 * gsx_upload_splats; a new gsx_upload_splats switches it off again. */
int gsx_upload_sh(gsx_ctx* ctx, const float* f_rest, int32_t sh_degree);
int64_t gsx_num_splats(const gsx_ctx* ctx);
int gsx_render_view(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, float* rgba_out);
/* n views of one size, F frames in flight (option "render_frames", default 4, 1..6; five and six measured slower than four): the context keeps F - 1 further HIP
 * streams with their own per-frame buffers that share the uploaded scene, and renders view k on stream k % F, each further
 * stream from a host thread of its own - the memory-bound front of one frame overlaps the VALU-bound blend tail of the
 * others (3 M splats / 1080p / SH 3: 935 views/s one at a time, 1252 / 1359 / 1396 with 2 / 3 / 4 in flight).  Same pixels
 * as gsx_render_view.  rgba_out: NULL, or n pointers (each NULL or height x width x 4 floats).  Afterwards
 * gsx_render_num_pairs* report the SUMS over the n views and gsx_render_image_device the last view of the context's own
 * stream (the last k with k % F == 0).  With profiling enabled the views are rendered one at a time. */
int gsx_render_views(gsx_ctx* ctx, int32_t n, const gsx_camera* cams, int32_t width, int32_t height, float* const* rgba_out);
void* gsx_render_image_device(gsx_ctx* ctx);
/* number of (tile, splat) pairs the last gsx_render_view sorted and blended */
int64_t gsx_render_num_pairs(const gsx_ctx* ctx);
/* ... and how many of them the blend kernel actually read (a tile stops once it is opaque) */
int64_t gsx_render_num_pairs_consumed(const gsx_ctx* ctx);
/* Selection hit test — performHitTesting, gs.js:361-395: the label of the splat whose projected centre is
 * nearest to (x, y) (canvas pixels, y measured from the BOTTOM as the viewer's click handler does,
 * gs.js:1377-1378) within 10 px, nearer NDC depth breaking exact ties; NO_SELECTION (-999999) if none.
 * *index_out = importance-order row of that splat or -1.  Uses the splats of gsx_upload_splats; *label_out is the
 * exact int32 that gsx_upload_splats was given for that splat (labelData[i], gs.js:390), not the texture's fp32 copy. */
int gsx_hit_test(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, double x, double y,
                 int32_t* label_out, int64_t* index_out);
/* Label edits — what the viewer does WITH the labels of gsx_upload_splats: highlight, recolour, hide and displace the
 * splats of a label.  The state mirrors the shaders' uniforms and the worker's visibilityMap; it changes how every
 * following gsx_render_view / gsx_render_views frame is drawn (all frames in flight see the same state) and nothing
 * while it is not set: frames without edits are bit-identical to those of a context that never had any.
 *
 *   selection_mode, selected_label   uSelectionMode / uSelectedLabel, gs.js:757-758, 795-797:
 *                                    rgb = mix(rgb, (1, 0, 0), 0.5) for the splats of the selected label
 *   enable_custom_color, custom_color  u_enableCustomColor / u_customColor, gs.js:760-761, 790-792: replaces the rgb of the
 *                                    selected label's splats (before the highlight)
 *   num_colors, color_labels, colors u_numCustomColors / u_customColorLabels / u_customColors, gs.js:762-780, 787 (filled as
 *                                    gs.js:26-42 does): rgb = mix(vColor.rgb, colors[i], 0.6) for the FIRST entry i whose
 *                                    label matches
 *   enable_displacement, num_displacements, displacement_labels, displacements
 *                                    u_enableDisplacement / u_numDisplacements / u_displacementLabels / u_displacementMap,
 *                                    gs.js:674-677, 686-704 (filled as gs.js:906-923): the first matching entry is added to
 *                                    the splat's centre before view * centre; with the flag set a splat without an entry
 *                                    gets + (0, 0, 0) as in the shader
 *   num_hidden, hidden_labels        the labels the worker's visibilityMap holds as false, gs.js:302-307, 320: the alpha
 *                                    byte of their splats is multiplied by 0.  NO_SELECTION (-999999) in the list is
 *                                    ignored as the worker ignores it (gs.js:617-622).
 *
 * Order, as in the fragment shader (gs.js:786-797): table colour, then custom_color, then the highlight.  vColor.rgb already
 * carries the depth fade (gs.js:741), so a table colour is 0.4 * fade * c + 0.6 * colors[i] (NOT faded), and custom_color is
 * not faded at all.  Alpha is never edited except by hiding.  With the SH colour switched on (gsx_upload_sh) vColor.rgb is
 * fade * clamp(0.5 + SH) and the edits apply on top of it in the same order; the SH direction is taken from the UNDISPLACED
 * position.  Neither is pinned by the reference (it has no SH colour).
 *
 * Label compare: the shaders see int(uintBitsToFloat(cen.w)), the label after a round trip through fp32 (gs.js:314, 699);
 * colours, custom_color, highlight and displacements compare THAT value with the int32 entries, so two labels beyond
 * +-2^24 that round to the same float are edited alike.  Hiding compares the exact int32 label (the worker's Map key,
 * gs.js:302-304).
 *
 * Displacement moves the vertex shader's centre only: the cull (gs.js:709-713), the Jacobian, the window position, the tile
 * rectangle and the depth fade.  The DEPTH ORDER DOES NOT MOVE: runSort (gs.js:417-462) reads the worker's buffer, which the
 * live viewer never displaces (nothing posts 'updateDisplacement'), so depth keys, the depth range and the dropped farthest
 * splat stay those of the undisplaced scene, and gsx_hit_test ignores every edit.  A reference quirk, reproduced.
 *
 * A hidden splat stays in the tile lists with alpha 0 (it contributes exactly 0 wherever its fade is finite).
 *
 * gsx_render_set_edits(ctx, NULL) clears the state; so does every gsx_upload_splats (the labels the state was resolved
 * against are gone).  The call resolves the tables ONCE into a 16-bit code per splat (one kernel over the n labels) instead
 * of the shader's two 100-entry loops per splat per frame; the arrays are copied, the caller may free them at once.
 * Errors: GSX_E_INVALID for a count outside 0..100, a NULL hidden_labels with num_hidden > 0, a non-finite colour or
 * displacement; GSX_E_STATE before gsx_upload_splats. */
#define GSX_EDIT_TABLE_MAX 100
typedef struct gsx_render_edits {
    int32_t selection_mode;
    int32_t selected_label;
    int32_t enable_custom_color;
    float custom_color[3];
    int32_t num_colors;
    int32_t color_labels[GSX_EDIT_TABLE_MAX];
    float colors[GSX_EDIT_TABLE_MAX][3];
    int32_t enable_displacement;
    int32_t num_displacements;
    int32_t displacement_labels[GSX_EDIT_TABLE_MAX];
    float displacements[GSX_EDIT_TABLE_MAX][3];
    int64_t num_hidden;
    const int32_t* hidden_labels;
} gsx_render_edits;
int gsx_render_set_edits(gsx_ctx* ctx, const gsx_render_edits* edits);
/* splats the current edit state hides (0 without one) */
int64_t gsx_render_num_hidden(const gsx_ctx* ctx);
/* test hooks (any pointer may be NULL): the packed .splat rows (n x 32 bytes) and importance
 * permutation (gs.js:527), the texture words (n x 8 u32, gs.js:311-353) and the last view's 16-bit
 * depth buckets (65536 = dropped by the JS counting sort, gs.js:443-457) */
int gsx_render_debug(gsx_ctx* ctx, uint8_t* buffer_out, uint32_t* order_out, uint32_t* texdata_out,
                     uint32_t* bucket_out);
/* test hook (any pointer may be NULL): what else an upload left on the device.  labels_out: the n exact int32 labels in
 * importance order (-999999 each without labels).  sh_out: the 3 * K * n floats of the SH planes as laid out by
 * gsx_upload_sh, coef[k][c][j] with K = (degree + 1)^2, k = 0 the f_dc plane, c the channel, j the importance-order row;
 * left alone while the SH colour is off.  *sh_degree_out: the degree 0..3, or -1 while the SH colour is off. */
int gsx_debug_render_scene(gsx_ctx* ctx, int32_t* labels_out, float* sh_out, int32_t* sh_degree_out);
/* test hook: the rasterizer's per-splat pre pass (depth keys, vertex shader, colours, tile rectangles) and the depth-bucket
 * kernel, run on the uploaded scene with the current SH and edit state for num_views cameras (1..6) of one frame size, and what
 * they wrote, per view.  multi = 0: one pre-kernel launch per view, as gsx_render_view issues it; multi = 1: ONE launch of the
 * several-view kernel for all of them, as gsx_render_views issues it per group of frames - in both cases through the launch
 * code of those entry points (grid, arguments, initial depth range).  compact: the option "render_compact" as the bucket kernel
 * sees it.  The pass runs in buffers of the call's own, filled with 0xFF bytes beforehand (a splat without a tile rectangle
 * writes no record: its 48 bytes stay 0xFF); frames rendered afterwards are not affected.  Any pointer may be NULL.
 *   depth   n int32      depth keys, gs.js:436-441           rect         n u32  tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24, 1 = no tile
 *   rec     n x 12 f32   (cx, cy, g0, g1, rgba, 0, 0)        pre          4 int32: min key, max key, splat 0's rect, unused
 *   bucket  n u32        16-bit bucket, 65536 = dropped      key          n u32  level-1 sort key
 *   rect_bucket n u32    rect after the bucket kernel (dropped splats cleared)      dropped  1 int32: splats dropped */
typedef struct gsx_debug_pre_view {
    int32_t* depth;
    uint32_t* rect;
    float* rec;
    int32_t* pre;
    uint32_t* bucket;
    uint32_t* key;
    uint32_t* rect_bucket;
    int32_t* dropped;
} gsx_debug_pre_view;
int gsx_debug_render_pre(gsx_ctx* ctx, int32_t num_views, const gsx_camera* cams, int32_t width, int32_t height, int32_t multi,
                         int32_t compact, const gsx_debug_pre_view* out);

/* ---------------------------------------------------------------------------------------------
 * lifting labeler — class maps lifted onto the splats through the rasterizer's blend.  A second producer of the label
 * field next to the vote: where assign_labels (dls.py:252-308) projects a Gaussian's centre and knows nothing of extent,
 * opacity or occlusion, this one gives every splat the class of the pixels it actually colours.
 *
 * The rule.  For a view (cam, width, height) and a height x width class map with values in [-1, n_classes-1], take the frame
 * exactly as gsx_render_view(ctx, cam, width, height) walks it: same pre pass, quantisation, depth order, tile lists,
 * `discard` rule and ONE_MINUS_DST_ALPHA, ONE blend.  For a pixel p and the k-th fragment at p, made by splat i,
 *     w = (1 - dst.a) * B,   dst.a = the alpha before this fragment,   B = exp(A) * alpha
 * is exactly the increment of the frame's alpha channel, and the view adds w to table[i][map[p] + 1].
 *   - A splat runSort drops gets nothing from that view, and the epilogue's repeated draws of splat 0 (gs.js:453-457) add
 *     nothing either: a viewer quirk that comes last and changes nobody else's transmittance.
 *   - Fixed point: each (pixel, fragment) weight is added as q = rint(w * 2^20), GSX_LIFT_ONE = 1 << 20
 *     (gsx_debug_lift_constants).  Partial sums on the chip are uint32 (a 16x16 tile gives at most 2^28 per record), the table
 *     is uint64, n x (n_classes + 1).  Integer sums do not depend on arrival order: a table is reproducible bit for bit from
 *     run to run, and two views accumulated together equal the sum of their separate tables exactly.
 *   - A lift frame runs as ONE depth phase whatever the option "render_phases" says; the frame's opacity cut stays: a tile
 *     stops once every pixel has 1 - dst.a < 1e-5, so what is left out is below 1e-5 per pixel in total.
 *   - The camera is used as gsx_render_view uses it (the viewer's convention, R^T (x - p), fx and fy against width x height),
 *     NOT as the vote uses it (R (x - p)).  Scaling fx, fy when the map is smaller than the camera's image is the caller's
 *     job (labeler.py does it).
 *   - With a render edit state set (gsx_render_set_edits) the lift calls fail with GSX_E_STATE.
 *   - Finalize, per splat i in the order of the arrays given to gsx_upload_splats (not importance order): total = the sum
 *     of the row; total < ceil(min_weight * 2^20) -> label -1; else the bin with the largest sum, the lowest bin winning a
 *     tie (label -1 is bin 0 and can win like any class, as in the vote).  share = winner / total as a double, 0 where
 *     total is 0.  All comparisons are on the integers.
 * A new gsx_upload_splats (or gsx_destroy) ends a lift run; lift calls before gsx_lift_begin return GSX_E_STATE.
 * ------------------------------------------------------------------------------------------- */
/* 1 <= n_classes <= 255, else GSX_E_INVALID.  Needs gsx_upload_splats (GSX_E_STATE).  Allocates and zeroes the table; a
 * failed allocation is GSX_E_HIP with a message naming the bytes asked for. */
int gsx_lift_begin(gsx_ctx* ctx, int32_t n_classes);
/* seg: HOST pointer, height x width row-major, any gsx_seg_dtype.  The label range is checked on the host before anything
 * is launched: GSX_E_RANGE fails THIS call and adds nothing.  The map has been read when the call returns.  The host waits
 * for the frame's pair count before the lifting kernel runs (a frame whose lists overflow the pair buffers is never counted
 * truncated or twice: the buffers grow first). */
int gsx_lift_view(gsx_ctx* ctx, const gsx_camera* cam, const void* seg, int32_t seg_dtype, int32_t width, int32_t height);
/* same, seg_dev is a DEVICE pointer read on the ctx stream, under the ordering rule of gsx_vote_view_device.  A label out of
 * range is recorded on the device (it counts as -1) and fails gsx_lift_finalize / gsx_lift_table with GSX_E_RANGE, naming
 * the view. */
int gsx_lift_view_device(gsx_ctx* ctx, const gsx_camera* cam, const void* seg_dev, int32_t seg_dtype, int32_t width,
                         int32_t height);
/* views lifted since gsx_lift_begin (0 outside a run) */
int32_t gsx_lift_num_views(const gsx_ctx* ctx);
/* 64-bit global atomics the lifting kernel issued for the last view (statistics, like gsx_render_num_pairs_consumed, which
 * after a lift view reports the records that kernel staged) */
int64_t gsx_lift_num_atomics(const gsx_ctx* ctx);
/* labels_out: n int32; share_out: n doubles or NULL; both in upload order.  min_weight: finite, >= 0.  May be called more
 * than once, and more views may follow. */
int gsx_lift_finalize(gsx_ctx* ctx, double min_weight, int32_t* labels_out, double* share_out);
/* table_out: n x (n_classes + 1) uint64, rows in upload order: for tests and for callers who want soft labels */
int gsx_lift_table(gsx_ctx* ctx, uint64_t* table_out);
/* test hook: out[8] = GSX_LIFT_ONE, its shift, the tile side, records per staged chunk, LDS accumulators per round, classes a
 * mixed wave reduces one by one, the largest n_classes, 0 */
int gsx_debug_lift_constants(int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * label frames — the splats' labels as the class map of a view: which pixels of this view belong to label L?  The transpose
 * of the lifting labeler: where a lift view adds a fragment's weight to table[splat][class of the pixel], a label view adds
 * the same weight to plane[label of the splat][pixel] and takes the arg-max per pixel.
 *
 * The rule.  For a view (cam, width, height) the frame is walked exactly as gsx_lift_view walks it: the same pre pass, depth
 * order and per-tile lists, ONE depth phase and no 32x32 bins, the same `discard` rule, the same opacity cut (a tile stops
 * once every pixel has 1 - dst.a < 1e-5, voted after every 256 records of its list), nothing from the splats runSort drops,
 * nothing from the epilogue's repeated draws of splat 0, the viewer's camera convention (R^T (x - p), fx and fy against
 * width x height; scaling them to a smaller frame is the caller's job).  The k-th fragment at pixel p, made by splat i, has
 *     w = (1 - dst.a) * B
 * and adds q = rint(w * 2^20) (GSX_LIFT_ONE, the lift's fixed point) to plane[label[i] + 1][p]: n_classes + 1 bins per pixel,
 * bin 0 = label -1, all accumulators uint32 (a pixel's total is at most 2^20 plus half a unit per fragment).  Per pixel:
 *     total  = the sum over the bins;
 *     total < max(1, ceil(min_weight * 2^20))  ->  label -1, weight 0;
 *     else the bin with the largest sum, the lowest bin winning a tie (bin 0 = label -1 can win, as in the lift and the
 *     vote); weight = the winner's sum.
 * All comparisons are on the integers: a map is the same bits from run to run.  Both this kernel and the lift's sum the same
 * integers q, so for any class map seg of the view
 *     sum over {p: seg[p] = c} of plane[b][p]  ==  sum over {i: label[i] = b - 1} of gsx_lift_table[i][c + 1]     exactly.
 * The output is a class map in the convention of every map this library takes: int32 in [-1, n_classes - 1], height x width,
 * row 0 = the top row.  gsx_label_map_device hands it to gsx_iou_label_maps_device, gsx_vote_view_device or
 * gsx_lift_view_device without leaving the GPU.
 *
 * The labels are those given to gsx_upload_splats; every one must lie in [-1, n_classes - 1] (checked by one kernel over the
 * n labels, once per upload and n_classes; the device then holds them as one byte per splat in importance order).  To label
 * the frame with other labels, upload again.
 * ------------------------------------------------------------------------------------------- */
/* label_out: height x width int32; weight_out, total_out: height x width uint32; planes_out: n_planes x height x width uint32,
 * plane k = the summed q of label plane_labels[k], zero where that label has no fragment, written in full on every call.  All
 * four are HOST pointers and any of them may be NULL (label_out = NULL leaves the map on the device only); 0 <= n_planes <= 256.
 * The call waits for its results.
 *   GSX_E_STATE        no gsx_upload_splats yet, splats uploaded without labels, a render edit state set (as for the lift),
 *                      gsx_render_views running on this context
 *   GSX_E_INVALID      cam NULL, width or height < 1, n_classes outside [1, 255], min_weight negative or not finite, n_planes
 *                      outside [0, 256] or > 0 without plane_labels, a plane label outside [-1, n_classes - 1]
 *   GSX_E_UNSUPPORTED  more than 4096 pixels per side
 *   GSX_E_RANGE        an uploaded label outside [-1, n_classes - 1]: the message names the first such upload row, nothing
 *                      else is launched
 * A failing call leaves the previous map (gsx_label_map_device) as it was.  The pair buffers are handled as gsx_lift_view
 * handles them: the host waits for the frame's pair count, the buffers grow and the lists are rebuilt before they are walked. */
int gsx_label_view(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, int32_t n_classes, double min_weight,
                   int32_t n_planes, const int32_t* plane_labels, int32_t* label_out, uint32_t* weight_out, uint32_t* total_out,
                   uint32_t* planes_out);
/* the height x width int32 map of the last successful gsx_label_view, device memory owned by the context, written on the ctx
 * stream (NULL before the first); valid until the next gsx_label_view or gsx_destroy */
void* gsx_label_map_device(gsx_ctx* ctx);
/* statistics: walks of a tile's list summed over the tiles of the last view.  A tile whose list holds D label bins walks it
 * ceil(D / WL) times, WL = labels per LDS window (gsx_debug_labelmap_constants); a tile without a list counts 0 */
int64_t gsx_label_num_passes(const gsx_ctx* ctx);
/* statistics: tiles of the last view whose list held exactly one label bin (they walk once and no label competes) */
int64_t gsx_label_num_single_tiles(const gsx_ctx* ctx);
/* test hook: out[8] = GSX_LIFT_ONE, its shift, the tile side, records per staged chunk, labels per window (WL), the largest
 * n_classes (255), 0, 0 */
int gsx_debug_labelmap_constants(int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * depth frames — next to a frame's colour: how far away is the surface at a pixel, and which splat is that surface?
 * gsx_hit_test (the reference's performHitTesting) picks the nearest projected CENTRE within 10 px whatever stands in front of
 * it; gsx_depth_view + gsx_depth_pick pick what the frame shows.
 *
 * The rule.  The frame is gsx_label_view's and gsx_lift_view's, step for step: the same pre pass, depth order and per-tile
 * lists, ONE depth phase and 16x16 tiles, the same `discard` rule, the same opacity cut (a tile stops once every pixel has
 * 1 - dst.a < 1e-5, voted after every 256 records of its list), nothing from the splats runSort drops, nothing from the
 * epilogue's repeated draws of splat 0, the viewer's camera convention.  For pixel p the fragments in walk order are
 * k = 0, 1, ...; fragment k has the weight q_k = rint(w_k * 2^20) (the lift's fixed point, GSX_LIFT_ONE), is made by splat i_k,
 * and has the depth key d_k = runSort's int32 key of i_k in this view, ((vp2 x + vp6 y + vp10 z) * 4096) | 0 (gs.js:436-441;
 * gsx_debug_render_pre shows it).  Then
 *     total[p]  = sum of q_k                      uint32: the very number gsx_label_view writes to total_out
 *     moment[p] = sum of q_k * d_k                int64 (q <= 2^20, |d| < 2^31, a pixel's sum of q stays near 2^20)
 *     cut       = max(1, ceil(quantile * 2^20)),  quantile in (0, 1]
 *     the SURFACE of p is the first k with q_0 + ... + q_k >= cut:
 *         surface_key[p]   = d_k
 *         surface_index[p] = the UPLOAD row of i_k (as gsx_lift_finalize reports rows), not the importance row
 *     a pixel whose total stays below the cut has no surface: index -1, key 0.
 * A tile without a list writes 0, 0, 0, -1.  Everything is integer arithmetic on integers: the maps are the same bits from run
 * to run, and for any class map seg of the view
 *     sum over {p: seg[p] = c} of moment[p]  ==  sum over i of d_i * gsx_lift_table[i][c + 1]     exactly.
 * The key is affine in view-space depth, key / 4096 = proj[10] * (z_view - view[14]) with the matrices gsx_render_view builds,
 * so scene units are one fp64 multiply-add away (gsx_depth_key_to_z): expected depth = moment / total * scale + offset.
 * The splats' labels are not needed.
 * ------------------------------------------------------------------------------------------- */
/* total_out: height x width uint32; moment_out: height x width int64; surface_key_out, surface_index_out: height x width
 * int32.  All four are HOST pointers and any of them may be NULL.  total_out and moment_out both NULL selects the
 * surface-only mode: a tile also stops once every pixel of the frame has its surface; the surface maps are bit for bit those
 * of the full walk.  The call waits for its results.
 *   GSX_E_STATE        no gsx_upload_splats yet, a render edit state set, gsx_render_views running on this context
 *   GSX_E_INVALID      cam NULL, width or height < 1, quantile not in (0, 1] or not finite
 *   GSX_E_UNSUPPORTED  more than 4096 pixels per side
 * A failing call leaves the previous view's maps as they were.  The pair buffers are handled as gsx_label_view handles them. */
int gsx_depth_view(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, double quantile, uint32_t* total_out,
                   int64_t* moment_out, int32_t* surface_key_out, int32_t* surface_index_out);
/* the height x width int32 maps of the last successful gsx_depth_view since the last gsx_upload_splats (NULL without one):
 * device memory owned by the context, written on the ctx stream; valid until the next gsx_depth_view, gsx_upload_splats or
 * gsx_destroy */
void* gsx_depth_surface_index_device(gsx_ctx* ctx);
void* gsx_depth_surface_key_device(gsx_ctx* ctx);
/* statistics: pixels of the last view with a surface */
int64_t gsx_depth_num_surface(const gsx_ctx* ctx);
/* host only, no context: z_view = key * scale + offset, from the view and projection matrices gsx_render_view builds for
 * (cam, width, height); the key truncates, so the result lies within one key unit (= scale) of the exact depth.
 * GSX_E_INVALID: a NULL argument, width or height < 1 */
int gsx_depth_key_to_z(const gsx_camera* cam, int32_t width, int32_t height, double* scale, double* offset);
/* the surface under a canvas point of the LAST depth view: x, y as gsx_hit_test takes them (y from the bottom): the pixel's
 * column is floor(x), its row height - 1 - floor(y).  label_out: the exact int32 given to gsx_upload_splats for that splat
 * (-999999, NO_SELECTION, when uploaded without labels); index_out: its upload row; z_out: key * scale + offset of that
 * view's camera.  A point outside the frame or a pixel without a surface gives -999999, -1, NaN and GSX_OK, as gsx_hit_test
 * does for a miss.  Copies a few bytes out of the device maps and renders nothing.  Any output may be NULL.
 * GSX_E_STATE: no depth view since the last gsx_upload_splats */
int gsx_depth_pick(gsx_ctx* ctx, double x, double y, int32_t* label_out, int64_t* index_out, double* z_out);
/* test hook: out[8] = GSX_LIFT_ONE, its shift, the tile side, records per staged chunk, 0, 0, 0, 0 */
int gsx_debug_depth_constants(int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * instance association — per-view segment ids made to mean the same object in every view.  A Mask2Former map numbers its
 * segments per image in acceptance order (dls.py:156-158): voted as they are, the ids mix objects.  A run walks the views in
 * order and keeps, per Gaussian, the global instance it was first given (a "memory bank"); a view's segment takes the
 * instance most of its Gaussians already carry, or opens a new one.  The relabelled maps are ordinary class maps with
 * n_classes = max_instances for gsx_vote_view* / gsx_lift_view*.
 *
 * State of a run: gid[n] (int32, -1 = none yet), G = instances so far, dropped = a counter.  One view (cam, map, image size):
 *   1. Sample.  Gaussian i is projected exactly as the vote projects it (dls.py:43-82, R (x - p), fp64), then scaled,
 *      truncated and clamped onto the map (dls.py:270-286).  An invisible Gaussian takes no part; a visible one has
 *      bin b = map[y_s, x_s] + 1 in 0 .. S.
 *   2. Table.  table[b][gid[i] + 1] += 1 over the visible Gaussians: uint32, (S + 1) x (M + 1); row 0 is the background,
 *      column 0 is "no instance yet".
 *   3. Decide (on the host).  The rows b >= 1 in order of descending size_b (the row sum), the lower b first among equal
 *      sizes.  size_b < min_size: remap[b-1] = -1.  Otherwise, among the instances g no earlier row of this view has taken
 *      and with table[b][g+1] > 0, the largest count, the lowest g among equal counts; if there is one and
 *      count * 2^20 >= q * size_b with q = ceil(min_overlap * 2^20), remap[b-1] = g and g is taken.  Otherwise, if G < M,
 *      remap[b-1] = G, it is taken and G += 1.  Otherwise remap[b-1] = -1 and dropped += 1.
 *   4. Remember.  Every visible Gaussian with b >= 1, remap[b-1] >= 0 and gid == -1 gets gid = remap[b-1]; the first
 *      assignment stays.
 *   5. Relabel.  out[p] = map[p] >= 0 ? remap[map[p]] : -1, int32, same shape.
 * Everything is an integer: a run is reproducible bit for bit (tests/assoc_model.py is the rule in numpy).
 * On the device one thread per Gaussian stores its bin as a byte (255 = invisible), which is why S <= 254, and the maps of the
 * vote hold a byte per pixel, which is why M <= 255.
 * A new gsx_upload_positions (or gsx_destroy) ends a run; calls before gsx_assoc_begin return GSX_E_STATE.
 * ------------------------------------------------------------------------------------------- */
/* 1 <= max_segments <= 254, 1 <= max_instances <= 255, min_overlap finite in [0, 1], min_size >= 1, else GSX_E_INVALID.
 * Needs gsx_upload_positions (GSX_E_STATE).  Starts a run: gid = -1 everywhere, G = 0, dropped = 0, no views. */
int gsx_assoc_begin(gsx_ctx* ctx, int32_t max_segments, int32_t max_instances, double min_overlap, int32_t min_size);
/* seg: HOST pointer, seg_h x seg_w row-major, any gsx_seg_dtype, values in [-1, max_segments - 1]; img_w, img_h as in
 * gsx_vote_view.  The raw map is staged into device memory through a pinned buffer and the device path runs.  The host
 * waits for the view's table (it decides on it), so the range is checked in the same wait: a value outside the range
 * anywhere in the map is GSX_E_RANGE, fails THIS call and changes nothing of the run.
 * remap_out: max_segments int32 (global instance of segment s, or -1), or NULL.  map_out_dev: DEVICE pointer of seg_h x seg_w
 * int32 that receives the relabelled map, or NULL.  Everything is done and both maps are the caller's again on return. */
int gsx_assoc_view(gsx_ctx* ctx, const gsx_camera* cam, const void* seg, int32_t seg_dtype, int32_t seg_w, int32_t seg_h, int32_t img_w,
                   int32_t img_h, int32_t* remap_out, void* map_out_dev);
/* same, seg_dev is a DEVICE pointer read on the ctx stream, under the ordering rule of gsx_vote_view_device */
int gsx_assoc_view_device(gsx_ctx* ctx, const gsx_camera* cam, const void* seg_dev, int32_t seg_dtype, int32_t seg_w, int32_t seg_h,
                          int32_t img_w, int32_t img_h, int32_t* remap_out, void* map_out_dev);
/* views associated, G, and the segments dropped since gsx_assoc_begin (0 outside a run) */
int32_t gsx_assoc_num_views(const gsx_ctx* ctx);
int32_t gsx_assoc_num_instances(const gsx_ctx* ctx);
int64_t gsx_assoc_num_dropped(const gsx_ctx* ctx);
/* gid_out: n int32 in the order of the arrays given to gsx_upload_positions */
int gsx_assoc_ids(gsx_ctx* ctx, int32_t* gid_out);
/* table_out: the last view's (max_segments + 1) x (max_instances + 1) uint32 table (zeros before the first view): a test hook,
 * and diagnostics for a caller who wants to see why a segment matched */
int gsx_assoc_table(gsx_ctx* ctx, uint32_t* table_out);
/* test hook: out[8] = 2^20, its shift, Gaussians per workgroup and step of the table kernel, the largest max_segments, the
 * largest max_instances, the 16-bit counters a workgroup's LDS copy of the table holds at most, the steps a workgroup takes at
 * most, 0 */
int gsx_debug_assoc_constants(int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * PLY files — replaces the plyfile calls of the reference: PlyData.read (dls.py:29, ply_handler.py:
 * 44-45) and PlyData([vertex], text=False).write (dls.py:331-332, ply_handler.py:35-37).
 * Only the vertex element (scalar properties) is kept, as save_labeled_ply does.  ascii and
 * binary_little_endian are read; rows are exposed in binary little-endian layout either way.
 * These entry points need no GPU and no ctx (errors: gsx_last_error(NULL)).
 * ------------------------------------------------------------------------------------------- */
typedef struct gsx_ply gsx_ply;
typedef enum gsx_ply_type {
    GSX_PLY_CHAR = 0, GSX_PLY_UCHAR = 1, GSX_PLY_SHORT = 2, GSX_PLY_USHORT = 3,
    GSX_PLY_INT = 4, GSX_PLY_UINT = 5, GSX_PLY_FLOAT = 6, GSX_PLY_DOUBLE = 7
} gsx_ply_type;
int gsx_ply_open(const char* path, gsx_ply** out);
void gsx_ply_close(gsx_ply* ply);
int64_t gsx_ply_num_vertices(const gsx_ply* ply);
int32_t gsx_ply_num_properties(const gsx_ply* ply);
/* i-th vertex property: name (owned by ply), gsx_ply_type, byte offset inside a row */
int gsx_ply_property(const gsx_ply* ply, int32_t i, const char** name, int32_t* type, int64_t* offset);
int64_t gsx_ply_row_stride(const gsx_ply* ply);
/* the vertex rows (num_vertices x row_stride bytes): a private copy-on-write mapping of the file or a
 * parsed buffer; writable, never written back to the source file; feeds gsx_upload_positions_strided */
void* gsx_ply_rows(gsx_ply* ply);
/* one property as floats (any scalar type is converted) / overwrite one property from floats */
int gsx_ply_read_f32(const gsx_ply* ply, const char* name, float* out);
int gsx_ply_set_f32(gsx_ply* ply, const char* name, const float* in);
/* writes every vertex property, plus a trailing `property int label` when labels != NULL
 * (save_labeled_ply, dls.py:318-332).  text != 0 writes ascii (k_means.py:193). */
int gsx_ply_write(const gsx_ply* ply, const char* path, const int32_t* labels, int32_t text);

/* ---------------------------------------------------------------------------------------------
 * test hook: the library's stable LSD radix sort of (u32 key, u32 value) pairs by key bits
 * [0, bits) — the primitive behind the Morton ordering and the rasterizer's (tile | depth16) order,
 * which restates the stable counting sort of gs.js:443-457.  Host arrays, sorted in place.
 * ------------------------------------------------------------------------------------------- */
int gsx_debug_sort_pairs(gsx_ctx* ctx, uint32_t* keys, uint32_t* values, int64_t n, int32_t bits);
/* the rasterizer's level-1 sort (csrc/sort.hip: radix_sort_pairs_drop): pairs whose key is 0xffffffff are left out by the first
 * pass; the others come back sorted (stable) in the first *kept_out slots, the slots behind them hold unspecified values */
int gsx_debug_sort_pairs_drop(gsx_ctx* ctx, uint32_t* keys, uint32_t* values, int64_t n, int32_t bits, int64_t* kept_out);
/* test hook: radix_sort_pairs_dev as a frame of the rasterizer calls it - the buffers hold `capacity` pairs, the launches are
 * sized for the capacity and the count is read on the device (a count above the capacity reads as 0).  keys / values
 * (capacity entries each) come back as the WHOLE result buffer; *where_out = 0: the sort ended in the buffers the input was
 * uploaded to (a slot the sort did not write still holds its input), 1: in the second pair, which held 0xff bytes before */
int gsx_debug_sort_pairs_dev(gsx_ctx* ctx, uint32_t* keys, uint32_t* values, int64_t capacity, int64_t count, int32_t bits,
                             int32_t* where_out);
/* test hook: the rasterizer's one-pass pair sort (csrc/sort.hip: radix_sort_values_wide), bits in [1, 11], nranges in
 * [1, 2048], the count on the device as above.  values_out (capacity entries, 0xff bytes where the sort wrote nothing): the
 * values in the stable order of key bits [0, bits); ranges_out (nranges x 2 int32): [first, last + 1) slot of every key
 * below nranges, written whatever the count */
int gsx_debug_sort_values_wide(gsx_ctx* ctx, const uint32_t* keys, const uint32_t* values, int64_t capacity, int64_t count,
                               int32_t bits, int32_t nranges, uint32_t* values_out, int32_t* ranges_out);
/* test hook: the rasterizer's exclusive scan of n >= 1 uint32 (csrc/render.hip: exclusive_scan_u32).  out[i] = the sum of
 * in[0 .. i) mod 2^32; *grand_out = the sum of all of them in 64 bits, exact while every 4096-entry tile's own sum is
 * below 2^32 */
int gsx_debug_exclusive_scan(gsx_ctx* ctx, const uint32_t* in, int64_t n, uint32_t* out, uint64_t* grand_out);
/* test hook: the lists' ranges from the sorted pair keys (csrc/render.hip: ranges_kernel) launched as a frame launches it -
 * sized for the capacity, the total on the device (above the capacity it reads as 0), the table zeroed first.
 * ranges_out (nlists x 2 int32): [first, last + 1) slot of every key that occurs below nlists, (0, 0) for the others */
int gsx_debug_ranges(gsx_ctx* ctx, const uint32_t* sorted_keys, int64_t capacity, int64_t total, int32_t nlists,
                     int32_t* ranges_out);
/* test hook: one depth phase's binning as a frame runs it (csrc/render.hip: bin_kernel COUNT -> exclusive_scan_u32 -> bin_kernel
 * EMIT, the grids and arguments of gsx_render_view) on the caller's arrays alone - no uploaded scene is needed and none of the
 * context's frame buffers or counters is touched.
 *   tile_rect  n u32            tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24 (tx1 < tx0 or ty1 < ty0: no tile)
 *   rec        n x 12 f32       the pre pass's records (cx, cy, g0, g1, ..); NULL allowed when exact == 0
 *   by_depth   len u32          the depth order; its first nvis entries are the splats the level-1 sort kept.  nvis goes to the
 *                               device as the u64 the kernel reads; the phase is [nvis / div0, nvis / div1) of the order (div0 = 0:
 *                               from the start), the launches cover m_cap slots
 *   height, tiles_x, tiles_y    the frame's height in pixels and its size in 16x16 tiles; bin32 != 0: the candidates are 32x32 bins
 *                               (the kernels then see (tiles_x + 1) / 2 lists per row); exact: the option "exact_cull"
 *   sat        NULL, or tiles_x * tiles_y bytes; with bin32 four bytes per bin, (tiles_x + 1) / 2 * ((tiles_y + 1) / 2) bins
 *   pair_cap                    capacity of the pair arrays
 * Outputs, all preset to 0xFF bytes: count_out m_cap u32 (pairs per slot of the phase), *total_out (64 bits), keys_out and
 * vals_out pair_cap u32 each (written only when the total fits pair_cap).
 * GSX_E_INVALID, before any launch, for whatever could make a kernel index outside these arrays: an entry of by_depth[0, nvis)
 * >= n, nvis > len, a non-empty rectangle outside tiles_x x tiles_y, tiles_x or tiles_y outside [1, 256], div1 < 1, div0 < 0,
 * m_cap < 1 or below the phase's length, pair_cap outside [1, 2^31 - 1], bin32 together with exact (gsx_render_view never
 * launches that pair), exact without rec, a NULL array */
int gsx_debug_bin(gsx_ctx* ctx, int64_t n, const uint32_t* tile_rect, const float* rec, const uint32_t* by_depth, int64_t len,
                  int64_t nvis, int64_t div0, int64_t div1, int64_t m_cap, int32_t height, int32_t tiles_x, int32_t tiles_y,
                  int32_t bin32, int32_t exact, const uint8_t* sat, int64_t pair_cap, uint32_t* count_out, uint64_t* total_out,
                  uint32_t* keys_out, uint32_t* vals_out);
/* test hook: the Morton order of the last upload with the option "spatial_sort" on - perm_out[i] (gsx_num_gaussians
 * entries) = the uploaded index of the position in slot i.  GSX_E_INVALID when the context holds no sorted order (fewer
 * than two positions, or the option was off) */
int gsx_debug_spatial_order(gsx_ctx* ctx, uint32_t* perm_out);
/* test hook, host only (no context, no GPU): the packed form of one map exactly as gsx_vote_view stages it in
 * pinned memory - u8 bins in strips of 16 pixel columns (tiled != 0; row-major otherwise) followed, at *coarse_off
 * (-1: none), by the 4x4-coarsened level.  out == NULL only reports *bytes.  *bad = 1 if a label was out of range. */
int gsx_debug_host_pack(const void* seg, int32_t seg_dtype, int32_t w, int32_t h, int32_t n_classes, int32_t tiled,
                        int32_t coarse, int32_t threads, uint8_t* out, int64_t out_cap, int64_t* bytes, int64_t* coarse_off,
                        int32_t* bad);
/* test hook, host only: the COMPACT transfer form in which gsx_vote_view sends a two-level map over PCIe (option
 * "host_compact", default 1): uint32 first_block[2 * bands of 8 pixel rows] | the coarse level as in the pool | one 16-byte
 * block (4 rows x 4 pixels) per mixed 4x4 cell.  A band holds two rows of cells; entry 2 * band + row says where that cell
 * row's blocks start, inside a cell row they follow the cell columns; the cell rows follow each other in the order their
 * workers reserved room.  out == NULL: *bytes = worst-case size; otherwise bytes in use.
 * Option "host_prefetch" (default 8192): bytes the narrowing loops prefetch ahead of themselves (NTA hint; a negative value
 * selects T0); "host_prefetch_burst" (default 1): a band that starts a new stream asks for that distance at once. */
int gsx_debug_host_pack_compact(const void* seg, int32_t seg_dtype, int32_t w, int32_t h, int32_t n_classes, int32_t threads,
                                uint8_t* out, int64_t out_cap, int64_t* bytes, int64_t* table_bytes, int64_t* stream_off,
                                int32_t* bad);
/* test hook, host only: `runs` fork-joins of pseudo-random size (1..max_parts parts) on ONE worker pool of `threads` threads;
 * returns how many parts did not run exactly once (0 = the pool is sound), -1 if the pool could not be created */
int64_t gsx_debug_workers_stress(int32_t threads, int32_t runs, int32_t max_parts);
/* test hook, host only: the D2H epilogue's widening pass - labels_out[i] = bins[i] - 1 (the labels cross PCIe as one byte
 * each, bin = label + 1), on `threads` worker threads */
int gsx_debug_widen_labels(int32_t threads, const uint8_t* bins, int64_t n, int32_t* labels_out);
/* statistics: (wave of 64 Gaussians, view) pairs the vote kernels skipped through the wave culling since the context
 * was created or since the last call with reset != 0 */
int gsx_vote_culled(gsx_ctx* ctx, int64_t* wave_views, int32_t reset);
/* test hook: what the fp32 filter in front of the projection's divisions (option "filter_project") assumes about the
 * hardware, measured on the device.  out[17]: [0] = the largest relative error of v_rcp_f32 over EVERY float in
 * [2^-41, 2^41], in units of 2^-24 (the filter's proof needs <= 3); [1..8] = v_fract_f32 and [9..16] =
 * v_cvt_flr_i32_f32 of +inf, -inf, -1e-10, NaN, 1920.5, -0.25, 3e38, -3e38. */
int gsx_debug_filter_check(gsx_ctx* ctx, double* out);
/* test hook, host only (no context, no GPU): the five world-space culling planes the vote kernels use to skip whole
 * waves for a view (option "wave_cull"), as out[5][5] = unit normal A, offset B, margin slope M: a sphere (c, r) with
 * A.c + B > r + M (|c|_1 + r) holds no Gaussian that project_gaussian (deep_learning_segmentation.py:43-82) would
 * accept (the margin is a million times the rounding error of the fp64 projection of any point of the sphere). */
int gsx_debug_cull_planes(const gsx_camera* cam, double* out);

/* ---------------------------------------------------------------------------------------------
 * k-means labeler: 3D_clustering/k_means.py:107-151 k_means_with_color (the reference's other producer of the
 * `label` field).  points / colors: n x 3 float32 each, row-major, on the host (x y z and
 * f_dc_0..2, k_means.py:17-28).  init_index[k]: the rows used as initial centroids - the reference draws them
 * with an unseeded np.random.choice (k_means.py:111), so the caller supplies them.  Runs at most max_iter
 * rounds of assign (nearest centroid by float64 squared distance in scipy's summation order, :116-122) and
 * update (float32 mean with numpy's in-order accumulation, :125-128), stops early when the centroids moved by
 * less than tol (:132-136), and labels every row by the centroids in hand (:142-147).
 * labels_out int32[n] (required); centroids_out float32[k*6], iterations_out, converged_out may be NULL.
 * 1 <= k <= min(n, 2048).
 * ------------------------------------------------------------------------------------------- */
int gsx_kmeans(gsx_ctx* ctx, int64_t n, const float* points, const float* colors, int32_t k, const int64_t* init_index,
               int32_t max_iter, double tol, int32_t* labels_out, float* centroids_out, int32_t* iterations_out,
               int32_t* converged_out);

/* ---------------------------------------------------------------------------------------------
 * region-growing labeler: 3D_clustering/region_growing.py ("rg.py"), the reference's geometry-only producer of a
 * segmentation.  points: n x 3 float32, row-major, on the host (rg.py:270 reads them from the PLY;
 * scipy's KD-tree widens them to float64, so distances are fp64 of the widened coordinates).
 * Order among neighbours, where scipy leaves equidistant points unspecified: nearer first, then lower index.
 * Option "nn_brute" (default 0): 1 = every query visits every point instead of a ring of grid cells, O(n^2): the
 * same lists bit for bit; normals and residuals equal up to the order in which the moments are added (tests).
 * ------------------------------------------------------------------------------------------- */
/* compute_normals (rg.py:78-129) and compute_residuals (rg.py:132-163) in one pass: for every point the covariance
 * of its k nearest points (itself included, as kd_tree.query includes it, rg.py:98), the eigenvector of the smallest
 * eigenvalue, flipped when dot(normal, p - centroid) > 0 (rg.py:120-121), normalised (rg.py:126); residual =
 * |dot(normal, p - centroid)| (rg.py:161).  All fp64 (the reference's float32 centroid, covariance and eigh are not
 * reproduced; tests/test_region_growing_gpu.py holds the measured distance).  normals_out double[n][3],
 * residuals_out double[n]; either may be NULL.  Where the two smallest eigenvalues coincide the normal is undefined
 * in the reference too: a unit vector comes back, never NaN.  No neighbour list is stored, whatever k.
 * GSX_E_INVALID: NULL points, n < 1, k < 3, k > n (the reference raises an IndexError), a non-finite coordinate. */
int gsx_normals(gsx_ctx* ctx, int64_t n, const float* points, int64_t k, double* normals_out, double* residuals_out);
/* test hook: the moments gsx_normals takes its normal from - moments_out double[n][9] = centroid x y z (the mean of the
 * k nearest points, rg.py:103), then the upper triangle xx xy xz yy yz zz of centered^T centered (rg.py:109) */
int gsx_debug_normals_moments(gsx_ctx* ctx, int64_t n, const float* points, int64_t k, double* moments_out);
/* test hook, needs no ctx and no GPU (errors: gsx_last_error(NULL)): the search grid gsx_normals / gsx_knn build for these
 * points and this k - the very host code they run (brute != 0: as under option "nn_brute").  origin_out[3], *h_out,
 * dims_out[3]: corner, cell edge and cells per axis; cell c = floor((double(p) - origin) * (1 / h)) clamped to [0, dims - 1]
 * per axis, cells numbered x fastest.  cell_start_out uint32[cells + 1]: the sorted positions [start[j], start[j + 1]) hold
 * cell j; order_out int32[n]: the original index at each sorted position.  Either may be NULL: ask for dims_out first.
 * GSX_E_INVALID: NULL points or a NULL origin_out / h_out / dims_out, n < 1, k < 1, a non-finite coordinate (found on the
 * host here); GSX_E_UNSUPPORTED: n > 2^31-1, as gsx_normals and gsx_knn. */
int gsx_debug_nn_grid(int64_t n, const float* points, int64_t k, int brute, double origin_out[3], double* h_out, int32_t dims_out[3],
                      uint32_t* cell_start_out, int32_t* order_out);
/* kd_tree.query(points[i], k)[1] for every i (rg.py:205): index_out int32[n][k], ascending distance (the point itself
 * first unless a duplicate with a lower index precedes it).  2 <= k <= min(64, n).  index_out may be NULL: the lists
 * stay on the device. */
int gsx_knn(gsx_ctx* ctx, int64_t n, const float* points, int32_t k, int32_t* index_out);
/* device pointer of the int32[n][k] lists of the last successful gsx_knn (NULL: none); valid until the next gsx_knn /
 * gsx_region_growing / gsx_smooth_labels / gsx_split_labels on the ctx (gsx_smooth_labels builds lists of its own when its
 * k <= 64, gsx_split_labels always: they replace the context's lists) */
void* gsx_knn_device(gsx_ctx* ctx);
/* segmentation_3D (rg.py:166-226) on the host; needs no ctx and no GPU (errors: gsx_last_error(NULL)).
 * normals double[n][3], residuals double[n], knn int32[n][k] (row i = the neighbours of i in visiting order).
 * A region starts at the available point of smallest residual (rg.py:194; lowest index among equals) and grows
 * through a FIFO front (rg.py:199-203): a neighbour still available is accepted iff |dot(normal[seed], normal[nb])| >
 * cos(angle_threshold) (rg.py:209-211) and joins the front iff residual[nb] < residual_threshold (rg.py:216-218).
 * labels_out[i] = rank of i's region by size, largest first, creation order among equal sizes (rg.py:224: Python's
 * stable sort); *n_regions_out (may be NULL) = number of regions.  The reference only recolours f_dc per region
 * (rg.py:229-245); the label is the form the other two labelers produce.
 * GSX_E_INVALID: a NULL array, n < 1, k < 1, a NaN residual or threshold, a neighbour index outside [0, n) - and, as
 * everywhere in this library (the C boundary maps std::bad_alloc so), running out of host memory; the text tells. */
int gsx_region_grow(int64_t n, const double* normals, const double* residuals, const int32_t* knn, int32_t k,
                    double residual_threshold, double angle_threshold, int32_t* labels_out, int32_t* n_regions_out);
/* the reference's main (rg.py:270-278): gsx_normals with k_normals, gsx_knn with k, gsx_region_grow.
 * normals_out, residuals_out, n_regions_out may be NULL. */
int gsx_region_growing(gsx_ctx* ctx, int64_t n, const float* points, int64_t k_normals, int32_t k, double residual_threshold,
                       double angle_threshold, int32_t* labels_out, double* normals_out, double* residuals_out,
                       int32_t* n_regions_out);

/* ---------------------------------------------------------------------------------------------
 * label clean-up: a majority filter over the k nearest neighbours, with hole filling.  It repairs a `label` field that one of
 * the three labelers wrote: the vote projects centres only and knows no occlusion (dls.py:43-82), so a Gaussian behind a wall
 * takes the wall's class and one that no view sees stays -1.  The reference has no such step; the rule below is the contract,
 * and it is all integers.
 * points: n x 3 float32, row-major, on the host; labels int32[n], any values; 1 <= k <= n; rounds >= 1; min_votes >= 1;
 * flags: GSX_SMOOTH_IGNORE | GSX_SMOOTH_FILL_ONLY.
 * N(i) = the k nearest points of i by the key (d2, index) - exactly the set gsx_knn / gsx_normals select: d2 is fp64 of the
 * widened coordinates, (dx*dx + dy*dy) + dz*dz without FMA; nearer first, then lower index.  N(i) holds i itself unless
 * duplicates with lower indices crowd it out.
 * One round, L = the labels at its start.  The update is Jacobi: every point reads L, the results go to a second buffer.
 *   count[c] = number of j in N(i) with L[j] == c; with GSX_SMOOTH_IGNORE the neighbours whose label is ignore_label cast no
 *   vote.  No neighbour votes: new[i] = L[i].  Otherwise m = the largest count and W = the labels that reach it; the winner
 *   is L[i] if L[i] is in W, else the smallest value in W (signed compare).  new[i] = the winner, unless m < min_votes: then
 *   new[i] = L[i].  With GSX_SMOOTH_FILL_ONLY, new[i] = L[i] whenever L[i] != ignore_label (only holes are filled).
 *   changed_out[r] = number of i with new[i] != L[i] in round r.
 * A round that changes nothing ends the run; *rounds_done_out = rounds executed, that one included; the later entries of
 * changed_out[rounds] are 0.  support_out[i] = count of i's final label among N(i) in the input of the last executed round
 * (0 when that label cast no vote).  labels_out int32[n] is required and may be `labels` itself; support_out, changed_out and
 * rounds_done_out may be NULL.
 * k <= 64: the lists are built once (as by gsx_knn: they replace the context's lists, see gsx_knn_device) and every round
 * runs over them, comparing raw labels: any number of distinct labels.  k > 64: every round searches again and counts dense
 * class ids in 16 bits: k <= 65535 and at most 4096 distinct labels.  Option "smooth_search" (default 0): 1 = that second
 * form for k <= 64 too; like "nn_brute" it never changes a result (tests).
 * Every error returns before any launch.  GSX_E_INVALID: a NULL points, labels or labels_out, n < 1, k < 1, k > n,
 * rounds < 1, min_votes < 1, unknown flag bits, a non-finite coordinate.  GSX_E_UNSUPPORTED: n > 2^31-1; with k > 64 (or
 * "smooth_search") k > 65535 or more than 4096 distinct labels.
 * ------------------------------------------------------------------------------------------- */
#define GSX_SMOOTH_IGNORE 1
#define GSX_SMOOTH_FILL_ONLY 2
int gsx_smooth_labels(gsx_ctx* ctx, int64_t n, const float* points, const int32_t* labels, int64_t k, int32_t rounds,
                      int32_t min_votes, int32_t ignore_label, int32_t flags, int32_t* labels_out, int32_t* support_out,
                      int64_t* changed_out, int32_t* rounds_done_out);
/* the same rounds over given neighbour lists, 1 <= k <= min(64, n).  knn: host int32[n][k] with every index in [0, n) - the
 * lists need not come from a search, and a row that names a point twice lets it vote twice - or NULL: the device lists of the
 * last gsx_knn / gsx_region_growing / gsx_smooth_labels (k <= 64) on the ctx, whose n and k must be these.
 * GSX_E_INVALID as above, and for k > 64 or a list index outside [0, n) (the text names row and column; nothing is
 * launched); GSX_E_STATE: knn == NULL without device lists of this n and k; GSX_E_UNSUPPORTED: n > 2^31-1. */
int gsx_smooth_labels_lists(gsx_ctx* ctx, int64_t n, int32_t k, const int32_t* knn, const int32_t* labels, int32_t rounds,
                            int32_t min_votes, int32_t ignore_label, int32_t flags, int32_t* labels_out, int32_t* support_out,
                            int64_t* changed_out, int32_t* rounds_done_out);
/* test hook: out[8] = the largest k of the list form, the most distinct labels of the search form, the bits of one counter of
 * its class table (two counters to a dword: class c is half c & 1 of dword c >> 1), the lanes of its winner scan (lane l reads
 * the dwords l, l + lanes, ..), the queries (waves) of a workgroup, 0, 0, 0 */
int gsx_debug_smooth_constants(int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * class labels into object instances: connected components of every label over the k-nearest-neighbour graph.  The viewer
 * works on one label value at a time (gsx_render_set_edits, gsx_hit_test, GSX_EDIT_TABLE_MAX entries), but SegFormer and
 * `--mask2former_map classes` give semantic classes: every chair of a scene carries one value, and a k-means cluster can hold
 * pieces that do not touch.  The reference has no step that turns a class into objects; the rule below is the contract.  It
 * is all integers plus one fp64 compare.
 * points: n x 3 float32, row-major, on the host; labels int32[n], any values; flags: GSX_SPLIT_IGNORE.
 * N(i) = the k nearest points of i, exactly the set and order gsx_knn returns.
 * Edge: points i and j (i != j) are joined iff all of
 *   - j is in N(i) or i is in N(j) (the closure is symmetric: one direction is enough);
 *   - labels[i] == labels[j];
 *   - neither label is ignored - a label is ignored only with GSX_SPLIT_IGNORE set and label == ignore_label;
 *   - d2(i, j) <= r2, with d2 = (dx*dx + dy*dy) + dz*dz in fp64 of the widened coordinates without FMA (the expression of
 *     gsx_knn's search, symmetric in i and j) and r2 = max_dist * max_dist, one fp64 product taken on the host.
 *     max_dist = +inf means no cut.
 * Component: a connected component of that graph over the non-ignored points; an isolated point is a component of size 1.
 * rep(i) = the smallest index in i's component, size = its number of points.  component_out[i] = rep(i), -1 for an ignored
 * point.
 * Instances: the components with size >= min_size, ranked by size descending, then rep ascending; with max_instances > 0 only
 * the first max_instances of them.  Instance id = rank, 0 .. M-1.
 * labels_out[i] = the instance id of i's component; -1 for ignored points, for components below min_size and for components
 * cut by max_instances (gsx_smooth_labels with GSX_SMOOTH_IGNORE | GSX_SMOOTH_FILL_ONLY repairs those).  labels_out int32[n] is
 * required and may be `labels` itself.  instance_label_out[m], instance_size_out[m], instance_rep_out[m] = the original
 * label, size and rep of instance m < M; the caller sizes each for n entries (int32[n] / int64[n] / int32[n]); each may be
 * NULL, as may component_out.  *n_instances_out = M; *n_components_out = the number of components before the size filter.
 * The result is a pure function of the inputs: it does not depend on the order in which the GPU joins things.
 * gsx_split_labels: 2 <= k <= min(64, n); the lists are built as by gsx_knn and replace the context's lists (see
 * gsx_knn_device).
 * Every error returns before any launch.  GSX_E_INVALID: a NULL points, labels or labels_out, n < 1, k out of range,
 * min_size < 1, max_instances < 0, max_dist NaN or <= 0, unknown flag bits, a non-finite coordinate.
 * GSX_E_UNSUPPORTED: n > 2^31-1.
 * ------------------------------------------------------------------------------------------- */
#define GSX_SPLIT_IGNORE 1
int gsx_split_labels(gsx_ctx* ctx, int64_t n, const float* points, const int32_t* labels, int32_t k, double max_dist,
                     int64_t min_size, int32_t max_instances, int32_t ignore_label, int32_t flags, int32_t* labels_out,
                     int32_t* component_out, int32_t* instance_label_out, int64_t* instance_size_out,
                     int32_t* instance_rep_out, int32_t* n_instances_out, int64_t* n_components_out);
/* the same over given neighbour lists, 1 <= k <= min(64, n).  knn: host int32[n][k] with every index in [0, n) - the lists
 * need not come from a search: a row may repeat an index, and may name the point itself (a self loop is no edge) - or NULL:
 * the device lists of the last gsx_knn / gsx_region_growing / gsx_smooth_labels (k <= 64) / gsx_split_labels on the ctx, whose
 * n and k must be these.  points may be NULL iff max_dist is +inf; given points are checked for finiteness either way.
 * GSX_E_INVALID as above (NULL points only with a finite max_dist), and for a list index outside [0, n) (the text names row
 * and column; nothing is launched); GSX_E_STATE: knn == NULL without device lists of this n and k; GSX_E_UNSUPPORTED:
 * n > 2^31-1. */
int gsx_split_labels_lists(gsx_ctx* ctx, int64_t n, int32_t k, const int32_t* knn, const float* points, const int32_t* labels,
                           double max_dist, int64_t min_size, int32_t max_instances, int32_t ignore_label, int32_t flags,
                           int32_t* labels_out, int32_t* component_out, int32_t* instance_label_out,
                           int64_t* instance_size_out, int32_t* instance_rep_out, int32_t* n_instances_out,
                           int64_t* n_components_out);

/* ---------------------------------------------------------------------------------------------
 * IoU evaluation of 2-D segmentations: Image_Segmentation/evaluation.py ("ev.py").  Everything is counted in
 * integers on the GPU and divided once on the host, so the results equal the reference's exactly.  Inputs are never written
 * (the reference's IoU overwrites the set pixels of both arguments with 1, ev.py:29-30; the Python front-end restates that).
 * Errors: GSX_E_INVALID (before anything is read) for a NULL pointer, h, w or a count <= 0, an unknown dtype, a device pointer
 * not aligned to its element; GSX_E_UNSUPPORTED for h * w >= 2^31, more than 65535 masks / ground truths / pairs, more than
 * 1 GiB of bit planes or tables.
 * ------------------------------------------------------------------------------------------- */
/* IoU (ev.py:24-35) of every mask with every ground truth - the body of the double loop of get_ious_from_masks (ev.py:46-50).
 * masks[n_masks], gts[n_gt]: HOST pointers to row-major h x w arrays of gsx_mask_dtype mask_dtype / gt_dtype.
 *   inter_out      int64 [n_masks][n_gt]   |mask & gt|                       np.sum(intersection), ev.py:32,35
 *   area_masks_out int64 [n_masks], area_gt_out int64 [n_gt]                 set pixels
 *   iou_out        double [n_masks][n_gt]  inter / (area_m + area_g - inter)  ev.py:35; NaN where the union is empty
 * Any output may be NULL.  The masks are copied up one at a time through a pinned staging pair and packed into bit planes
 * (one bit per pixel); only the planes and two raw masks are resident. */
int gsx_iou_masks(gsx_ctx* ctx, int32_t n_masks, const void* const* masks, int32_t mask_dtype, int32_t n_gt, const void* const* gts,
                  int32_t gt_dtype, int32_t h, int32_t w, int64_t* inter_out, int64_t* area_masks_out, int64_t* area_gt_out,
                  double* iou_out);
/* same, the arrays hold DEVICE pointers (instance masks of a model on this GPU); a pointer needs the alignment of its element
 * only (a view into a larger tensor).  Runs on the ctx stream, which the caller orders behind the producers of the masks; the
 * call returns after the counts have arrived on the host. */
int gsx_iou_masks_device(gsx_ctx* ctx, int32_t n_masks, const void* const* masks_dev, int32_t mask_dtype, int32_t n_gt,
                         const void* const* gts_dev, int32_t gt_dtype, int32_t h, int32_t w, int64_t* inter_out,
                         int64_t* area_masks_out, int64_t* area_gt_out, double* iou_out);
/* contingency tables of n_pairs pairs of label maps (gsx_seg_dtype, labels -1 .. n-1 as in gsx_vote_view; both class counts in
 * 1 .. 255): table_out int64 [n_pairs][n_pred_classes + 1][n_gt_classes + 1], entry [a][b] = pixels whose pred bin is a and
 * whose gt bin is b, bin = label + 1.  IoU(pred == a - 1, gt == b - 1) (ev.py:24-35) is n_ab / (row_a + col_b - n_ab).
 * A label out of range fails the call with GSX_E_RANGE; the text names the pair and the lowest flat pixel index at fault. */
int gsx_iou_label_maps(gsx_ctx* ctx, int32_t n_pairs, const void* const* pred, int32_t pred_dtype, int32_t n_pred_classes,
                       const void* const* gt, int32_t gt_dtype, int32_t n_gt_classes, int32_t h, int32_t w, int64_t* table_out);
int gsx_iou_label_maps_device(gsx_ctx* ctx, int32_t n_pairs, const void* const* pred_dev, int32_t pred_dtype, int32_t n_pred_classes,
                              const void* const* gt_dev, int32_t gt_dtype, int32_t n_gt_classes, int32_t h, int32_t w,
                              int64_t* table_out);
/* generate_segmentation_map (ev.py:59-69) without the colours: index_out int32 [h][w] = the highest list index whose mask is set
 * at the pixel (the last mask drawn owns it, ev.py:65-67), or -1.  Host pointers. */
int gsx_masks_top_index(gsx_ctx* ctx, int32_t n_masks, const void* const* masks, int32_t mask_dtype, int32_t h, int32_t w,
                        int32_t* index_out);
/* host only (no ctx, no GPU; errors: gsx_last_error(NULL)): iou_out[i] = (double)inter[i] / (double)(area_a[i] + area_b[i] -
 * inter[i]), ev.py:35 - one IEEE division, NaN for 0 / 0 */
int gsx_iou_from_counts(int64_t n, const int64_t* inter, const int64_t* area_a, const int64_t* area_b, double* iou_out);
/* host only: the best match of get_ious_from_masks (ev.py:44-54) over iou [n_masks][n_gt]: per mask start from (0, gt 0) and
 * move to gt i only if iou > best - the first of equal maxima wins, NaN never wins, no positive IoU reports (0, 0).
 * best_iou_out double [n_masks], best_gt_out int32 [n_masks]. */
int gsx_iou_best(int32_t n_masks, int32_t n_gt, const double* iou, double* best_iou_out, int32_t* best_gt_out);
/* test hook, host only: the units the IoU kernels are built on, out[8] = bytes of a lane's load in the pack kernel, pixels per
 * plane word, per wave and per workgroup of the pack kernel, the pair kernel's tile edge and the words per chunk of a slice
 * (small problems get slices of exactly one chunk), the table entries up to which the LDS path runs, the pixels a lane of the
 * table kernel run-length-merges */
int gsx_debug_iou_constants(int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * class maps from a segmentation network's output (dls.py:85-124, 142-144; SURVEY row 3's post-processing): int32 maps at the
 * image size, written on the device for gsx_vote_view_device / gsx_vote_views_device - no byte of a map visits the host.
 * Both calls run on the ctx stream (gsx_stream), which the caller orders behind the producer of the inputs, write only the
 * output map(s), read nothing back and synchronise nothing; inputs and outputs stay alive until the stream has passed.
 *
 * Nearest resize, per axis from S source to D destination pixels: s(d) = min(floor(d * (1.0 / ((double)D / S))), S - 1), in
 * double with two roundings - OpenCV's resizeNN, the rule behind the reference's cv2.INTER_NEAREST.  It is not
 * floor(d * S / D) and not torch's float32 floor(d * (float)S / D): S = 2, D = 98 sends destination 49 to source 0 here and
 * to source 1 under both others.  It covers upsampling and downsampling alike.  cv2 is not installed on this machine, so this
 * rule is restated from OpenCV's source and cannot be executed against.  Everything else is pinned by running the reference.
 *
 * Errors, before anything touches the device: GSX_E_INVALID for a NULL ctx or pointer (masks_dev, cls_dev and conf_dev may be
 * NULL only when K == 0), a size <= 0 (K == 0 is allowed), an unknown dtype, a pointer not aligned to its element (element
 * alignment is all that is asked: a view into a larger tensor works); GSX_E_UNSUPPORTED for C > 65535, for h * w,
 * out_h * out_w or n * out_h * out_w >= 2^31, and for n * ceil(h * w / 128) >= 2^31 workgroups.
 * ------------------------------------------------------------------------------------------- */
/* replaces dls.py:142-144 (outputs.logits.argmax(dim=1) and the cv2.resize of the map to the image size).
 * logits_dev: n contiguous volumes (n, C, h, w) of gsx_float_dtype dtype; maps_dev: int32 (n, out_h, out_w),
 * map[y][x] = argmax_c logits[c][sy(y)][sx(x)].  The arg-max is torch.argmax's: the first index of the maximum wins, a NaN
 * counts as the maximum and the first NaN wins, -0.0 == +0.0, all -inf gives 0. */
int gsx_segmap_from_logits(gsx_ctx* ctx, const void* logits_dev, int32_t dtype, int32_t n, int32_t C, int32_t h, int32_t w,
                           int32_t out_w, int32_t out_h, int32_t* maps_dev);
/* replaces dls.py:100-124 (process_yolo_segmentation after the model call).  masks_dev: K instance masks (K, mh, mw) of
 * gsx_float_dtype dtype; cls_dev, conf_dev: fp32 [K] on the device (conf is never read on the host); map_dev: int32 (out_h, out_w).
 * An instance counts iff conf > 0.5 in fp32 (0.5 itself and NaN do not, dls.py:117); a pixel is its iff the resized mask value
 * is > 0.5 (dls.py:121); later instances overwrite earlier ones whatever their confidence (the loop of dls.py:113-122 - its
 * comment says otherwise); the class id is truncated to int32 (dls.py:124) and unspecified when it is not finite; the
 * background, K == 0 and "nothing accepted" are -1 (dls.py:101). */
int gsx_segmap_from_masks(gsx_ctx* ctx, const void* masks_dev, int32_t dtype, int32_t K, int32_t mh, int32_t mw,
                          const float* cls_dev, const float* conf_dev, int32_t out_w, int32_t out_h, int32_t* map_dev);
/* test hook, host only: the units the kernels are built on, out[8] = pixels per workgroup of the arg-max and the instance
 * kernel, channel (instance) slices per workgroup (its waves), channels (instances) per step of a wave - slice s walks the
 * steps s, s + slices, .. -, elements per load of those kernels, output pixels per lane and threads per workgroup of the
 * resize kernel, threads per workgroup of the other two, 0 */
int gsx_debug_segmap_constants(int32_t* out);
/* replaces dls.py:156-158 after the model call: transformers' post_process_instance_segmentation(outputs, target_sizes=[(out_h,
 * out_w)]) from the selected slots on, op for op (tests/queries_model.py is the specification).  Runs on the ctx stream like
 * the two calls above, reads nothing back, synchronises nothing and writes only its outputs.
 * masks_dev: (Q, h, w) mask logits of gsx_float_dtype dtype, fp16 and bf16 widened to fp32 exactly.  The K slots are what
 * softmax(class logits)[:, :-1].flatten().topk(Q, sorted=False) selected, in that order: slot_query = index / C,
 * slot_label = index % C, slot_score; the same query may fill several slots.  (The selection stays with the caller: its order
 * is torch's own.)  All three are device arrays [K]; slot_label_dev may be NULL in mode GSX_QUERIES_SEGMENTS.
 *  1. bilinear (h, w) -> (mid_h, mid_w), torch's align_corners=False rule in fp32 per axis: scale = (float)S / D,
 *     src = max(scale * (d + 0.5f) - 0.5f, 0), i0 = (int)src, i1 = i0 + (i0 < S - 1), l1 = src - i0, l0 = 1 - l1,
 *     v = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11), every product and sum rounded to fp32 (no FMA; torch's
 *     CPU kernel fuses some, so against torch a pixel with |v| <= 2^-20 max|logit| may differ).  A pixel is set iff v > 0.
 *  2. pred = slot_score * ((float)sum / ((float)count + 1e-6f)): sum of sigmoid(v) over the set mid-grid pixels, accumulated in
 *     fp64 in a fixed order and rounded once; count of the set pixels.  A NaN anywhere in the slot's upsampled mask makes pred NaN.
 *  3. a slot is accepted iff a set pixel lies on a mid-grid column and row the target grid reads (step 5) and
 *     (double)pred >= threshold.  A slot with slot_query outside [0, Q) is rejected, reads nothing and scores 0.  Segment id =
 *     the number of accepted slots before it.
 *  4. each mid-grid pixel takes the highest accepted slot whose bit is set: its segment id (GSX_QUERIES_SEGMENTS, the
 *     reference's map) or its slot_label (GSX_QUERIES_LABELS); -1 without one.
 *  5. nearest resize to (out_h, out_w) by torch's rule, min((int)floorf(d * scale), S - 1) with scale = (float)S / D in fp32 -
 *     not OpenCV's rule above.
 * slot_segment_dev (int32 [K], the segment id or -1) and slot_pred_score_dev (fp32 [K], pred) may be NULL; together they stand
 * in for segments_info.  K == 0 writes an all -1 map.
 * Errors, before anything touches the device: GSX_E_INVALID for a NULL ctx, masks_dev or map_dev, a NULL slot array when K > 0,
 * a size <= 0, K < 0, an unknown dtype or mode, a pointer not aligned to its element, a non-finite threshold;
 * GSX_E_UNSUPPORTED for K > 1024 and for Q * h * w, mid_h * mid_w, out_h * out_w or K * mid_h * ceil(mid_w / 64) >= 2^31. */
typedef enum gsx_queries_mode {
    GSX_QUERIES_SEGMENTS = 0,
    GSX_QUERIES_LABELS = 1
} gsx_queries_mode;
int gsx_segmap_from_queries(gsx_ctx* ctx, const void* masks_dev, int32_t dtype, int32_t Q, int32_t h, int32_t w,
                            int32_t K, const int32_t* slot_query_dev, const float* slot_score_dev, const int32_t* slot_label_dev,
                            int32_t mid_w, int32_t mid_h, double threshold, int32_t mode, int32_t out_w, int32_t out_h,
                            int32_t* map_dev, int32_t* slot_segment_dev, float* slot_pred_score_dev);
/* test hook, host only: the units the query kernels are built on, out[8] = mid-grid columns per wave (one bit word), rows per
 * workgroup of the mask kernel (one partial sum), rows per wave, slots per ballot word of the segment-id scan, waves of the
 * accept kernel (wave s reduces the slots s, s + waves, ..), the most slots of a call, threads per workgroup of the mask kernel, 0 */
int gsx_debug_queries_constants(int32_t* out);
/* test hook, host only: the units the device map pack (gsx_vote_view_device, gsx_vote_views_device, "host_pack" = 0) is built on,
 * out[8] = cells (threads) per workgroup, maps per launch, pixel columns per strip and pixel rows per band of the full-resolution
 * level, cells per strip and cell rows per band of the coarse level, pool-form maps per H2D copy (slots per group of the pinned
 * ring), the most compact records per H2D copy and expansion launch */
int gsx_debug_segpack_constants(int32_t* out);

/* ---------------------------------------------------------------------------------------------
 * profiling hooks (HIP events on the ctx stream around each kernel launch)
 * ------------------------------------------------------------------------------------------- */
int gsx_profile_enable(gsx_ctx* ctx, int on);
int gsx_profile_reset(gsx_ctx* ctx);
/* the index-th kernel name seen since profiling was first enabled, or NULL past the end */
const char* gsx_profile_name(gsx_ctx* ctx, int32_t index);
/* worker threads (including the caller) gsx_vote_view packs host maps with; starts the pool if need be */
int gsx_host_threads(gsx_ctx* ctx);
/* the pool size a context would choose on its own in this process right now (no context, no GPU needed) */
int gsx_default_host_threads(void);
/* name: "vote_fused_labels", "seg_pack", "iou_pack", "iou_pairs", "iou_table", "iou_top_index", "segmap_argmax", "segmap_masks", "segmap_resize", "queries_sampled", "queries_mask", "queries_accept", "queries_compose", ...; returns launches and total milliseconds since reset */
int gsx_profile_get(gsx_ctx* ctx, const char* name, int64_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* GSX_H */
