/* f3ds.h -- C-ABI of libf3ds: MI355X-native supervoxel + hierarchical-merge segmenter.
 *
 * One call replaces, for one XYZRGBA frame, the whole hot path of the reference
 * (citations are into /root/reference):
 *
 *   frame prelude  (z<0 -> |z|)                         src/supervoxel_clustering.cpp:313-340
 *   pcl::SupervoxelClustering<PointXYZRGBA> sequence    src/supervoxel_clustering.cpp:348-367
 *   Clustering::set_initialstate / cluster(threshold)   src/clustering.cpp:605-612, 670-679
 *   Clustering::get_labeled_cloud / get_colored_cloud   src/clustering.cpp:631-663
 *
 * The reference has no FFI of its own (it is a C++ CLI); a maintainer who wants to keep
 * main() and swap the path would bind exactly these entry points (INTEGRATION.md shows the
 * replacement block for main()).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Threading: one f3ds_ctx per host thread / stream; calls on one ctx are serial.
 * Errors: negative int codes (f3ds_strerror); nothing throws across this boundary.
 * Memory: caller owns every in/out buffer; the ctx owns its device scratch (grow-only).
 */
#ifndef F3DS_H_
#define F3DS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F3DS_VERSION 120

/* label written for points that belong to no region (non-finite input point, or a voxel no
 * supervoxel ever claimed).  The reference never emits such points at all
 * (Clustering::get_labeled_cloud only walks owned voxels, src/clustering.cpp:640-663). */
#define F3DS_NO_LABEL 0xFFFFFFFFu

/* error codes */
#define F3DS_OK 0
#define F3DS_ERR_ARG (-1)          /* null pointer / bad parameter value                        */
#define F3DS_ERR_NO_DEVICE (-2)    /* HIP runtime found no usable GPU                           */
#define F3DS_ERR_HIP (-3)          /* a HIP call failed (f3ds_last_hip_error has the text)      */
#define F3DS_ERR_DEPTH (-4)        /* voxel grid needs more than 21 octree levels               */
#define F3DS_ERR_LOGIC (-5)        /* call order (e.g. recluster before segment):
                                      std::logic_error in src/clustering.cpp:671-673            */
#define F3DS_ERR_RANGE (-6)        /* lambda outside [0,1] / bins < 0:
                                      std::invalid_argument in src/clustering.cpp:578,593       */
#define F3DS_ERR_UNSUPPORTED (-7)  /* degenerate input the device path refuses (documented)     */
#define F3DS_ERR_IO (-8)           /* PCD file could not be read / written                      */
#define F3DS_ERR_EQ_BIN (-9)       /* --EQ with delta_g == 1.0: map::at throws in the reference
                                      (src/clustering.cpp:371-372, t_g has no clamp)            */
#define F3DS_ERR_CAPACITY (-10)    /* output buffer too small                                   */
#define F3DS_ERR_BUSY (-11)        /* frame pipeline: every slot in flight / oldest frame not done yet */
#define F3DS_ERR_EMPTY (-12)       /* frame pipeline: nothing submitted that has not been taken */
#define F3DS_ERR_OUT_OF_RANGE (-13) /* std::out_of_range in the reference: an adjacency names a
                                      supervoxel label that is not in the set (map::at,
                                      src/clustering.cpp:228-229); all_thresh bounds outside
                                      [0,1] (:694-698)                                           */

/* enums mirror include/supervoxel_clustering/clustering.h:58-68 */
enum { F3DS_LAB_CIEDE00 = 0, F3DS_RGB_EUCL = 1 };
enum { F3DS_NORMALS_DIFF = 0, F3DS_CONVEX_NORMALS_DIFF = 1 };
enum { F3DS_MANUAL_LAMBDA = 0, F3DS_ADAPTIVE_LAMBDA = 1, F3DS_EQUALIZATION = 2 };

/* CLI flags of the reference (src/supervoxel_clustering.cpp:187-298) as a plain struct */
typedef struct f3ds_params {
    float voxel_res;          /* -v   default 0.008                                      */
    float seed_res;           /* -s   default 0.08                                       */
    float w_color;            /* -c   default 0.2                                        */
    float w_spatial;          /* -z   default 0.4                                        */
    float w_normal;           /* -n   default 1.0                                        */
    int32_t use_transform;    /* !--NT  (setUseSingleCameraTransform, :349)              */
    int32_t color_metric;     /* --RGB -> F3DS_RGB_EUCL, else F3DS_LAB_CIEDE00           */
    int32_t geom_metric;      /* --CVX -> F3DS_CONVEX_NORMALS_DIFF                       */
    int32_t merging;          /* --ML / --AL / --EQ                                      */
    float lambda;             /* --ML value; used only under F3DS_MANUAL_LAMBDA          */
    int32_t bins;             /* --EQ value; used only under F3DS_EQUALIZATION           */
    float threshold;          /* -t                                                      */
    int32_t leaf_order;       /* 0: octree leaves ascending (PCL >= 1.9), 1: descending  */
    int32_t fold_negative_z;  /* main()'s z<0 -> |z| (:317-321); the CLI always sets 1   */
} f3ds_params;

typedef struct f3ds_result {
    uint64_t n_points;            /* N                                                   */
    uint64_t n_finite;            /* points with finite x,y,z                            */
    uint32_t n_voxels;            /* V  occupied voxels                                  */
    uint32_t octree_depth;        /* levels of the voxel grid cube                       */
    uint32_t n_seed_cells;        /* occupied seed-resolution cells before filtering     */
    uint32_t n_seeds;             /* seeds kept = supervoxel helpers created             */
    uint32_t n_supervoxels;       /* S  non-empty supervoxels after the sweeps           */
    uint32_t n_edges;             /* E  undirected supervoxel adjacencies                */
    uint32_t n_merges;            /* merges performed below the threshold                */
    uint32_t n_regions;           /* K  regions left                                     */
    uint32_t sweeps;              /* max_depth-1 label-propagation sweeps                */
    float lambda;                 /* lambda actually used (Clustering::get_lambda)       */
    float ms_total;               /* wall time of the call, host clock                   */
    float ms_stage[8];            /* device time per stage (HIP events): 0 voxelise,
                                     1 neighbours+normals, 2 seeds, 3 sweeps, 4 supervoxel
                                     summaries+edges, 5 merge, 6 labels; 7 = the voxel-normal
                                     kernel's launch alone (part of stage 1): HIP event pair
                                     around that dispatch on the call's stream          */
} f3ds_result;

typedef struct f3ds_ctx f3ds_ctx;

void f3ds_default_params(f3ds_params* p);
int f3ds_version(void);
/* "f3ds 1.2.0 src:<16 hex digits>": the digits are the SHA-256 prefix of the sources the library was built from
 * (csrc/Makefile writes it at build time); tests and bench.py compare it with the sources on disk so that a stale
 * prebuilt libf3ds.so fails loudly.  A library built with the timing experiments compiled in ends in " +whatif"; a
 * process whose environment opens the development switches (below) gets " +dev" appended. */
const char* f3ds_version_string(void);
/* 1 when F3DS_DEV is set (to anything but "0") in the environment: only then does the library read its development
 * switches (F3DS_MERGE_NW, F3DS_VOX_TILES, ... -- kernel layouts and test hooks, none changes results).
 * Without it they are ignored, whatever the environment holds. */
int f3ds_dev_mode(void);
const char* f3ds_strerror(int code);
const char* f3ds_last_hip_error(void);

/* number of visible GPUs (0 when there is none); never initialises a device */
int f3ds_device_count(void);

/* create a context on `device` with its own stream.  Fails with F3DS_ERR_NO_DEVICE when the
 * HIP runtime has no GPU: there is no CPU fallback in this library. */
int f3ds_create(int device, f3ds_ctx** out);
void f3ds_destroy(f3ds_ctx* ctx);

/* run on a caller-provided hipStream_t (e.g. a torch stream) instead of the ctx's own */
int f3ds_set_stream(f3ds_ctx* ctx, void* hip_stream);

/* Segment one frame.  `points` is N records {float x,y,z; uint32 rgba} (16 B, rgba packed
 * a<<24|r<<16|g<<8|b as PCL does).  points_on_device / labels_on_device say where the caller's
 * buffers live.  point_labels receives N region ids (0..K-1 in the order of
 * Clustering::get_labeled_cloud, F3DS_NO_LABEL for points outside every region).
 * Synchronous: returns after the labels are in the caller's buffer. */
int f3ds_segment(f3ds_ctx* ctx, const void* points, size_t n, int points_on_device,
                 const f3ds_params* params, uint32_t* point_labels, int labels_on_device,
                 f3ds_result* result);

/* A batch of independent frames on one GPU, one context per frame (BASELINE.json config 5 puts 8
 * frames on each GPU).  Same result per frame as f3ds_segment; every kernel of the path is one
 * dispatch for all frames and all merge loops run as one dispatch.  points[i] / point_labels[i] /
 * counts[i] belong to ctxs[i]; results may be NULL.  Synchronous.  The batch runs on the stream set
 * with f3ds_set_stream on ctxs[0] if there is one, else on one of a few library-owned streams per
 * device (one per hardware queue), so that batch calls from several host threads run side by side.
 * Host buffers (points_on_device / labels_on_device == 0): the uploads and downloads of ALL calls on a device go
 * through one library-owned copy stream, one copy after the other -- the PCIe link moves 55 GB/s one way alone and ~16
 * each way when uploads and downloads of different calls overlap; the call's kernels wait for its uploads by event.
 * Pinned (hipHostMalloc) buffers are what makes these copies asynchronous; pageable ones work and are slower. */
int f3ds_segment_batch(f3ds_ctx** ctxs, int nctx, const void* const* points, const size_t* counts,
                       int points_on_device, const f3ds_params* params, uint32_t* const* point_labels,
                       int labels_on_device, f3ds_result* results);

/* ---- RGB-D frames: a depth image, a colour image and pinhole intrinsics in, the records built on the device ----
 * Pixel (u, v) becomes point v * width + u.  u16 depth d: invalid iff d == 0, else z = (float)d * depth_scale; f32 depth d:
 * invalid iff !(d > 0) or d is infinite (NaN, zero and negatives included), else z = d * depth_scale.  A valid pixel gets
 * x = (((float)u - cx) * z) / fx, y = (((float)v - cy) * z) / fy and z as is, every operation one rounded f32 operation; an
 * invalid one gets quiet NaN in x, y and z (such a point belongs to no voxel and is labelled F3DS_NO_LABEL).  The colour word
 * is a<<24 | r<<16 | g<<8 | b: F3DS_COLOR_RGB8 = 3 bytes r, g, b per pixel, alpha 255; F3DS_COLOR_RGBA8 = 4 bytes r, g, b, a;
 * F3DS_COLOR_PACKED = a u32 per pixel that is the word itself.  Rows are addressed through the pitches; nothing but the
 * element's own alignment is assumed of them (RGB8 rows with an odd pitch are fine). */
enum { F3DS_DEPTH_U16 = 0, F3DS_DEPTH_F32 = 1 };
enum { F3DS_COLOR_RGB8 = 0, F3DS_COLOR_RGBA8 = 1, F3DS_COLOR_PACKED = 2 };
typedef struct f3ds_rgbd_format {
    uint32_t width, height;
    int32_t depth_type;           /* F3DS_DEPTH_*                                            */
    float depth_scale;            /* metres per depth unit, e.g. 0.001f                      */
    int32_t color_format;         /* F3DS_COLOR_*                                            */
    uint32_t depth_pitch, color_pitch;   /* bytes per image row; 0 = tightly packed          */
    float fx, fy, cx, cy;
} f3ds_rgbd_format;

/* host arithmetic only, no device needed: the width * height records the device path builds, bit for bit.  F3DS_ERR_ARG for a NULL
 * pointer, width or height 0, width * height > 0x7fffffff, an unknown enum value, fx / fy / depth_scale not finite, fx or fy
 * equal to 0, depth_scale <= 0, cx or cy not finite, a non-zero pitch smaller than a row, or a depth pitch that is no multiple
 * of the depth element's size (the rgbd entry points below refuse the same). */
int f3ds_deproject(const f3ds_rgbd_format* fmt, const void* depth, const void* color, void* points16);

/* f3ds_segment / f3ds_segment_batch on the records of f3ds_deproject, which are built on the device (d_deproject): the same
 * labels, f3ds_result counts and F3DS_DBG_* arrays, and afterwards the context answers every call it answers after
 * f3ds_segment (truth labels are one per pixel).  Host images go through the device's copy stream like host points, at 5 to 8
 * bytes per pixel where the records take 16; images_on_device: they are read where they are.  One format for the whole batch.
 * A frame whose pixels are all invalid returns F3DS_OK with all labels F3DS_NO_LABEL. */
int f3ds_segment_rgbd(f3ds_ctx* ctx, const f3ds_rgbd_format* fmt, const void* depth, const void* color, int images_on_device,
                      const f3ds_params* params, uint32_t* point_labels, int labels_on_device, f3ds_result* result);
int f3ds_segment_rgbd_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth, const void* const* color,
                            int images_on_device, const f3ds_params* params, uint32_t* const* point_labels, int labels_on_device,
                            f3ds_result* results);

/* the XYZRGBA records the context's last segment call ran on, when the context owns them (an rgbd call, or a call with host
 * points); F3DS_ERR_LOGIC when they were the caller's device buffer or nothing has run.  points16 == NULL: count only.
 * F3DS_ERR_CAPACITY when cap (in records) is smaller than the count. */
int f3ds_get_points(f3ds_ctx* ctx, void* points16, size_t cap, int dst_on_device, size_t* n_out);

/* ---- label tracker: persistent ids for the regions of consecutive RGB-D frames ----------------------------------------------
 * A frame's region ids are ranks (0..K-1) and relate to nothing in the next frame.  A tracker turns each frame's labels into TRACK IDS that
 * follow surfaces: it holds the previous frame on the device -- per pixel a slot (that frame's region label, or F3DS_NO_LABEL) and an f32 depth
 * (NaN = invalid) --, the previous format, a host table prev_id[slot] and next_id (0 at creation).  One update, bit for bit (csrc/f3ds_track.h):
 *  1. point     pixel p = v * width + u gets (x, y, z) by the rule of f3ds_deproject; it is VALID iff its depth is, LABELLED iff valid and label[p] != F3DS_NO_LABEL.
 *  2. transform with a pose (12 floats, row-major 3 x 4, p_prev = R p_cur + t): xp = ((r00*x + r01*y) + r02*z) + t0, likewise yp, zp, every operation one
 *               rounded f32 operation, none fused; a NULL pose is the identity and does no arithmetic.
 *  3. project   uf = (xp * fx) / zp + cx, vf = (yp * fy) / zp + cy, us = uf + 0.5f, vs = vf + 0.5f.  The point lands on pixel (floor(us), floor(vs)) of the
 *               previous frame iff zp > 0, zp is finite, 0 <= us < (float)width and 0 <= vs < (float)height (comparisons with NaN fail).
 *  4. vote      a labelled pixel of region i that lands on q votes for j = slot[q] iff j != F3DS_NO_LABEL and fabsf(zp - z_prev[q]) <= depth_tol * zp; otherwise
 *               it is a no-vote.  size[i] = the labelled pixels of region i (votes and no-votes), count[i][j] = its votes for j.  On the first update, or
 *               after a reset, every labelled pixel is a no-vote.
 *  5. assign    (integers only) entry (i, j, c = count[i][j]) is eligible iff c >= max(min_votes, 1) and (uint64)c * 1000 >= (uint64)min_permille * size[i].
 *               Eligible entries are visited by c descending, then i ascending, then j ascending; one is taken iff region i has no id yet and slot j has not been
 *               claimed: id[i] = prev_id[j].  Then the regions with size[i] > 0 and no id get next_id++ in ascending i; regions with size[i] == 0 get
 *               F3DS_NO_LABEL and use no id.  Ids are never reused; a next_id that would reach 0xFFFFFFFF is F3DS_ERR_UNSUPPORTED.
 *  6. output    track_ids[p] = F3DS_NO_LABEL if label[p] == F3DS_NO_LABEL, else id[label[p]] (also where the depth is invalid).  New state: slot[p] = label[p]
 *               if labelled, else F3DS_NO_LABEL; z_prev[p] = z if valid, else NaN; prev_id = id; the format is remembered.
 * So ids follow surfaces and not label numbers; of the parts of a split region the one with more votes keeps the id; a merged region takes the id with
 * more votes and the other id retires.
 * The colour fields of the format are not looked at.  labels: one u32 per pixel, < n_regions or F3DS_NO_LABEL (what f3ds_segment_rgbd wrote and
 * f3ds_result.n_regions counts).  inputs_on_device: depth and labels are device memory, read where they are; host ones go through the device's copy stream.
 * ids_on_device likewise for track_ids.  Synchronous.  The work per pixel is on the device (csrc/f3ds_track.inc); the host sees the distinct (i, j) pairs only.
 * Errors: F3DS_ERR_ARG for a NULL pointer, what f3ds_deproject refuses of a format, a non-finite pose entry, depth_tol negative or not finite,
 * min_permille > 1000, a format whose width, height or intrinsics differ from the remembered one (reset first) and a label >= n_regions other than
 * F3DS_NO_LABEL (found on the device; the tracker is then unchanged); F3DS_ERR_UNSUPPORTED for n_regions > 0x00FFFFFF; F3DS_ERR_NO_DEVICE as f3ds_create;
 * F3DS_ERR_LOGIC from f3ds_tracker_get_ids before any update.  A frame without a valid pixel, or n_regions == 0, is F3DS_OK with all ids F3DS_NO_LABEL, and
 * leaves a state the next frame matches nothing in.  Threading as for a context: one tracker per host thread. */
typedef struct f3ds_track_params {
    uint32_t min_votes;           /* default 16                                              */
    uint32_t min_permille;        /* default 300: votes per thousand labelled pixels of the region */
    float depth_tol;              /* default 0.05f, relative to zp                           */
} f3ds_track_params;
typedef struct f3ds_track_result {
    uint32_t n_regions;           /* as given                                                */
    uint32_t n_nonempty;          /* regions with a labelled pixel                           */
    uint32_t n_matched;           /* ... that took a previous id                             */
    uint32_t n_new;               /* ... that got a new one                                  */
    uint32_t n_retired;           /* previous slots that had an id and were not claimed      */
    uint32_t n_entries;           /* distinct (i, j) pairs with votes                        */
    uint32_t next_id;             /* after the update                                        */
    uint32_t first_frame;         /* 1: there was no previous frame (first update, or after a reset); f3ds_track_assign writes 0 */
    uint64_t n_labelled, n_votes; /* labelled pixels; those of them that voted               */
} f3ds_track_result;
typedef struct f3ds_tracker f3ds_tracker;
void f3ds_default_track_params(f3ds_track_params* p);
/* a tracker on `device` with a stream of its own; params == NULL: the defaults */
int f3ds_tracker_create(int device, const f3ds_track_params* params, f3ds_tracker** out);
void f3ds_tracker_destroy(f3ds_tracker* t);
int f3ds_tracker_set_stream(f3ds_tracker* t, void* hip_stream);
/* forget the previous frame and the format; next_id is kept */
int f3ds_tracker_reset(f3ds_tracker* t);
int f3ds_tracker_update(f3ds_tracker* t, const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, int inputs_on_device,
                        const float* pose12 /* NULL = identity */, uint32_t* track_ids, int ids_on_device, f3ds_track_result* result /* may be NULL */);
/* id[] of the last update that returned F3DS_OK: n_regions entries.  id_of_region == NULL: count only; F3DS_ERR_CAPACITY when cap is smaller than the count */
int f3ds_tracker_get_ids(f3ds_tracker* t, uint32_t* id_of_region, size_t cap, size_t* n_out);
/* host arithmetic only, no device needed: steps 2 and 3 for n records {float x, y, z; uint32 rgba} -- pixel[k] = the previous frame's pixel index record k lands
 * on, or -1; zp[k] = its depth there (written for every record) */
int f3ds_track_reproject(const f3ds_rgbd_format* fmt, const float* pose12, const void* points16, size_t n, int32_t* pixel, float* zp);
/* host arithmetic only, no device needed: step 5.  size: n_regions; entries: n_entries rows (i, j, c), every (i, j) at most once, any order; prev_id: n_prev;
 * *next_id in and out; id_of_region: n_regions out; result may be NULL, params == NULL: the defaults.  F3DS_ERR_ARG also for an entry with i >= n_regions,
 * j >= n_prev, prev_id[j] == F3DS_NO_LABEL or c > size[i].  On an error nothing is written. */
int f3ds_track_assign(const f3ds_track_params* params, const uint32_t* size, uint32_t n_regions, const uint32_t* entries, size_t n_entries,
                      const uint32_t* prev_id, uint32_t n_prev, uint32_t* next_id, uint32_t* id_of_region, f3ds_track_result* result);

/* ---- region table: one fixed-size row per region of a label image over an RGB-D frame ----------------------------------------
 * What a consumer that follows objects asks of a frame: where each region is in the image, where it is in space, how big it is and what colour it has,
 * without downloading the label image.  labels: one u32 per pixel, < n_regions or F3DS_NO_LABEL -- what f3ds_segment_rgbd wrote, a level of
 * f3ds_labels_at_thresholds, or any other label image of the frame.  Row i is region i, so the row of a tracked region has the track id
 * id_of_region[i] of f3ds_tracker_get_ids.  The definition, bit for bit (csrc/f3ds_regions.h):
 *   point    pixel p = v * width + u gets (x, y, z) by the rule of f3ds_deproject; it is LABELLED iff its depth is valid and label[p] != F3DS_NO_LABEL
 *            (as in the tracker).  A pixel with a label and an invalid depth contributes to nothing.
 *   fixed    for a finite f32 a, fix(a) = (int64_t)rint(clamp((double)a, -32768.0, 32768.0) * 65536.0), rint rounding half to even: units of 2^-16 m.  A
 *            labelled pixel is CLAMPED iff the clamp changed one of its three coordinates.
 *   order    minima and maxima of floats are taken in the total order of key(bits) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): -0 is below +0.
 *   row      the fields below over the labelled pixels of the region; with color == NULL mean_rgb is 0.0f in every non-empty row.
 *   empty    a region without a labelled pixel has first_pixel = u_min = v_min = 0xFFFFFFFF, u_max = v_max = 0, lo = +inf, hi = -inf and
 *            centroid = mean_rgb = the quiet NaN 0x7FC00000.
 * Every field is an integer count, a minimum, a maximum or a sum of integers: the result does not depend on the order of evaluation, and the device
 * gives the bits of the host function.
 * Errors (both functions alike): F3DS_ERR_ARG for a NULL fmt, depth or labels, for NULL rows unless n_regions == 0, for what f3ds_deproject refuses of
 * a format (the two colour fields are looked at only when color != NULL) and for a label >= n_regions other than F3DS_NO_LABEL (the device function finds
 * it on the device and reports it at the call's one wait); rows and result are then not written, on the host or on the device.  F3DS_ERR_UNSUPPORTED for
 * n_regions > 0x00FFFFFF.  n_regions == 0, or a frame without a labelled pixel, is F3DS_OK: the rows, if there are any, are all empty. */
typedef struct f3ds_region_row {
    uint32_t n_pixels;                   /* labelled pixels of the region                                  */
    uint32_t first_pixel;                /* smallest pixel index among them                                */
    uint32_t u_min, v_min, u_max, v_max; /* inclusive pixel box                                            */
    float lo[3], hi[3];                  /* box of the points (x, y, z), in the order of key               */
    float centroid[3];                   /* (float)(((double)sum_fix / (double)n_pixels) / 65536.0)        */
    float mean_rgb[3];                   /* (float)((double)sum_channel / (double)n_pixels); r, g, b of the colour word */
} f3ds_region_row;
typedef struct f3ds_region_table_result { uint32_t n_regions, n_nonempty; uint64_t n_labelled, n_clamped; } f3ds_region_table_result;
/* host arithmetic only, no device needed: the definition */
int f3ds_region_table_host(const f3ds_rgbd_format* fmt, const void* depth, const void* color /* may be NULL */, const uint32_t* labels,
                           uint32_t n_regions, f3ds_region_row* rows, f3ds_region_table_result* result /* may be NULL */);
/* the same rows from the device, in one read of the images (csrc/f3ds_regions.inc).  inputs_on_device: depth, color and labels are device memory and
 * read where they are; host inputs go through the device's copy stream like those of f3ds_tracker_update.  rows_on_device: rows is device memory;
 * host rows arrive with the call's one small download.  Synchronous.  Runs on ctx's stream and uses scratch of its own only: every other call on the
 * context behaves as if this one never happened (as f3ds_evaluate_levels).  Also F3DS_ERR_ARG for a NULL ctx. */
int f3ds_region_table(f3ds_ctx* ctx, const f3ds_rgbd_format* fmt, const void* depth, const void* color, const uint32_t* labels, uint32_t n_regions,
                      int inputs_on_device, f3ds_region_row* rows, int rows_on_device, f3ds_region_table_result* result);

/* ---- region contacts: one fixed-size row per pair of regions of a label image that touch ------------------------------------
 * The region table's companion: which regions touch in the image, along how long a border, and whether the border is a surface contact or one object in
 * front of another -- without downloading the label image.  labels, n_regions and the region ids are the region table's (any label image of the frame; a
 * row's a and b index the table's rows and f3ds_tracker_get_ids).  The definition, bit for bit (csrc/f3ds_contacts.h):
 *   point    pixel p = v * width + u gets z by the rule of f3ds_deproject; it is LABELLED iff its depth is valid and label[p] != F3DS_NO_LABEL (as in the
 *            tracker and the table).  The colour fields of the format are not looked at.
 *   pairs    every pixel p forms a pair with its right neighbour p + 1 when u + 1 < width and with its lower neighbour p + width when v + 1 < height:
 *            4-connectivity, each unordered pixel pair once.  A pair is a CONTACT iff both pixels are labelled and their labels differ; it belongs to
 *            (a, b) = (smaller label, larger label).  A label over an invalid depth takes part in nothing.
 *   class    za, zb: the depths of a's and b's pixel.  g = fabsf(za - zb) (one rounded f32 subtraction), zn = za < zb ? za : zb.  The pair is CLOSE iff
 *            g <= depth_tol * zn (one rounded f32 product; the comparison fails on NaN).  A pair that is not close has a in front iff za < zb, else b.
 *            Nothing is fused.
 *   gap      sum_fix_gap adds fix(g) of the region table (units of 2^-16 m, g clamped to 32768 m; rint rounds half to even).
 *   rows     one row per (a, b) with at least one contact, by a ascending, then b ascending.  result->n_contacts = the number of rows, result->n_pairs
 *            and result->n_close the sums of those two fields over the rows.
 *   capacity *n_out receives the row count on F3DS_OK and on F3DS_ERR_CAPACITY.  rows == NULL: count only, cap is ignored.  cap smaller than the count:
 *            F3DS_ERR_CAPACITY, no row is written, result is written.
 * Every field is an integer count, a minimum or a sum of integers: the result does not depend on the order of evaluation, and the device gives the bits
 * of the host function.  4-connectivity in the image only: no diagonal pairs, no contact normals in space.
 * Errors (both functions alike): F3DS_ERR_ARG for a NULL fmt, depth, labels or n_out, for what f3ds_deproject refuses of a format (the two colour fields
 * are neutralised as in f3ds_tracker_update), for a depth_tol that is negative or not finite, and for a label >= n_regions other than F3DS_NO_LABEL on any
 * pixel, also one without a neighbour or over an invalid depth (the device function finds it on the device and reports it at the call's one wait); rows,
 * n_out and result are then not written, on the host or on the device.  F3DS_ERR_UNSUPPORTED for n_regions > 0x00FFFFFF.  n_regions == 0 with every label
 * F3DS_NO_LABEL, one region, a 1 x 1 image and a frame without a labelled pixel are F3DS_OK with zero rows. */
typedef struct f3ds_region_contact {          /* 32 bytes */
    uint32_t a, b;            /* region ids, a < b                                                      */
    uint32_t n_pairs;         /* contact pairs between a and b                                          */
    uint32_t n_close;         /* ... whose two depths agree                                             */
    uint32_t n_a_front;       /* ... not close, and a's pixel is the nearer one; b is in front in the   */
                              /*     remaining n_pairs - n_close - n_a_front                            */
    uint32_t n_horizontal;    /* ... whose pixels are left/right neighbours (the rest: upper/lower)     */
    uint32_t first_pixel;     /* smallest index p of a pair's first (left or upper) pixel               */
    float    mean_gap;        /* (float)(((double)sum_fix_gap / (double)n_pairs) * 2^-16), metres       */
} f3ds_region_contact;
typedef struct f3ds_region_contacts_result { uint32_t n_regions, n_contacts; uint64_t n_pairs, n_close; } f3ds_region_contacts_result;
/* host arithmetic only, no device needed: the definition */
int f3ds_region_contacts_host(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, float depth_tol,
                              f3ds_region_contact* rows, size_t cap, size_t* n_out, f3ds_region_contacts_result* result /* may be NULL */);
/* the same rows from the device (csrc/f3ds_contacts.inc).  inputs_on_device: depth and labels are device memory and read where they are; host inputs go
 * through the device's copy stream like those of f3ds_region_table.  rows_on_device: rows is device memory (cap rows of it); host rows arrive with the
 * call's one download (a second one only for more than 2048 rows).  Synchronous.  Runs on ctx's stream and uses scratch of its own (and the sort's
 * histogram and scan buffers, which hold nothing between calls): every other call on the context behaves as if this one never happened.  Also
 * F3DS_ERR_ARG for a NULL ctx.  result may be NULL. */
int f3ds_region_contacts(f3ds_ctx* ctx, const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, float depth_tol,
                         int inputs_on_device, f3ds_region_contact* rows, size_t cap, int rows_on_device, size_t* n_out,
                         f3ds_region_contacts_result* result);

/* ---- region shapes: one fixed-size row per region of a label image: covariance, plane and principal axes -----------------------
 * The third member of the family: is a region a plane, which way does it face, how thick is it and along which direction is it long -- without
 * downloading the label image.  labels, n_regions and the region ids are the region table's: row i is region i, the table's row i and
 * f3ds_tracker_get_ids()[i].  No colour image; the two colour fields of the format are not looked at.  With a plane per row, a contact row (a, b) joins
 * two shape rows and says convex, concave or coplanar.  The definition, bit for bit (csrc/f3ds_shapes.h):
 *   point     the region table's: pixel p = v * width + u gets (x, y, z) by the rule of f3ds_deproject; it is LABELLED iff its depth is valid and
 *             label[p] != F3DS_NO_LABEL.
 *   fixed     the table's: f_a = fix(a) for a in x, y, z, units of 2^-16 m, |f_a| <= 2^31; a labelled pixel is CLAMPED iff the clamp changed one of its three
 *             coordinates.  So n_labelled, n_clamped, n_pixels and centroid are the table's bits.
 *   moments   per region, as exact integers over its labelled pixels: n (the count), S_a = sum f_a, M_ab = sum f_a * f_b for the six pairs ab in
 *             xx, xy, xz, yy, yz, zz.  n < 2^31, so |S_a| < 2^62 and |M_ab| < 2^93.
 *   scatter   N_ab = n * M_ab - S_a * S_b, exactly (|N_ab| < 2^125: a signed 128-bit integer).  There is no cancellation error: a flat region at constant
 *             depth has N_zz == 0 and cov[5] the bits of +0.0, however far away it is.
 *   cov       in f64, C_ab = (((double)N_ab / (double)n) / (double)n) * 2^-32, where (double)N_ab is the exact integer rounded to nearest, ties to even,
 *             once; (double)n is exact; the two divisions are IEEE; the scaling is exact.  cov[k] = (float)C_k in the order xx, xy, xz, yy, yz, zz.
 *   eigen     cyclic Jacobi on the symmetric f64 matrix C (indices 0, 1, 2 = x, y, z) with V = the identity.  Exactly 8 sweeps, each over (p, q) = (0, 1),
 *             (0, 2), (1, 2) in this order.  A rotation is skipped iff C[p][q] == 0.0.  Otherwise, in this order:
 *               theta = (C[q][q] - C[p][p]) / (2.0 * C[p][q])
 *               t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0)), negated if theta < 0
 *               c = 1.0 / sqrt(t * t + 1.0), s = t * c
 *               C[p][p] -= t * C[p][q];  C[q][q] += t * C[p][q]  (the old C[p][q] in both);  C[p][q] = C[q][p] = 0
 *               for the third index r: C[r][p], C[r][q] = c * C[r][p] - s * C[r][q], s * C[r][p] + c * C[r][q], both from the old values, and mirrored
 *               for k = 0, 1, 2: V[k][p], V[k][q] = c * V[k][p] - s * V[k][q], s * V[k][p] + c * V[k][q], both from the old values
 *             Only f64 + - * / and sqrt, every operation rounded once and nothing fused; nothing data-dependent ends the loop but the exact-zero skip.
 *             Afterwards lambda_k = C[k][k] belongs to column k of V.
 *   order     a lambda below 0 becomes +0.0.  The three (lambda, column) pairs are sorted by lambda ascending, ties by column index ascending.
 *             eigenvalue[k] = (float)lambda_k.
 *   normal    v = the column of lambda_0 as Jacobi left it (not renormalised).  With the f64 centroid c_a = ((double)S_a / (double)n) * 2^-16 (centroid[a] is
 *             (float)c_a), d = (v_x * c_x + v_y * c_y) + v_z * c_z in f64.  If d > 0, v and d are negated.  normal = (float)v, plane_d = (float)(-d).
 *   axis      w = the column of lambda_2.  Its component of largest magnitude, the first in x, y, z order among equal magnitudes, decides: w is negated iff
 *             that component is < 0.  axis = (float)w.
 *   curvature sum = (lambda_0 + lambda_1) + lambda_2 (after the clamp); curvature = sum > 0 ? (float)(lambda_0 / sum) : 0.0f.
 *   empty     a region without a labelled pixel has n_pixels = 0 and the quiet NaN 0x7FC00000 in all twenty floats.
 * A region of one point, of identical points, has an all-zero C: nothing rotates, V stays the identity, the eigenvalues are 0, 0, 0 and normal is
 * (-1, 0, 0) or (1, 0, 0) by the flip rule.  That, and the normal of a region whose points lie on a line, is defined but MEANINGLESS: look at
 * eigenvalue[1] before believing a normal, and at eigenvalue[2] before believing an axis.
 * Everything that meets more than one pixel is a sum of integers: the result does not depend on the order of evaluation, and the device gives the bits of
 * the host function.
 * Errors (both functions alike): F3DS_ERR_ARG for a NULL fmt, depth or labels, for NULL rows unless n_regions == 0, for what f3ds_deproject refuses of
 * a format (the two colour fields are neutralised as in f3ds_region_contacts) and for a label >= n_regions other than F3DS_NO_LABEL (the device function
 * finds it on the device and reports it at the call's one wait); rows and result are then not written, on the host or on the device.
 * F3DS_ERR_UNSUPPORTED for n_regions > 0x00FFFFFF.  n_regions == 0, or a frame without a labelled pixel, is F3DS_OK: the rows, if there are any, are all
 * empty. */
typedef struct f3ds_region_shape {      /* 84 bytes, 21 words */
    uint32_t n_pixels;        /* labelled pixels of the region (the table's n_pixels)                     */
    float centroid[3];        /* the table's centroid, the same bits                                      */
    float cov[6];             /* xx, xy, xz, yy, yz, zz: population covariance (divided by n), m^2        */
    float eigenvalue[3];      /* of cov, ascending, negatives clamped to +0                               */
    float normal[3];          /* unit eigenvector of eigenvalue[0], turned towards the camera (origin)    */
    float axis[3];            /* unit eigenvector of eigenvalue[2]: the direction the region is long in   */
    float plane_d;            /* normal . p + plane_d = 0 is the plane through the centroid; >= 0         */
    float curvature;          /* eigenvalue[0] / (sum of the three): PCL's surface variation; 0 if sum 0  */
} f3ds_region_shape;
typedef struct f3ds_region_shapes_result { uint32_t n_regions, n_nonempty; uint64_t n_labelled, n_clamped; } f3ds_region_shapes_result;
/* host arithmetic only, no device needed: the definition */
int f3ds_region_shapes_host(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions,
                            f3ds_region_shape* rows, f3ds_region_shapes_result* result /* may be NULL */);
/* the same rows from the device, in one read of the image and the labels (csrc/f3ds_shapes.inc).  inputs_on_device: depth and labels are device memory
 * and read where they are; host inputs go through the device's copy stream like those of f3ds_region_table.  rows_on_device: rows is device memory; host
 * rows arrive with the call's one small download.  Synchronous.  Runs on ctx's stream and uses scratch of its own only: every other call on the context
 * behaves as if this one never happened.  Also F3DS_ERR_ARG for a NULL ctx.  result may be NULL. */
int f3ds_region_shapes(f3ds_ctx* ctx, const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions,
                       int inputs_on_device, f3ds_region_shape* rows, int rows_on_device, f3ds_region_shapes_result* result);

/* ---- region boxes: one fixed-size row per region of a label image: the box along the region's own axes, and its plane residuals ---
 * A member of the family for the question the others leave open: how big is a region along its OWN axes, and is it a plane or does it merely have most of
 * its mass near one.  The table's lo / hi is a box in camera axes (a table top seen at an angle gets a box that is mostly air); the shapes' eigenvalues are
 * variances, not extents.  labels, n_regions and the region ids are the region table's: row i is region i.  No colour image; the two colour fields of the
 * format are not looked at.  Two passes over the pixels -- the shapes, then every pixel measured in the frame of its region -- in one call.  The
 * definition, bit for bit (csrc/f3ds_boxes.h):
 *   point      the family's: pixel p = v * width + u gets (x, y, z) by the rule of f3ds_deproject; it is LABELLED iff its depth is valid and
 *              label[p] != F3DS_NO_LABEL.  fixed and CLAMPED are the table's.  n_labelled, n_clamped, n_nonempty and n_pixels are the bits of
 *              f3ds_region_shapes.
 *   shape      S_i = the row f3ds_region_shapes defines for region i.  A non-NULL `shapes` receives exactly those rows, the same bits as that call.
 *   frame      of a non-empty region, from the public floats of S_i only: c = S_i.centroid, n = S_i.normal, l = S_i.axis, m = n x l with
 *              m_x = n_y * l_z - n_z * l_y, m_y = n_z * l_x - n_x * l_z, m_z = n_x * l_y - n_y * l_x: each component two rounded f32 products and one
 *              rounded f32 subtraction.  n, m, l go into the row as they are: unit and orthogonal to f32 accuracy only (some 2^-22), not exactly.
 *   coordinate q_a for a in x, y, z = (float)((double)f_a * 2^-16) with the f_a of `fixed`: the coordinate on the grid of 2^-16 m, clamped to +-32768 (a NaN
 *              to -32768), converted once.  These are the points the shape row was computed from: its centroid lives on the same grid, so a pixel is
 *              measured against the frame in the units the frame was made in.  Every q_a is finite, so nothing below produces a NaN from a valid frame.
 *   projection d_a = q_a - c_a; for each axis e in n, m, l: t_e = (d_x * e_x + d_y * e_y) + d_z * e_z.  Every operation is one rounded f32 operation, in
 *              this order, nothing fused.  The bits of t_e are canonicalised (t != t ? 0x7FC00000 : bits): a frame nobody foresaw cannot make host and
 *              device differ in a NaN's sign or payload.
 *   extents    lo[k], hi[k] (k = 0, 1, 2 for n, m, l) = the minimum and maximum of t over the region's labelled pixels in the total order of
 *              key(bits) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000), the table's: -0 below +0.  They are relative to the CENTROID, not to center.
 *   plane      r = fabsf(t_n).  The pixel is an INLIER iff r <= plane_tol (plane_tol may be 0 and may be +inf).  sum_fix_r adds fix(r), units of 2^-16 m;
 *              mean_abs_residual = (float)(((double)sum_fix_r / (double)n_pixels) * 2^-16).
 *   box        half[k] = (hi[k] - lo[k]) * 0.5f, mid[k] = (lo[k] + hi[k]) * 0.5f, center_a = ((c_a + mid[0] * n_a) + mid[1] * m_a) + mid[2] * l_a, each
 *              operation rounded once.  The box is the eight points center +- half[0] n +- half[1] m +- half[2] l.
 *   empty      a region without a labelled pixel has n_pixels = n_inliers = 0 and the quiet NaN 0x7FC00000 in all 22 floats.
 * A region of one point or of points on a line has a frame that is defined but MEANINGLESS, as in the shapes: look at S_i.eigenvalue[1] before believing
 * axis_n and half[0], at eigenvalue[2] before believing axis_l.  A region at one constant depth z has half[0] == 0 exactly: cov has an exactly zero z row, the
 * Jacobi sweeps leave n = (0, 0, -1), q_z == c_z for every pixel (both are the one depth on the grid), and t_n is +-0 for every pixel: lo[0], hi[0] and
 * mean_abs_residual are zeros and every pixel is an inlier even at plane_tol == 0.
 * Everything that meets more than one pixel is a count, a minimum, a maximum or a sum of integers: the result does not depend on the order of evaluation,
 * and the device gives the bits of the host function.
 * Errors (both functions alike, in this order): what f3ds_region_shapes answers with F3DS_ERR_ARG before it looks at a pixel, with `rows` in the role of
 * its rows (`shapes` may always be NULL); F3DS_ERR_ARG for a plane_tol that is negative or NaN; F3DS_ERR_UNSUPPORTED for n_regions > 0x00FFFFFF;
 * F3DS_ERR_ARG for a label >= n_regions other than F3DS_NO_LABEL (the device function finds it on the device and reports it at the call's one wait).
 * After an error neither rows, shapes nor result is written, on the host or on the device.  n_regions == 0, or a frame without a labelled pixel, is
 * F3DS_OK: the rows, if there are any, are all empty. */
typedef struct f3ds_region_box {      /* 96 bytes, 24 words */
    uint32_t n_pixels;        /* labelled pixels of the region (the table's / the shapes' n_pixels)   */
    uint32_t n_inliers;       /* ... whose distance to the region's plane is <= plane_tol             */
    float center[3];          /* centre of the box, camera coordinates                                 */
    float axis_n[3];          /* the shape row's normal, the same bits                                 */
    float axis_m[3];          /* axis_n x axis_l                                                       */
    float axis_l[3];          /* the shape row's axis, the same bits                                   */
    float lo[3], hi[3];       /* extent of the points along n, m, l, relative to the CENTROID          */
    float half[3];            /* half extents along n, m, l; half[0] is half the region's thickness    */
    float mean_abs_residual;  /* mean |distance to the plane|, metres                                  */
} f3ds_region_box;
typedef struct f3ds_region_boxes_result { uint32_t n_regions, n_nonempty; uint64_t n_labelled, n_clamped, n_inliers; } f3ds_region_boxes_result;
/* host arithmetic only, no device needed: the definition */
int f3ds_region_boxes_host(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, float plane_tol,
                           f3ds_region_box* rows, f3ds_region_shape* shapes /* may be NULL */, f3ds_region_boxes_result* result /* may be NULL */);
/* the same rows from the device: the kernels of f3ds_region_shapes, a frame per region and a second read of the image and the labels in those frames,
 * recorded back to back with ONE wait (csrc/f3ds_boxes.inc).  inputs_on_device: depth and labels are device memory and read where they are; host inputs go
 * through the device's copy stream like those of f3ds_region_table.  rows_on_device covers both outputs: rows, and shapes unless it is NULL, are device
 * memory; host rows arrive with the call's one download.  Synchronous.  Runs on ctx's stream and uses scratch of its own only: every other call on the
 * context behaves as if this one never happened.  Also F3DS_ERR_ARG for a NULL ctx.  result may be NULL. */
int f3ds_region_boxes(f3ds_ctx* ctx, const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, float plane_tol,
                      int inputs_on_device, f3ds_region_box* rows, f3ds_region_shape* shapes /* may be NULL */, int rows_on_device,
                      f3ds_region_boxes_result* result);

/* ---- region components: split the regions of a label image into their connected parts -----------------------------------------
 * A region of the segmenter is merged in space, so in the image one label regularly covers disjoint pieces: a table top left and right of the object
 * on it, a wall behind a chair, speckles around depth holes.  The table, the contacts, the shapes and the tracker describe region i as one thing; run
 * on the image this function writes -- with n_regions = n_components -- they describe each piece.  The output is a label image again, and one row per
 * component says which region it came from.  The definition, bit for bit (csrc/f3ds_components.h):
 *   point      the family's: pixel p = v * width + u gets z by the rule of f3ds_deproject; it is LABELLED iff its depth is valid and
 *              label[p] != F3DS_NO_LABEL.  The colour fields of the format are not looked at.
 *   pairs      the contacts': p with p + 1 when u + 1 < width, with p + width when v + 1 < height.  4-connectivity, no diagonals.
 *   link       a pair is a LINK iff both pixels are labelled, their labels are equal, and the pair is CLOSE by the contacts' rule: g = fabsf(za - zb),
 *              zn = za < zb ? za : zb, g <= depth_tol * zn (one rounded f32 subtraction, one rounded f32 product, false on NaN).  depth_tol = +inf
 *              links every equal-label pair of finite depths; depth_tol = 0 links equal depths only.
 *   component  a class of the labelled pixels under the transitive closure of the links.  Its root is its smallest pixel index, its size its pixel count.
 *   kept       a component is kept iff its size is at least max(min_pixels, 1).
 *   numbering  kept components are numbered 0, 1, ... by ascending root: raster order of the first pixel.  comp_labels[p] = the number of p's component
 *              if p is labelled and the component is kept, else F3DS_NO_LABEL (also for a label over an invalid depth).  Row k describes component k.
 *   result     n_components kept and n_dropped dropped components; n_labelled labelled pixels, n_kept of them in kept components; reserved = 0.
 *   capacity   the contacts': *n_out receives n_components on F3DS_OK and on F3DS_ERR_CAPACITY.  rows == NULL: no rows, cap is ignored.  cap smaller
 *              than the count: F3DS_ERR_CAPACITY; the image and the result are written and no row is.
 * Everything is a class of an equivalence relation, a minimum or an integer count: the result does not depend on the order of evaluation, and the
 * device gives the bits of the host function.
 * Errors (both functions alike): F3DS_ERR_ARG for a NULL fmt, depth, labels, comp_labels or n_out, for comp_labels == labels, for what f3ds_deproject
 * refuses of a format (the two colour fields are neutralised as in f3ds_region_contacts), for a depth_tol that is negative or NaN, and for a label
 * >= n_regions other than F3DS_NO_LABEL on any pixel (the device function finds it on the device and reports it at the call's one wait); then nothing is
 * written: no image, no row, no n_out, no result.  F3DS_ERR_UNSUPPORTED for n_regions > 0x00FFFFFF.  n_regions == 0 with every label F3DS_NO_LABEL, a
 * 1 x 1 image and a frame without a labelled pixel are F3DS_OK with zero components. */
typedef struct f3ds_component_params { float depth_tol; uint32_t min_pixels; } f3ds_component_params;   /* defaults 0.05f, 1 */
typedef struct f3ds_region_component {      /* 12 bytes */
    uint32_t region;        /* the input label of the component's pixels          */
    uint32_t first_pixel;   /* its smallest pixel index                            */
    uint32_t n_pixels;      /* its labelled pixels                                 */
} f3ds_region_component;
typedef struct f3ds_region_components_result {
    uint32_t n_regions, n_components, n_dropped, reserved;   /* kept / dropped components; reserved = 0 */
    uint64_t n_labelled, n_kept;                              /* labelled pixels; those in kept components */
} f3ds_region_components_result;
void f3ds_default_component_params(f3ds_component_params* params);
/* host arithmetic only, no device needed: the definition (a raster scan that flood-fills from every labelled pixel not yet reached).  params == NULL:
 * the defaults.  comp_labels: width * height words. */
int f3ds_region_components_host(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions,
                                const f3ds_component_params* params, uint32_t* comp_labels, f3ds_region_component* rows, size_t cap, size_t* n_out,
                                f3ds_region_components_result* result /* may be NULL */);
/* the same image and rows from the device (csrc/f3ds_components.inc: a tiled union-find).  inputs_on_device: depth and labels are device memory and read
 * where they are; host inputs go through the device's copy stream like those of f3ds_region_table.  outputs_on_device: comp_labels and rows (cap rows of
 * it) are device memory; host outputs arrive with the call's one download (a second one only for more than 2048 rows).  Synchronous.  Runs on ctx's
 * stream and uses scratch of its own (and the scan's tile sums, which hold nothing between calls): every other call on the context behaves as if this
 * one never happened.  Also F3DS_ERR_ARG for a NULL ctx. */
int f3ds_region_components(f3ds_ctx* ctx, const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions,
                           const f3ds_component_params* params, int inputs_on_device, uint32_t* comp_labels, f3ds_region_component* rows, size_t cap,
                           int outputs_on_device, size_t* n_out, f3ds_region_components_result* result);
/* development: the device's algorithm (tiles, seams, flatten, numbering: the step functions of csrc/f3ds_components.h) run sequentially on the host at a
 * tile size of tile_w x tile_h pixels (1 <= tile_w <= 64); the contract of f3ds_region_components_host.  No device needed. */
int f3ds_region_components_tiled(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions,
                                 const f3ds_component_params* params, uint32_t tile_w, uint32_t tile_h, uint32_t* comp_labels,
                                 f3ds_region_component* rows, size_t cap, size_t* n_out, f3ds_region_components_result* result);

/* ---- region joints: one fixed-size row per pair of touching regions: the border in space and the dihedral relation of the two planes -----
 * The sixth member of the family joins the contacts with the shapes: a contact row (a, b) and the two shape rows S_a, S_b become one row that says where
 * in space the border runs, which way, and whether the two planes meet in a convex edge, a concave corner, lie in one plane, or merely hide one another.
 * labels, n_regions and the region ids are the region table's.  The definition, bit for bit (csrc/f3ds_joints.h):
 *   point, pairs, contact, close   the contacts', word for word.  The rows are the rows of f3ds_region_contacts at the same depth_tol: the pairs (a, b),
 *              their order and count, n_pairs and n_close are the same bits, and so are *n_out and the result's n_joints (the contacts' n_contacts),
 *              n_pairs and n_close.  n_surface = the number of rows with n_close > 0.
 *   samples    every CLOSE pair contributes both of its pixels' points (x, y, z by the rule of f3ds_deproject) as two samples of (a, b); a pixel in
 *              two close pairs of the same (a, b) counts twice.  The samples' moments are the shapes': every coordinate through the table's fix, then
 *              n, S_a and M_ab as exact integer sums.  The finish of the shapes on these moments gives centroid (its centroid), direction (its axis) and
 *              spread (its eigenvalue); nothing else of that shape row is looked at.  A frame has at most 4 * width * height samples and the shapes'
 *              finish wants n < 2^31: width * height > 0x1FFFFFFF is F3DS_ERR_UNSUPPORTED, after the family's checks.
 *   regions    S_a, S_b = the rows f3ds_region_shapes defines for a and b (both non-empty: each has a labelled pixel in a contact).  Only their public
 *              floats are used: c = centroid, n = normal, d = plane_d.  Every operation below is one rounded f32 operation, nothing fused, in this order:
 *                cos_angle = (n_a.x * n_b.x + n_a.y * n_b.y) + n_a.z * n_b.z
 *                h_ab = ((n_a.x * c_b.x + n_a.y * c_b.y) + n_a.z * c_b.z) + d_a;  h_ba likewise with a and b swapped
 *                e_a, e_b: the same form with the border centroid (the row's `centroid`) in place of the other region's centroid
 *                delta_g = the reference's normals_diff (src/clustering.cpp:53-96) on (n_a, c_a, n_b, c_b); F3DS_JOINT_REF_CONVEX iff its is_convex
 *              Every float of the row is canonicalised as in the boxes (t != t ? 0x7FC00000 : bits).  Two identical centroids give a NaN delta_g and no flag.
 *   kind       n_close == 0: F3DS_JOINT_OCCLUSION; centroid, direction, spread, e_a and e_b are the quiet NaN 0x7FC00000, the other fields as above.
 *              Otherwise F3DS_JOINT_COPLANAR iff cos_angle >= cos_coplanar && fabsf(h_ab) <= plane_tol && fabsf(h_ba) <= plane_tol (comparisons fail on
 *              NaN); otherwise F3DS_JOINT_CONVEX iff h_ab + h_ba < 0 (one f32 add); otherwise F3DS_JOINT_CONCAVE.  Normals face the camera, so the far
 *              face of a box edge lies below the near face's plane (convex) and a wall stands above the floor's plane (concave).
 *   shapes     a non-NULL `shapes` receives the n_regions rows of f3ds_region_shapes, the same bits, as in f3ds_region_boxes.
 *   capacity   the contacts': *n_out receives the row count on F3DS_OK and on F3DS_ERR_CAPACITY.  rows == NULL: count only, cap is ignored.  cap smaller
 *              than the count: F3DS_ERR_CAPACITY, no row is written; shapes and result are.
 * A region of one point or of points on a line has a plane that is defined but MEANINGLESS, as in the shapes: look at eigenvalue[1] of S_a and S_b before
 * believing kind, cos_angle or the h and e fields, and at spread[2] before believing direction (a border of one close pair has two samples).
 * Everything that meets more than one pixel is an integer sum or a count, and the finish is one function for host and device: the device gives the bits
 * of the host function under any schedule.  Not built: samples of occlusion borders, 8-connected pairs, joints of clouds without an image grid.
 * Errors (both functions alike): the contacts' (a NULL fmt, depth, labels or n_out, a refused format, a depth_tol that is negative or not finite:
 * F3DS_ERR_ARG), F3DS_ERR_ARG for a plane_tol that is negative or NaN and for a cos_coplanar that is NaN or outside [-1, 1], then F3DS_ERR_UNSUPPORTED for
 * n_regions > 0x00FFFFFF or width * height > 0x1FFFFFFF, then F3DS_ERR_ARG for a label >= n_regions other than F3DS_NO_LABEL (the device function finds
 * it on the device and reports it at the call's one wait).  params == NULL: the defaults.  After an error nothing is written: no row, no shape row, no
 * n_out, no result. */
enum { F3DS_JOINT_OCCLUSION = 0, F3DS_JOINT_COPLANAR = 1, F3DS_JOINT_CONVEX = 2, F3DS_JOINT_CONCAVE = 3 };
#define F3DS_JOINT_REF_CONVEX 0x100u   /* flag in `kind`: the reference's is_convex on the two regions */
typedef struct f3ds_joint_params { float depth_tol, plane_tol, cos_coplanar; } f3ds_joint_params;   /* defaults 0.05f, 0.01f, 0.9659258f (15 degrees) */
typedef struct f3ds_region_joint {      /* 80 bytes, 20 words */
    uint32_t a, b;            /* region ids, a < b: the contact row's                                   */
    uint32_t n_pairs, n_close;/* the bits of f3ds_region_contacts at the same depth_tol                 */
    float centroid[3];        /* of the border samples                                                  */
    float direction[3];       /* the direction the border runs in (the shapes' `axis` rule)             */
    float spread[3];          /* eigenvalues of the samples' covariance, ascending                      */
    float cos_angle;          /* n_a . n_b                                                              */
    float delta_g;            /* the reference's normals_diff on the two regions                        */
    float h_ab, h_ba;         /* signed distance of b's centroid from a's plane, and of a's from b's    */
    float e_a, e_b;           /* signed distance of the border centroid from a's and from b's plane     */
    uint32_t kind;            /* F3DS_JOINT_* | F3DS_JOINT_REF_CONVEX                                   */
} f3ds_region_joint;
typedef struct f3ds_region_joints_result { uint32_t n_regions, n_joints, n_surface, reserved; uint64_t n_pairs, n_close; } f3ds_region_joints_result;
void f3ds_default_joint_params(f3ds_joint_params* params);
/* host arithmetic only, no device needed: the definition.  shapes: n_regions rows or NULL */
int f3ds_region_joints_host(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, const f3ds_joint_params* params,
                            f3ds_region_joint* rows, size_t cap, size_t* n_out, f3ds_region_shape* shapes /* may be NULL */,
                            f3ds_region_joints_result* result /* may be NULL */);
/* the same rows from the device: the kernels of f3ds_region_shapes, one pass over the borders, the sort of its records and one finish per row, recorded
 * back to back with ONE wait (csrc/f3ds_joints.inc).  inputs_on_device: depth and labels are device memory and read where they are; host inputs go
 * through the device's copy stream like those of f3ds_region_table.  rows_on_device covers both outputs: rows (cap rows of it), and shapes unless it is
 * NULL, are device memory; host rows arrive with the call's one download (a second one only for more than 2048 rows).  Synchronous.  Runs on ctx's stream
 * and uses scratch of its own (and the sort's histogram and scan buffers, which hold nothing between calls): every other call on the context behaves as
 * if this one never happened.  Also F3DS_ERR_ARG for a NULL ctx.  result may be NULL.  A frame with more than 32768 border records runs once more with
 * room for all (the same bits). */
int f3ds_region_joints(f3ds_ctx* ctx, const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions,
                       const f3ds_joint_params* params, int inputs_on_device, f3ds_region_joint* rows, size_t cap,
                       f3ds_region_shape* shapes /* may be NULL */, int rows_on_device, size_t* n_out, f3ds_region_joints_result* result);
/* the batch form, by the rules of the batch forms below (rows as the contacts': NULL or a NULL entry counts only, caps beside rows; shapes as the boxes':
 * for every frame or for none; status[i] may be F3DS_ERR_CAPACITY: n_out[i], results[i] and shapes[i] are written, no row is) */
int f3ds_region_joints_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth, const uint32_t* const* labels,
                             const uint32_t* n_regions, const f3ds_joint_params* params, int inputs_on_device,
                             f3ds_region_joint* const* rows /* NULL: counts only */, const size_t* caps /* nctx */,
                             f3ds_region_shape* const* shapes /* NULL: none; else every entry non-NULL */, int rows_on_device, size_t* n_out /* nctx */,
                             f3ds_region_joints_result* results, int* status);

/* ---- batch forms of the five region calls: nctx frames of ONE format, one dispatch per kernel, one wait --------------------------
 * Shaped like f3ds_segment_rgbd_batch: one context per frame (all on one device, none twice), one f3ds_rgbd_format for the batch, arrays of nctx per-frame
 * pointers and counts.  Nothing new is defined numerically:
 *   frame i    every output of frame i (rows[i], shapes[i], comp_labels[i], n_out[i], results[i]) holds the bits the lone call on ctxs[i] with frame i's
 *              arguments writes, which are the bits of the f3ds_*_host definition.
 *   refusals   of the call as a whole; nothing is written then, `status` included: F3DS_ERR_ARG for NULL ctxs, nctx < 1, a NULL or repeated context or contexts
 *              on different devices; F3DS_ERR_ARG for a NULL pointer array the call needs (depth, labels, n_regions; rows of the table, shapes and boxes;
 *              comp_labels; n_out; caps beside rows); then whatever the lone call refuses before it looks at a pixel, frame by frame in order -- the first
 *              refusing frame's code is returned.  `color` (table) and `shapes` (boxes) are for every frame or for none: a NULL array means none, and a NULL
 *              entry of a non-NULL array is F3DS_ERR_ARG (a NULL shapes[i] is allowed where n_regions[i] is 0).  rows[i] may be NULL where the lone call
 *              allows it (n_regions[i] == 0; contacts and components: that frame is only counted).
 *   status     status[i] (status may be NULL) = what the lone call returns once it has looked at pixels: F3DS_OK, F3DS_ERR_ARG for a label >= n_regions[i]
 *              other than F3DS_NO_LABEL (nothing of frame i is written), F3DS_ERR_CAPACITY for contacts and components (n_out[i] and results[i] are
 *              written, no row is; the image of the components is).  A failing frame does not disturb the others.  The call returns F3DS_OK if every frame
 *              is, else the status of the lowest failing frame.  A HIP failure fails the whole call.
 *   contexts   every context's state is as if the call never happened, as for the lone calls.  The call runs on ctxs[0]'s stream (a context with another
 *              stream is waited for first) and is synchronous: the uploads of host inputs are queued together and awaited once, everything that comes down
 *              comes in ONE download -- with device outputs the nctx heads of 32 bytes alone -- and the call waits once.  Frames beyond the ordinary case cost
 *              further downloads: host row arrays of contacts / components longer than 2048 rows, and a contacts frame with more than 32768 contact
 *              records, which runs once more on its own after the batch (the same bits).
 * Each lone call is its batch form with nctx = 1. */
int f3ds_region_table_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth,
                            const void* const* color /* NULL: no colour image for any frame; else every entry non-NULL */, const uint32_t* const* labels,
                            const uint32_t* n_regions /* nctx */, int inputs_on_device, f3ds_region_row* const* rows, int rows_on_device,
                            f3ds_region_table_result* results /* nctx, may be NULL */, int* status /* nctx, may be NULL */);
int f3ds_region_shapes_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth, const uint32_t* const* labels,
                             const uint32_t* n_regions, int inputs_on_device, f3ds_region_shape* const* rows, int rows_on_device,
                             f3ds_region_shapes_result* results, int* status);
int f3ds_region_boxes_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth, const uint32_t* const* labels,
                            const uint32_t* n_regions, float plane_tol, int inputs_on_device, f3ds_region_box* const* rows,
                            f3ds_region_shape* const* shapes /* NULL: none; else every entry non-NULL */, int rows_on_device,
                            f3ds_region_boxes_result* results, int* status);
int f3ds_region_contacts_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth, const uint32_t* const* labels,
                               const uint32_t* n_regions, float depth_tol, int inputs_on_device, f3ds_region_contact* const* rows /* NULL: counts only */,
                               const size_t* caps /* nctx */, int rows_on_device, size_t* n_out /* nctx */, f3ds_region_contacts_result* results, int* status);
int f3ds_region_components_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth, const uint32_t* const* labels,
                                 const uint32_t* n_regions, const f3ds_component_params* params, int inputs_on_device, uint32_t* const* comp_labels,
                                 f3ds_region_component* const* rows /* NULL: no rows */, const size_t* caps /* nctx */, int outputs_on_device,
                                 size_t* n_out /* nctx */, f3ds_region_components_result* results, int* status);

/* ---- region rows of a point cloud: what the table, the shapes and the boxes say of a region, for labels WITHOUT an image grid -----
 * The segmenter's first input is a cloud (f3ds_segment, the fused scenes, a lidar sweep); the region family above needs a depth image.  This call describes
 * the regions of n labelled RECORDS: points16 is what f3ds_segment takes, n records {float x, y, z; uint32 rgba}; labels is one u32 per record, < n_regions
 * or F3DS_NO_LABEL -- what f3ds_segment wrote, a level of f3ds_labels_at_thresholds, track ids, any relabelling.  Row i is region i.  Nothing is defined
 * numerically anew; the definition, bit for bit (csrc/f3ds_cloud.h):
 *   point      with params->fold_negative_z != 0 a z below 0 is replaced by fabsf(z): the segmenter's prelude rule (f3ds_params.fold_negative_z, main()'s
 *              z < 0 -> |z|, which f3ds_segment applies to every point it reads).  Point i is LABELLED iff x, y and z are all finite after the fold and
 *              labels[i] != F3DS_NO_LABEL.  A label over a non-finite point contributes nothing.  Only labelled points contribute.
 *   fixed      the table's, word for word: fix(a) = (int64)rint(clamp((double)a, -32768, 32768) * 65536), units of 2^-16 m clamped to +-32768; a labelled
 *              point is CLAMPED iff the clamp changed one of its coordinates.
 *   order      minima and maxima of floats in the total order of key(bits) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): -0 below +0.
 *   row        n_points, first_point (the smallest index i of a labelled point of the region), lo, hi, centroid and mean_rgb follow the rules that
 *              f3ds_region_row gives n_pixels, first_pixel, lo, hi, centroid and mean_rgb, with "point i" read for "pixel p" (mean_rgb: r = bits 16-23,
 *              g = bits 8-15, b = bits 0-7 of the colour word).  cov, eigenvalue, normal, axis, plane_d and curvature are those of f3ds_region_shape on the
 *              same moments (n, S_a, M_ab as exact integers, the 128-bit scatter, the eight Jacobi sweeps): one call of the shapes' finish.
 *              "Towards the camera" remains "towards the origin": normal . centroid <= 0.  For a fused cloud the origin is a convention of whoever fused
 *              it, not a viewpoint; (normal, plane_d) is the same plane either way.
 *   empty      a region without a labelled point has n_points = 0, first_point = 0xFFFFFFFF, lo = +inf, hi = -inf, the quiet NaN 0x7FC00000 in every other
 *              float, reserved = 0.
 *   boxes      optional (NULL: none): n_regions rows of the existing f3ds_region_box, by the definition of f3ds_region_boxes with "pixel" read as "point"
 *              and S_i taken as the shape fields of cloud row i -- the frame from the public floats (c = centroid, n = normal, l = axis, m = n x l), q
 *              from the fixed coordinates, t, lo / hi / half, inliers at params->plane_tol, mean_abs_residual.  A second pass over the points, which
 *              depends on the finish of the first.
 *   result     n_nonempty regions with a labelled point, n_labelled and n_clamped points, n_inliers the sum of the boxes' n_inliers (0 without boxes).
 * Everything that meets more than one point is a count, a minimum, a maximum or a sum of integers: the result does not depend on the order of the points
 * (first_point apart, which names an index) nor on the order of evaluation, and the device gives the bits of the host function.
 * Errors (host and device alike, in this order): F3DS_ERR_ARG for a NULL labels, for a NULL points16 with n > 0 (the device form excepted, below), for NULL
 * rows unless n_regions == 0, and for a plane_tol that is negative or NaN (+inf is a tolerance; it is checked without boxes too); F3DS_ERR_UNSUPPORTED for
 * n_regions > 0x00FFFFFF or n > 0x7FFFFFFF; F3DS_ERR_ARG for a label >= n_regions other than F3DS_NO_LABEL on any point, a non-finite one included (the
 * device function finds it on the device and reports it at the call's one wait).  After an error nothing is written.  n == 0, or no labelled point, is
 * F3DS_OK with all rows empty.  params may be NULL: the defaults.  Joints, contacts, components and the tracker of clouds are not built. */
typedef struct f3ds_cloud_params {
    float plane_tol;            /* the boxes' inlier distance, metres; default 0.01         */
    int32_t fold_negative_z;    /* f3ds_params.fold_negative_z; default 0                   */
} f3ds_cloud_params;
void f3ds_default_cloud_params(f3ds_cloud_params* p);
typedef struct f3ds_cloud_region {      /* 128 bytes, 32 words */
    uint32_t n_points;        /* labelled points of the region                                           */
    uint32_t first_point;     /* the smallest index of one of them; 0xFFFFFFFF if there is none          */
    float lo[3], hi[3];       /* box of the points, the cloud's axes                                     */
    float centroid[3];
    float mean_rgb[3];        /* 0 ... 255                                                               */
    float cov[6];             /* xx, xy, xz, yy, yz, zz, square metres                                   */
    float eigenvalue[3];      /* ascending                                                               */
    float normal[3];          /* eigenvector of eigenvalue[0], turned towards the origin                 */
    float axis[3];            /* eigenvector of eigenvalue[2], largest component non-negative            */
    float plane_d;            /* normal . x + plane_d = 0 through the centroid                           */
    float curvature;          /* eigenvalue[0] / (sum of the three), 0 if the sum is 0                   */
    uint32_t reserved;        /* 0                                                                       */
} f3ds_cloud_region;
typedef struct f3ds_cloud_regions_result { uint32_t n_regions, n_nonempty; uint64_t n_labelled, n_clamped, n_inliers; } f3ds_cloud_regions_result;
/* host arithmetic only, no device needed: the definition */
int f3ds_cloud_regions_host(const void* points16, size_t n, const uint32_t* labels, uint32_t n_regions, const f3ds_cloud_params* params /* may be NULL */,
                            f3ds_cloud_region* rows, f3ds_region_box* boxes /* may be NULL */, f3ds_cloud_regions_result* result /* may be NULL */);
/* the same rows from the device (csrc/f3ds_cloud.inc).  inputs_on_device: points16 and labels are device memory and read where they are; host inputs go
 * through the device's copy stream like those of f3ds_region_table.  points16 == NULL means the records the context's last segment call ran on, by the
 * rule of f3ds_get_points: F3DS_ERR_LOGIC when the context does not own them (the caller's device buffer), F3DS_ERR_ARG if n differs from their count
 * -- an rgbd frame, or a frame segmented from host points, is described without a second upload (labels are then host or device memory as
 * inputs_on_device says).  These two come after the refusals above.  rows_on_device covers rows and boxes; host rows arrive with the call's one download.
 * Synchronous.  Runs on ctx's stream and uses scratch of its own only: every other call on the context behaves as if this one never happened.  The box pass
 * is recorded back to back with the first: the call waits once.  The points are walked in input order when n_regions <= 96 and in the order of
 * (label, index) -- a radix sort first -- beyond; the bits are the same (F3DS_DBG_CLOUD_PATH tells which).  Also F3DS_ERR_ARG for a NULL ctx. */
int f3ds_cloud_regions(f3ds_ctx* ctx, const void* points16, size_t n, const uint32_t* labels, uint32_t n_regions, const f3ds_cloud_params* params,
                       int inputs_on_device, f3ds_cloud_region* rows, f3ds_region_box* boxes /* may be NULL */, int rows_on_device,
                       f3ds_cloud_regions_result* result /* may be NULL */);
/* nctx frames at once, by the rules of the batch forms of the region calls above (whole-call refusals, per-frame status, one dispatch per kernel with
 * grid.y = frame, one download, one wait), with one difference: every frame has its own point count counts[i], and a frame with counts[i] == 0 is legal.
 * Also refused as a whole: NULL points, counts, labels, n_regions or rows arrays.  points[i] may be NULL as in the lone call. */
int f3ds_cloud_regions_batch(f3ds_ctx** ctxs, int nctx, const void* const* points, const size_t* counts, const uint32_t* const* labels,
                             const uint32_t* n_regions, const f3ds_cloud_params* params, int inputs_on_device, f3ds_cloud_region* const* rows,
                             f3ds_region_box* const* boxes /* NULL: none; else every entry non-NULL */, int rows_on_device,
                             f3ds_cloud_regions_result* results, int* status);

/* Clustering::cluster(threshold) again on the supervoxels of the last f3ds_segment call, with
 * possibly different metric / merging settings (src/clustering.cpp:670-679).  Only the merge
 * fields of `params` are read. */
int f3ds_recluster(f3ds_ctx* ctx, const f3ds_params* params, uint32_t* point_labels,
                   int labels_on_device, f3ds_result* result);

/* Clustering::get_labeled_cloud / get_colored_cloud of the last call: one record per owned
 * voxel, regions in ascending label order, voxels in leaf order inside each supervoxel,
 * supervoxels in merge-concatenation order (src/clustering.cpp:640-663, 793-812).
 * Any of xyz / label / rgba may be NULL.  rgba = Glasbey[label % 256]. */
int f3ds_get_voxel_cloud(f3ds_ctx* ctx, float* xyz, uint32_t* label, uint32_t* rgba, size_t cap,
                         size_t* n_out);

/* parity hooks: copy an intermediate array of the last call to host memory */
enum {
    F3DS_DBG_GRID = 0,            /* 5 x f64: min_x, min_y, min_z, resolution, depth            */
    F3DS_DBG_VOXEL_KEYS = 1,      /* V x 3 u32, leaf order                                      */
    F3DS_DBG_VOXEL_COUNT = 2,     /* V u32 points per voxel                                     */
    F3DS_DBG_VOXEL_XYZ = 3,       /* V x 3 f32 centroid                                         */
    F3DS_DBG_VOXEL_RGB = 4,       /* V x 3 f32 mean colour                                      */
    F3DS_DBG_VOXEL_NORMAL = 5,    /* V x 4 f32 (w = 0)                                          */
    F3DS_DBG_VOXEL_NEIGHBORS = 6, /* V x 27 i32, slot = (dx+1)*9+(dy+1)*3+(dz+1), -1 = none     */
    F3DS_DBG_POINT_VOXEL = 7,     /* N i32 voxel of each input point, -1 = non-finite           */
    F3DS_DBG_SEED_ORIG = 8,       /* n_seed_cells i32: nearest voxel per occupied seed cell     */
    F3DS_DBG_SEED_KEPT = 9,       /* n_seeds i32: voxels that became helpers (label = index+1)  */
    F3DS_DBG_VOXEL_SVLABEL = 10,  /* V u32 supervoxel label after the sweeps, 0 = none          */
    F3DS_DBG_VOXEL_DIST = 11,     /* V f32 VoxelData::distance_ after the sweeps                */
    F3DS_DBG_SV_LABELS = 12,      /* S u32 labels of non-empty supervoxels, ascending           */
    F3DS_DBG_SV_CENTROID = 13,    /* S x 10 f32: xyz, rgb, normal4 of each (same order)         */
    F3DS_DBG_EDGES = 14,          /* E x 2 u32 (a<b), sorted                                    */
    F3DS_DBG_EDGE_DELTAS = 15,    /* E x 2 f32 (delta_c, delta_g)                               */
    F3DS_DBG_EDGE_WEIGHTS = 16,   /* E f32 initial weights                                      */
    F3DS_DBG_MERGES = 17,         /* n_merges x 3 u32: a, b, weight bits                        */
    F3DS_DBG_VOXEL_REGION = 18,   /* V u32 final region id per voxel (F3DS_NO_LABEL = none)     */
    F3DS_DBG_SV_REGION = 19,      /* S u32 surviving label each supervoxel ended in             */
    F3DS_DBG_TILE_LIST_LEN = 21,  /* ceil(V / 128) u32: length of each 128-voxel tile's one-ring list (the LDS tiles of the normals and
                                     the sweeps); 0xFFFFFFFF = the tile did not fit the tables and took the global-memory path.  Diagnostics */
    F3DS_DBG_SWEEP_STATS = 22,    /* 4 u32: label-propagation sweeps of the last run that evaluated every voxel from their start / only the tiles marked
                                     dirty (incremental R rounds) / started incremental and fell back to the chain walker because the last R round
                                     still changed a word / were skipped because the sweep before them had changed nothing (a fixed point: the
                                     remaining iterations of expandSupervoxels are no-ops).  Diagnostics and tests (all kinds end in the same bits) */
    F3DS_DBG_STAGE0_PATH = 23,    /* 1 u32: how the last frame was voxelised -- 1 = the tile path (the points stay where they are, only per-tile voxel
                                     descriptors are sorted: frames of a batch), 0 = the sort path (every point's key through a radix sort: lone frames,
                                     unorganised clouds, very dense voxels).  Diagnostics and tests: the two paths give the same bits              */
    F3DS_DBG_LAUNCH_SHAPE = 24,   /* 3 u32: the launch widths of the last call that ran kernels for this context -- workgroups per frame that a
                                     streaming kernel gets at most (its share of the batch's budget), that a gathering kernel gets at most (2048), and
                                     the frames of that call.  Diagnostics and tests: the development switch F3DS_GRID_CAP sets both widths, and
                                     results do not depend on them                                                                                   */
    F3DS_DBG_MERGE_LAYOUT = 20    /* 2 u32: which merge kernel the last cluster stage ran -- waves per frame (4, 8; 0 = d_merge,
                                     everything in global memory) and where it kept the per-edge arrays (2 = order keys + endpoints in
                                     LDS, 0 = in global memory).  Diagnostics (bench.py names the kernel it timed): results do not depend on it */
};
/* One more selector, outside the enum of the segment path's hooks because it describes a call of the region family and needs no frame: 1 u32, how the
 * last f3ds_cloud_regions[_batch] call that ran kernels for this context walked its points -- 1 = direct (input order), 2 = ordered (sorted by label
 * first), 0 = no such call yet.  Diagnostics and tests: the development switch F3DS_CLOUD_PATH=direct|ordered forces one, and the two give the same bits. */
#define F3DS_DBG_CLOUD_PATH 25
int f3ds_get_debug(f3ds_ctx* ctx, int what, void* dst, size_t cap_bytes, size_t* bytes_out);
/* Diagnostics, host arithmetic only (no device needed): the LDS carve-up of the merge kernel d_merge_il_t<waves, keys_in_lds> for a frame with n_edges
 * adjacencies -- the same function the launch and the kernel use (csrc/f3ds_kernels.inc, merge_il_offsets).  out[0] = dynamic LDS bytes, out[1] = voxel rows the
 * speculative second merge of an epoch may absorb (128; 256, 512 or 1024 in the 8-wave layout where LDS has room), out[2] = edge slots, out[3] = 1 if the layout fits a
 * compute unit's LDS (else the cluster stage takes the next layout, at last d_merge).  waves: 4 or 8; keys_in_lds: 2 or 0.  Returns F3DS_ERR_ARG otherwise. */
int f3ds_merge_layout_info(uint32_t n_edges, int waves, int keys_in_lds, uint32_t out[4]);
/* The limits of the kernels and of the host's batch-wide decisions, by name (diagnostics and tests; host arithmetic only, no device needed).  Each value is the
 * constant the code itself uses: NT_RING1, VL_MAX_RUN, MC_TL_CAP, EDGE_MULT, WIDE_CAP, ...; a kernel's workgroup size is "<kernel>::BLOCK"; the reasons for a
 * rerun in F3DS_TRACE_ERR output are OVF_*; the three floating margins of the seed kernels (SEED_NN_MARGIN, SEED_NN_ULP, SEED_PRUNE_MARGIN) come as the bit
 * pattern of the double.  f3ds_constant returns F3DS_ERR_ARG for a name it does not know; f3ds_constant_name(i) is the i-th name, NULL behind the last. */
int f3ds_constant(const char* name, uint64_t* value);
const char* f3ds_constant_name(size_t index);
/* What stage 0 of a batch call does for fresh contexts whose live frames have at most max_depth octree levels (0 .. 21) and max_points points, n_contexts
 * contexts in the call, F3DS_VOX_TILES = vox_tiles (0, 1 = unset, 2) and F3DS_SORT_PAIRS = sort_pairs: out[0] = 1 the tile path / 0 the point sort, out[1] = bits of
 * a tile's number in a descriptor key, out[2] = bits of a point's index in a one-word sort key (-1: the sort moves (key, index) pairs), out[3] = bits of the
 * sort key without the index.  The function segment_batch calls (csrc/f3ds_batch_policy.h); host arithmetic only. */
int f3ds_stage0_plan(int max_depth, uint32_t max_points, int n_contexts, int vox_tiles, int sort_pairs, int32_t out[4]);
/* The other batch-wide decisions, the same way.  f3ds_policy_capacity: entries of a growing buffer -- F3DS_CAP_EDGES: the adjacency list of count seeds at
 * edge_mult = mult; F3DS_CAP_EVENTS: the weight history of count edges at ev_mult = mult; F3DS_CAP_LEAF_POOL: the leaf pool of count seeds at pool_mult = mult;
 * F3DS_CAP_ILIST: the incident-list pool of count edges and n_seeds seeds at ilist_mult = mult under F3DS_ILIST_SLACK = slack.  f3ds_policy_grow: a multiplier
 * after an overflow, given its cap.  f3ds_policy_dense_penalty: the calls a context stays off the tile path after its next refusal.  f3ds_policy_launch:
 * out[0] = threads of the normals kernel in a call of `frames` frames (normals_forced: F3DS_NORMALS_THREADS, 0 unset), out[1] = workgroups per frame of a
 * streaming kernel (grid_target: F3DS_GRID_TARGET; grid_cap_forced: F3DS_GRID_CAP, 0 unset), out[2] = of a gathering kernel. */
enum { F3DS_CAP_EDGES = 0, F3DS_CAP_EVENTS = 1, F3DS_CAP_LEAF_POOL = 2, F3DS_CAP_ILIST = 3 };
int f3ds_policy_capacity(int what, uint32_t count, uint32_t n_seeds, uint32_t mult, uint32_t slack, uint32_t* out);
int f3ds_policy_grow(uint32_t mult, uint32_t cap, uint32_t* out);
uint32_t f3ds_policy_dense_penalty(uint32_t penalty);
int f3ds_policy_launch(int frames, int normals_forced, uint32_t grid_target, uint32_t grid_cap_forced, uint32_t out[3]);
/* Where a batch form of the label-image family puts the outputs of its frames in the staging buffer it downloads (csrc/f3ds_label_image.h, li_stage_layout): frame i
 * has fixed_bytes[i] bytes of fixed size and, with stage_rows, stage_rows[i] rows of row_bytes bytes whose count the device decides.  slots[3 i ..] = (offset of the
 * fixed bytes, offset of the rows, rows the first download brings); *first_bytes = the length of that download; *total = the bytes in all. */
int f3ds_policy_stage_layout(size_t n_frames, const size_t* fixed_bytes, const size_t* stage_rows, size_t row_bytes, size_t first_rows, size_t* slots, size_t* first_bytes, size_t* total);

/* ---- the VCCS result itself: what main() reads back from pcl::SupervoxelClustering after extract()
 * (src/supervoxel_clustering.cpp:359-367).  All valid after f3ds_segment; call with NULL outputs for the count. */

/* getVoxelCentroidCloud (:359) + getLabeledVoxelCloud: one entry per voxel in leaf order: centroid, mean colour
 * as 0x00RRGGBB (VoxelData::getPoint truncation), supervoxel label (0 = none). */
int f3ds_get_voxel_centroid_cloud(f3ds_ctx* ctx, float* xyz, uint32_t* rgba, uint32_t* sv_label, size_t cap, size_t* n_out);

/* the supervoxel_clusters map + makeSupervoxelNormalCloud (:356,360): per non-empty supervoxel, ascending label:
 * label, centroid xyz, mean rgb (float), unit normal, number of voxels. */
int f3ds_get_supervoxels(f3ds_ctx* ctx, uint32_t* label, float* xyz, float* rgb, float* normal, uint32_t* n_voxels,
                         size_t cap, size_t* n_out);

/* getSupervoxelAdjacency (:365) after clear_adjacency: pairs (a < b) of adjacent supervoxel labels, sorted. */
int f3ds_get_supervoxel_adjacency(f3ds_ctx* ctx, uint32_t* pairs, size_t cap_pairs, size_t* n_out);

/* get_currentstate().second after cluster() (:444): adjacency of the merged regions as sorted pairs (a < b) of the surviving
 * supervoxel labels -- the graph visualize() draws between the centroids of supervoxel_clusters.at(label) (:636-672). */
int f3ds_get_region_adjacency(f3ds_ctx* ctx, uint32_t* pairs, size_t cap_pairs, size_t* n_out);

/* ---- the merge half on its own: Clustering on supervoxels the CALLER supplies ------------------------------------------
 * Clustering::set_initialstate(ClusteringT segm, AdjacencyMapT adj) takes "the output of some supervoxel algorithm"
 * (include/supervoxel_clustering/clustering.h:142, src/clustering.cpp:600-612; main() passes PCL's own supervoxel_clusters
 * and getSupervoxelAdjacency result, src/supervoxel_clustering.cpp:365,424).  This entry is that call + cluster(threshold)
 * (src/clustering.cpp:670-679) on plain arrays: a maintainer with PCL runs real PCL supervoxels through the GPU merge loop.
 *
 * One f3ds_supervoxel_set row per map entry (pcl::Supervoxel<PointXYZRGBA>): label = the map key (distinct, any u32, any
 * order: the ascending-key iteration of std::map is rebuilt here); voxels_ = voxel_xyz / voxel_rgba[voxel_offset[i] ..
 * voxel_offset[i+1]) in the cloud's own order (rgba packed as PCL does, a<<24|r<<16|g<<8|b; only r g b are read:
 * ColorUtilities::mean_color, src/color_utilities.cpp:117-142); centroid_ (x y z) and normal_ (normal_x/y/z).  Every
 * supervoxel must hold at least one voxel (PCL emits no empty ones).
 * adjacency_pairs = the multimap in ITERATION order, n_pairs (first, second) rows; rows with first > second are dropped
 * (clear_adjacency, :476-486), the rest become the initial weight-map entries in that order (adj2weight: all keys -1, so
 * insertion order; ties between equal weights later resolve in this order).  Rows are stably sorted by `first` in case the
 * caller did not iterate a multimap.  F3DS_ERR_OUT_OF_RANGE for an endpoint that is no row of the set (map::at throws
 * std::out_of_range, :228-229); F3DS_ERR_ARG for a pair listed twice or a self-adjacency (the reference dereferences an
 * erased supervoxel at the first merge that meets one).
 * Outputs (either may be NULL): region_of_sv[i] = label of the surviving supervoxel row i ended in (the key it has in
 * get_currentstate().first); voxel_labels[v] = get_labeled_cloud() id (0..K-1, regions in ascending key) of input voxel v.
 * Afterwards the context answers f3ds_recluster (other metric / threshold on the same supervoxels), f3ds_get_voxel_cloud,
 * f3ds_get_regions, f3ds_get_region_voxels, f3ds_get_region_adjacency, f3ds_get_supervoxel_adjacency and the merge-side
 * F3DS_DBG_* arrays (labels are the caller's); the VCCS-side accessors return F3DS_ERR_LOGIC. */
typedef struct f3ds_supervoxel_set {
    uint32_t n_supervoxels;
    const uint32_t* label;          /* n_supervoxels                                      */
    const uint32_t* voxel_offset;   /* n_supervoxels + 1, ascending, voxel_offset[0] = 0  */
    const float* voxel_xyz;         /* 3 per voxel                                        */
    const uint32_t* voxel_rgba;     /* 1 per voxel                                        */
    const float* centroid_xyz;      /* 3 per supervoxel                                   */
    const float* normal;            /* 3 per supervoxel                                   */
} f3ds_supervoxel_set;
int f3ds_cluster_supervoxels(f3ds_ctx* ctx, const f3ds_supervoxel_set* sv, const uint32_t* adjacency_pairs, size_t n_pairs,
                             const f3ds_params* params, uint32_t* region_of_sv, uint32_t* voxel_labels, f3ds_result* result);

/* get_currentstate().first after cluster() (src/clustering.cpp:619-624; read at src/supervoxel_clustering.cpp:443-449): the
 * merged regions in ascending key.  Per region: its key (label of the surviving supervoxel), number of voxels, centroid_
 * (computeCentroid of the concatenated voxels_, :412-414), normal_ (:416-425) and the mean colour mean_color() gives.  Any
 * output may be NULL.  Valid after f3ds_segment / f3ds_recluster / f3ds_cluster_supervoxels. */
int f3ds_get_regions(f3ds_ctx* ctx, uint32_t* label, uint32_t* n_voxels, float* centroid_xyz, float* normal, float* mean_rgb,
                     size_t cap, size_t* n_out);
/* the regions' voxels_ clouds, concatenated in the order of f3ds_get_regions (n_voxels[] splits them), each in the
 * concatenation order merge() builds (voxels_a ++ voxels_b, :408): position, colour (0x00RRGGBB, the voxel's own, not the
 * Glasbey colour of f3ds_get_voxel_cloud) and the voxel's index -- leaf ordinal after f3ds_segment (the row of
 * f3ds_get_voxel_centroid_cloud), input voxel index after f3ds_cluster_supervoxels -- with which the caller gathers any other
 * per-voxel attribute (Supervoxel::normals_, :409).  Any output may be NULL. */
int f3ds_get_region_voxels(f3ds_ctx* ctx, float* xyz, uint32_t* rgba, uint32_t* voxel_index, size_t cap, size_t* n_out);

/* ---- evaluation against ground truth and automatic threshold (the path run when -t is omitted) ----
 * Mirrors Testing::eval_performance (src/testing.cpp:239-406) and Clustering::all_thresh / best_thresh
 * (src/clustering.cpp:691-774) on the frame of the last f3ds_segment call.  truth_point_labels holds
 * one ground-truth label per input point (the PCD `label` field).  The truth cloud is built like
 * main() does (src/supervoxel_clustering.cpp:387-400): points coloured by label -> voxel mean colour ->
 * one truth label per distinct voxel colour, in first-appearance order. */
typedef struct f3ds_performance { float voi, precision, recall, fscore, wov, fpr, fnr; } f3ds_performance;

/* scores of the current segmentation (Testing(get_labeled_cloud(), truth).eval_performance()) */
int f3ds_evaluate(f3ds_ctx* ctx, const uint32_t* truth_point_labels, f3ds_performance* out);

/* all_thresh(start, end, step) + best_thresh: clusters at every threshold start, start+step, ... <= end
 * (float accumulation as in the reference), scores each, returns the best by F-score and leaves the
 * context clustered at that threshold (point_labels receives its labels; may be NULL).
 * thresholds / scores (capacity cap) receive the sweep; n_out its length. */
int f3ds_auto_threshold(f3ds_ctx* ctx, const f3ds_params* params, const uint32_t* truth_point_labels,
                        float start, float end, float step, float* thresholds, f3ds_performance* scores,
                        size_t cap, size_t* n_out, float* best_threshold, f3ds_performance* best_score,
                        uint32_t* point_labels, int labels_on_device, f3ds_result* result);

/* ---- hierarchy levels: the segmentation at many thresholds from ONE merge run -------------------------------------------
 * Clustering::cluster(state, t) merges the cheapest adjacency while its weight is below t (src/clustering.cpp:384-401); no merge
 * depends on t, so the run to t <= T is a prefix of the run to T (all_thresh relies on it, :691-728).  The "cluster run" of a
 * context is the latest of f3ds_segment, f3ds_segment_batch, f3ds_recluster and f3ds_cluster_supervoxels, at its threshold T.
 * Level l (threshold t_l, any order, repeats allowed, finite and <= T) applies the logged merges before the FIRST merge i whose
 * weight fails w_i < t_l (logged weights are not monotone: a count of weights below t_l is not the same); a t_l equal to a logged
 * weight stops at that merge.  Level l is bit-equal to f3ds_recluster with the run's params and threshold = t_l: the same labels
 * (F3DS_NO_LABEL included), region count and merge count.  The context's state does not change (regions, voxel cloud,
 * adjacency, F3DS_DBG_* arrays and a later f3ds_recluster behave as if the call never happened).
 * point_labels: k * n words, level-major (level l's n labels at point_labels + l * n); n = the frame's points, or its input
 * voxels after f3ds_cluster_supervoxels (like that call's voxel_labels).  labels_on_device: a device buffer written in place;
 * host buffers go through the device's copy stream like f3ds_segment_batch's labels (asynchronous when pinned) and are complete
 * when the call returns.  n_regions (k words, may be NULL): regions per level.  One merge-log pass, one prefix pass and one
 * label pass on the device (csrc/f3ds_levels.inc): K levels cost about one relabel, not K merge loops.
 * Errors: F3DS_ERR_ARG for a NULL pointer, k < 1 or a NaN / infinite threshold; F3DS_ERR_OUT_OF_RANGE for t_l > T;
 * F3DS_ERR_LOGIC before any cluster run (a frame without voxels included), as f3ds_recluster. */
int f3ds_labels_at_thresholds(f3ds_ctx* ctx, const float* thresholds, int k, uint32_t* point_labels, int labels_on_device,
                              uint32_t* n_regions /* k, may be NULL */);
/* the same for every context of a batch (one GPU, one dispatch per kernel for all frames, grid.y = frame): point_labels[i] belongs
 * to ctxs[i] (k * n_i words); n_regions (nctx * k words, context-major, may be NULL).  Every threshold must be <= each context's T. */
int f3ds_labels_at_thresholds_batch(f3ds_ctx** ctxs, int nctx, const float* thresholds, int k, uint32_t* const* point_labels,
                                    int labels_on_device, uint32_t* n_regions /* nctx * k, may be NULL */);
/* ---- scores of hierarchy levels: f3ds_evaluate for K thresholds of the last cluster run, on the device, from ONE merge log ----
 * Level l is the segmentation f3ds_labels_at_thresholds defines for t_l (the first logged merge i with !(w_i < t_l) stops the
 * prefix; any order, repeats allowed).  scores[l] are the scores of f3ds_recluster(threshold = t_l) followed by
 * f3ds_evaluate(truth): precision, recall, fscore, wov, fpr and fnr bit for bit; voi is computed with the library's own logf
 * (f3ds::m_logf, the same bits on every compiler) where f3ds_evaluate takes libm's, and differs from it by at most 1e-5.
 * n_regions[l] (may be NULL) is f3ds_labels_at_thresholds' region count.
 * Truth handling is f3ds_evaluate's: label colours Glasbey[label & 255] averaged per voxel, one truth label per distinct voxel
 * colour in first-appearance (leaf) order; N = the frame's voxels.  A ghost leaf adds to its segment's size always and to the
 * intersection only if that voxel is not already in that segment at that level.  truth_on_device: the labels are device memory.
 * No dense segment x label table is built at any level (csrc/f3ds_eval_levels.inc): scratch grows with the non-zero entries and
 * there is no limit on regions x labels as in f3ds_evaluate.  The context's state does not change (regions, voxel cloud,
 * adjacency, F3DS_DBG_* arrays and a later f3ds_evaluate, f3ds_recluster or f3ds_auto_threshold behave as if the call never
 * happened); only scratch of its own is written.
 * Errors, in this order: F3DS_ERR_ARG for a NULL pointer, k < 1, nctx < 1, a NaN threshold, contexts on different devices or a
 * context named twice; F3DS_ERR_LOGIC before any cluster run, for a frame without voxels or after f3ds_cluster_supervoxels (as
 * f3ds_evaluate); F3DS_ERR_OUT_OF_RANGE for t_l > T; F3DS_ERR_ARG for an infinite threshold.  F3DS_ERR_UNSUPPORTED for a frame of
 * 2^24 or more voxels (sizes are added as integers that a float must hold exactly). */
int f3ds_evaluate_levels(f3ds_ctx* ctx, const uint32_t* truth_point_labels, int truth_on_device, const float* thresholds, int k,
                         f3ds_performance* scores /* k */, uint32_t* n_regions /* k, may be NULL */);
/* the same for every context of a batch on one GPU: one dispatch per kernel for all frames and levels.  truth_point_labels[i]
 * holds ctxs[i]'s n_i labels; scores: nctx * k, context-major; n_regions likewise, may be NULL */
int f3ds_evaluate_levels_batch(f3ds_ctx** ctxs, int nctx, const uint32_t* const* truth_point_labels, int truth_on_device,
                               const float* thresholds, int k, f3ds_performance* scores, uint32_t* n_regions);
/* Clustering::best_thresh (src/clustering.cpp:759-774) over scored levels; host arithmetic only, no device needed.  The levels
 * are visited by ascending threshold (of equal thresholds the first given counts: std::map::insert), the first whose fscore is
 * strictly greater than the best so far -- starting from 0 -- is kept.  *best_index = -1 when no level has fscore > 0 (the
 * reference then returns threshold 0 and zero scores).  F3DS_ERR_ARG for a NULL pointer, k < 1 or a NaN threshold. */
int f3ds_best_level(const float* thresholds, const f3ds_performance* scores, int k, int* best_index);

/* the dendrogram: the merges of the last cluster run in the order performed -- survivor[i] took absorbed[i] at weight[i] -- as
 * supervoxel labels (the label space of f3ds_get_supervoxels / F3DS_DBG_SV_REGION; the caller's keys after
 * f3ds_cluster_supervoxels).  Any output may be NULL; n_out receives the merge count (F3DS_ERR_CAPACITY if cap is smaller). */
int f3ds_get_merge_tree(f3ds_ctx* ctx, uint32_t* survivor, uint32_t* absorbed, float* weight, size_t cap, size_t* n_out);

/* SupervoxelClustering::refineSupervoxels(num_itr, refined_supervoxel_clusters) (src/supervoxel_clustering.cpp:369-375) on
 * the supervoxels of the last f3ds_segment call: num_itr times { normals again from the owned two-ring, reseed every
 * supervoxel at the voxel nearest to its centroid, expand again }.  As in the reference, the refined supervoxels feed
 * nothing downstream (the clustering keeps the unrefined ones, :424): they live beside the frame's state and are read
 * with the two getters below; every other call keeps describing the unrefined supervoxels. */
int f3ds_refine_supervoxels(f3ds_ctx* ctx, int num_itr);
/* per voxel in leaf order (the order of f3ds_get_voxel_centroid_cloud): refined supervoxel label (0 = none) --
 * getLabeledVoxelCloud / the per-voxel view of refined_full_labeled_cloud (:375) -- and refined normal (3 floats) */
int f3ds_get_refined_voxels(f3ds_ctx* ctx, uint32_t* sv_label, float* normal, size_t cap, size_t* n_out);
/* refined_supervoxel_clusters / makeSupervoxelNormalCloud(refined) (:373-374): layout of f3ds_get_supervoxels */
int f3ds_get_refined_supervoxels(f3ds_ctx* ctx, uint32_t* label, float* xyz, float* rgb, float* normal, uint32_t* n_voxels,
                                 size_t cap, size_t* n_out);

/* ---- frame pipeline (row N4: the streaming surface the reference's ROS launch file points at,
 * launch/supervoxel_clustering.launch:3-6, README.md:72) ----------------------------------------
 * Frames go in from host memory one at a time and come out in submission order.  Up to `depth`
 * frames are in flight: each has a context and pinned staging for its points and labels, `groups`
 * host threads pick up whatever is queued -- one frame when the producer is slow (latency of a lone
 * frame), a run of consecutive frames with equal parameters as one f3ds_segment_batch when frames
 * arrive faster than they finish (throughput of the batched path) -- so H2D of one group overlaps
 * the kernels and the merge loop of the others.  Results per frame are those of f3ds_segment.
 * submit/next may be called from different threads (one producer, one consumer). */
typedef struct f3ds_stream f3ds_stream;
int f3ds_stream_create(int device, int depth, int groups, f3ds_stream** out);
void f3ds_stream_destroy(f3ds_stream* s);
/* pinned input buffer of the slot the next submit will use, sized for n points; filling it in place
 * (e.g. f3ds_pcd_read straight into it) saves submit's copy.  F3DS_ERR_BUSY when depth frames are in flight. */
int f3ds_stream_buffer(f3ds_stream* s, size_t n, void** points16);
/* queue a frame (host memory; copied unless it is the pointer f3ds_stream_buffer gave).  Never blocks:
 * F3DS_ERR_BUSY when depth frames are in flight -- take one with f3ds_stream_next first. */
int f3ds_stream_submit(f3ds_stream* s, const void* points, size_t n, const f3ds_params* params, uint64_t tag);
/* queue an RGB-D frame (host images, f3ds_rgbd_format above; both are copied into the slot's pinned staging, rows packed tightly).
 * Its width * height labels come out through f3ds_stream_next / f3ds_stream_peek like those of any frame, and point and rgbd
 * submissions may be mixed on one stream: consecutive frames share a batch call when they are of one kind and have equal
 * formats and parameters.  Results are those of f3ds_segment_rgbd.  Never blocks (F3DS_ERR_BUSY as above). */
int f3ds_stream_submit_rgbd(f3ds_stream* s, const f3ds_rgbd_format* fmt, const void* depth, const void* color,
                            const f3ds_params* params, uint64_t tag);
/* oldest frame not taken yet: its labels (n_out of them) into point_labels, its tag and result.  wait != 0 blocks
 * until it is done, else F3DS_ERR_BUSY while it is running; F3DS_ERR_EMPTY when nothing is in flight;
 * F3DS_ERR_CAPACITY (frame stays) when cap < its point count; n_out and tag are set in all three cases but EMPTY.
 * Otherwise the frame leaves the pipeline and the call returns the frame's own status. */
int f3ds_stream_next(f3ds_stream* s, uint32_t* point_labels, size_t cap, size_t* n_out, uint64_t* tag, f3ds_result* result, int wait);
/* the oldest frame's labels where they are (the slot's pinned buffer) instead of a copy: valid until the frame is
 * taken with f3ds_stream_next(s, NULL, 0, ...).  Same waiting rule and return values as f3ds_stream_next. */
int f3ds_stream_peek(f3ds_stream* s, const uint32_t** point_labels, size_t* n_out, uint64_t* tag, f3ds_result* result, int wait);
/* frames submitted and not taken */
int f3ds_stream_pending(f3ds_stream* s);

/* ---- multi-GPU batch driver, one process (BASELINE.json config 5: a batch of independent frames sharded over the
 * GPUs of a node, label output gathered on one GPU).  The reference has no counterpart (single-threaded CLI,
 * CMakeLists.txt:5).  Frame i runs on devices[i mod n_devices], one host thread per GPU; the per-point labels of all
 * frames then go to devices[0] in ONE grouped RCCL send/recv exchange (the ragged form of ncclGather, each peer over its
 * own xGMI link) and from there to the caller's host buffers.  librccl is loaded at run time; with one device no RCCL
 * call is made (unless F3DS_MULTI_FORCE_RCCL is set: development).  Results per frame are those of f3ds_segment.
 * F3DS_MULTI_LOGICAL=1 (tests on 1-GPU boxes): `devices` may name one GPU several times -- every entry is a device of its own
 * to the driver (worker thread, contexts, label blocks), the exchange a device-to-device copy in place of ncclSend / ncclRecv. */
typedef struct f3ds_multi f3ds_multi;
/* devices == NULL: devices 0..n_devices-1.  max_frames_per_device bounds one f3ds_multi_segment call. */
int f3ds_multi_create(const int* devices, int n_devices, int max_frames_per_device, f3ds_multi** out);
void f3ds_multi_destroy(f3ds_multi* m);
int f3ds_multi_devices(const f3ds_multi* m);
/* index into `devices` of the GPU frame `frame` of a call runs on */
int f3ds_multi_device_of_frame(const f3ds_multi* m, int frame);
/* points[i]: counts[i] records of 16 B in host memory; point_labels[i]: host buffer of counts[i] uint32 (may be NULL);
 * results may be NULL.  F3DS_ERR_CAPACITY when n_frames > n_devices * max_frames_per_device. */
int f3ds_multi_segment(f3ds_multi* m, const void* const* points, const size_t* counts, int n_frames, const f3ds_params* params,
                       uint32_t* const* point_labels, f3ds_result* results);
/* Pipelined form: f3ds_multi_submit queues a batch (same arguments; the pointer arrays are copied; the point buffers, the label
 * buffers AND the `results` array are written / read asynchronously by the driver's threads and must stay valid until the batch
 * is collected) and returns a ticket; the GPUs compute batch k+1 while batch k's labels are gathered on
 * devices[0] and copied to the host buffers.  At most two batches are in flight: F3DS_ERR_BUSY when the batch submitted two
 * calls ago has not been collected yet.  f3ds_multi_collect waits for a batch and returns its status (once per ticket).
 * f3ds_multi_segment == submit + collect. */
int f3ds_multi_submit(f3ds_multi* m, const void* const* points, const size_t* counts, int n_frames, const f3ds_params* params,
                      uint32_t* const* point_labels, f3ds_result* results, int* ticket);
int f3ds_multi_collect(f3ds_multi* m, int ticket);
/* allocate the label blocks for batches of max_frames_per_device frames of up to max_points_per_frame points now (otherwise they
 * grow inside the first batches); F3DS_ERR_BUSY while a batch is in flight */
int f3ds_multi_reserve(f3ds_multi* m, size_t max_points_per_frame);
/* the gathered label block on devices[0] of the batch gathered last (device pointer): device d's frames, in frame order, start
 * at the sum of the point counts of the devices before d; valid until the batch after the next one is submitted */
const uint32_t* f3ds_multi_gathered_labels(const f3ds_multi* m);
/* the gathered block of a given batch (ticket of f3ds_multi_submit): NULL unless that batch has been gathered without error and its
 * slot has not been handed to a later batch */
const uint32_t* f3ds_multi_gathered_labels_of(f3ds_multi* m, int ticket);
const char* f3ds_multi_last_error(void);

/* ---- host-side helpers either side of the path (no GPU needed) -------------------------- */

/* PCD v0.7 reader (ascii / binary / binary_compressed), replaces pcl::io::loadPCDFile at
 * src/supervoxel_clustering.cpp:313.  Fields x y z + rgb|rgba (+ optional label).  Call with
 * points == NULL to get the point count.  labels may be NULL; missing label field -> 0. */
int f3ds_pcd_read(const char* path, void* points16, uint32_t* labels, size_t cap, size_t* n_out,
                  uint32_t* width, uint32_t* height);
/* PCD writer: fields "x y z rgba" (+ "label" when labels != NULL); mode 0 ascii, 1 binary */
int f3ds_pcd_write(const char* path, const float* xyz, const uint32_t* rgba,
                   const uint32_t* labels, size_t n, int mode);

/* deterministic synthetic frames (SplitMix64): kind 0 = pinhole RGB-D room (width x height
 * pixels), kind 1 = fused multi-view room scene with width*height
 * samples (config 4).  nan_permille = invalid-depth pixels per thousand. */
int f3ds_synth_frame(int kind, uint64_t seed, uint32_t width, uint32_t height,
                     uint32_t nan_permille, void* points16);

/* Glasbey-style lookup used for the coloured cloud (256 entries, r<<16|g<<8|b) */
uint32_t f3ds_label_color(uint32_t label);

#ifdef __cplusplus
}
#endif
#endif /* F3DS_H_ */
