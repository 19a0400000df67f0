// f3ds_cloud.h -- the rules of the region rows of a point cloud (f3ds_cloud_regions, f3ds_cloud_regions_host, include/f3ds.h), shared by
// the HIP kernels (f3ds_cloud.inc) and the host function (f3ds_host.cpp).
//
// One fixed-size row per region of a LABELLED CLOUD -- n records {x, y, z, rgba} and n labels, no image grid: what the region table (f3ds_regions.h) and the
// region shapes (f3ds_shapes.h) say of a region of a label image, in one row, and optionally the region boxes (f3ds_boxes.h) in a second pass.  Nothing is
// defined anew: a point goes through rg_pixel and sh_pixel, a row comes out of rg_finish and ONE call of sh_finish, a box out of bx_frame, bx_pixel and
// bx_finish.  Everything that meets more than one point is a count, a minimum, a maximum or an exact integer sum: any schedule gives the same bits.
//   point      record i = {x, y, z, rgba}.  With fold_negative_z a z below 0 becomes fabsf(z) -- n_prelude (f3ds_numerics.h), the segmenter's prelude rule
//              (main()'s z < 0 -> |z|, src/supervoxel_clustering.cpp:317-321; f3ds_segment applies it to every point it reads, first in d_bbox, f3ds_kernels.inc,
//              with the fold_negative_z of f3ds_params).  Point i is LABELLED iff x, y and z are all finite
//              after the fold and labels[i] != F3DS_NO_LABEL.  A label over a non-finite point contributes nothing (but must still be in range).
//   fixed      the table's rg_fix with its clamped flag; the order of minima and maxima the table's rg_key.
//   moments    the shapes': n, S_a, M_ab as two 64-bit half-sums each (f3ds_shapes.h: |M| < 2^93 does not fit one 64-bit word).
//   accumulator CdAcc: n, first, six keys, three S, twelve half-sums of M, three colour sums: 8 words and 18 64-bit sums, 44 words, 176 bytes.
//   finish     cd_finish: rg_finish on (n, first, keys, S, colour sums), sh_finish on (n, S, M); the row takes the table's n_pixels, first_pixel, lo, hi, centroid,
//              mean_rgb and the shapes' cov ... curvature.  The two centroids are the same expression on the same integers.
//   towards the camera   is "towards the origin", as in the shapes: normal . centroid <= 0.  For a fused cloud (several views, a map) the origin is a convention
//              of whoever fused it, not a viewpoint; the plane (normal, plane_d) is the same plane either way, only its sign convention refers to the origin.
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_CLOUD_H_
#define F3DS_CLOUD_H_

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_numerics.h"
#include "f3ds_regions.h"
#include "f3ds_shapes.h"
#include "f3ds_boxes.h"

namespace f3ds {

constexpr uint64_t CD_MAX_POINTS = 0x7FFFFFFFull;      // the moments' bound (n < 2^31), and a point index is a u32 below the empty first_point
constexpr uint32_t CD_PATH_DIRECT = 1u, CD_PATH_ORDERED = 2u;      // F3DS_DBG_CLOUD_PATH

// the accumulator of one region.  w: [0] points, [1] first point, [2..4] rg_key of lo, [5..7] rg_key of hi; s: [0..2] S (two's complement), [3..8] the hi
// half-sums of xx, xy, xz, yy, yz, zz, [9..14] their lo half-sums (ShAcc's s[]), [15..17] the sums of r, g, b.  [0] and s[] add, [1..4] take minima, [5..7] maxima.
constexpr int CD_W = 8, CD_S = 18, CD_WORDS = CD_W + 2 * CD_S;
struct CdAcc { uint32_t w[CD_W]; uint64_t s[CD_S]; };
static_assert(sizeof(CdAcc) == 4 * CD_WORDS, "an accumulator is 44 words");
static_assert(sizeof(f3ds_cloud_region) == 128, "a row is 32 words");

// word k (0 ... CD_WORDS - 1) of an empty accumulator
F3DS_HD uint32_t cd_empty_word(uint32_t k) { return k == 0u ? 0u : k == 1u ? RG_NONE : k < 5u ? RG_KEY_POS_INF : k < 8u ? RG_KEY_NEG_INF : 0u; }
F3DS_HD void cd_empty(CdAcc& a) {
    for (int k = 0; k < CD_W; ++k) a.w[k] = cd_empty_word((uint32_t)k);
    for (int k = 0; k < CD_S; ++k) a.s[k] = 0u;
}
// the fold, then: are the three coordinates finite?  z is the folded one afterwards.
F3DS_HD bool cd_finite(float x, float y, float& z, int fold_negative_z) {
    n_prelude(z, fold_negative_z);
    return m_isfinitef(x) && m_isfinitef(y) && m_isfinitef(z);
}
// what one labelled point (after the fold) adds to its region: the table's rg_pixel and the shapes' sh_pixel, every word of `a` written.  Returns: clamped?
F3DS_HD bool cd_point(uint32_t i, float x, float y, float z, uint32_t rgba, CdAcc& a) {
    RgAcc r; ShAcc s;
    const bool clamped = rg_pixel(i, 0u, 0u, x, y, z, rgba, r);
    sh_pixel(x, y, z, s);
    a.w[0] = 1u; a.w[1] = i;
    for (int k = 0; k < 3; ++k) { a.w[2 + k] = r.w[6 + k]; a.w[5 + k] = r.w[9 + k]; a.s[15 + k] = r.s[3 + k]; }
    for (int k = 0; k < SH_S; ++k) a.s[k] = s.s[k];
    return clamped;
}
// a += b, field by field
F3DS_HD void cd_merge(CdAcc& a, const CdAcc& b) {
    a.w[0] += b.w[0];
    for (int k = 1; k < 5; ++k) if (b.w[k] < a.w[k]) a.w[k] = b.w[k];
    for (int k = 5; k < 8; ++k) if (b.w[k] > a.w[k]) a.w[k] = b.w[k];
    for (int k = 0; k < CD_S; ++k) a.s[k] += b.s[k];
}
// the row of an accumulator, and the shape row it was made of (the frame of the boxes is bx_frame of that).  An empty one: n_points = 0, first_point =
// 0xFFFFFFFF, lo = +inf, hi = -inf, the quiet NaN 0x7FC00000 in every other float.
F3DS_HD void cd_finish(const CdAcc& a, f3ds_cloud_region* row, f3ds_region_shape* shape) {
    RgAcc r; ShAcc s;
    rg_empty(r); sh_empty(s);
    r.w[0] = a.w[0]; r.w[1] = a.w[1];
    for (int k = 0; k < 3; ++k) { r.w[6 + k] = a.w[2 + k]; r.w[9 + k] = a.w[5 + k]; r.s[k] = a.s[k]; r.s[3 + k] = a.s[15 + k]; }
    for (int k = 0; k < SH_S; ++k) s.s[k] = a.s[k];
    s.n = a.w[0];
    f3ds_region_row t;
    rg_finish(r, &t);
    sh_finish(s, shape);
    f3ds_cloud_region o;
    o.n_points = t.n_pixels; o.first_point = t.first_pixel;
    for (int k = 0; k < 3; ++k) {
        o.lo[k] = t.lo[k]; o.hi[k] = t.hi[k]; o.centroid[k] = t.centroid[k]; o.mean_rgb[k] = t.mean_rgb[k];
        o.eigenvalue[k] = shape->eigenvalue[k]; o.normal[k] = shape->normal[k]; o.axis[k] = shape->axis[k];
    }
    for (int k = 0; k < 6; ++k) o.cov[k] = shape->cov[k];
    o.plane_d = shape->plane_d; o.curvature = shape->curvature; o.reserved = 0u;
    *row = o;
}

// What both entry points refuse before they look at a point, in this order; *use = the parameters they work with (NULL: the defaults).  device_form: a NULL
// points16 stands for the context's own records and is judged by the caller.
inline int cd_check(const void* points16, uint64_t n, const uint32_t* labels, uint32_t n_regions, const f3ds_cloud_params* params, const f3ds_cloud_region* rows,
                    bool device_form, f3ds_cloud_params* use) {
    if (!labels || (!points16 && n && !device_form) || (!rows && n_regions)) return F3DS_ERR_ARG;
    if (params) *use = *params; else { use->plane_tol = 0.01f; use->fold_negative_z = 0; }
    if (!(use->plane_tol >= 0.0f)) return F3DS_ERR_ARG;      // (NaN too; +inf is a tolerance)
    if (n_regions > RG_MAX_REGIONS || n > CD_MAX_POINTS) return F3DS_ERR_UNSUPPORTED;
    return F3DS_OK;
}

// ---- which way the device walks the points (f3ds_cloud.inc), decided on the host from K alone ----
// The workgroup's LDS table has 2^CD_SLOT_BITS slots, found by linear probing from (label * 0x9E3779B1) >> (32 - CD_SLOT_BITS), at most CD_PROBES steps (the
// family's LI_SLOTS and LI_PROBES).  The labels of a call are 0 ... K - 1, so which slots they can ever occupy is a function of K: with unlimited probing the
// set of occupied slots does not depend on the order of arrival, and every partial set is a subset of it.  A label probes through occupied slots only and
// ends on its own, so it needs at most as many steps as the longest run of occupied slots of the full set: where that run is <= CD_PROBES no label ever
// fails to find a slot, whatever the order of the points -- the DIRECT walk (input order) then never leaves LDS.  cd_longest_run says so for every K up to
// CD_DIRECT_MAX_K (the static_assert below walks them all; the run is 6 at K = 96, and reaches 9 at K = 103).  Beyond it an unorganised cloud would push
// what does not fit to the global accumulators point by point, so the ORDERED walk sorts (label, index) first and a span meets few labels again.
constexpr int CD_SLOT_BITS = 7, CD_SLOTS = 1 << CD_SLOT_BITS, CD_PROBES = 8;
constexpr uint32_t CD_DIRECT_MAX_K = 96;      // three quarters of the table
constexpr uint32_t cd_hash(uint32_t l) { return (uint32_t)(l * 0x9E3779B1u) >> (32 - CD_SLOT_BITS); }
constexpr int cd_longest_run(uint32_t K) {
    bool occ[CD_SLOTS] = {};
    for (uint32_t l = 0; l < K && l < (uint32_t)CD_SLOTS; ++l) {
        uint32_t h = cd_hash(l);
        while (occ[h]) h = (h + 1u) & (uint32_t)(CD_SLOTS - 1);
        occ[h] = true;
    }
    int best = 0, run = 0;
    for (int i = 0; i < 2 * CD_SLOTS; ++i) { if (occ[i & (CD_SLOTS - 1)]) { if (++run > best) best = run; } else run = 0; }
    return best < CD_SLOTS ? best : CD_SLOTS;
}
constexpr bool cd_direct_never_overflows() {
    for (uint32_t K = 1; K <= CD_DIRECT_MAX_K; ++K) if (cd_longest_run(K) > CD_PROBES) return false;
    return true;
}
static_assert(cd_direct_never_overflows(), "the direct walk must find every label a slot within CD_PROBES steps");
inline uint32_t cd_choose_path(uint32_t K) { return K <= CD_DIRECT_MAX_K ? CD_PATH_DIRECT : CD_PATH_ORDERED; }

}  // namespace f3ds
#endif  // F3DS_CLOUD_H_
