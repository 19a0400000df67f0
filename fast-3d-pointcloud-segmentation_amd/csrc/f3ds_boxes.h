// f3ds_boxes.h -- the rules of the region boxes (f3ds_region_boxes, f3ds_region_boxes_host, include/f3ds.h), shared by the HIP
// kernels (f3ds_boxes.inc) and the host function (f3ds_host.cpp).
//
// One fixed-size row per region of a label image over a depth image: the box of the region's points along the region's own axes, and how far the points lie
// from the region's plane.  The axes are those of the region's shape row (f3ds_shapes.h), so the box needs TWO passes over the pixels: the shapes first, then
// every pixel measured in the frame of its region.  Everything of the second pass that meets more than one pixel is a count, a minimum, a maximum or an integer
// sum of a per-pixel value whose float evaluation order is fixed: any schedule gives the same bits.
//   point      the region table's (f3ds_regions.h): n_depth_to_z / n_deproject, LABELLED iff the depth is valid and label[p] != F3DS_NO_LABEL.
//   frame      bx_frame: c, n, l from the public floats of the shape row, m = n x l (two rounded products and one rounded subtraction a component), plane_tol.
//   coordinate q_a = (float)((double)rg_fix(a) * 2^-16): the point on the grid of 2^-16 m that the shape's moments -- and so the frame's centroid -- are made of,
//              clamped as there, finite whatever the depth scale.  Measuring the raw f32 against a centroid that lives on that grid would put up to 2^-17 m of
//              grid offset into every t: a region at one constant depth would not lie on its own plane.
//   projection d = q - c; t_e = (d_x * e_x + d_y * e_y) + d_z * e_z for e in n, m, l; NaN bits canonicalised as rg_pixel does.
//   extents    minima and maxima of t in the order of rg_key.
//   plane      r = |t_n|; INLIER iff r <= plane_tol; the sum of rg_fix(r) in units of 2^-16 m.
//   finish     bx_finish: half, mid, center, mean_abs_residual as include/f3ds.h says; the same code on the host and on the device.
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_BOXES_H_
#define F3DS_BOXES_H_

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_regions.h"
#include "f3ds_shapes.h"

namespace f3ds {

// the frame of one region: 16 floats, one 64-byte line.  c: the centroid; n, m, l: the axes; tol: the call's plane_tol (the same in every frame: a pixel
// finds everything it needs in its region's line).
struct alignas(16) BxFrame { float c[3], n[3], m[3], l[3], tol, pad[3]; };
static_assert(sizeof(BxFrame) == 64, "a frame is 16 words");

// the accumulator of one region.  w: [0] pixels, [1] inliers, [2..4] rg_key of lo along n, m, l, [5..7] rg_key of hi; s: the fixed-point sum of |t_n| (two's
// complement).  [0], [1] and s add, [2..4] take minima, [5..7] maxima.  10 words and 6 of padding: 64 bytes.
constexpr int BX_W = 8, BX_WORDS = 16;
struct BxAcc { uint32_t w[BX_W]; uint64_t s; uint32_t pad[BX_WORDS - BX_W - 2]; };
static_assert(sizeof(BxAcc) == 4 * BX_WORDS, "an accumulator is 10 words and 6 of padding");
static_assert(sizeof(f3ds_region_box) == 96, "a row is 24 words");

// word k (0 ... BX_WORDS - 1) of an empty accumulator
F3DS_HD uint32_t bx_empty_word(uint32_t k) { return k < 2u ? 0u : k < 5u ? RG_KEY_POS_INF : k < 8u ? RG_KEY_NEG_INF : 0u; }
F3DS_HD void bx_empty(BxAcc& a) {
    for (int k = 0; k < BX_W; ++k) a.w[k] = bx_empty_word((uint32_t)k);
    a.s = 0u;
    for (int k = 0; k < BX_WORDS - BX_W - 2; ++k) a.pad[k] = 0u;
}

// the frame of a region from the public floats of its shape row; an empty region's frame is NaN and no pixel asks for it
F3DS_HD void bx_frame(const f3ds_region_shape& s, float plane_tol, BxFrame& f) {
    for (int k = 0; k < 3; ++k) { f.c[k] = s.centroid[k]; f.n[k] = s.normal[k]; f.l[k] = s.axis[k]; f.pad[k] = 0.0f; }
    const float a0 = f.n[1] * f.l[2], b0 = f.n[2] * f.l[1];
    const float a1 = f.n[2] * f.l[0], b1 = f.n[0] * f.l[2];
    const float a2 = f.n[0] * f.l[1], b2 = f.n[1] * f.l[0];
    f.m[0] = a0 - b0; f.m[1] = a1 - b1; f.m[2] = a2 - b2;
    f.tol = plane_tol;
}

// what one labelled pixel adds to its region, measured in the region's frame: every word of `a` but the padding is written.  Returns: clamped?
F3DS_HD bool bx_pixel(float x, float y, float z, const BxFrame& f, BxAcc& a) {
    bool clamped = false;
    const float q[3] = {(float)((double)rg_fix(x, clamped) * 0.0000152587890625), (float)((double)rg_fix(y, clamped) * 0.0000152587890625),
                        (float)((double)rg_fix(z, clamped) * 0.0000152587890625)};      // (2^-16: the product is exact, the conversion rounds once)
    const float d0 = q[0] - f.c[0], d1 = q[1] - f.c[1], d2 = q[2] - f.c[2];
    const float p0 = d0 * f.n[0], p1 = d1 * f.n[1], p2 = d2 * f.n[2];
    const float tn = (p0 + p1) + p2;
    const float u0 = d0 * f.m[0], u1 = d1 * f.m[1], u2 = d2 * f.m[2];
    const float tm = (u0 + u1) + u2;
    const float v0 = d0 * f.l[0], v1 = d1 * f.l[1], v2 = d2 * f.l[2];
    const float tl = (v0 + v1) + v2;
    const float t[3] = {tn, tm, tl};
    for (int k = 0; k < 3; ++k) {
        const uint32_t bits = t[k] != t[k] ? RG_QNAN : m_bitsf(t[k]);
        a.w[2 + k] = a.w[5 + k] = rg_key(bits);
    }
    const float r = m_absf(tn);
    bool unused = false;
    a.w[0] = 1u; a.w[1] = r <= f.tol ? 1u : 0u;
    a.s = (uint64_t)rg_fix(r, unused);
    return clamped;
}
// a += b, field by field
F3DS_HD void bx_merge(BxAcc& a, const BxAcc& b) {
    a.w[0] += b.w[0]; a.w[1] += b.w[1];
    for (int k = 2; k < 5; ++k) if (b.w[k] < a.w[k]) a.w[k] = b.w[k];
    for (int k = 5; k < 8; ++k) if (b.w[k] > a.w[k]) a.w[k] = b.w[k];
    a.s += b.s;
}
// the row of an accumulator and its region's frame.  An empty one: n_pixels = n_inliers = 0 and the quiet NaN 0x7FC00000 in all 22 floats.
F3DS_HD void bx_finish(const BxAcc& a, const BxFrame& f, f3ds_region_box* row) {
    f3ds_region_box r;
    r.n_pixels = a.w[0]; r.n_inliers = a.w[1];
    if (a.w[0] == 0u) {
        const float q = m_from_bitsf(RG_QNAN);
        for (int k = 0; k < 3; ++k) r.center[k] = r.axis_n[k] = r.axis_m[k] = r.axis_l[k] = r.lo[k] = r.hi[k] = r.half[k] = q;
        r.mean_abs_residual = q;
        *row = r;
        return;
    }
    float mid[3];
    for (int k = 0; k < 3; ++k) {
        r.axis_n[k] = f.n[k]; r.axis_m[k] = f.m[k]; r.axis_l[k] = f.l[k];
        r.lo[k] = m_from_bitsf(rg_unkey(a.w[2 + k])); r.hi[k] = m_from_bitsf(rg_unkey(a.w[5 + k]));
        const float ext = r.hi[k] - r.lo[k], sum = r.lo[k] + r.hi[k];
        r.half[k] = ext * 0.5f; mid[k] = sum * 0.5f;
    }
    for (int k = 0; k < 3; ++k) {
        const float e0 = mid[0] * f.n[k], e1 = mid[1] * f.m[k], e2 = mid[2] * f.l[k];
        r.center[k] = ((f.c[k] + e0) + e1) + e2;
    }
    r.mean_abs_residual = (float)(((double)(int64_t)a.s / (double)a.w[0]) * 0.0000152587890625);      // 2^-16, exact
    *row = r;
}

// What both entry points refuse before they look at a pixel, in li_check's order: missing rows and what li_check calls an argument error, then the tolerance,
// then too many regions; *use = the format they work with.
inline int bx_check(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, float plane_tol, const f3ds_region_box* rows,
                    f3ds_rgbd_format* use, RgbdLayout* lay) {
    if (!rows && n_regions) return F3DS_ERR_ARG;
    const int rc = li_check(fmt, depth, nullptr, labels, n_regions, use, lay);
    if (rc == F3DS_ERR_ARG) return rc;
    if (!(plane_tol >= 0.0f)) return F3DS_ERR_ARG;      // (NaN too; +inf is a tolerance)
    return rc;
}

}  // namespace f3ds
#endif  // F3DS_BOXES_H_
