// f3ds_regions.h -- the rules of the region table (f3ds_region_table, f3ds_region_table_host, include/f3ds.h), shared by the HIP
// kernels (f3ds_regions.inc) and the host function (f3ds_host.cpp).
//
// One fixed-size row per region of a label image over a depth (and colour) image: pixel count, first pixel, pixel box, box of the points, centroid, mean colour.
// Every field is a count, a minimum, a maximum or a sum of integers, so the order in which the pixels are visited does not matter: any schedule gives the same bits.
//   point      pixel p = v * width + u gets (x, y, z) from n_depth_to_z / n_deproject (f3ds_numerics.h); it is LABELLED iff its depth is valid and
//              label[p] != F3DS_NO_LABEL (the tracker's definition, f3ds_track.h).  Only labelled pixels contribute.
//   fixed      rg_fix(a) = (int64_t)rint(clamp((double)a, -32768, 32768) * 65536): units of 2^-16 m, |rg_fix| <= 2^31, so 2^31 - 1 of them add up inside 64 bits.
//              A labelled pixel is CLAMPED iff the clamp changed one of its coordinates.
//   order      minima and maxima of floats in the total order of rg_key(bits) = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000): -0 below +0, a u32 comparison.
//   finish     rg_finish: centroid = (float)(((double)sum_fix / (double)n) * 2^-16), mean_rgb = (float)((double)sum / (double)n): IEEE f64 operations and one
//              conversion, the same code on the host and on the device.
// A coordinate that is not finite (a depth_scale that overflows f32) is outside the contract but stays defined: a NaN becomes the quiet NaN 0x7FC00000 before it
// is keyed, and clamps to -32768.
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_REGIONS_H_
#define F3DS_REGIONS_H_

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_rgbd.h"
#include "f3ds_label_image.h"

namespace f3ds {

constexpr uint32_t RG_NONE = 0xFFFFFFFFu;         // F3DS_NO_LABEL; the empty first_pixel, u_min, v_min
constexpr uint32_t RG_MAX_REGIONS = LI_MAX_REGIONS;
constexpr uint32_t RG_QNAN = 0x7FC00000u;
constexpr uint32_t RG_KEY_POS_INF = 0xFF800000u;  // rg_key(+inf): the empty minimum
constexpr uint32_t RG_KEY_NEG_INF = 0x007FFFFFu;  // rg_key(-inf): the empty maximum

// the accumulator of one region.  w: [0] pixels, [1] first pixel, [2] u_min, [3] v_min, [4] u_max, [5] v_max, [6..8] rg_key of lo, [9..11] rg_key of hi;
// s: the fixed-point sums of x, y, z (two's complement) and the sums of r, g, b.  [0] and s[] add, [1..3] and [6..8] take minima, [4], [5] and [9..11] maxima.
constexpr int RG_W = 12, RG_S = 6, RG_WORDS = RG_W + 2 * RG_S;
struct RgAcc { uint32_t w[RG_W]; uint64_t s[RG_S]; };
static_assert(sizeof(RgAcc) == 4 * RG_WORDS, "an accumulator is 24 words");
static_assert(sizeof(f3ds_region_row) == 72, "a row is 18 words");

// word k (0 ... RG_WORDS - 1) of an empty accumulator
F3DS_HD uint32_t rg_empty_word(uint32_t k) { return k == 0u ? 0u : k < 4u ? RG_NONE : k < 6u ? 0u : k < 9u ? RG_KEY_POS_INF : k < 12u ? RG_KEY_NEG_INF : 0u; }
F3DS_HD void rg_empty(RgAcc& a) {
    for (int k = 0; k < RG_W; ++k) a.w[k] = rg_empty_word((uint32_t)k);
    for (int k = 0; k < RG_S; ++k) a.s[k] = 0u;
}

F3DS_HD uint32_t rg_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
F3DS_HD uint32_t rg_unkey(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
// the clamp of rg_fix: a as a double inside [-32768, 32768] (the value itself or one of the two ends)
F3DS_HD double rg_clamp(float a, bool& clamped) {
    double d = (double)a;
    if (!(d >= -32768.0)) { d = -32768.0; clamped = true; }      // (NaN too)
    else if (d > 32768.0) { d = 32768.0; clamped = true; }
    return d;
}
F3DS_HD int64_t rg_fix(float a, bool& clamped) { return (int64_t)__builtin_rint(rg_clamp(a, clamped) * 65536.0); }

// what one labelled pixel adds to its region: every word of `a` is written.  rgba: the colour word of n_color_word (0 without a colour image).  Returns: clamped?
F3DS_HD bool rg_pixel(uint32_t p, uint32_t u, uint32_t v, float x, float y, float z, uint32_t rgba, RgAcc& a) {
    a.w[0] = 1u; a.w[1] = p; a.w[2] = u; a.w[3] = v; a.w[4] = u; a.w[5] = v;
    const float c[3] = {x, y, z};
    bool clamped = false;
    for (int k = 0; k < 3; ++k) {
        const uint32_t bits = c[k] != c[k] ? RG_QNAN : m_bitsf(c[k]);
        a.w[6 + k] = a.w[9 + k] = rg_key(bits);
        a.s[k] = (uint64_t)rg_fix(c[k], clamped);
    }
    a.s[3] = (rgba >> 16) & 255u; a.s[4] = (rgba >> 8) & 255u; a.s[5] = rgba & 255u;
    return clamped;
}
// a += b, field by field
F3DS_HD void rg_merge(RgAcc& a, const RgAcc& b) {
    a.w[0] += b.w[0];
    for (int k = 1; k < 4; ++k) if (b.w[k] < a.w[k]) a.w[k] = b.w[k];
    for (int k = 4; k < 6; ++k) if (b.w[k] > a.w[k]) a.w[k] = b.w[k];
    for (int k = 6; k < 9; ++k) if (b.w[k] < a.w[k]) a.w[k] = b.w[k];
    for (int k = 9; k < 12; ++k) if (b.w[k] > a.w[k]) a.w[k] = b.w[k];
    for (int k = 0; k < RG_S; ++k) a.s[k] += b.s[k];
}
// the row of an accumulator.  An empty one: first_pixel = u_min = v_min = 0xFFFFFFFF, u_max = v_max = 0, lo = +inf, hi = -inf, centroid = mean_rgb = quiet NaN.
F3DS_HD void rg_finish(const RgAcc& a, f3ds_region_row* row) {
    f3ds_region_row r;
    r.n_pixels = a.w[0]; r.first_pixel = a.w[1]; r.u_min = a.w[2]; r.v_min = a.w[3]; r.u_max = a.w[4]; r.v_max = a.w[5];
    for (int k = 0; k < 3; ++k) { r.lo[k] = m_from_bitsf(rg_unkey(a.w[6 + k])); r.hi[k] = m_from_bitsf(rg_unkey(a.w[9 + k])); }
    if (a.w[0] == 0u) {
        for (int k = 0; k < 3; ++k) r.centroid[k] = r.mean_rgb[k] = m_from_bitsf(RG_QNAN);
    } else {
        const double n = (double)a.w[0];
        for (int k = 0; k < 3; ++k) {
            r.centroid[k] = (float)(((double)(int64_t)a.s[k] / n) * 0.0000152587890625);      // 2^-16, exact
            r.mean_rgb[k] = (float)((double)a.s[3 + k] / n);
        }
    }
    *row = r;
}

// What both entry points refuse before they look at a pixel: missing rows, then li_check; *use = the format they work with.
inline int rg_check(const f3ds_rgbd_format* fmt, const void* depth, const void* color, const uint32_t* labels, uint32_t n_regions, const f3ds_region_row* rows,
                    f3ds_rgbd_format* use, RgbdLayout* lay) {
    if (!rows && n_regions) return F3DS_ERR_ARG;
    return li_check(fmt, depth, color, labels, n_regions, use, lay);
}

}  // namespace f3ds
#endif  // F3DS_REGIONS_H_
