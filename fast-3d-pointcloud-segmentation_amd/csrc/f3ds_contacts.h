// f3ds_contacts.h -- the rules of the region contacts (f3ds_region_contacts, f3ds_region_contacts_host, include/f3ds.h), shared by the
// HIP kernels (f3ds_contacts.inc) and the host function (f3ds_host.cpp).
//
// One fixed-size row per PAIR of regions of a label image that touch in the image (4-connectivity), over a depth image.  Every field is a count, a minimum or
// a sum of integers, so the order in which the pixel pairs are visited does not matter: any schedule gives the same bits.
//   point      pixel p = v * width + u gets z from n_depth_to_z (f3ds_numerics.h); it is LABELLED iff its depth is valid and label[p] != F3DS_NO_LABEL (the
//              tracker's and the table's definition).
//   pairs      p with its right neighbour p + 1 (u + 1 < width) and with its lower neighbour p + width (v + 1 < height): every unordered pixel pair once.  A pair
//              is a CONTACT iff both pixels are labelled and their labels differ; it belongs to (a, b) = (smaller label, larger label).
//   class      za, zb: the depths of a's and b's pixel.  g = fabsf(za - zb), zn = za < zb ? za : zb; CLOSE iff g <= depth_tol * zn (one rounded product; false
//              on NaN: the form of tk_votes); a pair that is not close has a IN FRONT iff za < zb, else b.
//   gap        sum_fix_gap adds rg_fix(g) (f3ds_regions.h: units of 2^-16 m, clamped to 32768 m; the clamp flag is not looked at).
//   finish     ct_mean_gap: (float)(((double)sum_fix_gap / (double)n_pairs) * 2^-16): IEEE f64 operations and one conversion, the same code on the host and on
//              the device.
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_CONTACTS_H_
#define F3DS_CONTACTS_H_

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_rgbd.h"
#include "f3ds_regions.h"

namespace f3ds {

constexpr uint32_t CT_NONE = 0xFFFFFFFFu;         // F3DS_NO_LABEL; the empty first_pixel
constexpr uint32_t CT_MAX_REGIONS = RG_MAX_REGIONS;
constexpr uint64_t CT_NO_KEY = ~0ull;             // no pair: above every key and every hole

// the accumulator of one pair of regions, seven words.  w: [0] contact pairs, [1] close ones, [2] those with a in front, [3] horizontal ones, [4] the smallest
// first pixel; s: the fixed-point sum of the gaps.  [0..3] and s add, [4] takes the minimum.
constexpr int CT_W = 5, CT_WORDS = CT_W + 2;
struct CtAcc { uint32_t w[CT_W]; uint64_t s; };
static_assert(sizeof(f3ds_region_contact) == 32, "a row is 8 words");

enum CtClass { CT_CLOSE = 0, CT_A_FRONT = 1, CT_B_FRONT = 2 };

F3DS_HD void ct_empty(CtAcc& a) { a.w[0] = a.w[1] = a.w[2] = a.w[3] = 0u; a.w[4] = CT_NONE; a.s = 0u; }

// the class of a contact pair and its gap g
F3DS_HD int ct_class(float za, float zb, float depth_tol, float& g) {
    g = m_absf(za - zb);
    const float zn = za < zb ? za : zb;
    const float bound = depth_tol * zn;
    if (g <= bound) return CT_CLOSE;
    return za < zb ? CT_A_FRONT : CT_B_FRONT;
}
// the sort key of the pair (a, b), a < b < K: (a << kb) | b with kb = ct_bits(K); ct_hole(K) is above every key
F3DS_HD int ct_bits(uint32_t K) { int b = 0; const uint32_t v = K ? K - 1u : 0u; while (b < 32 && (v >> b)) ++b; return b; }
F3DS_HD uint64_t ct_key(uint32_t a, uint32_t b, int kb) { return ((uint64_t)a << kb) | b; }
F3DS_HD uint64_t ct_hole(uint32_t K, int kb) { return (uint64_t)K << kb; }
F3DS_HD int ct_sort_bits(uint32_t K) { int b = 0; const uint64_t h = ct_hole(K, ct_bits(K)); while (b < 64 && (h >> b)) ++b; return b; }

// what one contact pair adds to the accumulator of its (a, b): every word of `acc` is written.  p: the pair's first (left or upper) pixel with label lp and depth
// zp; its right (horizontal) or lower neighbour has label lq != lp and depth zq.  Returns the pair's a and b.
F3DS_HD void ct_pair(uint32_t p, bool horizontal, uint32_t lp, float zp, uint32_t lq, float zq, float depth_tol, uint32_t& a, uint32_t& b, CtAcc& acc) {
    const bool p_is_a = lp < lq;
    a = p_is_a ? lp : lq; b = p_is_a ? lq : lp;
    float g;
    const int cls = ct_class(p_is_a ? zp : zq, p_is_a ? zq : zp, depth_tol, g);
    bool clamped = false;
    acc.w[0] = 1u; acc.w[1] = cls == CT_CLOSE ? 1u : 0u; acc.w[2] = cls == CT_A_FRONT ? 1u : 0u; acc.w[3] = horizontal ? 1u : 0u; acc.w[4] = p;
    acc.s = (uint64_t)rg_fix(g, clamped);
}
// a += b, field by field
F3DS_HD void ct_merge(CtAcc& a, const CtAcc& b) {
    for (int k = 0; k < 4; ++k) a.w[k] += b.w[k];
    if (b.w[4] < a.w[4]) a.w[4] = b.w[4];
    a.s += b.s;
}
F3DS_HD float ct_mean_gap(uint64_t sum_fix_gap, uint32_t n_pairs) {
    return (float)(((double)(int64_t)sum_fix_gap / (double)n_pairs) * 0.0000152587890625);      // 2^-16, exact
}
// the row of the accumulator of (a, b); n_pairs >= 1
F3DS_HD void ct_finish(uint32_t a, uint32_t b, const CtAcc& acc, f3ds_region_contact* row) {
    f3ds_region_contact r;
    r.a = a; r.b = b; r.n_pairs = acc.w[0]; r.n_close = acc.w[1]; r.n_a_front = acc.w[2]; r.n_horizontal = acc.w[3]; r.first_pixel = acc.w[4];
    r.mean_gap = ct_mean_gap(acc.s, acc.w[0]);
    *row = r;
}

// What both entry points refuse before they look at a pixel, in this order: a missing n_out and li_check's arguments, depth_tol, li_check's region cap; *use =
// the format they work with.
inline int ct_check(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, float depth_tol, const size_t* n_out,
                    f3ds_rgbd_format* use, RgbdLayout* lay) {
    if (!n_out) return F3DS_ERR_ARG;
    const int rc = li_check(fmt, depth, nullptr, labels, n_regions, use, lay);
    if (rc == F3DS_ERR_ARG) return rc;
    if (!m_isfinitef(depth_tol) || !(depth_tol >= 0.0f)) return F3DS_ERR_ARG;
    return rc;
}

}  // namespace f3ds
#endif  // F3DS_CONTACTS_H_
