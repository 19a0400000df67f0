// f3ds_joints.h -- the rules of the region joints (f3ds_region_joints, f3ds_region_joints_host, include/f3ds.h), shared by the HIP
// kernels (f3ds_joints.inc) and the host function (f3ds_host.cpp).
//
// One fixed-size row per PAIR of regions of a label image that touch: the contacts' counts, the border's samples in space, and the join of the two regions'
// shape rows.  Everything that meets more than one pixel is a count or an exact integer sum, and the finish is one function: any schedule gives the same bits.
//   pairs      the contacts' (f3ds_contacts.h): ct_pair decides a, b and CLOSE; n_pairs and n_close are its words [0] and [1].
//   samples    a CLOSE pair adds both of its pixels' points: two sh_pixel contributions (f3ds_shapes.h) merged by sh_merge.  The accumulator of a pair of
//              regions is the two counts and a ShAcc; its n is always 2 * n_close.
//   finish     jt_finish: sh_finish on the samples (centroid, axis, eigenvalue), then the join with the public floats of the two shape rows, every operation
//              one rounded f32 operation in the order written, then the kind.  Every float is canonicalised (a NaN becomes 0x7FC00000).
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_JOINTS_H_
#define F3DS_JOINTS_H_

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_numerics.h"
#include "f3ds_regions.h"
#include "f3ds_contacts.h"
#include "f3ds_shapes.h"

namespace f3ds {

static_assert(sizeof(f3ds_region_joint) == 80, "a row is 20 words");
constexpr uint64_t JT_MAX_PIXELS = 0x1FFFFFFFull;      // 4 samples a pixel at most, and sh_finish wants n < 2^31

// the accumulator of one pair of regions
struct JtAcc { uint32_t n_pairs, n_close; ShAcc sh; };
// ... and as a record in memory: [0] n_pairs, [1] n_close, [2] sh.n, [3] 0, then the fifteen sums as (lo, hi) words: 34 words, 8-byte aligned
constexpr int JT_WORDS = 4 + 2 * SH_S;

F3DS_HD void jt_empty(JtAcc& a) { a.n_pairs = a.n_close = 0u; sh_empty(a.sh); }

// what one contact pair adds to the accumulator of its (a, b): every word of `acc` is written.  p, horizontal, lp, zp, lq, zq: as ct_pair takes them; P, Q: the
// points of the pair's first and second pixel (n_deproject).  Returns the pair's a and b.
F3DS_HD void jt_pair(uint32_t p, bool horizontal, uint32_t lp, float zp, uint32_t lq, float zq, float depth_tol, const float P[3], const float Q[3], uint32_t& a, uint32_t& b,
                     JtAcc& acc) {
    CtAcc c;
    ct_pair(p, horizontal, lp, zp, lq, zq, depth_tol, a, b, c);
    acc.n_pairs = c.w[0]; acc.n_close = c.w[1];
    if (c.w[1]) {
        ShAcc second;
        sh_pixel(P[0], P[1], P[2], acc.sh);
        sh_pixel(Q[0], Q[1], Q[2], second);
        sh_merge(acc.sh, second);
    } else sh_empty(acc.sh);
}
// a += b, field by field
F3DS_HD void jt_merge(JtAcc& a, const JtAcc& b) { a.n_pairs += b.n_pairs; a.n_close += b.n_close; sh_merge(a.sh, b.sh); }

F3DS_HD void jt_to_words(const JtAcc& a, uint32_t* w) {
    w[0] = a.n_pairs; w[1] = a.n_close; w[2] = a.sh.n; w[3] = 0u;
    for (int k = 0; k < SH_S; ++k) { w[4 + 2 * k] = (uint32_t)a.sh.s[k]; w[5 + 2 * k] = (uint32_t)(a.sh.s[k] >> 32); }
}
F3DS_HD void jt_from_words(const uint32_t* w, JtAcc& a) {
    a.n_pairs = w[0]; a.n_close = w[1]; a.sh.n = w[2]; a.sh.pad = 0u;
    for (int k = 0; k < SH_S; ++k) a.sh.s[k] = ((uint64_t)w[5 + 2 * k] << 32) | w[4 + 2 * k];
}

// n . c + d, the signed distance of c from the plane (n, d): two rounded adds of three rounded products, then one more add
F3DS_HD float jt_plane(const float n[3], const float c[3], float d) {
    const float p0 = n[0] * c[0], p1 = n[1] * c[1], p2 = n[2] * c[2];
    const float s = (p0 + p1) + p2;
    return s + d;
}
F3DS_HD float jt_canon(float t) { return t != t ? m_from_bitsf(RG_QNAN) : t; }

// the row of the accumulator of (a, b), n_pairs >= 1, joined with the shape rows of a and b.  Returns: a surface border (n_close > 0)?
F3DS_HD bool jt_finish(uint32_t a, uint32_t b, const JtAcc& acc, const f3ds_region_shape& Sa, const f3ds_region_shape& Sb, const f3ds_joint_params& prm, f3ds_region_joint* row) {
    f3ds_region_joint r;
    r.a = a; r.b = b; r.n_pairs = acc.n_pairs; r.n_close = acc.n_close;
    const float q = m_from_bitsf(RG_QNAN);
    const bool surface = acc.n_close != 0u;
    if (surface) {
        f3ds_region_shape s;
        sh_finish(acc.sh, &s);
        for (int k = 0; k < 3; ++k) { r.centroid[k] = s.centroid[k]; r.direction[k] = s.axis[k]; r.spread[k] = s.eigenvalue[k]; }
        r.e_a = jt_plane(Sa.normal, r.centroid, Sa.plane_d);
        r.e_b = jt_plane(Sb.normal, r.centroid, Sb.plane_d);
    } else {
        for (int k = 0; k < 3; ++k) r.centroid[k] = r.direction[k] = r.spread[k] = q;
        r.e_a = r.e_b = q;
    }
    const float c0 = Sa.normal[0] * Sb.normal[0], c1 = Sa.normal[1] * Sb.normal[1], c2 = Sa.normal[2] * Sb.normal[2];
    r.cos_angle = (c0 + c1) + c2;
    r.h_ab = jt_plane(Sa.normal, Sb.centroid, Sa.plane_d);
    r.h_ba = jt_plane(Sb.normal, Sa.centroid, Sb.plane_d);
    r.delta_g = n_normals_diff(Sa.normal, Sa.centroid, Sb.normal, Sb.centroid);
    const bool ref_convex = n_is_convex(Sa.normal, Sa.centroid, Sb.normal, Sb.centroid);
    uint32_t kind;
    if (!surface) kind = F3DS_JOINT_OCCLUSION;
    else if (r.cos_angle >= prm.cos_coplanar && m_absf(r.h_ab) <= prm.plane_tol && m_absf(r.h_ba) <= prm.plane_tol) kind = F3DS_JOINT_COPLANAR;
    else {
        const float both = r.h_ab + r.h_ba;
        kind = both < 0.0f ? F3DS_JOINT_CONVEX : F3DS_JOINT_CONCAVE;
    }
    r.kind = kind | (ref_convex ? F3DS_JOINT_REF_CONVEX : 0u);
    for (int k = 0; k < 3; ++k) { r.centroid[k] = jt_canon(r.centroid[k]); r.direction[k] = jt_canon(r.direction[k]); r.spread[k] = jt_canon(r.spread[k]); }
    r.cos_angle = jt_canon(r.cos_angle); r.delta_g = jt_canon(r.delta_g); r.h_ab = jt_canon(r.h_ab); r.h_ba = jt_canon(r.h_ba); r.e_a = jt_canon(r.e_a); r.e_b = jt_canon(r.e_b);
    *row = r;
    return surface;
}

// What both entry points refuse before they look at a pixel, in this order: the contacts' argument errors, the two tolerances of the join, too many regions,
// too many pixels; *use = the format they work with, *prm = the parameters (the defaults for NULL).
inline int jt_check(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, const f3ds_joint_params* params, const size_t* n_out,
                    f3ds_rgbd_format* use, RgbdLayout* lay, f3ds_joint_params* prm) {
    if (params) *prm = *params; else { prm->depth_tol = 0.05f; prm->plane_tol = 0.01f; prm->cos_coplanar = 0.9659258f; }
    const int rc = ct_check(fmt, depth, labels, n_regions, prm->depth_tol, n_out, use, lay);
    if (rc == F3DS_ERR_ARG) return rc;
    if (!(prm->plane_tol >= 0.0f)) return F3DS_ERR_ARG;      // (NaN too; +inf is a tolerance)
    if (!(prm->cos_coplanar >= -1.0f && prm->cos_coplanar <= 1.0f)) return F3DS_ERR_ARG;      // (NaN too)
    if (rc) return rc;
    return (uint64_t)lay->n > JT_MAX_PIXELS ? F3DS_ERR_UNSUPPORTED : F3DS_OK;
}

}  // namespace f3ds
#endif  // F3DS_JOINTS_H_
