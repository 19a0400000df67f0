// f3ds_shapes.h -- the rules of the region shapes (f3ds_region_shapes, f3ds_region_shapes_host, include/f3ds.h), shared by the HIP
// kernels (f3ds_shapes.inc) and the host function (f3ds_host.cpp).
//
// One fixed-size row per region of a label image over a depth image: pixel count, centroid, covariance of the points, its eigenvalues, the plane through the
// centroid and the direction the region is long in.  Everything that depends on more than one pixel is an exact integer sum, so the order in which the pixels
// are visited does not matter: any schedule gives the same bits.
//   point      the region table's (f3ds_regions.h): n_depth_to_z / n_deproject, LABELLED iff the depth is valid and label[p] != F3DS_NO_LABEL.
//   fixed      the table's rg_fix, with its clamped flag: f_x, f_y, f_z in units of 2^-16 m, |f| <= 2^31.
//   moments    per region n, S_a = sum f_a and M_ab = sum f_a * f_b for ab in xx, xy, xz, yy, yz, zz, as exact integers.  n < 2^31, so |S| < 2^62 and
//              |M| < 2^93: M does not fit 64 bits.  It is kept as two 64-bit sums of the halves of each product p (an int64, |p| <= 2^62): hi adds p >> 32
//              (arithmetic), lo adds p & 0xFFFFFFFF; |hi| < 2^61, lo < 2^63, and M = hi * 2^32 + lo.  Only 64-bit integer adds meet more than one pixel.
//   scatter    N_ab = n * M_ab - S_a * S_b, exact in a signed 128-bit integer (|N| < 2^125): no cancellation error.
//   cov        C_ab = (((double)N_ab / (double)n) / (double)n) * 2^-32: (double)N_ab is the integer rounded to nearest even once (sh_to_double), the divisions
//              are IEEE, the scaling is exact.
//   eigen      sh_jacobi: 8 cyclic sweeps of Jacobi rotations in f64, + - * / and n_sqrt only, each operation rounded once.
//   finish     sh_finish: order, signs, plane and curvature as include/f3ds.h says; the same code on the host and on the device.
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_SHAPES_H_
#define F3DS_SHAPES_H_

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_numerics.h"
#include "f3ds_rgbd.h"
#include "f3ds_regions.h"

namespace f3ds {

__extension__ typedef __int128 sh_i128;
__extension__ typedef unsigned __int128 sh_u128;

// the accumulator of one region.  s: [0..2] S_x, S_y, S_z (two's complement); [3..8] the hi half-sums of xx, xy, xz, yy, yz, zz (two's complement); [9..14] their
// lo half-sums.  n: the pixel count.  31 words and one of padding: 128 bytes, one cache line a region.  Every field adds.
constexpr int SH_S = 15, SH_WORDS = 32;
struct ShAcc { uint64_t s[SH_S]; uint32_t n, pad; };
static_assert(sizeof(ShAcc) == 4 * SH_WORDS, "an accumulator is 31 words and one of padding");
static_assert(sizeof(f3ds_region_shape) == 84, "a row is 21 words");

F3DS_HD void sh_empty(ShAcc& a) {
    for (int k = 0; k < SH_S; ++k) a.s[k] = 0u;
    a.n = 0u; a.pad = 0u;
}
// what one labelled pixel adds to its region: every word of `a` is written.  Returns: clamped?
F3DS_HD bool sh_pixel(float x, float y, float z, ShAcc& a) {
    bool clamped = false;
    const int64_t fx = rg_fix(x, clamped), fy = rg_fix(y, clamped), fz = rg_fix(z, clamped);
    const int64_t p[6] = {fx * fx, fx * fy, fx * fz, fy * fy, fy * fz, fz * fz};      // (|f| <= 2^31: no product leaves 2^62)
    a.s[0] = (uint64_t)fx; a.s[1] = (uint64_t)fy; a.s[2] = (uint64_t)fz;
    for (int k = 0; k < 6; ++k) { a.s[3 + k] = (uint64_t)(p[k] >> 32); a.s[9 + k] = (uint64_t)p[k] & 0xFFFFFFFFull; }
    a.n = 1u; a.pad = 0u;
    return clamped;
}
// a += b, field by field
F3DS_HD void sh_merge(ShAcc& a, const ShAcc& b) {
    for (int k = 0; k < SH_S; ++k) a.s[k] += b.s[k];
    a.n += b.n;
}

// the integer v as a double, rounded to nearest even once.  Above 64 bits: the top 64 bits of the magnitude with a sticky bit for what is below them (far under
// the rounding position), converted by the one correctly rounded u64 -> f64 conversion, and scaled by a power of two.
F3DS_HD double sh_to_double(sh_i128 v) {
    const bool neg = v < 0;
    const sh_u128 mag = neg ? (sh_u128)0 - (sh_u128)v : (sh_u128)v;
    const uint64_t h = (uint64_t)(mag >> 64), l = (uint64_t)mag;
    double d;
    if (h == 0u) d = (double)l;
    else {
        const int sh = __builtin_clzll(h);                       // 0 ... 63
        const sh_u128 m = mag << sh;                             // bit 127 set
        const uint64_t top = (uint64_t)(m >> 64) | ((uint64_t)m != 0u ? 1ull : 0ull);
        d = (double)top * m_pow2(64 - sh);
    }
    return neg ? -d : d;
}

// one Jacobi rotation of the symmetric C in the (P, Q) plane, R the third index; V's columns P and Q get the same update.  Skipped iff C[P][Q] == 0.0.
template <int P, int Q, int R> F3DS_HD void sh_rotate(double (&C)[3][3], double (&V)[3][3]) {
    const double apq = C[P][Q];
    if (apq == 0.0) return;
    const double theta = (C[Q][Q] - C[P][P]) / (2.0 * apq);
    double t = 1.0 / (m_abs(theta) + n_sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / n_sqrt(t * t + 1.0), s = t * c;
    C[P][P] -= t * apq;
    C[Q][Q] += t * apq;
    C[P][Q] = C[Q][P] = 0.0;
    const double arp = C[R][P], arq = C[R][Q];
    C[R][P] = C[P][R] = c * arp - s * arq;
    C[R][Q] = C[Q][R] = s * arp + c * arq;
    for (int k = 0; k < 3; ++k) {
        const double vp = V[k][P], vq = V[k][Q];
        V[k][P] = c * vp - s * vq;
        V[k][Q] = s * vp + c * vq;
    }
}
constexpr int SH_SWEEPS = 8;
// exactly SH_SWEEPS sweeps over (0,1), (0,2), (1,2), V = I at the start: the eigenvalues are C's diagonal afterwards, the eigenvectors V's columns
F3DS_HD void sh_jacobi(double (&C)[3][3], double (&V)[3][3]) {
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SH_SWEEPS; ++sweep) {
        sh_rotate<0, 1, 2>(C, V);
        sh_rotate<0, 2, 1>(C, V);
        sh_rotate<1, 2, 0>(C, V);
    }
}
// columns A and B = A + 1 of (lam, V) change places iff lam[A] > lam[B]: three of these sort stably, ties by column index
template <int A, int B> F3DS_HD void sh_order(double (&lam)[3], double (&V)[3][3]) {
    if (!(lam[A] > lam[B])) return;
    const double t = lam[A]; lam[A] = lam[B]; lam[B] = t;
    for (int k = 0; k < 3; ++k) { const double u = V[k][A]; V[k][A] = V[k][B]; V[k][B] = u; }
}

// the row of an accumulator.  An empty one: n_pixels = 0 and the quiet NaN 0x7FC00000 in all twenty floats.
F3DS_HD void sh_finish(const ShAcc& a, f3ds_region_shape* row) {
    f3ds_region_shape r;
    r.n_pixels = a.n;
    if (a.n == 0u) {
        const float q = m_from_bitsf(RG_QNAN);
        for (int k = 0; k < 3; ++k) r.centroid[k] = r.eigenvalue[k] = r.normal[k] = r.axis[k] = q;
        for (int k = 0; k < 6; ++k) r.cov[k] = q;
        r.plane_d = r.curvature = q;
        *row = r;
        return;
    }
    const double n = (double)a.n;
    const int64_t S[3] = {(int64_t)a.s[0], (int64_t)a.s[1], (int64_t)a.s[2]};
    double cen[3];
    for (int k = 0; k < 3; ++k) {
        cen[k] = ((double)S[k] / n) * 0.0000152587890625;      // 2^-16, exact: the table's centroid before its conversion
        r.centroid[k] = (float)cen[k];
    }
    double cov[6];
    for (int k = 0; k < 6; ++k) {
        const int ia = k < 3 ? 0 : (k < 5 ? 1 : 2), ib = k < 3 ? k : (k < 5 ? k - 2 : 2);
        const sh_i128 M = (sh_i128)(int64_t)a.s[3 + k] * (sh_i128)4294967296ll + (sh_i128)a.s[9 + k];
        const sh_i128 N = (sh_i128)(int64_t)a.n * M - (sh_i128)S[ia] * (sh_i128)S[ib];
        cov[k] = ((sh_to_double(N) / n) / n) * (1.0 / 4294967296.0);      // 2^-32, exact
        r.cov[k] = (float)cov[k];
    }
    double C[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}}, V[3][3];
    sh_jacobi(C, V);
    double lam[3] = {C[0][0], C[1][1], C[2][2]};
    for (int k = 0; k < 3; ++k) if (lam[k] < 0.0) lam[k] = 0.0;
    sh_order<0, 1>(lam, V); sh_order<1, 2>(lam, V); sh_order<0, 1>(lam, V);
    for (int k = 0; k < 3; ++k) r.eigenvalue[k] = (float)lam[k];
    // the normal: column 0 as Jacobi left it, turned towards the origin
    double v[3] = {V[0][0], V[1][0], V[2][0]};
    double d = (v[0] * cen[0] + v[1] * cen[1]) + v[2] * cen[2];
    if (d > 0.0) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; d = -d; }
    for (int k = 0; k < 3; ++k) r.normal[k] = (float)v[k];
    r.plane_d = (float)(-d);
    // the axis: column 2, its component of largest magnitude (the first of equal ones) made non-negative
    const double w[3] = {V[0][2], V[1][2], V[2][2]};
    double big = w[0];
    if (m_abs(w[1]) > m_abs(big)) big = w[1];
    if (m_abs(w[2]) > m_abs(big)) big = w[2];
    const bool flip = big < 0.0;
    for (int k = 0; k < 3; ++k) r.axis[k] = (float)(flip ? -w[k] : w[k]);
    const double sum = (lam[0] + lam[1]) + lam[2];
    r.curvature = sum > 0.0 ? (float)(lam[0] / sum) : 0.0f;
    *row = r;
}

// What both entry points refuse before they look at a pixel, as the region table: missing rows, then li_check; *use = the format they work with.
inline int sh_check(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, const f3ds_region_shape* rows, f3ds_rgbd_format* use,
                    RgbdLayout* lay) {
    if (!rows && n_regions) return F3DS_ERR_ARG;
    return li_check(fmt, depth, nullptr, labels, n_regions, use, lay);
}

}  // namespace f3ds
#endif  // F3DS_SHAPES_H_
