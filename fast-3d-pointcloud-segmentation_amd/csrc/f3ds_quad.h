// f3ds_quad.h -- device-only pieces of the merge loop's re-weighting that the micro-benchmarks time on their own (tools/ubench/ubench_math.hip):
// CIEDE2000 on the four lanes of a quad, the edge weight built on it, rgb -> Lab on three lanes, and the plane normal of a wave whose lanes hold the nine
// running sums (plane_normal_wave, with wave_pick).  Included by f3ds_kernels.inc inside its anonymous namespace, and by tests/devprobe/devprobe.hip, which
// runs every function here beside its one-lane original (f3ds_numerics.h, f3ds_algo.h) and compares the bits with a g++ build of the originals.
#ifndef F3DS_QUAD_H_
#define F3DS_QUAD_H_
// ------------------------------------------------------------------------------------------------
// CIEDE2000 spread over the four lanes of a quad (the merge loop re-weights a few dozen edges per merge
// and is otherwise idle: one lane per edge leaves the ~20 transcendental sequences of n_ciede00 in a row).
// Every sub-expression is the one of n_ciede00 (f3ds_numerics.h), on the same operands, in the same
// order -- only WHICH lane evaluates it changes: the two atan2 run side by side in lanes 0/1, the four
// cosines of T in lanes 0..3, sin(dh'/2) beside sin(2 dtheta), the three later square roots together.
// All four lanes must be active and hold the same lab1 / lab2; all return the same result.
// ------------------------------------------------------------------------------------------------
// the f64 constants of f3ds_math.h / n_ciede00 read from a copy of M_TABLE in LDS (see f3ds_math.h "where the f64 constants come from")
struct m_lds {
    __attribute__((address_space(3))) const double* t;
    __device__ __forceinline__ double operator()(int i) const { return t[i]; }
};
// A provider whose table address the compiler cannot see through: the loads behind it stay where the arithmetic is.  (The table never changes, so with a plain pointer
// every constant is loop-invariant and is hoisted out of the merge loop: ~100 VGPRs held for good, the loop's own state spilled to scratch.)
__device__ __forceinline__ m_lds m_lds_here(const double* tab) {
    __attribute__((address_space(3))) const double* p = (__attribute__((address_space(3))) const double*)tab;
    asm volatile("" : "+v"(p));
    return m_lds{p};
}
template <int K>
__device__ inline double quad_bcast(double x) {
    constexpr int ctrl = K | (K << 2) | (K << 4) | (K << 6);          // quad_perm [K,K,K,K]
    const long long b = __builtin_bit_cast(long long, x);
    const int lo = __builtin_amdgcn_mov_dpp((int)(b & 0xFFFFFFFFll), ctrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), ctrl, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}
template <int K>
__device__ inline float quad_bcastf(float x) {
    constexpr int ctrl = K | (K << 2) | (K << 4) | (K << 6);
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), ctrl, 0xF, 0xF, true));
}
// (n_ciede00_quad_sq: the radicand in double, as n_ciede00_sq)
template <class MC = m_lit>
__device__ inline double n_ciede00_quad_sq(const float lab1[3], const float lab2[3], int q, MC mc = MC()) {
    const double PI = mc(MC_CIE_PI), TWO_PI = mc(MC_CIE_2PI);
    const double P25_7 = mc(MC_CIE_25_7);
    const float L1 = lab1[0], a1 = lab1[1], b1 = lab1[2];
    const float L2 = lab2[0], a2 = lab2[1], b2 = lab2[2];
    // lanes 0 / 1 carry colour 1 / colour 2 through the per-colour chain (lanes 2, 3 repeat colour 2)
    const float am = q == 0 ? a1 : a2, bm = q == 0 ? b1 : b2;
    const float cabf = n_sqrtf(am * am + bm * bm);
    const double Cab1 = (double)quad_bcastf<0>(cabf), Cab2 = (double)quad_bcastf<1>(cabf);
    const double Cab = (Cab1 + Cab2) / 2.0;
    const double Cab7 = n_pow7(Cab);
    const double G = 0.5 * (1.0 - n_sqrt(Cab7 / (Cab7 + P25_7)));
    const double apm = (1.0 + G) * (double)am;
    const double Cpm = n_sqrt(apm * apm + (double)(bm * bm));
    double hpm = m_atan2((double)bm, apm, mc);      // (evaluated for every lane, selected: no branch around it)
    hpm = hpm < 0 ? hpm + TWO_PI : hpm;
    hpm = (m_abs(apm) + (double)m_absf(bm)) != 0.0 ? hpm : 0.0;
    const double Cp1 = quad_bcast<0>(Cpm), Cp2 = quad_bcast<1>(Cpm);
    const double hp1 = quad_bcast<0>(hpm), hp2 = quad_bcast<1>(hpm);
    const double Cp_prod = Cp2 * Cp1;
    const double dL = (double)(L2 - L1);
    const double dC = Cp2 - Cp1;
    double dhp = hp2 - hp1;
    if (dhp > PI) dhp -= TWO_PI;
    else if (dhp < -PI) dhp += TWO_PI;
    if (Cp_prod == 0.0) dhp = 0.0;
    const double Lp = (double)(L2 + L1) / 2.0;
    const double Cp = (Cp1 + Cp2) / 2.0;
    double hp = (hp1 + hp2) / 2.0;
    if (m_abs(hp1 - hp2) > PI) hp -= PI;
    if (hp < 0) hp += TWO_PI;
    if (Cp_prod == 0.0) hp = hp1 + hp2;
    const double Lpm502 = (Lp - mc(MC_CIE_50)) * (Lp - mc(MC_CIE_50));
    // the four cosines of T, one per lane
    const double carg = q == 0 ? hp - mc(MC_CIE_PI_6) : (q == 1 ? 2.0 * hp : (q == 2 ? mc(MC_CIE_3) * hp + mc(MC_CIE_PI_30) : 4.0 * hp - mc(MC_CIE_63PI_180)));
    const double cq = m_cos(carg, mc);
    const double T = 1.0 - mc(MC_CIE_017) * quad_bcast<0>(cq) + mc(MC_CIE_024) * quad_bcast<1>(cq) + mc(MC_CIE_032) * quad_bcast<2>(cq) - mc(MC_CIE_020) * quad_bcast<3>(cq);
    const double e = (mc(MC_CIE_180_PI) * hp - mc(MC_CIE_275)) / mc(MC_CIE_25);
    const double dtheta = mc(MC_CIE_30PI_180) * m_exp(-(e * e), mc);
    const double Cp7 = n_pow7(Cp);
    // sqrt(Cp_prod) | sqrt(Cp7 / (Cp7 + 25^7)) | sqrt(20 + (Lp - 50)^2) in lanes 0 | 1 | 2
    const double sarg = q == 0 ? Cp_prod : (q == 1 ? Cp7 / (Cp7 + P25_7) : mc(MC_CIE_20) + Lpm502);
    const double sq = n_sqrt(sarg);
    // sin(dh'/2) | sin(2 dtheta) in lanes 0 | 1
    const double sn = m_sin(q == 0 ? dhp / 2.0 : 2.0 * dtheta, mc);
    const double dH = 2.0 * quad_bcast<0>(sq) * quad_bcast<0>(sn);
    const double Rc = 2.0 * quad_bcast<1>(sq);
    const double kLSL = 1.0 * (1.0 + mc(MC_CIE_0015) * Lpm502 / quad_bcast<2>(sq));
    const double kLSC = 1.0 * (1.0 + mc(MC_CIE_0045) * Cp);
    const double kHSH = 1.0 * (1.0 + mc(MC_CIE_0015) * Cp * T);
    const double RT = -quad_bcast<1>(sn) * Rc;
    const double tL = dL / kLSL, tC = dC / kLSC, tH = dH / kHSH;
    return tL * tL + tC * tC + tH * tH + RT * tC * tH;
}
template <class MC = m_lit>
__device__ inline float n_ciede00_quad(const float lab1[3], const float lab2[3], int q, MC mc = MC()) {
    return (float)n_sqrt(n_ciede00_quad_sq(lab1, lab2, q, mc));
}
// a_edge_weight with the quad version of the colour distance (LAB_CIEDE00 only)
template <class MC = m_lit>
__device__ inline float edge_weight_quad(const MergeParams& p, const float* r1, const float* r2, int q, int* err, MC mc = MC()) {
    const float dc = n_ciede00_quad(r1 + 9, r2 + 9, q, mc) / F3DS_LAB_RANGE;
    float dg = n_normals_diff(r1 + 3, r1, r2 + 3, r2);
    if (p.geom_metric == 1 && n_is_convex(r1 + 3, r1, r2 + 3, r2)) dg *= 0.5;
    return a_tc(p, dc, err) + a_tg(p, dg, err);
}
// n_rgb2lab (f3ds_numerics.h) for a wave whose lane k < 3 holds the mean of colour channel k in `mine` (the other lanes repeat channel 2): the three gamma
// curves and the three cube roots are evaluated side by side, everything else as there.  Every lane returns L, a, b.
// Gamma curve and cube root are evaluated for every lane and the linear pieces selected afterwards (same values: no branch, no divergence between the three lanes).
// (base: the first of the three lanes -- 0 for a wave, 16 r for row r of a wave that holds four colours, one per row; `lane` counts from it)
template <class MC = m_lit>
__device__ inline void lab_three_lanes(float mine, int lane, float lab[3], MC mc = MC(), int base = 0) {
    const float v = mine / 255;
    const float gam = (float)m_pow_pos((double)((v + 0.055f) / 1.055f), mc(MC_GAMMA_EXP), mc);
    const float cl = v <= 0.04045f ? v / 12.92f : gam;
    const float c0 = __shfl(cl, base, 64), c1 = __shfl(cl, base + 1, 64), c2 = __shfl(cl, base + 2, 64);
    const float X = (c0 * 0.412453f + c1 * 0.357580f + c2 * 0.180423f) / 0.950456f;
    const float Y = (c0 * 0.212671f + c1 * 0.715160f + c2 * 0.072169f);
    const float Z = (c0 * 0.019334f + c1 * 0.119193f + c2 * 0.950227f) / 1.088754f;
    const float t = lane == 0 ? X : (lane == 1 ? Y : Z);
    const float cb = (float)m_cbrt_pos((double)t, mc);
    const float fl = t > 0.008856f ? cb : 7.787f * t + 16.0f / 116.0f;          // n_lab_f
    const float fx = __shfl(fl, base, 64), fy = __shfl(fl, base + 1, 64), fz = __shfl(fl, base + 2, 64);
    lab[0] = Y > 0.008856f ? 116.0f * fy - 16.0f : 903.3f * Y;
    lab[1] = 500.0f * (fx - fy);
    lab[2] = 200.0f * (fy - fz);
}
// n_plane_normal (f3ds_numerics.h) for a whole wave whose lane k < 9 holds raw sum k: the same operations on the same values, but the
// 21 IEEE divisions (64 cycles each on one lane after the other) are taken side by side: lane k divides sum k by the count, lanes 0..5 the
// covariance entries by the scale, lanes 0..2 the eigenvector and the final normal by their lengths.  count >= 3 (the caller keeps the
// generic function for less).  cen = the centroid (sums 6..8 over the count: the same quotients).
__device__ inline float wave_pick(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
template <class MC>
__device__ inline void plane_normal_wave(float acc, unsigned count, int lane, float cen[3], float out[4], MC mc) {
    const float cnt = (float)count;
    const float qa = acc / cnt;
    float a[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = wave_pick(qa, k);
    cen[0] = a[6]; cen[1] = a[7]; cen[2] = a[8];
    const float c00 = a[0] - a[6] * a[6], c01 = a[1] - a[6] * a[7], c02 = a[2] - a[6] * a[8];
    const float c11 = a[3] - a[7] * a[7], c12 = a[4] - a[7] * a[8], c22 = a[5] - a[8] * a[8];
    float scale = m_absf(c00);
    float t;
    t = m_absf(c01); if (t > scale) scale = t;
    t = m_absf(c02); if (t > scale) scale = t;
    t = m_absf(c11); if (t > scale) scale = t;
    t = m_absf(c12); if (t > scale) scale = t;
    t = m_absf(c22); if (t > scale) scale = t;
    if (scale <= F3DS_FLT_MIN) scale = 1.0f;
    const float cm = lane == 0 ? c00 : (lane == 1 ? c01 : (lane == 2 ? c02 : (lane == 3 ? c11 : (lane == 4 ? c12 : c22))));
    const float qm = cm / scale;
    float m00 = wave_pick(qm, 0), m01 = wave_pick(qm, 1), m02 = wave_pick(qm, 2), m11 = wave_pick(qm, 3), m12 = wave_pick(qm, 4), m22 = wave_pick(qm, 5);
    float r[3];
    n_roots(m00, m01, m02, m11, m12, m22, r, mc);
    m00 -= r[0]; m11 -= r[0]; m22 -= r[0];
    float v1[3], v2[3], v3[3];
    n_cross(m00, m01, m02, m01, m11, m12, v1);      // row0 x row1
    n_cross(m00, m01, m02, m02, m12, m22, v2);      // row0 x row2
    n_cross(m01, m11, m12, m02, m12, m22, v3);      // row1 x row2
    const float l1 = n_sum3(v1[0] * v1[0], v1[1] * v1[1], v1[2] * v1[2]);
    const float l2 = n_sum3(v2[0] * v2[0], v2[1] * v2[1], v2[2] * v2[2]);
    const float l3 = n_sum3(v3[0] * v3[0], v3[1] * v3[1], v3[2] * v3[2]);
    float v[3], l;
    if (l1 >= l2 && l1 >= l3) { v[0] = v1[0]; v[1] = v1[1]; v[2] = v1[2]; l = l1; }
    else if (l2 >= l1 && l2 >= l3) { v[0] = v2[0]; v[1] = v2[1]; v[2] = v2[2]; l = l2; }
    else { v[0] = v3[0]; v[1] = v3[1]; v[2] = v3[2]; l = l3; }
    const float sl = n_sqrtf(l);
    const float qn = (lane == 0 ? v[0] : (lane == 1 ? v[1] : v[2])) / sl;
    float nx = wave_pick(qn, 0), ny = wave_pick(qn, 1), nz = wave_pick(qn, 2);
    const float nw = -1.0f * ((nx * a[6] + ny * a[7]) + (nz * a[8] + 0.0f * 1.0f));
    const float cos_theta = ((0.0f - cen[0]) * nx + (0.0f - cen[1]) * ny) + ((0.0f - cen[2]) * nz + 0.0f * nw);
    if (cos_theta < 0.0f) { nx *= -1.0f; ny *= -1.0f; nz *= -1.0f; }
    const float z = (nx * nx + ny * ny) + (nz * nz + 0.0f);
    if (z > 0.0f) {
        const float sz = n_sqrtf(z);
        const float qz = (lane == 0 ? nx : (lane == 1 ? ny : nz)) / sz;
        nx = wave_pick(qz, 0); ny = wave_pick(qz, 1); nz = wave_pick(qz, 2);
    }
    out[0] = nx; out[1] = ny; out[2] = nz; out[3] = 0.0f;
}
#endif  // F3DS_QUAD_H_
