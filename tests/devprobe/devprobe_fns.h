// devprobe_fns.h -- one dispatch table over the one-lane per-element functions of csrc/f3ds_math.h, f3ds_numerics.h, f3ds_algo.h and
// f3ds_eval_levels.h (test infrastructure only).  devprobe_host.cpp compiles it with g++ and the flags of tests/emul (the reference side),
// devprobe.hip with hipcc and the product's own flags for gfx950; tests/test_devprobe_gpu.py compares the two bit for bit.
//
// A row is NI 32-bit words in and NO words out (dp_shape).  Floats and unsigned integers travel as their bits, a double as two words (low word
// first).  fn + DP_TABLE evaluates the same function with its f64 constants read from a copy of the table (m_tab on the host, m_lds over an LDS
// copy on the device) instead of literals.
#ifndef F3DS_DEVPROBE_FNS_H_
#define F3DS_DEVPROBE_FNS_H_

#include "../../fast-3d-pointcloud-segmentation_amd/csrc/f3ds_algo.h"
#include "../../fast-3d-pointcloud-segmentation_amd/csrc/f3ds_eval_levels.h"

namespace f3ds {

enum {
    // 0..10: the ids of f3ds_oracle_math (exp log sin cos atan2 cbrt pow logf atan2f cosf sinf): in a, b (doubles) -> one double
    DP_TRANSFORM = 11,       // x y z use_transform -> x y z
    DP_POINT_KEY = 12,       // mn[3] mx[3] voxel_res x y z use_transform -> key[3] depth max_key error min[3] max[3] (doubles)
    DP_MORTON = 13,          // x y z depth -> n_morton (2 words) n_demorton of it (3) n_pack_key (2)
    DP_PLANE_NORMAL = 14,    // accu[9] count view_point[3] -> normal[4]
    DP_VOXEL_DISTANCE = 15,  // c[9] v[9] seed_res w_normal w_color w_spatial -> distance
    DP_RGB2LAB = 16,         // rgb[3] -> lab[3]
    DP_CIEDE00 = 17,         // lab1[3] lab2[3] -> distance
    DP_RGB_EUCL = 18,        // a[3] b[3] -> distance
    DP_NORMALS_DIFF = 19,    // n1[3] c1[3] n2[3] c2[3] -> value
    DP_IS_CONVEX = 20,       // n1[3] c1[3] n2[3] c2[3] -> 0 / 1
    DP_DELTA_C_G = 21,       // r1[12] r2[12] color_metric geom_metric -> dc dg
    DP_WEIGHT_KEY = 22,      // w -> key
    DP_FOLD = 23,            // n (<= DP_FOLD_MAX) then n feature rows of 6 (xyz rgb) -> acc[12]: a_payload_row + a_fold_row in list order
    DP_REGION_FROM_ACC = 24, // acc[12] count -> rec[16]
    DP_TC = 25,              // merging lambda bins d cdf[DP_CDF] -> value err
    DP_TG = 26,              // the same for a_tg
    DP_EDGE_WEIGHT = 27,     // r1[12] r2[12] color_metric geom_metric merging lambda bins cdf_c[DP_CDF] cdf_g[DP_CDF] -> weight err
    DP_NORMAL_CEN = 28,      // accu[9] count -> normal[4] centroid[3]: n_plane_normal with the centroid as view point (what plane_normal_wave restates)
    DP_CIEDE00_SQ = 29,      // lab1[3] lab2[3] -> n_ciede00_sq, the radicand of n_ciede00 before the rounding to float (a double)
    DP_COUNT = 30,
    DP_TABLE = 100
};
#define DP_CDF 8
#define DP_FOLD_MAX 8

F3DS_HD float dp_f(uint32_t w) { return m_from_bitsf(w); }
F3DS_HD double dp_d(const uint32_t* w) { return m_from_bits((uint64_t)w[0] | ((uint64_t)w[1] << 32)); }
F3DS_HD void dp_put_d(uint32_t* o, double v) { const uint64_t u = m_bits(v); o[0] = (uint32_t)u; o[1] = (uint32_t)(u >> 32); }
F3DS_HD void dp_floats(const uint32_t* in, float* f, int n) { for (int k = 0; k < n; ++k) f[k] = dp_f(in[k]); }
F3DS_HD void dp_put_floats(uint32_t* out, const float* f, int n) { for (int k = 0; k < n; ++k) out[k] = m_bitsf(f[k]); }

F3DS_HD bool dp_shape(int fn, int* ni, int* no) {
    if (fn >= DP_TABLE) fn -= DP_TABLE;
    if (fn >= 0 && fn <= 10) { *ni = 4; *no = 2; return true; }
    switch (fn) {
        case DP_TRANSFORM: *ni = 4; *no = 3; return true;
        case DP_POINT_KEY: *ni = 11; *no = 18; return true;
        case DP_MORTON: *ni = 4; *no = 7; return true;
        case DP_PLANE_NORMAL: *ni = 13; *no = 4; return true;
        case DP_VOXEL_DISTANCE: *ni = 22; *no = 1; return true;
        case DP_RGB2LAB: *ni = 3; *no = 3; return true;
        case DP_CIEDE00: *ni = 6; *no = 1; return true;
        case DP_RGB_EUCL: *ni = 6; *no = 1; return true;
        case DP_CIEDE00_SQ: *ni = 6; *no = 2; return true;
        case DP_NORMALS_DIFF: *ni = 12; *no = 1; return true;
        case DP_IS_CONVEX: *ni = 12; *no = 1; return true;
        case DP_DELTA_C_G: *ni = 26; *no = 2; return true;
        case DP_WEIGHT_KEY: *ni = 1; *no = 1; return true;
        case DP_FOLD: *ni = 1 + 6 * DP_FOLD_MAX; *no = 12; return true;
        case DP_REGION_FROM_ACC: *ni = 13; *no = 16; return true;
        case DP_TC: case DP_TG: *ni = 4 + DP_CDF; *no = 2; return true;
        case DP_EDGE_WEIGHT: *ni = 29 + 2 * DP_CDF; *no = 2; return true;
        case DP_NORMAL_CEN: *ni = 10; *no = 7; return true;
    }
    return false;
}

// MergeParams of a DP_TC / DP_TG / DP_EDGE_WEIGHT row: in = merging lambda bins; the cdf tables are the caller's float copies
F3DS_HD MergeParams dp_merge_params(const uint32_t* in, int color_metric, int geom_metric, const float* cdf_c, const float* cdf_g) {
    MergeParams p;
    p.color_metric = color_metric; p.geom_metric = geom_metric; p.merging = (int)in[0]; p.lambda = dp_f(in[1]);
    p.bins = (int)in[2] > DP_CDF ? DP_CDF : (int)in[2];          // (the row carries DP_CDF table entries)
    p.cdf_c = cdf_c; p.cdf_g = cdf_g;
    return p;
}

template <class K> F3DS_HD double dp_math(int fn, double a, double b, K mc) {
    switch (fn) {
        case 0: return m_exp(a, mc);
        case 1: return m_log(a, mc);
        case 2: return m_sin(a, mc);
        case 3: return m_cos(a, mc);
        case 4: return m_atan2(a, b, mc);
        case 5: return m_cbrt_pos(a, mc);
        case 6: return m_pow_pos(a, b, mc);
        case 7: return (double)m_logf((float)a, mc);
        case 8: return (double)m_atan2f((float)a, (float)b, mc);
        case 9: return (double)m_cosf((float)a, mc);
        case 10: return (double)m_sinf((float)a, mc);
    }
    return 0.0;
}

// one row of function fn (0 <= fn < DP_COUNT); mc = the provider of the f64 constants for the functions that take one
template <class K> F3DS_HD void dp_eval(int fn, const uint32_t* in, uint32_t* out, K mc) {
    if (fn <= 10) { dp_put_d(out, dp_math(fn, dp_d(in), dp_d(in + 2), mc)); return; }
    switch (fn) {
        case DP_TRANSFORM: {
            float x = dp_f(in[0]), y = dp_f(in[1]), z = dp_f(in[2]);
            n_transform(x, y, z, (int)in[3]);
            out[0] = m_bitsf(x); out[1] = m_bitsf(y); out[2] = m_bitsf(z);
        } break;
        case DP_POINT_KEY: {
            float f[10]; dp_floats(in, f, 10);
            GridInfo g;
            n_grid_from_bbox(f, f + 3, f[6], g);
            unsigned key[3] = {0u, 0u, 0u};
            if (!g.error) n_point_key(g, f[7], f[8], f[9], (int)in[10], key);
            out[0] = key[0]; out[1] = key[1]; out[2] = key[2];
            out[3] = (uint32_t)g.depth; out[4] = g.max_key; out[5] = (uint32_t)g.error;
            for (int a = 0; a < 3; ++a) { dp_put_d(out + 6 + 2 * a, g.min[a]); dp_put_d(out + 12 + 2 * a, g.max[a]); }
        } break;
        case DP_MORTON: {
            const int depth = in[3] > 21u ? 21 : (int)in[3];          // (the deepest tree n_key_bit_size accepts)
            const uint64_t c = n_morton(in[0], in[1], in[2], depth);
            unsigned key[3];
            n_demorton(c, depth, key);
            const uint64_t p = n_pack_key(in[0], in[1], in[2]);
            out[0] = (uint32_t)c; out[1] = (uint32_t)(c >> 32); out[2] = key[0]; out[3] = key[1]; out[4] = key[2];
            out[5] = (uint32_t)p; out[6] = (uint32_t)(p >> 32);
        } break;
        case DP_PLANE_NORMAL: {
            float a[9], vp[3], n4[4];
            dp_floats(in, a, 9); dp_floats(in + 10, vp, 3);
            n_plane_normal(a, in[9], vp, n4);
            dp_put_floats(out, n4, 4);
        } break;
        case DP_NORMAL_CEN: {
            float a[9], cen[3], n4[4];
            dp_floats(in, a, 9);
            const float cnt = (float)in[9];
            cen[0] = a[6] / cnt; cen[1] = a[7] / cnt; cen[2] = a[8] / cnt;
            n_plane_normal(a, in[9], cen, n4);
            dp_put_floats(out, n4, 4); dp_put_floats(out + 4, cen, 3);
        } break;
        case DP_VOXEL_DISTANCE: {
            float f[22]; dp_floats(in, f, 22);
            out[0] = m_bitsf(n_voxel_distance(f, f + 9, f[18], f[19], f[20], f[21]));
        } break;
        case DP_RGB2LAB: {
            float rgb[3], lab[3]; dp_floats(in, rgb, 3);
            n_rgb2lab(rgb, lab);
            dp_put_floats(out, lab, 3);
        } break;
        case DP_CIEDE00: {
            float f[6]; dp_floats(in, f, 6);
            out[0] = m_bitsf(n_ciede00(f, f + 3, mc));
        } break;
        case DP_CIEDE00_SQ: {
            float f[6]; dp_floats(in, f, 6);
            dp_put_d(out, n_ciede00_sq(f, f + 3, mc));
        } break;
        case DP_RGB_EUCL: {
            float f[6]; dp_floats(in, f, 6);
            out[0] = m_bitsf(n_rgb_eucl(f, f + 3));
        } break;
        case DP_NORMALS_DIFF: {
            float f[12]; dp_floats(in, f, 12);
            out[0] = m_bitsf(n_normals_diff(f, f + 3, f + 6, f + 9));
        } break;
        case DP_IS_CONVEX: {
            float f[12]; dp_floats(in, f, 12);
            out[0] = n_is_convex(f, f + 3, f + 6, f + 9) ? 1u : 0u;
        } break;
        case DP_DELTA_C_G: {
            float f[24], dc, dg; dp_floats(in, f, 24);
            n_delta_c_g(f, f + 12, (int)in[24], (int)in[25], &dc, &dg, mc);
            out[0] = m_bitsf(dc); out[1] = m_bitsf(dg);
        } break;
        case DP_WEIGHT_KEY: out[0] = n_weight_key(dp_f(in[0])); break;
        case DP_FOLD: {
            float acc[12];
            for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
            const uint32_t n = in[0] < (uint32_t)DP_FOLD_MAX ? in[0] : (uint32_t)DP_FOLD_MAX;
            for (uint32_t i = 0; i < n; ++i) {
                float vf[6], row[12];
                dp_floats(in + 1 + 6 * i, vf, 6);
                a_payload_row(vf, row);
                a_fold_row(acc, row, i + 1u);
            }
            dp_put_floats(out, acc, 12);
        } break;
        case DP_REGION_FROM_ACC: {
            float acc[12], rec[16]; dp_floats(in, acc, 12);
            a_region_from_acc(acc, in[12], rec);
            dp_put_floats(out, rec, 16);
        } break;
        case DP_TC: case DP_TG: {
            float cdf[DP_CDF]; dp_floats(in + 4, cdf, DP_CDF);
            const MergeParams p = dp_merge_params(in, 0, 0, cdf, cdf);
            int err = 0;
            const float v = fn == DP_TC ? a_tc(p, dp_f(in[3]), &err) : a_tg(p, dp_f(in[3]), &err);
            out[0] = m_bitsf(v); out[1] = (uint32_t)err;
        } break;
        case DP_EDGE_WEIGHT: {
            float f[24], cc[DP_CDF], cg[DP_CDF];
            dp_floats(in, f, 24); dp_floats(in + 29, cc, DP_CDF); dp_floats(in + 29 + DP_CDF, cg, DP_CDF);
            const MergeParams p = dp_merge_params(in + 26, (int)in[24], (int)in[25], cc, cg);
            int err = 0;
            const float w = a_edge_weight(p, f, f + 12, &err, mc);
            out[0] = m_bitsf(w); out[1] = (uint32_t)err;
        } break;
    }
}

// ---- evl_scores<evl_m_logf> with evl_visit_order / evl_match_column on one CSR table -------------------------------------------------------
// dims = {K, M, N, offset of the table's K-sized arrays, of its M-sized arrays, of its roff (K + 1 words), of its entries, 0}; the arrays of all
// tables are concatenated.  Scratch (same offsets): visited / order / match / in are M-sized, used / ci / cc K-sized.  A column's entries are
// gathered from the CSR rows in descending row order (evl_match_column takes them in any order).  out = the seven scores.  Every loop is bounded
// by the K, M and entry count passed in.
struct DpEvlArrays {
    const uint32_t* dims; const uint32_t* ssize; const uint32_t* tsize; const uint32_t* roff; const uint32_t* col; const uint32_t* cnt;
    unsigned char* visited; unsigned char* used; uint32_t* order; uint32_t* match; uint32_t* in; uint32_t* ci; uint32_t* cc;
    uint32_t* out;
};
F3DS_HD void dp_evl_one(const DpEvlArrays& A, uint32_t t) {
    const uint32_t* d = A.dims + 8 * (size_t)t;
    const uint32_t K = d[0], M = d[1], N = d[2];
    const uint32_t* ssize = A.ssize + d[3]; const uint32_t* tsize = A.tsize + d[4]; const uint32_t* roff = A.roff + d[5];
    const uint32_t* col = A.col + d[6]; const uint32_t* cnt = A.cnt + d[6];
    unsigned char* visited = A.visited + d[4]; unsigned char* used = A.used + d[3];
    uint32_t* order = A.order + d[4]; uint32_t* match = A.match + d[4]; uint32_t* in = A.in + d[4];
    uint32_t* ci = A.ci + d[3]; uint32_t* cc = A.cc + d[3];
    for (uint32_t i = 0; i < K; ++i) used[i] = 0;
    for (uint32_t j = 0; j < M; ++j) { match[j] = EVL_UNMATCHED; in[j] = 0u; }
    const uint32_t nv = evl_visit_order(M, tsize, visited, order);
    for (uint32_t v = 0; v < nv && v < M; ++v) {
        const uint32_t j = order[v];
        uint32_t n = 0;
        for (uint32_t i = K; i-- > 0;)
            for (uint32_t e = roff[i]; e < roff[i + 1]; ++e)
                if (col[e] == j && n < K) { ci[n] = i; cc[n] = cnt[e]; ++n; }
        const uint32_t row = evl_match_column(ci, cc, n, used, &in[j]);
        match[j] = row;
        if (row != EVL_UNMATCHED) used[row] = 1;
    }
    const f3ds_performance r = evl_scores(K, ssize, M, tsize, roff, col, cnt, match, in, N, evl_m_logf());
    const float f[7] = {r.voi, r.precision, r.recall, r.fscore, r.wov, r.fpr, r.fnr};
    dp_put_floats(A.out + 7 * (size_t)t, f, 7);
}

}  // namespace f3ds
#endif  // F3DS_DEVPROBE_FNS_H_
