// f3ds_eval_levels.h -- the scoring rules of f3ds_evaluate over a SPARSE contingency table, as F3DS_HD code: the building block for
// scoring many hierarchy levels (f3ds_labels_at_thresholds) without one dense K x M table per level.  The device
// scorer behind f3ds_evaluate_levels (f3ds_eval_levels.inc) is built from it: its kernels call the functions below
// or cite the one they parallelise.  tests/eval_levels_harness/ (tests/test_eval_levels_cpu.py) checks it against f3ds_scores_from_table;
// tests/devprobe/devprobe.hip compiles it with hipcc for gfx950 and tests/test_devprobe_gpu.py::test_evl_scores_on_the_device compares
// all seven scores with the g++ build, bit for bit.
//
// They are the rules of f3ds_scores_from_table (f3ds_eval.h, Testing::eval_performance, the reference's src/testing.cpp:88-136,
// 239-406) restated for a table that holds only its non-zero entries:
//   table    K rows (segments, ids 0..K-1) x M columns (truth labels); the entries (i, j, count > 0) in (i ascending, j ascending)
//            order as CSR: row i's entries are col[roff[i] .. roff[i+1]) / cnt[...], columns ascending.  ssize[i] / tsize[j] are the
//            cloud sizes, N the voxel count of the frame.
//   visit    truth labels by descending size; of labels of equal size only the lowest j is visited (std::map::insert keeps the first,
//            testing.cpp:97-100), the others stay unmatched.
//   match    a visited label j takes, among the rows of its non-zero entries that are not used yet, the one with the largest count
//            (the lowest row among equal counts); if all of them are used it stays unmatched.  A label without any non-zero entry takes
//            row 0 when row 0 is unused (the argmax of an all-zero column) and stays unmatched otherwise.
//   sums     h_s over rows ascending, h_t over labels ascending, mi over the entries in (i, j) order, then p, r, fp, fn, w over labels
//            ascending: the expressions of f3ds_scores_from_table, term for term (-ffp-contract=off on both compilers).
// The logarithm is a template parameter: device code takes f3ds::m_logf (evl_m_logf: the same bits from g++ and hipcc, whereas libm and
// ocml differ in the last bit); the harness also runs the routine with std::log, where all seven scores equal f3ds_scores_from_table
// bit for bit.
#ifndef F3DS_EVAL_LEVELS_H_
#define F3DS_EVAL_LEVELS_H_

#include "f3ds_math.h"
#include "../../include/f3ds.h"

namespace f3ds {

constexpr uint32_t EVL_UNMATCHED = 0xFFFFFFFFu;

struct evl_m_logf {
    F3DS_HD float operator()(float x) const { return m_logf(x); }
};

// is entry (count c, row i) a better match than (cb, ib)?  the larger count, then the lower row (the first maximum of the column)
F3DS_HD bool evl_better(uint32_t c, uint32_t i, uint32_t cb, uint32_t ib) { return c > cb || (c == cb && i < ib); }
// is label j visited?  (no lower label has its size)
F3DS_HD bool evl_visited(const uint32_t* tsize, uint32_t j) {
    for (uint32_t q = 0; q < j; ++q) if (tsize[q] == tsize[j]) return false;
    return true;
}
// the visiting order: order[0 .. return value) = the visited labels by descending size.  visited[0 .. M) is scratch: the flags are
// computed once, then each visited label's position is the count of visited labels of larger size -- O(M^2) in all, and both passes
// are independent per label (one thread per label on the device; the order is per frame, not per level: tsize does not change).
F3DS_HD uint32_t evl_visit_order(uint32_t M, const uint32_t* tsize, unsigned char* visited, uint32_t* order) {
    for (uint32_t j = 0; j < M; ++j) visited[j] = evl_visited(tsize, j) ? 1 : 0;
    uint32_t n = 0;
    for (uint32_t j = 0; j < M; ++j) {
        if (!visited[j]) continue;
        uint32_t pos = 0;
        for (uint32_t q = 0; q < M; ++q) pos += (visited[q] && tsize[q] > tsize[j]) ? 1u : 0u;
        order[pos] = j; ++n;
    }
    return n;
}
// The same order by sorting, for the host: the labels by (size descending, label ascending), of every run of equal sizes the first.  O(M log M).
// rank[k] (may be NULL) = the position of order[k] among the visited labels in ascending label order: the device scorer stores a label's match
// there, so that its sums over the matched labels run in evl_scores' order (labels ascending).
inline uint32_t evl_visit_order_sorted(uint32_t M, const uint32_t* tsize, uint32_t* order, uint32_t* rank) {
    uint32_t* all = new uint32_t[M ? M : 1];
    for (uint32_t j = 0; j < M; ++j) all[j] = j;
    // (a merge sort written out: the header takes nothing from <algorithm>, device builds include it too)
    struct cmp { const uint32_t* t; bool operator()(uint32_t a, uint32_t b) const { return t[a] > t[b] || (t[a] == t[b] && a < b); } } less{tsize};
    for (uint32_t width = 1; width < M; width *= 2) {      // bottom-up merge sort
        uint32_t* tmp = new uint32_t[M];
        for (uint32_t lo = 0; lo < M; lo += 2 * width) {
            const uint32_t mid = lo + width < M ? lo + width : M, hi = lo + 2 * width < M ? lo + 2 * width : M;
            uint32_t a = lo, b = mid, o = lo;
            while (a < mid && b < hi) tmp[o++] = less(all[b], all[a]) ? all[b++] : all[a++];
            while (a < mid) tmp[o++] = all[a++];
            while (b < hi) tmp[o++] = all[b++];
        }
        delete[] all; all = tmp;
    }
    uint32_t n = 0;
    for (uint32_t k = 0; k < M; ++k) if (k == 0 || tsize[all[k]] != tsize[all[k - 1]]) order[n++] = all[k];
    delete[] all;
    if (rank)
        for (uint32_t k = 0; k < n; ++k) { uint32_t r = 0; for (uint32_t q = 0; q < n; ++q) r += order[q] < order[k] ? 1u : 0u; rank[k] = r; }
    return n;
}
// the match of one visited label over its column (entries (row ci[e], count cc[e]), e < n, in any order): the row, or EVL_UNMATCHED;
// *in receives the matched entry's count (0 for the empty-column match of row 0)
F3DS_HD uint32_t evl_match_column(const uint32_t* ci, const uint32_t* cc, uint32_t n, const unsigned char* used, uint32_t* in) {
    *in = 0;
    if (n == 0) return used[0] ? EVL_UNMATCHED : 0u;
    uint32_t best = EVL_UNMATCHED, bc = 0;
    for (uint32_t e = 0; e < n; ++e)
        if (!used[ci[e]] && (best == EVL_UNMATCHED || evl_better(cc[e], ci[e], bc, best))) { best = ci[e]; bc = cc[e]; }
    *in = best == EVL_UNMATCHED ? 0u : bc;
    return best;
}

// the terms of the three entropy sums: evl_scores adds them in its own order; the device scorer computes them lane-parallel and adds them in that order
template <class LogF> F3DS_HD float evl_entropy_term(float x, float N, LogF lg) { return lg(x / N) * x / N; }
template <class LogF> F3DS_HD float evl_mi_term(float N, float r, float p, float q, LogF lg) { return lg((N * r) / (p * q)) * r / N; }
// the two non-integer terms of a matched label (precision, weighted overlap); in, g, s as in evl_scores
F3DS_HD float evl_p_term(float inj, float g, float s) { return inj * g / s; }
F3DS_HD float evl_w_term(float inj, float g, uint32_t ssize_i, uint32_t tsize_j, uint32_t in_j) { const float un = (float)(ssize_i + tsize_j - in_j); return inj * g / un; }
// the last step of evl_scores: the seven fields from the finished sums
F3DS_HD f3ds_performance evl_finish(float h_s, float h_t, float mi, float p, float r, float fp, float fn, float w, float N) {
    f3ds_performance out;
    out.voi = h_s + h_t - 2 * mi;
    out.precision = p / N; out.recall = r / N; out.fpr = fp / N; out.fnr = fn / N;
    out.fscore = (out.precision == 0 && out.recall == 0) ? 0.0f : 2 * (out.precision * out.recall) / (out.precision + out.recall);
    out.wov = w / N;
    return out;
}

// The seven scores from the sparse table and a matching (match[j] = row or EVL_UNMATCHED, in[j] = the matched entry's count).
// Term for term f3ds_scores_from_table; the caller guarantees K >= 1 and M >= 1.
template <class LogF>
F3DS_HD f3ds_performance evl_scores(uint32_t K, const uint32_t* ssize, uint32_t M, const uint32_t* tsize, const uint32_t* roff, const uint32_t* col,
                                    const uint32_t* cnt, const uint32_t* match, const uint32_t* in, uint32_t n_truth_points, LogF lg) {
    const float N = (float)n_truth_points;
    float h_s = 0, h_t = 0, mi = 0;
    for (uint32_t i = 0; i < K; ++i) {
        const float p = (float)ssize[i];
        h_s -= evl_entropy_term(p, N, lg);
    }
    for (uint32_t j = 0; j < M; ++j) {
        const float q = (float)tsize[j];
        h_t -= evl_entropy_term(q, N, lg);
    }
    for (uint32_t i = 0; i < K; ++i) {
        const float p = (float)ssize[i];
        for (uint32_t e = roff[i]; e < roff[i + 1]; ++e) {
            const float q = (float)tsize[col[e]];
            const float r = (float)cnt[e];
            if (r != 0) mi += evl_mi_term(N, r, p, q, lg);
        }
    }
    float p = 0, r = 0, fp = 0, fn = 0, w = 0;
    for (uint32_t j = 0; j < M; ++j) {
        const float g = (float)tsize[j];
        if (match[j] == EVL_UNMATCHED) { fn += g; continue; }
        const uint32_t i = match[j];
        const float inj = (float)in[j], s = (float)ssize[i];
        p += evl_p_term(inj, g, s); r += inj; fp += (s - inj); fn += (g - inj);
        w += evl_w_term(inj, g, ssize[i], tsize[j], in[j]);      // (over |A u B| of the two multisets)
    }
    return evl_finish(h_s, h_t, mi, p, r, fp, fn, w, N);
}

}  // namespace f3ds
#endif  // F3DS_EVAL_LEVELS_H_
