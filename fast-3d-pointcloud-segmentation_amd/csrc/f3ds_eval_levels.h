// f3ds_eval_levels.h -- the scoring rules of f3ds_evaluate over a SPARSE contingency table, as F3DS_HD code: the building block for
// scoring many hierarchy levels (f3ds_labels_at_thresholds) without one dense K x M table per level.  No library
// code calls it yet; tests/eval_levels_harness/ (tests/test_eval_levels_cpu.py) checks it against f3ds_scores_from_table.  The only
// device build of it so far is the test probe: tests/devprobe/devprobe.hip compiles it with hipcc for gfx950 and
// tests/test_devprobe_gpu.py::test_evl_scores_on_the_device compares all seven scores with the g++ build, bit for bit.
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

// The seven scores from the sparse table and a matching (match[j] = row or EVL_UNMATCHED, in[j] = the matched entry's count).
// Term for term f3ds_scores_from_table; the caller guarantees K >= 1 and M >= 1.
template <class LogF>
F3DS_HD f3ds_performance evl_scores(uint32_t K, const uint32_t* ssize, uint32_t M, const uint32_t* tsize, const uint32_t* roff, const uint32_t* col,
                                    const uint32_t* cnt, const uint32_t* match, const uint32_t* in, uint32_t n_truth_points, LogF lg) {
    f3ds_performance out;
    const float N = (float)n_truth_points;
    float h_s = 0, h_t = 0, mi = 0;
    for (uint32_t i = 0; i < K; ++i) {
        const float p = (float)ssize[i];
        h_s -= lg(p / N) * p / N;
    }
    for (uint32_t j = 0; j < M; ++j) {
        const float q = (float)tsize[j];
        h_t -= lg(q / N) * q / N;
    }
    for (uint32_t i = 0; i < K; ++i) {
        const float p = (float)ssize[i];
        for (uint32_t e = roff[i]; e < roff[i + 1]; ++e) {
            const float q = (float)tsize[col[e]];
            const float r = (float)cnt[e];
            if (r != 0) mi += lg((N * r) / (p * q)) * r / N;
        }
    }
    out.voi = h_s + h_t - 2 * mi;
    float p = 0, r = 0, fp = 0, fn = 0, w = 0;
    for (uint32_t j = 0; j < M; ++j) {
        const float g = (float)tsize[j];
        if (match[j] == EVL_UNMATCHED) { fn += g; continue; }
        const uint32_t i = match[j];
        const float inj = (float)in[j], s = (float)ssize[i];
        p += inj * g / s; r += inj; fp += (s - inj); fn += (g - inj);
        const float un = (float)(ssize[i] + tsize[j] - in[j]);      // |A u B| of the two multisets
        w += inj * g / un;
    }
    out.precision = p / N; out.recall = r / N; out.fpr = fp / N; out.fnr = fn / N;
    out.fscore = (out.precision == 0 && out.recall == 0) ? 0.0f : 2 * (out.precision * out.recall) / (out.precision + out.recall);
    out.wov = w / N;
    return out;
}

}  // namespace f3ds
#endif  // F3DS_EVAL_LEVELS_H_
