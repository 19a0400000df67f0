// Host check of the sparse scoring rules of csrc/f3ds_eval_levels.h (F3DS_HD code, for host and device) against f3ds_scores_from_table
// (csrc/f3ds_eval.h, the dense host scoring of f3ds_evaluate).  Built by tests/test_eval_levels_cpu.py with g++ into a temporary
// directory and called through ctypes.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../fast-3d-pointcloud-segmentation_amd/csrc/f3ds_eval.h"
#include "../../fast-3d-pointcloud-segmentation_amd/csrc/f3ds_eval_levels.h"

using namespace f3ds;

namespace {
struct std_logf {
    float operator()(float x) const { return std::log(x); }
};
// the sparse form of a dense K x M table, the visiting order and the matching (f3ds_eval_levels.h), then the seven sums with `lg`
template <class LogF>
f3ds_performance sparse_scores(uint32_t K, uint32_t M, const uint32_t* table, const uint32_t* ssize, const uint32_t* tsize, uint32_t N, LogF lg) {
    std::vector<uint32_t> roff(K + 1, 0), col, cnt;
    for (uint32_t i = 0; i < K; ++i) {
        for (uint32_t j = 0; j < M; ++j)
            if (table[(size_t)i * M + j]) { col.push_back(j); cnt.push_back(table[(size_t)i * M + j]); }
        roff[i + 1] = (uint32_t)col.size();
    }
    // columns (rows in any order: scrambled here on purpose)
    std::vector<std::vector<uint32_t>> ci(M), cc(M);
    for (uint32_t i = K; i-- > 0;)
        for (uint32_t e = roff[i]; e < roff[i + 1]; ++e) { ci[col[e]].push_back(i); cc[col[e]].push_back(cnt[e]); }
    std::vector<uint32_t> order(M), match(M, EVL_UNMATCHED), in(M, 0);
    std::vector<unsigned char> used(K, 0), visited(M);
    const uint32_t nv = evl_visit_order(M, tsize, visited.data(), order.data());
    for (uint32_t t = 0; t < nv; ++t) {
        const uint32_t j = order[t];
        const uint32_t row = evl_match_column(ci[j].data(), cc[j].data(), (uint32_t)ci[j].size(), used.data(), &in[j]);
        match[j] = row;
        if (row != EVL_UNMATCHED) used[row] = 1;
    }
    const uint32_t* cp = col.empty() ? nullptr : col.data();
    const uint32_t* np = cnt.empty() ? nullptr : cnt.data();
    return evl_scores(K, ssize, M, tsize, roff.data(), cp, np, match.data(), in.data(), N, lg);
}
}  // namespace

// out: 21 floats -- f3ds_scores_from_table, the sparse routine with std::log, the sparse routine with m_logf (7 each, f3ds_performance order)
extern "C" void evl_check(uint32_t K, uint32_t M, const uint32_t* table, const uint32_t* ssize, const uint32_t* tsize, uint32_t N, float* out) {
    const std::vector<uint32_t> t(table, table + (size_t)K * M), s(ssize, ssize + K), g(tsize, tsize + M);
    const f3ds_performance r[3] = {f3ds_scores_from_table(t, s, g, N), sparse_scores(K, M, table, ssize, tsize, N, std_logf()),
                                   sparse_scores(K, M, table, ssize, tsize, N, evl_m_logf())};
    for (int k = 0; k < 3; ++k) {
        const float v[7] = {r[k].voi, r[k].precision, r[k].recall, r[k].fscore, r[k].wov, r[k].fpr, r[k].fnr};
        for (int q = 0; q < 7; ++q) out[k * 7 + q] = v[q];
    }
}
