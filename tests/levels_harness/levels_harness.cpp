// Host replay of a merge log through the hierarchy-level rules of csrc/f3ds_levels.h (the same definitions the HIP kernels use).
// Built by tests/test_levels_cpu.py with g++ into a temporary directory and called through ctypes.
#include <cstdint>
#include <vector>

#include "../../fast-3d-pointcloud-segmentation_amd/csrc/f3ds_levels.h"

using namespace f3ds;

// labels (k x n, level-major) and region counts of k thresholds.  alive0[h]: supervoxel h (1..S0) held voxels; merges: n_merges x
// (survivor, absorbed, weight bits); point_sv[i]: supervoxel of point i (0 = none).  Returns 0, or -1 for a malformed log.
extern "C" int lv_replay(uint32_t S0, const unsigned char* alive0, const uint32_t* merges, uint32_t n_merges, const float* thr, uint32_t k,
                         uint32_t n, const uint32_t* point_sv, uint32_t* labels, uint32_t* n_regions) {
    std::vector<uint32_t> into(S0 + 1u, 0u), at(S0 + 1u, LV_NOT_ABSORBED), id(S0 + 1u);
    for (uint32_t i = 0; i < n_merges; ++i) {
        const uint32_t a = merges[(size_t)i * 3], b = merges[(size_t)i * 3 + 1];
        if (a > S0 || b > S0 || at[b] != LV_NOT_ABSORBED) return -1;
        into[b] = a; at[b] = i;
    }
    for (uint32_t l = 0; l < k; ++l) {
        const uint32_t p = lv_prefix(merges, n_merges, thr[l]);
        uint32_t count = 0;
        for (uint32_t h = 0; h <= S0; ++h) id[h] = (h > 0 && lv_alive(alive0[h] != 0, at[h], p)) ? count++ : 0xFFFFFFFFu;
        n_regions[l] = count;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t o = point_sv[i];
            labels[(size_t)l * n + i] = (o && o <= S0) ? id[lv_root(into.data(), at.data(), o, p)] : 0xFFFFFFFFu;
        }
    }
    return 0;
}
