// The reference side of the d_centroid / d_sv_fill probes: the shared header's sequential functions compiled by g++ with the flags of tests/emul
// (as devprobe_host.cpp).  Loops over a given leaf order, nothing else.
#include <cstddef>
#include <cstdint>

#include "f3ds_algo.h"

using namespace f3ds;

extern "C" {

// a_centroid_finish on n rows of (nine sums, count) -> n rows of 12
int kp_host_centroid_finish(const float* sums, const uint32_t* counts, size_t n, float* rows) {
    for (size_t i = 0; i < n; ++i) a_centroid_finish(sums + i * 9, counts[i], rows + i * 12);
    return 0;
}
// one supervoxel: a_payload_row of its n leaves in the given order (rows[n x 12]), a_fold_row over them (acc[12]), n_rgb2lab of the running mean colour (lab[3])
int kp_host_sv(const float* vf, const int* leaves, uint32_t n, float* rows, float* acc, float* lab) {
    for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
    for (uint32_t j = 0; j < n; ++j) {
        a_payload_row(vf + (size_t)leaves[j] * 12, rows + (size_t)j * 12);
        a_fold_row(acc, rows + (size_t)j * 12, j + 1u);
    }
    n_rgb2lab(acc + 9, lab);
    return 0;
}

}  // extern "C"
