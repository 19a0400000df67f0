// f3ds_levels.h -- the rules of the hierarchy levels (f3ds_labels_at_thresholds, include/f3ds.h), shared by the HIP kernels
// (f3ds_levels.inc) and the host harness of the CPU tests (tests/levels_harness/).
//
// Clustering::cluster(state, t) (the reference's src/clustering.cpp:384-401) merges the cheapest adjacency while its weight is
// below t, and nothing in a merge depends on t: the run to t is a prefix of the run to any T >= t (all_thresh, :691-728, relies on
// it).  The merge log of a run to T -- entry i = (survivor a_i, absorbed b_i, weight w_i) -- therefore holds every level t <= T:
//   prefix   level t applies merges 0 .. p-1, p = the first i with !(w_i < t) (n_merges if none).  Logged weights are not monotone
//            (a merge can re-weight an edge below an earlier minimum), so p is the first failing index, not a count.
//   alive    supervoxel h is a region of the level iff it held voxels (alive0) and was not absorbed before p: at[h] >= p, where
//            at[h] = the log index that absorbed h (UINT32_MAX if none) and into[h] = the survivor that took it.
//   root     any other h walks h -> into[h] while at[h] < p.  at strictly increases along the walk (a survivor is absorbed, if
//            ever, after it absorbed), so the walk ends, at the region that holds h.
// Region ids are ascending surviving h, as in stage 6 (d_relabel, Clustering::get_labeled_cloud :640-663).
#ifndef F3DS_LEVELS_H_
#define F3DS_LEVELS_H_

#include "f3ds_math.h"

namespace f3ds {

constexpr uint32_t LV_NOT_ABSORBED = 0xFFFFFFFFu;

// does merge i (logged weight w) stop level t?
F3DS_HD bool lv_stops(float w, float t) { return !(w < t); }
// the prefix length of level t (serial form; the device takes the same minimum with a workgroup reduction)
F3DS_HD uint32_t lv_prefix(const uint32_t* merges, uint32_t n_merges, float t) {
    for (uint32_t i = 0; i < n_merges; ++i) if (lv_stops(m_from_bitsf(merges[(size_t)i * 3 + 2]), t)) return i;
    return n_merges;
}
// is h a region of the level with prefix p?
F3DS_HD bool lv_alive(bool alive0, uint32_t at_h, uint32_t p) { return alive0 && at_h >= p; }
// the region (surviving supervoxel) that holds h at the level with prefix p
F3DS_HD uint32_t lv_root(const uint32_t* into, const uint32_t* at, uint32_t h, uint32_t p) {
    while (at[h] < p) h = into[h];
    return h;
}

}  // namespace f3ds
#endif  // F3DS_LEVELS_H_
