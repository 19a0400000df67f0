// f3ds_hip.hip -- the MI355X (gfx950) device pipeline behind include/f3ds.h.
//
// Stage map (kernel functors d_<name> live in f3ds_kernels.inc; reference citations are in include/f3ds.h,
// csrc/f3ds_numerics.h, csrc/f3ds_algo.h):
//   0 voxelise   d_bbox -> d_grid, then one of two paths:
//                tile path (batches): d_tile_keys -> radix sort of the tile descriptors -> d_desc_part / d_desc_offsets / d_desc_apply -> d_tile_place -> d_voxel_list_accum
//                sort path (lone frames, refused frames): d_keys -> radix sort of the points -> d_seg_count / scan / d_seg_write -> d_voxel_gather_accum
//                (F3DS_SPLIT_VOXEL_ACCUM, development: the sort path as d_heads / scan / d_segstart -> d_point_gather -> d_voxel_accum)
//   1 neighbours d_vox_table (leaf keys -> one table entry per 4x4x4 block of cells, after either path of stage 0), d_neighbors (the 27 cells through that table), d_normals_t<384 | 256 threads> (two-ring ordered covariance, LDS tile)
//   2 seeds      d_chunkbox, d_seed_grow, d_seed_keys, radix sort, d_cell_hash, d_seed_nn, d_seed_filter
//   3 sweeps     per sweep: d_sweep_begin, d_sweep_R_first (pre-pass | round 0), d_sweep_R_round x2 | d_sweep_R + d_sweep_R_tail, d_sweep_claim,
//                d_centroid (both mark dirty tiles on the spot)  
//   4 summaries  d_sv_fill (payload rows + ordered leaf sums), d_edges, radix sort, d_edge_init,
//                d_edge_deltas, d_lambda / d_cdf_*, d_edge_weights
//   5 merge      d_inc_build, d_merge_il_t<4 or 8 waves, per-edge arrays in LDS or L2> (one persistent workgroup per frame), d_merge (global memory)
//   6 labels     d_relabel (union-find relabel in LDS + per-point label write; d_region_ids + d_point_labels beyond 12 k supervoxels)
//   levels       (f3ds_labels_at_thresholds, off the segment path) d_level_log, d_level_prefix, d_level_labels | d_level_tables + d_level_points (f3ds_levels.inc)
//   level scores (f3ds_evaluate_levels, off the segment path) d_truth_*, d_level_log / prefix / tables, d_evl_base_keys, radix sort, d_evl_heads / scan / d_evl_reduce,
//                d_evl_level_keys, radix sort + reduce, d_evl_col_keys, radix sort, d_evl_ht, d_evl_score (f3ds_eval_levels.inc)
// Every frame RECORDS its kernel calls; flush() zips the records of a batch into one dispatch per kernel (grid.y = frame).
//
// Layout in HBM: points stay as the caller's 16-byte records (one global_load_dwordx4 per lane);
// everything per voxel is SoA rows of 12 floats (48 B, 16-B aligned: xyz rgb normal pad) so a
// lane reads a neighbour with three dwordx4 loads; per-voxel neighbour table is V x 27 int32 (plus its 27 x V transpose).
// Float summation order is the reference's everywhere: parallel across outputs, sequential in
// reference order inside each reduction.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <atomic>
#include <map>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <mutex>
#include <set>
#include <vector>

#include "../../include/f3ds.h"
#include "f3ds_algo.h"
#include "f3ds_glasbey.h"
#include "f3ds_eval.h"
#include "f3ds_dev.h"
#include "f3ds_levels.h"
#include "f3ds_eval_levels.h"
#include "f3ds_rgbd.h"
#include "f3ds_label_image.h"
#include "f3ds_track.h"
#include "f3ds_regions.h"
#include "f3ds_contacts.h"
#include "f3ds_shapes.h"
#include "f3ds_boxes.h"
#include "f3ds_joints.h"
#include "f3ds_components.h"
#include "f3ds_cloud.h"
#include "f3ds_batch_policy.h"

using namespace f3ds;

#include "f3ds_kernels.inc"
#include "f3ds_levels.inc"
#include "f3ds_eval_levels.inc"
#include "f3ds_track.inc"
#include "f3ds_regions.inc"
#include "f3ds_pairs.inc"
#include "f3ds_contacts.inc"
#include "f3ds_shapes.inc"
#include "f3ds_boxes.inc"
#include "f3ds_joints.inc"
#include "f3ds_components.inc"
#include "f3ds_cloud.inc"

// ================================================================================================
// batched launch machinery
//
// Every kernel body above works on ONE frame.  The host records, per frame, the sequence of kernel
// calls a stage needs (functor type, grid width, LDS bytes, packed arguments) without launching
// anything; flush() then zips the per-frame sequences -- they are identical in shape, only the
// arguments differ -- into one dispatch per kernel with grid.y = number of frames.  A batch of 32
// frames therefore costs the launches of one frame, and every dispatch is 32 times wider.
// ================================================================================================
namespace {

thread_local std::string g_last_hip_error;
#define HIPCHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { g_last_hip_error = std::string(#expr) + ": " + hipGetErrorString(e_); return F3DS_ERR_HIP; } } while (0)

template <class... Ts> struct ArgPack;
template <> struct ArgPack<> {};
template <class T, class... Ts> struct ArgPack<T, Ts...> { T head; ArgPack<Ts...> tail; };

template <class K, class... Done>
__device__ __forceinline__ void unpack_call(const ArgPack<>&, Done... d) { K{}(d...); }
template <class K, class T, class... Ts, class... Done>
__device__ __forceinline__ void unpack_call(const ArgPack<T, Ts...>& p, Done... d) { unpack_call<K>(p.tail, d..., p.head); }

// A kernel body may ask for a register budget (WAVES_PER_SIMD = w: at most 512 / w VGPRs) so that workgroups of OTHER kernels fit beside its own
// on a CU: the long-running, latency-bound kernels (the merge loop, the voxel normals) otherwise fence whole CUs off for the wide ones.
template <class K, class = void> struct waves_per_simd { static constexpr int v = 1; };
template <class K> struct waves_per_simd<K, std::void_t<decltype(K::WAVES_PER_SIMD)>> { static constexpr int v = K::WAVES_PER_SIMD; };
// The single-workgroup-per-frame kernels (serial scans, the seed-grid growth, the sweep's device-side decisions) sit on every call's critical path and do little:
// with other calls' wide kernels on the chip their waves are raised in priority (F3DS_EXP_NO_LATENCY_PRIO: A/B)
template <class K, class = void> struct is_latency_kernel { static constexpr bool v = false; };
template <class K> struct is_latency_kernel<K, std::void_t<decltype(K::LATENCY_KERNEL)>> { static constexpr bool v = K::LATENCY_KERNEL; };
template <class K, class Pack>
__global__ __launch_bounds__(K::BLOCK, waves_per_simd<K>::v) void k_batched(const Pack* frames) {
#ifndef F3DS_EXP_NO_LATENCY_PRIO
    if constexpr (is_latency_kernel<K>::v) __builtin_amdgcn_s_setprio(3);
#endif
    const Pack p = frames[f3ds_frame()];      // XCD-aware (frame, block) mapping: f3ds_kernels.inc
    unpack_call<K>(p);
}

template <class F> struct op_traits;
template <class C, class... Ps> struct op_traits<void (C::*)(Ps...) const> { using pack = ArgPack<std::decay_t<Ps>...>; };
template <class K> using pack_of = typename op_traits<decltype(&K::operator())>::pack;

inline void fill_pack(ArgPack<>&) {}
template <class T, class... Ts, class A, class... As>
inline void fill_pack(ArgPack<T, Ts...>& p, A a, As... as) {
    static_assert(std::is_convertible<A, T>::value && !(std::is_pointer<T>::value && std::is_integral<A>::value),
                  "rec<K>(): an argument does not convert implicitly to the kernel's parameter type (wrong element type, swapped arguments?)");
    p.head = a; fill_pack(p.tail, as...);
}

typedef hipError_t (*LaunchFn)(uint32_t gx, uint32_t nf, uint32_t lds, hipStream_t st, const void* dargs);
template <class K>
hipError_t launch_fn(uint32_t gx, uint32_t nf, uint32_t lds, hipStream_t st, const void* dargs) {
    using Pack = pack_of<K>;
    if (lds > 48u * 1024u) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_batched<K, Pack>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_batched<K, Pack>), dim3(gx ? gx : 1u, nf), dim3(K::BLOCK), lds, st, static_cast<const Pack*>(dargs));
    return hipGetLastError();
}
struct Cmd { LaunchFn fn; uint32_t gx, lds, bytes, off; };

// dirty-tile sweeps: a sweep that changed at most V >> shift voxels lets the next one skip clean tiles.
// F3DS_INC_SHIFT=-1 turns the skipping off (every sweep evaluates every voxel), 32 forces it always.
const int g_inc_shift = [] { const char* e = dev_getenv("F3DS_INC_SHIFT"); return e ? atoi(e) : 6; }();

// Development / test switches (none is needed in production and none changes results).  The environment is read ONCE per entry
// call of the library (f3ds_segment_batch, f3ds_recluster, f3ds_refine_supervoxels, f3ds_evaluate, ...) into this per-thread struct -- not per frame on the hot path,
// where hundreds of getenv() scans per call would also race with a setenv from another thread.  Tests still see per-call values.
struct Switches {
    bool direct_labels = false, copy_stream = true, copy_duplex = false, split_voxel_accum = false, sweep_tiles = true, merge_spec = true, force_global_merge = false, no_stream_pool = false, sort_pairs = false, host_prof = false, trace_err = false, vox_hash = true, vox_tiles_forced = false, levels_global = false;
    int normals_threads = 0, merge_nw = 0, merge_keys = -1; uint32_t tile_holes = 0, ilist_slack = f3ds_policy::ILIST_SLACK, r_rounds = F3DS_R_ROUNDS, grid_cap = 0, rgc_first_cap = 0, rgj_first_cap = 0, cloud_path = 0; long relabel_lds_cap = -1;
    void read() {
        auto on = [](const char* n) { return dev_getenv(n) != nullptr; };
        auto num = [](const char* n, long dflt) { const char* e = dev_getenv(n); return e ? atol(e) : dflt; };
        direct_labels = num("F3DS_DIRECT_LABELS", 0) != 0; copy_stream = num("F3DS_COPY_STREAM", 1) != 0; copy_duplex = num("F3DS_COPY_STREAM", 1) == 2; split_voxel_accum = on("F3DS_SPLIT_VOXEL_ACCUM"); sweep_tiles = num("F3DS_SWEEP_TILES", 1) != 0; merge_spec = num("F3DS_MERGE_SPEC", 1) != 0;
        force_global_merge = on("F3DS_FORCE_GLOBAL_MERGE"); no_stream_pool = on("F3DS_NO_STREAM_POOL"); sort_pairs = on("F3DS_SORT_PAIRS");
        host_prof = on("F3DS_HOST_PROF"); trace_err = on("F3DS_TRACE_ERR");
        vox_tiles_forced = num("F3DS_VOX_TILES", 1) == 2;      // (2: also for lone frames -- tests)
        vox_hash = num("F3DS_VOX_TILES", 1) != 0 && !sort_pairs && !split_voxel_accum;      // (0: stage 0 by sorting the points, as until round 4; the two development switches of that path imply it)
        normals_threads = (int)num("F3DS_NORMALS_THREADS", 0); tile_holes = (uint32_t)num("F3DS_SWEEP_TILE_HOLES", 0);
        { const long v = num("F3DS_MERGE_NW", 0); merge_nw = v == 4 ? 4 : (v ? 8 : 0); }
        { const char* e = dev_getenv("F3DS_MERGE_KEYS"); merge_keys = !e ? -1 : (!strcmp(e, "lds") ? 2 : (!strcmp(e, "global") ? 1 : 0)); }
        relabel_lds_cap = num("F3DS_RELABEL_LDS_CAP", -1);
        levels_global = num("F3DS_LEVELS_GLOBAL", 0) != 0;      // (tests: the hierarchy levels take the global-table form on small frames too)
        { const long v = num("F3DS_R_ROUNDS_RUN", F3DS_R_ROUNDS); r_rounds = v >= 1 && v <= F3DS_R_ROUNDS ? (uint32_t)v : (uint32_t)F3DS_R_ROUNDS; }
        { const long v = num("F3DS_ILIST_SLACK", f3ds_policy::ILIST_SLACK); ilist_slack = v >= 1 && v <= (long)f3ds_policy::ILIST_SLACK ? (uint32_t)v : f3ds_policy::ILIST_SLACK; }      // tests: a short incident-list pool (the merge stage then reruns with a larger one)
        { const long v = num("F3DS_GRID_CAP", 0); grid_cap = v >= 1 && v <= (long)f3ds_policy::WIDE_CAP ? (uint32_t)v : 0u; }      // tests: 1 ... 2048 workgroups per frame, exactly, for grid_for() and grid_wide(): the grid-stride loops make several trips on small frames (0: unset)
        { const long v = num("F3DS_RGC_FIRST_CAP", 0); rgc_first_cap = v >= 1 && v <= 0x7fffffffl ? (uint32_t)v : 0u; }      // tests: a short first record buffer of f3ds_region_contacts (the frame then runs again with room for all; 0: unset)
        { const char* e = dev_getenv("F3DS_CLOUD_PATH"); cloud_path = !e ? 0u : (!strcmp(e, "direct") ? CD_PATH_DIRECT : (!strcmp(e, "ordered") ? CD_PATH_ORDERED : 0u)); }      // tests: how f3ds_cloud_regions walks its points, whatever K says (0: unset)
        { const long v = num("F3DS_RGJ_FIRST_CAP", 0); rgj_first_cap = v >= 1 && v <= 0x7fffffffl ? (uint32_t)v : 0u; }      // tests: likewise the first record buffer of f3ds_region_joints
    }
};
thread_local Switches g_sw;
// where the per-edge arrays of a 4-wave merge loop live when the call shares the device with other batch calls: 0 = global memory (52 KB of LDS per
// workgroup: two fit a unit, and a voxel-normal workgroup beside them), 2 = LDS (up to 140 KB).  F3DS_MERGE_SHARED_RES=0|2 (A/B runs), read once.
const int g_merge_shared_res = [] { const char* e = dev_getenv("F3DS_MERGE_SHARED_RES"); return e && atoi(e) == 2 ? 2 : 0; }();

// Device scratch of a context: typed, grow-only buffers (ensure(), below).  F3DS_SCRATCH is THE list of them: it declares the members of f3ds_ctx, numbers their slots in
// the device-wide high-water table, and is what pregrow_scratch() and f3ds_destroy() walk.  A new buffer is one X(element type, name) here and nothing else.
#define F3DS_SCRATCH(X) \
    X(P16, pts) /* rgbd frames: the two images as uploaded */ X(unsigned char, img_depth) X(unsigned char, img_color) X(P16, spts) X(uint64_t, keys0) X(uint64_t, keys1) X(uint32_t, vals0) X(uint32_t, vals1) X(uint32_t, flags) X(uint32_t, incl) X(uint32_t, tiles) X(uint32_t, hist) X(uint32_t, seg_start) X(int, pt_voxel) X(uint32_t, labels) \
    X(uint32_t, vkey) X(uint32_t, vcount) X(float, vf) X(int, nbr) X(int, nbrT) X(uint64_t, hkeys) X(uint32_t, hvals) X(float, boxes) X(uint32_t, ckey) X(uint32_t, cell_start) X(uint64_t, chk) X(uint32_t, chv) X(uint32_t, chvals) X(int, seed_orig) X(uint32_t, keep) X(int, seed_kept) \
    X(uint32_t, owner0) X(uint32_t, ownR) X(float, dist0) X(unsigned char, R) X(float, hc) X(uint32_t, hcount) X(uint32_t, hlo) X(uint32_t, hhi) X(int, ghost_vox) X(unsigned char, ghost_active) X(unsigned char, ghost_done) X(uint32_t, ghost_head) X(uint32_t, ghost_next) \
    X(uint32_t, loff) X(float, rows) X(int, row_voxel) X(float, racc0) X(uint32_t, rcnt0) X(float, rrec0) X(unsigned char, ralive0) X(uint64_t, ehk) X(uint64_t, ekeys0) X(uint64_t, ekeys1) X(uint32_t, evals0) X(uint32_t, evals1) X(uint32_t, ea0) X(uint32_t, eb0) \
    X(uint32_t, ea) X(uint32_t, eb) X(float, ew) X(uint32_t, eku) X(int, ehist) X(unsigned char, ealive) X(uint32_t, ev_epoch) X(uint32_t, ev_key) X(int, ev_prev) X(float, racc) X(uint32_t, rcnt) X(float, rrec) X(unsigned char, ralive) X(uint32_t, rhead) X(uint32_t, rtail) X(uint32_t, lnext) X(uint32_t, parent) X(uint32_t, markA) X(uint32_t, markB) X(uint32_t, tl) X(uint32_t, merges) \
    /* refineSupervoxels works on copies */ X(float, r_vf) X(uint32_t, r_owner) X(float, r_dist) X(float, r_hc) X(uint32_t, r_hcount) X(uint32_t, r_hlo) X(uint32_t, r_hhi) X(int, r_gvox) X(unsigned char, r_gact) X(unsigned char, r_gdone) X(uint32_t, r_ghead) X(uint32_t, r_gnext) X(uint32_t, r_tl) X(uint32_t, r_tcnt) X(int, r_seed) X(uint32_t, r_L) \
    X(uint32_t, tstamp) X(uint32_t, tround) X(uint32_t, hdirty) X(uint32_t, htiles) X(uint32_t, htcnt) X(uint32_t, vwl) X(uint32_t, vwl2) X(uint32_t, vtmask) \
    /* ground-truth evaluation */ X(uint32_t, glut) X(uint32_t, truth_pts) X(uint32_t, tsum) X(uint32_t, tcol) X(uint32_t, tlab) X(uint32_t, ctab) X(uint32_t, csize) X(uint32_t, eroot) X(uint32_t, eincl) \
    /* stage 0, tile path: per (tile, entry) point count / list base / leaf ordinal; per point its (entry, rank in tile); per-leaf point lists */ X(uint32_t, hcnt) X(uint32_t, pslot) X(uint32_t, vlist) \
    /* f3ds_cluster_supervoxels: the caller's supervoxels as uploaded */ X(uint32_t, u_src) X(uint32_t, u_voff) X(float, u_xyz) X(uint32_t, u_rgba) X(float, u_cent) X(float, u_nrm) \
    X(float, deltas) X(uint64_t, skeys0) X(uint64_t, skeys1) X(uint32_t, svals0) X(uint32_t, svals1) X(uint32_t, cdf_hist) X(float, cdf) X(uint32_t, root) X(uint32_t, rincl) X(uint32_t, rrank) X(uint2, pool) X(uint32_t, rstart) X(uint32_t, rnleaf) X(uint32_t, rcap) X(uint32_t, tile_n1) X(uint32_t, tile_ord) X(uint32_t, tile_slots) X(uint32_t, ilist) X(uint32_t, istart) X(uint32_t, ilen) X(uint32_t, icap) \
    /* hierarchy levels */ X(uint32_t, lv_into) X(uint32_t, lv_at) X(uint32_t, lv_pfx) X(float, lv_thr) X(uint32_t, lv_tab) X(uint32_t, lv_nreg) X(uint32_t, lv_out) \
    /* level scores (f3ds_eval_levels.inc): sort buffers, base table, reduced level entries, ghost list, per-level sizes / flags / terms, truth sizes and visiting order, matches, counts and results of a batch */ \
    X(uint64_t, evl_k0) X(uint64_t, evl_k1) X(uint32_t, evl_v0) X(uint32_t, evl_v1) X(uint32_t, evl_flag) X(uint64_t, evl_bkey) X(uint32_t, evl_bcnt) X(uint64_t, evl_ukey) X(uint32_t, evl_ucnt) X(uint32_t, evl_glist) \
    X(uint32_t, evl_ssize) X(unsigned char, evl_used) X(float, evl_hterm) X(float, evl_mterm) X(float, evl_tterm) X(uint32_t, evl_tsize) X(uint32_t, evl_order) X(uint32_t, evl_slot) X(uint32_t, evl_counts) X(uint32_t, evl_out) \
    /* the label-image calls (the tracker update and the five region calls): family-wide staging, which holds nothing once a call has returned (every call waits before it returns) -- the images and labels of a host caller as uploaded, and the head with what a host caller gets behind it on its way down */ \
    X(unsigned char, li_depth) X(unsigned char, li_color) X(uint32_t, li_lab) X(unsigned char, li_out) \
    /* ... and below it each call's private working state, which a run of the call that replays (the contacts' second run) finds as it left it */ \
    /* label tracker (f3ds_track.inc; the sort and the reduction use the evl_ buffers of the tracker's private context): the ends of the entries' runs, the packed entries, id[], the ids of a host caller */ \
    X(uint32_t, trk_end) X(uint32_t, trk_out) X(uint32_t, trk_id) X(uint32_t, trk_tid) \
    /* region table (f3ds_regions.inc): the accumulators */ \
    X(RgAcc, rgt_acc) \
    /* region contacts (f3ds_contacts.inc): the records' keys and indices (twice: the sort), the records, the runs' flags, keys, starts and ends, the run count */ \
    X(uint64_t, rgc_k0) X(uint64_t, rgc_k1) X(uint32_t, rgc_v0) X(uint32_t, rgc_v1) X(uint32_t, rgc_rec) X(uint32_t, rgc_flag) X(uint64_t, rgc_ukey) X(uint32_t, rgc_ustart) X(uint32_t, rgc_uend) X(uint32_t, rgc_cnt) \
    /* region shapes (f3ds_shapes.inc): the accumulators */ \
    X(ShAcc, rgs_acc) \
    /* region boxes (f3ds_boxes.inc; pass one adds into rgs_acc): the frames, the accumulators of pass two, its head, the shape rows of a caller who wants none */ \
    X(BxFrame, rgx_frame) X(BxAcc, rgx_acc) X(uint32_t, rgx_head) X(f3ds_region_shape, rgx_shape) \
    /* region joints (f3ds_joints.inc): the shapes' accumulators and head, the shape rows of a caller who wants none, then as the contacts: the records' keys and indices (twice: the sort), the records, the runs' flags, keys, starts and ends, the run count */ \
    X(ShAcc, rgj_sacc) X(uint32_t, rgj_shead) X(f3ds_region_shape, rgj_shape) X(uint64_t, rgj_k0) X(uint64_t, rgj_k1) X(uint32_t, rgj_v0) X(uint32_t, rgj_v1) X(uint32_t, rgj_rec) X(uint32_t, rgj_flag) X(uint64_t, rgj_ukey) X(uint32_t, rgj_ustart) X(uint32_t, rgj_uend) X(uint32_t, rgj_cnt) \
    /* region components (f3ds_components.inc): a parent, a size and a flag word per pixel */ \
    X(uint32_t, rgk_parent) X(uint32_t, rgk_cnt) X(uint32_t, rgk_flag) \
    /* region rows of a cloud (f3ds_cloud.inc): the records of a host caller as uploaded (its labels ride in li_lab), the accumulators, the keys (twice: the sort), then the box pass: the shape rows, the frames, the accumulators of pass two and its head */ \
    X(P16, rgp_pts) X(CdAcc, rgp_acc) X(uint64_t, rgp_k0) X(uint64_t, rgp_k1) X(f3ds_region_shape, rgp_shape) X(BxFrame, rgp_frame) X(BxAcc, rgp_bacc) X(uint32_t, rgp_head)
template <class T> struct Scratch { T* p = nullptr; size_t cap = 0; int slot = -1; };      // cap: bytes allocated; slot: position in F3DS_SCRATCH
#define F3DS_SCRATCH_SLOT(T, name) S_##name,
#define F3DS_SCRATCH_MEMBER(T, name) Scratch<T> name{nullptr, 0, S_##name};
#define F3DS_SCRATCH_VISIT(T, name) if (const int rc_ = f(name)) return rc_;
enum ScratchSlot { F3DS_SCRATCH(F3DS_SCRATCH_SLOT) N_SCRATCH };

}  // namespace

struct f3ds_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[11] = {};            // 0..7 stage boundaries, 9 / 10 around the d_normals launch
    DevCounters* d_dc = nullptr;
    DevCounters* h_dc = nullptr;       // pinned
    GridInfo* d_grid = nullptr;
    GridInfo* h_grid = nullptr;        // pinned (only read by f3ds_get_debug)
    SeedGrid* d_sgrid = nullptr;
    // recorded, not yet launched kernel calls of this frame
    std::vector<Cmd> cmds;
    std::vector<unsigned char> blob;
    std::vector<uintptr_t> pend;       // device addresses the recorded calls refer to (pointer arguments; every aligned word of struct arguments)
    MultiOp ops = {}; uint32_t ops_grid = 0;      // fills / copies recorded in a row and not yet turned into a d_multi_op call (flush_ops)
    // pinned + device staging for the packed arguments of a batch (owned by the batch's first context)
    unsigned char* h_args[2] = {nullptr, nullptr}; unsigned char* d_args[2] = {nullptr, nullptr}; size_t args_cap = 0;      // two arenas, used in turn: a flush never waits for the stream
    hipEvent_t ev_args[2] = {nullptr, nullptr}; bool args_used[2] = {false, false}; int args_flip = 0;
    hipEvent_t ev_copy[3] = {nullptr, nullptr, nullptr};      // uploads queued on the device's copy stream / labels ready on the call's stream / downloads done on the copy stream
    DevCounters* d_dcblk = nullptr; DevCounters* h_dcblk = nullptr; size_t dcblk_cap = 0;      // the batch's counters, one slot per frame
    unsigned char* h_li = nullptr; size_t h_li_cap = 0;      // pinned: the head of a region call (and a host caller's rows and image) on their way down (li_out_buffers)
    // frame state
    bool have_frame = false;
    bool live = false;
    int rc = 0;
    f3ds_params prm;
    FrameArgs fa;
    const P16* d_pts = nullptr;
    uint32_t n = 0, V = 0, C = 0, S0 = 0, E = 0, hmask = 0;
    uint64_t *ks = nullptr; uint32_t *vs = nullptr;      // sorted point keys / indices
    uint64_t *cks = nullptr; uint32_t *cvs = nullptr;    // sorted seed-cell keys / voxels
    uint64_t *eks = nullptr;                             // sorted edge keys
    f3ds_result res;
    bool merge_in_lds = false;
    int merge_kind = 0;                // which merge kernel the last cluster stage ran (MergeKind)
    uint32_t ev_mult = f3ds_policy::EV_MULT;             // weight-history events per initial edge the merge loop may write
    uint32_t pool_mult = 1;            // leaf pool size factor (grown on demand like ev_mult)
    uint32_t vox_cap = 0;              // bound on the leaves of the current frame that stage 0's tile path sized its buffers by
    bool vox_hashed = false;           // stage 0 of the current frame took the tile path (seg_vox_tiles)
    bool vox_dense = false;            // this context met a frame the tile path refuses (an unorganised cloud, a voxel of more than VL_MAX_RUN points): its frames take the sort path ...
    uint32_t vox_dense_wait = 0, vox_dense_penalty = f3ds_policy::DENSE_PENALTY;      // ... for this many calls, then the tile path is tried again (8, 16, ... 1024 calls after every further refusal): one odd frame
                                                             // does not cost a long-lived context the faster stage 0 for good
    uint32_t ilist_mult = 1;           // incident-list pool size factor (its own: a leaf-pool overflow must not grow the list pool too)
    uint32_t edge_mult = f3ds_policy::EDGE_MULT;           // adjacency list room per seed (S0 * edge_mult + 1024), grown on demand
    bool relabel_lds = true;           // stage 6 as one kernel (the region-id table fits LDS for every frame of the batch)
    int refined_itr = -1;              // >= 0: the r_* buffers hold the state after that many refinement iterations of this frame
    int idxbits = -1;                  // >= 0: the sorted point keys carry the point index in their low bits
    uint32_t* user_labels = nullptr;   // device label buffer of the caller for the current call (else c->labels + copy)
    MergeDev mdev; MergeLds mlds; float host_lambda = 0.5f;
    // device scratch (grow-only): one typed member per entry of F3DS_SCRATCH; each_scratch(f) calls f on every one of them until one returns non-zero
    F3DS_SCRATCH(F3DS_SCRATCH_MEMBER)
    template <class F> int each_scratch(F&& f) { F3DS_SCRATCH(F3DS_SCRATCH_VISIT) return 0; }
    uint32_t cloud_path = 0;           // how the last f3ds_cloud_regions call of this context walked its points (CD_PATH_*; F3DS_DBG_CLOUD_PATH)
    uint32_t launch_shape[3] = {0, 0, 0};      // cap of grid_for(), cap of grid_wide(), frames of the last entry call that recorded kernels for this context (F3DS_DBG_LAUNCH_SHAPE)
    std::vector<uint32_t> tsize;       // voxels per truth label (evaluation)
    float cluster_T = 0.0f;            // threshold of the last cluster run: f3ds_labels_at_thresholds serves levels t <= cluster_T from its merge log
    // f3ds_cluster_supervoxels: the state is caller-supplied supervoxels (no points, no voxel grid).  user_label[h] = the caller's label of internal
    // supervoxel h (h = rank in ascending label + 1; [0] = 0), user_row[h] = its row in the caller's arrays; empty after f3ds_segment
    bool user_mode = false;
    std::vector<uint32_t> user_label, user_row;
};

namespace {

// A recorded, not yet flushed kernel call holds raw device pointers: a buffer such a call refers to must not be freed and
// reallocated before the flush (the dispatch would write into freed memory).  rec<>() notes the address of every pointer-typed
// argument (and, for the few struct arguments -- SweepFrame, MergeDev, MergeLds --, every 8-byte word of the struct, which is
// where their pointer members sit); scalar arguments are never mistaken for addresses.  Checked on every regrow.
bool referenced_by_pending_calls(const f3ds_ctx* c, const void* mem, size_t cap) {
    const uintptr_t lo = (uintptr_t)mem, hi = lo + cap;
    for (const uintptr_t w : c->pend) if (w >= lo && w < hi) return true;
    for (uint32_t k = 0; k < c->ops.n; ++k) {      // (fills / copies recorded and not yet merged into a call)
        const uintptr_t d = (uintptr_t)c->ops.dst[k], sp = (uintptr_t)c->ops.src[k];
        if ((d >= lo && d < hi) || (sp >= lo && sp < hi)) return true;
    }
    return false;
}
template <class A> inline void note_arg(f3ds_ctx* c, const A& a) {
    if constexpr (std::is_pointer<A>::value) { if (a) c->pend.push_back((uintptr_t)a); }
    else if constexpr (std::is_class<A>::value) {
        static_assert(std::is_trivially_copyable<A>::value, "kernel arguments must be plain data");
        for (size_t off = 0; off + 8 <= sizeof(A); off += 8) { uintptr_t w; memcpy(&w, reinterpret_cast<const unsigned char*>(&a) + off, 8); if (w) c->pend.push_back(w); }
    }
}
// Scratch is grow-only per context, and sized by the largest frame ANY context of the device has seen: g_scratch_hwm holds,
// per buffer slot, the largest request so far.  A context that has to grow a buffer -- or meets a request below the mark
// while nothing recorded refers to the buffer -- goes straight to the mark (if that is within 4x of its own request), so that
// a pool of contexts fed with frames of varying size stops allocating after every context has been used twice (hipFree waits for the whole device: a
// regrow in steady state stalls every batch in flight).
std::atomic<size_t> g_scratch_hwm[16][N_SCRATCH];
std::atomic<unsigned long long> g_scratch_allocs{0};      // hipMalloc calls for scratch so far (F3DS_HOST_PROF prints it per batch)
template <class T>
int regrow(Scratch<T>& b, size_t mark) {      // trades the allocation for one of mark + 25 % + 64 bytes: the contents are lost
    g_scratch_allocs.fetch_add(1, std::memory_order_relaxed);
    if (b.p) { HIPCHECK(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    const size_t want = mark + mark / 4 + 64;
    HIPCHECK(hipMalloc(&b.p, want));
    b.cap = want;
    return F3DS_OK;
}
template <class T>
int ensure(f3ds_ctx* c, Scratch<T>& b, size_t count, T** out) {
    size_t bytes = count * sizeof(T);
    if (bytes < 256) bytes = 256;
    size_t target = bytes;
    std::atomic<size_t>& hwm = g_scratch_hwm[c->device & 15][b.slot];
    size_t seen = hwm.load(std::memory_order_relaxed);
    while (seen < bytes && !hwm.compare_exchange_weak(seen, bytes, std::memory_order_relaxed)) {}
    if (seen > target && seen <= 4 * bytes) target = seen;      // (a frame of another scale altogether does not size this one)
    // ENSURE is an idempotent getter while the buffer covers the request: contents are only ever discarded when the request does not
    // fit (the caller is about to overwrite the buffer anyway).  The device-wide mark sizes such a regrow; buffers that are merely
    // below the mark are brought up to it by pregrow_scratch() at the start of a segment call, when no buffer holds frame state.
    if (b.cap < bytes) {
        if (b.p && (!c->cmds.empty() || c->ops.n) && referenced_by_pending_calls(c, b.p, b.cap)) {
            fprintf(stderr, "f3ds: internal error: regrowing a buffer that a recorded kernel call refers to\n");
            return F3DS_ERR_LOGIC;
        }
        static const bool trace = dev_getenv("F3DS_TRACE_ALLOC") != nullptr;
        if (trace && b.p) fprintf(stderr, "f3ds: regrow slot %d: cap %zu, request %zu, mark %zu, pending calls %zu\n", b.slot, b.cap, bytes, target, c->cmds.size());
        if (const int rc = regrow(b, target)) return rc;
    }
    *out = b.p;
    return F3DS_OK;
}
// Start of a segment call: nothing is recorded and no buffer holds state of a frame that will be read again (the call starts a new
// frame), so this is the one moment a context may trade a buffer for a larger one without losing anything.  Every allocated buffer
// that is below the device-wide mark of its slot (within 4x) goes to the mark (see g_scratch_hwm).
int pregrow_scratch(f3ds_ctx* c) {
    return c->each_scratch([c](auto& b) -> int {
        if (!b.p) return F3DS_OK;
        const size_t mark = g_scratch_hwm[c->device & 15][b.slot].load(std::memory_order_relaxed);
        if (b.cap >= mark || mark > 4 * b.cap) return F3DS_OK;
        return regrow(b, mark);
    });
}
#define ENSURE(buf, count, ptr) do { int rc_ = ensure(c, buf, (size_t)(count), &ptr); if (rc_) return rc_; } while (0)

// Workgroups per frame of a wide kernel.  A launch covers all frames of the batch (grid.y = frame), so a frame gets its
// share of a launch-wide budget of ~3 k workgroups (12 per CU) and the kernels loop (grid-stride) over the rest: with
// 192 frames per launch the streaming kernels of the sweeps run 1.5-2x faster on 32 fat workgroups per frame than on
// 300 thin ones (per-workgroup prologue: argument pack, counters, stamps), see DESIGN.md 4b.  The hash-probing /
// gathering kernels want every wave they can get and keep the old cap (grid_wide).  Set per batch call (one host thread).
thread_local size_t g_grid_cap = f3ds_policy::WIDE_CAP;
thread_local size_t g_wide_cap = f3ds_policy::WIDE_CAP;    // cap of grid_wide(): 2048 unless F3DS_GRID_CAP narrows every launch
thread_local int g_batch_frames = 1;      // frames of the batch call this thread is running
// batch calls inside f3ds_segment_batch right now, per device: a call whose merge dispatch shares the chip with other calls takes the 4-wave merge kernel (choose_merge_kind)
std::atomic<int> g_batch_calls[16];
struct BatchCallCount { int d; explicit BatchCallCount(int dev) : d(dev & 15) { g_batch_calls[d].fetch_add(1, std::memory_order_relaxed); } ~BatchCallCount() { g_batch_calls[d].fetch_sub(1, std::memory_order_relaxed); } };
size_t grid_cap_for_batch(int frames) {
    static const size_t target = dev_getenv("F3DS_GRID_TARGET") ? (size_t)atol(dev_getenv("F3DS_GRID_TARGET")) : f3ds_policy::GRID_TARGET;      // with six calls in flight: 24 576: 2 150, 12 288: 2 250, 6 144: 2 280, 3 072 ... 1 024: 2 340 Mpoints/s
    return f3ds_policy::grid_cap_for_batch(frames, target, g_sw.grid_cap);
}
// Start of every entry call that records kernels, after g_sw.read(): the launch widths of this call, noted in its frames (F3DS_DBG_LAUNCH_SHAPE).
// F3DS_GRID_CAP (development) replaces both caps by the given one; unset, grid_for() gets the batch's share and grid_wide() 2048 as ever.
inline void set_launch_shape(f3ds_ctx* const* frames, int nframes) {
    g_grid_cap = grid_cap_for_batch(nframes);
    g_wide_cap = f3ds_policy::wide_cap(g_sw.grid_cap);
    g_batch_frames = nframes;
    for (int i = 0; i < nframes; ++i) { frames[i]->launch_shape[0] = (uint32_t)g_grid_cap; frames[i]->launch_shape[1] = (uint32_t)g_wide_cap; frames[i]->launch_shape[2] = (uint32_t)nframes; }
}
inline uint32_t grid_wide(size_t work, int block) {
    size_t g = (work + block - 1) / block;
    return (uint32_t)(g < 1 ? 1 : (g > g_wide_cap ? g_wide_cap : g));
}
inline uint32_t grid_for(size_t work, int block) {
    size_t g = (work + block - 1) / block;
    if (g < 1) g = 1;
    if (g > g_grid_cap) g = g_grid_cap;
    return (uint32_t)g;
}
inline uint32_t pow2_ge(size_t x) { uint32_t p = 1; while (p < x) p <<= 1; return p; }
using f3ds_policy::bits_for;
constexpr f3ds_policy::TileLimits VT_LIMITS = {VT_TILE, (uint32_t)VT_CNT_BITS, VT_ENT_MAX, VT_TAB};
inline uint32_t seed_cell_grid(uint32_t C) { return (C + SEED_CELLS_PER_WG - 1u) / SEED_CELLS_PER_WG; }      // d_seed_nn / d_seed_filter: a wave per seed cell

// record one kernel call of frame `c` (nothing is launched here)
template <class K, class... As> void rec(f3ds_ctx* c, uint32_t gx, uint32_t lds, As... as);
// the fills / copies recorded since the last other call become one d_multi_op call (every frame of a batch records the same sequence, so the same grouping)
inline void flush_ops(f3ds_ctx* c) {
    if (!c->ops.n) return;
    const MultiOp m = c->ops; const uint32_t g = c->ops_grid;
    c->ops.n = 0; c->ops_grid = 0;
    rec<d_multi_op>(c, g, 0u, m);
}
template <class K, class... As>
void rec(f3ds_ctx* c, uint32_t gx, uint32_t lds, As... as) {
    if constexpr (!std::is_same<K, d_multi_op>::value) flush_ops(c);
    using Pack = pack_of<K>;
    static_assert(std::is_trivially_copyable<Pack>::value, "kernel arguments must be plain data");
    Pack p;
    memset(&p, 0, sizeof p);
    fill_pack(p, as...);
    (note_arg(c, as), ...);
    Cmd cmd; cmd.fn = &launch_fn<K>; cmd.gx = gx; cmd.lds = lds; cmd.bytes = (uint32_t)sizeof(Pack); cmd.off = (uint32_t)c->blob.size();
    c->blob.resize(c->blob.size() + sizeof(Pack));
    memcpy(c->blob.data() + cmd.off, &p, sizeof(Pack));
    c->cmds.push_back(cmd);
}
inline void rec_op(f3ds_ctx* c, void* dst, const void* src, uint32_t value, size_t bytes) {
    const uint32_t words = (uint32_t)((bytes + 3) / 4);
    if (c->ops.n == (uint32_t)MULTI_OPS) flush_ops(c);
    MultiOp& m = c->ops;
    if (m.n == 0) memset(&m, 0, sizeof m);
    m.dst[m.n] = static_cast<uint32_t*>(dst); m.src[m.n] = static_cast<const uint32_t*>(src); m.val[m.n] = value; m.words[m.n] = words; m.n++;      // (d_multi_op fills / copies any buffer word by word)
    const uint32_t g = grid_for(words, d_multi_op::BLOCK);
    if (g > c->ops_grid) c->ops_grid = g;
}
inline void rec_fill(f3ds_ctx* c, void* dst, uint32_t value, size_t bytes) { rec_op(c, dst, nullptr, value, bytes); }
inline void rec_copy(f3ds_ctx* c, void* dst, const void* src, size_t bytes) { rec_op(c, dst, src, 0u, bytes); }
// forget everything recorded and not launched
inline void reset_recording(f3ds_ctx* c) { c->cmds.clear(); c->blob.clear(); c->pend.clear(); c->ops.n = 0; c->ops_grid = 0; }

// a batch: the frames that are still being processed together, one stream, one argument arena
struct Batch {
    std::vector<f3ds_ctx*> fr;
    hipStream_t st = nullptr;
    f3ds_ctx* owner = nullptr;     // holds the argument arena and the stage events
};
// An entry point that records kernels starts from one of these two (after g_sw.read() and hipSetDevice): the batch on its owner's stream, the launch
// widths of the call, and nothing left recorded in its frames.  One context ...
inline Batch batch_of(f3ds_ctx* c) {
    Batch b; b.owner = c; b.st = c->stream;
    set_launch_shape(&c, 1); reset_recording(c);
    b.fr.push_back(c);
    return b;
}
// ... or ctxs[0..nctx) on the first one's stream: a context with another stream is waited for first (the frame state is read on the owner's stream)
int batch_of(f3ds_ctx** ctxs, int nctx, Batch& b) {
    b.owner = ctxs[0]; b.st = ctxs[0]->stream;
    set_launch_shape(ctxs, nctx);
    for (int i = 0; i < nctx; ++i) {
        if (ctxs[i]->stream != b.st) HIPCHECK(hipStreamSynchronize(ctxs[i]->stream));
        reset_recording(ctxs[i]);
        b.fr.push_back(ctxs[i]);
    }
    return F3DS_OK;
}

thread_local double g_t_wait = 0, g_t_launch = 0;
// F3DS_TRACE_ERR=1: say which stage refused a frame (development aid)
static int trace_err(int code, const char* where, const f3ds_ctx* c) {
    if (code && g_sw.trace_err)
        fprintf(stderr, "f3ds: error %d after %s (V %u, seeds %u, edges %u, chain overflow %d, capacity flag %d)\n", code, where, c->V, c->S0, c->h_dc->n_edges,
                c->h_dc->r_overflow, c->h_dc->ev_overflow);
    return code;
}
static inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// wait for an event / a stream; the time goes to the call's "waiting for the GPU" account
inline hipError_t timed_sync(hipEvent_t e) { const double t0 = now_ms(); const hipError_t r = hipEventSynchronize(e); g_t_wait += now_ms() - t0; return r; }
inline hipError_t timed_sync(hipStream_t st) { const double t0 = now_ms(); const hipError_t r = hipStreamSynchronize(st); g_t_wait += now_ms() - t0; return r; }
// A stage that runs again starts from cleared counters: the listed fields of DevCounters go to zero on the device (in stream order) and in the host's copy
template <class F> int clear_counter(f3ds_ctx* c, hipStream_t st, F DevCounters::*f) { c->h_dc->*f = 0; HIPCHECK(hipMemsetAsync(&(c->d_dc->*f), 0, sizeof(F), st)); return F3DS_OK; }
template <class... Fs> int clear_counters(f3ds_ctx* c, hipStream_t st, Fs DevCounters::*... f) { int rc = F3DS_OK; (void)((rc = clear_counter(c, st, f)) || ...); return rc; }
// zip the recorded calls of all live frames into batched dispatches
int flush(Batch& b, hipEvent_t before_launch = nullptr) {      // before_launch: recorded after the argument upload, right before the first dispatch
    if (b.fr.empty()) return F3DS_OK;
    for (f3ds_ctx* c : b.fr) flush_ops(c);
    const size_t ncmd = b.fr[0]->cmds.size();
    for (f3ds_ctx* c : b.fr) if (c->cmds.size() != ncmd) return F3DS_ERR_UNSUPPORTED;   // frames must take the same path
    if (ncmd == 0) return F3DS_OK;
    const uint32_t nf = (uint32_t)b.fr.size();
    size_t total = 0;
    std::vector<size_t> off(ncmd);
    for (size_t j = 0; j < ncmd; ++j) { off[j] = total; total += (((size_t)b.fr[0]->cmds[j].bytes * nf) + 63u) & ~(size_t)63u; }
    f3ds_ctx* o = b.owner;
    if (o->args_cap < total) {
        HIPCHECK(hipStreamSynchronize(b.st));
        for (int k = 0; k < 2; ++k) {
            if (o->h_args[k]) HIPCHECK(hipHostFree(o->h_args[k]));
            if (o->d_args[k]) HIPCHECK(hipFree(o->d_args[k]));
            o->h_args[k] = o->d_args[k] = nullptr; o->args_used[k] = false;
        }
        o->args_cap = total * 2;
        for (int k = 0; k < 2; ++k) {
            HIPCHECK(hipHostMalloc(&o->h_args[k], o->args_cap, hipHostMallocDefault));
            HIPCHECK(hipMalloc(&o->d_args[k], o->args_cap));
            if (!o->ev_args[k]) HIPCHECK(hipEventCreateWithFlags(&o->ev_args[k], hipEventDisableTiming));
        }
    }
    // The argument blocks of a flush travel pinned arena -> device arena -> kernels.  Two arena pairs are used in turn and an event marks the
    // end of the last dispatch that reads a pair, so the host packs and launches stage k+1 while stage k still runs: the only wait here is
    // for the flush before the previous one, which is long over (round 2 synchronised the stream at every flush).
    const int fl = o->args_flip; o->args_flip ^= 1;
    if (o->args_used[fl]) HIPCHECK(timed_sync(o->ev_args[fl]));
    unsigned char* const h_args = o->h_args[fl]; unsigned char* const d_args = o->d_args[fl];
    const double tl0 = now_ms();
    for (size_t j = 0; j < ncmd; ++j)
        for (uint32_t i = 0; i < nf; ++i) {
            const Cmd& cm = b.fr[i]->cmds[j];
            if (cm.fn != b.fr[0]->cmds[j].fn) return F3DS_ERR_UNSUPPORTED;
            memcpy(h_args + off[j] + (size_t)i * cm.bytes, b.fr[i]->blob.data() + cm.off, cm.bytes);
        }
    HIPCHECK(hipMemcpyAsync(d_args, h_args, total, hipMemcpyHostToDevice, b.st));
    if (before_launch) HIPCHECK(hipEventRecord(before_launch, b.st));
    for (size_t j = 0; j < ncmd; ++j) {
        uint32_t gx = 1, lds = 0;
        for (uint32_t i = 0; i < nf; ++i) { const Cmd& cm = b.fr[i]->cmds[j]; if (cm.gx > gx) gx = cm.gx; if (cm.lds > lds) lds = cm.lds; }
        HIPCHECK(b.fr[0]->cmds[j].fn(gx, nf, lds, b.st, d_args + off[j]));
    }
    HIPCHECK(hipEventRecord(o->ev_args[fl], b.st)); o->args_used[fl] = true;
    for (f3ds_ctx* c : b.fr) reset_recording(c);
    g_t_launch += now_ms() - tl0;
    return F3DS_OK;
}
// flush, then bring every live frame's counters to the host
int flush_sync(Batch& b) {
    int rc = flush(b);
    if (rc) return rc;
    const size_t nf = b.fr.size();
    if (nf == 1) HIPCHECK(hipMemcpyAsync(b.fr[0]->h_dc, b.fr[0]->d_dc, sizeof(DevCounters), hipMemcpyDeviceToHost, b.st));
    else if (nf > 1) {
        // one gather kernel + one copy instead of a copy per frame
        f3ds_ctx* o = b.owner;
        if (o->dcblk_cap < nf) {
            HIPCHECK(hipStreamSynchronize(b.st));
            if (o->d_dcblk) HIPCHECK(hipFree(o->d_dcblk));
            if (o->h_dcblk) HIPCHECK(hipHostFree(o->h_dcblk));
            o->dcblk_cap = nf * 2;
            HIPCHECK(hipMalloc(&o->d_dcblk, o->dcblk_cap * sizeof(DevCounters)));
            HIPCHECK(hipHostMalloc(&o->h_dcblk, o->dcblk_cap * sizeof(DevCounters), hipHostMallocDefault));
        }
        for (size_t i = 0; i < nf; ++i) rec<d_dc_gather>(b.fr[i], 1u, 0u, b.fr[i]->d_dc, o->d_dcblk + i);
        if ((rc = flush(b))) return rc;
        HIPCHECK(hipMemcpyAsync(o->h_dcblk, o->d_dcblk, nf * sizeof(DevCounters), hipMemcpyDeviceToHost, b.st));
    }
    HIPCHECK(timed_sync(b.st));
    HIPCHECK(hipGetLastError());
    if (nf > 1) for (size_t i = 0; i < nf; ++i) *b.fr[i]->h_dc = b.owner->h_dcblk[i];
    return F3DS_OK;
}

// inclusive scan of n uint32 values (in -> out): always the same three calls so that frames of
// different sizes record identical sequences
int scan_u32(f3ds_ctx* c, const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t nt = n ? (n + SCAN_TILE - 1) / SCAN_TILE : 1u;
    uint32_t* tiles;
    ENSURE(c->tiles, nt, tiles);
    rec<d_scan_tiles>(c, nt, 0u, in, out, tiles, n);
    rec<d_scan_single>(c, 1u, 0u, tiles, nt);
    rec<d_scan_add>(c, nt, 0u, out, tiles, n);
    return F3DS_OK;
}
// stable sort of (key,val) pairs on the low `total_bits` bits (the same for every frame of a batch)
// (n_dev: the element count lives on the device and `n` only bounds it -- pair sorts only)
int radix_sort(f3ds_ctx* c, uint64_t* k0, uint32_t* v0, uint64_t* k1, uint32_t* v1, uint32_t n, int total_bits, uint64_t** keys_out, uint32_t** vals_out, int base_shift = 0, const uint32_t* n_dev = nullptr) {
    *keys_out = k0; if (vals_out) *vals_out = v0;
    if (total_bits <= 0) return F3DS_OK;
    const int passes = (total_bits + RS_MAXBITS - 1) / RS_MAXBITS;
    const int per = (total_bits + passes - 1) / passes;
    const uint32_t nb = n ? (n + RS_TILE - 1) / RS_TILE : 1u;
    uint32_t* hist;
    ENSURE(c->hist, (size_t)RS_BINS * nb, hist);
    int shift = 0;
    for (int p = 0; p < passes; ++p) {
        const int bits = (total_bits - shift) < per ? (total_bits - shift) : per;
        rec<d_radix_hist>(c, nb, 0u, k0, n, base_shift + shift, bits, hist, nb, n_dev);
        rec<d_scan_single>(c, 1u, 0u, hist, (uint32_t)((1u << bits) * nb));
        if (v0) rec<d_radix_scatter>(c, nb, 0u, k0, v0, k1, v1, n, base_shift + shift, bits, hist, nb, n_dev);
        else rec<d_radix_scatter_k>(c, nb, 0u, k0, k1, n, base_shift + shift, bits, hist, nb);      // payload in the key's low bits
        std::swap(k0, k1); std::swap(v0, v1);
        shift += bits;
    }
    *keys_out = k0; if (vals_out) *vals_out = v0;
    return F3DS_OK;
}

// ---------------------------------------------------------------- per-frame stage recorders ------
// stage 0a: bounding box and grid
int seg_bbox(f3ds_ctx* c) {
    rec<d_init_counters>(c, 1u, 0u, c->d_dc);
    rec<d_bbox>(c, grid_for(c->n, 256 * 8) < 512 ? grid_for(c->n, 256 * 8) : 512u, 0u, c->d_pts, c->n, c->fa, c->d_dc);
    rec<d_grid>(c, 1u, 0u, c->d_dc, c->prm.voxel_res, c->d_grid);
    return F3DS_OK;
}
// stage 0b: Morton keys, stable sort, voxel segments
int seg_sort(f3ds_ctx* c, int sort_bits, int idxbits) {      // idxbits >= 0: (code << idxbits) | index in one array; -1: (key, index) pairs
    const uint32_t n = c->n;
    uint64_t *k0, *k1; uint32_t *v0 = nullptr, *v1 = nullptr, *flags, *incl, *seg_start; int* pt_voxel;
    ENSURE(c->keys0, n, k0); ENSURE(c->keys1, n, k1);
    if (idxbits < 0) { ENSURE(c->vals0, n, v0); ENSURE(c->vals1, n, v1); }
    ENSURE(c->flags, n, flags); ENSURE(c->incl, n, incl); ENSURE(c->seg_start, (size_t)n + 1, seg_start);
    ENSURE(c->pt_voxel, n, pt_voxel);
    c->idxbits = idxbits;
    const int ks = idxbits < 0 ? 0 : idxbits;
    rec<d_keys>(c, grid_for(n, d_keys::BLOCK), 0u, c->d_pts, n, c->fa, c->d_grid, k0, v0, ks);
    c->vs = nullptr;
    int rc = radix_sort(c, k0, v0, k1, v1, n, sort_bits, &c->ks, &c->vs, ks);
    if (rc) return rc;
    const uint64_t invalid = 1ull << (3 * c->h_dc->depth);
    if (g_sw.split_voxel_accum) {      // development: round 2's chain (d_point_gather reads the rank array)
        rec<d_heads>(c, grid_for(n, d_heads::BLOCK), 0u, c->ks, n, invalid, flags, ks);
        if ((rc = scan_u32(c, flags, incl, n))) return rc;
        rec<d_segstart>(c, grid_for(n, d_segstart::BLOCK), 0u, c->ks, flags, incl, n, invalid, seg_start, &c->d_dc->n_voxels, &c->d_dc->n_valid, ks);
        return F3DS_OK;
    }
    const uint32_t nt = n ? (n + SCAN_TILE - 1) / SCAN_TILE : 1u;
    uint32_t* tiles; ENSURE(c->tiles, nt, tiles);
    rec<d_seg_count>(c, nt, 0u, c->ks, n, invalid, ks, tiles);
    rec<d_scan_single>(c, 1u, 0u, tiles, nt);
    rec<d_seg_write>(c, nt, 0u, c->ks, n, invalid, ks, tiles, seg_start, &c->d_dc->n_voxels, &c->d_dc->n_valid);
    return F3DS_OK;
}
// stage 0b + 0c without sorting the points (f3ds_kernels.inc, "stage 0 without sorting the points"): per-tile LDS grouping, sort of the tiles' descriptors, per-leaf
// point lists, ordered leaf sums.  Everything is recorded before V is known: buffers and grids are sized by bounds, the kernels read the counts from the device.
int seg_vox_tiles(f3ds_ctx* c, int code_bits, int tile_bits) {      // (code_bits, tile_bits: the same for every frame of a batch -- the frames record the same sort passes)
    const uint32_t n = c->n;
    const uint32_t ntiles = (n + VT_TILE - 1u) / VT_TILE;
    const uint64_t dcap64 = (uint64_t)ntiles * VT_ENT_MAX;
    if (!f3ds_policy::tile_path_fits(code_bits, tile_bits, n, VT_LIMITS)) return F3DS_ERR_UNSUPPORTED;      // (the caller takes the sort path: segment_batch_from asks the same question first)
    const uint32_t dcap = (uint32_t)dcap64;
    const uint64_t fin = c->h_dc->n_finite;
    const uint32_t capV = (uint32_t)std::max<uint64_t>(256u, std::min<uint64_t>(fin, dcap));
    c->vox_cap = capV;
    uint64_t *k0, *k1; uint32_t *ploc, *v0, *v1, *part, *vkey, *vcount, *seg_start, *list; uint2* bo_te; float* vf; int* pt_voxel;
    const uint32_t nchunks = (dcap + DS_CHUNK - 1u) / DS_CHUNK;
    ENSURE(c->pslot, n, ploc); ENSURE(c->keys0, dcap, k0); ENSURE(c->keys1, dcap, k1); ENSURE(c->vals0, dcap, v0); ENSURE(c->vals1, dcap, v1);
    { uint32_t* w; ENSURE(c->hcnt, (size_t)ntiles * VT_TAB * 2 + 2u * nchunks, w); bo_te = reinterpret_cast<uint2*>(w); part = w + (size_t)ntiles * VT_TAB * 2; }      // ONE allocation, two views: the tiles' (base, entry) tables as uint2 pairs, then the chunk partials as words
    ENSURE(c->vkey, (size_t)capV * 3, vkey); ENSURE(c->vcount, capV, vcount); ENSURE(c->vf, (size_t)capV * 12, vf);
    ENSURE(c->seg_start, (size_t)capV + 1, seg_start); ENSURE(c->vlist, n, list); ENSURE(c->pt_voxel, n, pt_voxel);
    { uint32_t *f, *incl; ENSURE(c->flags, capV, f); ENSURE(c->incl, capV, incl); }      // (the seed stage scans V / C flags through them without asking)
    c->idxbits = -1; c->ks = nullptr; c->vs = nullptr;
    rec<d_tile_keys>(c, std::min<uint32_t>(ntiles, (uint32_t)g_grid_cap * 16u), 0u, c->d_pts, n, c->fa, c->d_grid, ploc, k0, v0, dcap, tile_bits, c->d_dc);
    uint64_t* ks; uint32_t* vs;
    int rc = radix_sort(c, k0, v0, k1, v1, dcap, code_bits + tile_bits, &ks, &vs, VT_CNT_BITS, &c->d_dc->seg_count);      // (the bits above the count field)
    if (rc) return rc;
    rec<d_desc_part>(c, nchunks, 0u, ks, dcap, tile_bits, part, c->d_dc);
    rec<d_desc_offsets>(c, 1u, 0u, part, dcap, capV, seg_start, c->d_dc);
    rec<d_desc_apply>(c, nchunks, 0u, ks, vs, dcap, capV, tile_bits, c->fa, c->d_grid, part, bo_te, seg_start, vkey, c->d_dc);
    rec<d_tile_place>(c, std::min<uint32_t>(ntiles, (uint32_t)g_grid_cap * 16u), 0u, ploc, n, bo_te, list, pt_voxel, c->d_dc);
    rec<d_voxel_list_accum>(c, std::min<uint32_t>(grid_wide(capV, d_voxel_list_accum::BLOCK), std::max<uint32_t>(64u, grid_wide(n / 8u, d_voxel_list_accum::BLOCK))), 0u, c->d_pts, list, seg_start, c->fa, vf, vcount, c->d_dc, capV);
    c->vox_hashed = true;
    return F3DS_OK;
}
// the voxel table of the neighbour search (f3ds_kernels.inc, vt_* / bt_*) from the leaf keys, then the search.  Grids of depth <= 12: an entry of two words per 4x4x4 block, at most V
// of them, in the hkeys buffer; deeper grids: an entry per voxel, keys in hkeys and ordinals in hvals.  The kernels choose by the depth on the device, as the host does here.
// wgs: workgroups that build the table -- one on the tile path (workgroup-scope atomics), several for a frame that has the chip to itself.
int seg_neighbors(f3ds_ctx* c, uint32_t wgs) {
    const uint32_t V = c->V;
    const bool blocks = c->h_dc->depth <= N_BLOCK_DEPTH_MAX;
    const uint32_t cap = blocks ? pow2_ge((size_t)V + 16) : pow2_ge((size_t)V * 2 + 16);
    const size_t words = blocks ? (size_t)cap * 2 : cap;      // (8-byte words of hkeys)
    uint32_t* hvals = nullptr; int *nbr, *nbrT; uint64_t* hkeys;
    c->hmask = cap - 1;
    ENSURE(c->nbr, (size_t)V * 27, nbr); ENSURE(c->nbrT, (size_t)V * 27, nbrT); ENSURE(c->hkeys, words, hkeys);
    if (!blocks) ENSURE(c->hvals, cap, hvals);
    rec_fill(c, hkeys, 0xFFFFFFFFu, words * 8);
    rec<d_vox_table>(c, wgs, 0u, c->vkey.p, V, c->d_grid, hkeys, hvals, c->hmask);
    rec<d_neighbors>(c, grid_wide((size_t)V * 27, d_neighbors::BLOCK), 0u, c->vkey.p, c->d_dc, c->d_grid, c->fa.leaf_order, hkeys, hvals, c->hmask, nbr, nbrT);
    return F3DS_OK;
}
// stage 0c + 1 + 2a: voxel sums, neighbour tables, normals, seed grid growth
int seg_voxels(f3ds_ctx* c) {
    const uint32_t V = c->V, n = c->n;
    if (c->vox_hashed) return seg_neighbors(c, 1u);      // the leaf sums exist already (seg_vox_tiles)
    uint32_t *vkey, *vcount; float *vf;
    ENSURE(c->vkey, (size_t)V * 3, vkey); ENSURE(c->vcount, V, vcount); ENSURE(c->vf, (size_t)V * 12, vf);
    if (g_sw.split_voxel_accum) {      // development: round 2's two kernels (a sorted copy of the frame in between)
        P16* spts; ENSURE(c->spts, n, spts);
        rec<d_point_gather>(c, grid_wide(n, d_point_gather::BLOCK), 0u, c->d_pts, c->vs, c->ks, c->idxbits < 0 ? 0 : c->idxbits, c->incl.p, n, c->d_dc, spts, c->pt_voxel.p);
        rec<d_voxel_accum>(c, grid_wide(V, d_voxel_accum::BLOCK), 0u, spts, c->ks, c->idxbits < 0 ? 0 : c->idxbits, c->seg_start.p, c->d_dc, c->fa, c->d_grid, vkey, vcount, vf);
    } else
        rec<d_voxel_gather_accum>(c, grid_wide(V, d_voxel_gather_accum::BLOCK), 0u, c->d_pts, c->vs, c->ks, c->idxbits < 0 ? 0 : c->idxbits, c->seg_start.p, n, c->d_dc, c->fa, c->d_grid, vkey, vcount, vf, c->pt_voxel.p);
    return seg_neighbors(c, grid_for(V, 4096));
}
// stage 1b: voxel normals -- ONE launch per batch call, bracketed by its own pair of events (f3ds_result.ms_stage[7]: besides the merge
// loop the only kernel of the path whose launch duration is measured live, bench.py's roofline picks the longer of the two)
int seg_normals(f3ds_ctx* c) {
    const uint32_t nt = (c->V + NT_TILE - 1) / NT_TILE;
    uint32_t *tn1, *tord, *tslots;      // the tiles' one-ring tables, built on the way for the sweeps (d_sweep_R_pre, d_sweep_claim)
    ENSURE(c->tile_n1, nt, tn1); ENSURE(c->tile_ord, (size_t)nt * NT_RING1, tord); ENSURE(c->tile_slots, (size_t)nt * SW_SLOT_WORDS * NT_TILE, tslots);
    // One workgroup per tile by default.  F3DS_NORMALS_WGS=<n> (experiment): a launch-wide budget of n workgroups, each walking a run of
    // tiles -- placed once, a 72 KB six-wave workgroup then keeps its compute unit instead of competing for one per tile.  With six calls in flight the
    // launch drops from 50-100 ms to 30 ms and the sweeps of the other calls grow by as much (2 140-2 155 vs 2 170 Mpoints/s on one box); alone it is
    // twice as slow (83 vs 43 us per frame: two rounds of long-lived workgroups).  The chip's compute-unit time is conserved; only work removed counts.
#ifdef F3DS_NORMALS_LOOP
    static const uint32_t budget = dev_getenv("F3DS_NORMALS_WGS") ? (uint32_t)atoi(dev_getenv("F3DS_NORMALS_WGS")) : 0u;
#else
    static const uint32_t budget = 0u;      // (the tile loop is compiled in with make EXTRA=-DF3DS_NORMALS_LOOP only)
#endif
    const uint32_t share = budget ? std::max(2u, budget / (uint32_t)g_batch_frames) : nt;
    // 256 threads per tile for the calls of a batch pipeline (their workgroups fit beside the 4-wave merge loops of the other calls), 384 otherwise (kernels.inc)
    const int nthr_env = g_sw.normals_threads;
    const uint32_t holes = g_sw.tile_holes;
    if (f3ds_policy::normals_threads(g_batch_frames, nthr_env) == 256)
        rec<d_normals_t<256>>(c, std::min(nt, share), 0u, c->vf.p, c->nbr.p, c->d_dc, tn1, tord, tslots, holes);
    else
        rec<d_normals_t<384>>(c, std::min(nt, share), 0u, c->vf.p, c->nbr.p, c->d_dc, tn1, tord, tslots, holes);
    return F3DS_OK;
}
// stage 2a: seed grid growth
int seg_seed_grid(f3ds_ctx* c) {
    const uint32_t V = c->V;
    float* boxes; const float* vf = c->vf.p;
    const uint32_t nchunks = (V + SEED_CHUNK - 1) / SEED_CHUNK;
    ENSURE(c->boxes, (size_t)nchunks * 6, boxes);
    rec<d_chunkbox>(c, nchunks, 0u, vf, c->d_dc, boxes);
    rec<d_seed_grow>(c, 1u, 0u, vf, boxes, c->d_dc, c->prm.seed_res, c->d_sgrid);
    return F3DS_OK;
}
// stage 2b: seed cells (sort voxels by cell)
int seg_seed_cells(f3ds_ctx* c, int sort_bits, int max_sdepth) {
    const uint32_t V = c->V;
    uint32_t *ckey, *cell_start, *v0, *v1; uint64_t *k0 = c->keys0.p, *k1 = c->keys1.p;
    ENSURE(c->vals0, V, v0); ENSURE(c->vals1, V, v1);
    ENSURE(c->ckey, (size_t)V * 3, ckey); ENSURE(c->cell_start, (size_t)V + 1, cell_start);
    rec<d_seed_keys>(c, grid_for(V, d_seed_keys::BLOCK), 0u, c->vf.p, c->d_dc, c->d_sgrid, ckey, k0, v0);
    int rc = radix_sort(c, k0, v0, k1, v1, V, sort_bits, &c->cks, &c->cvs);
    if (rc) return rc;
    const uint64_t climit = max_sdepth >= 21 ? 0xFFFFFFFFFFFFFFFFull : (1ull << (3 * max_sdepth));
    rec<d_heads>(c, grid_for(V, d_heads::BLOCK), 0u, c->cks, V, climit, c->flags.p, 0);
    if ((rc = scan_u32(c, c->flags.p, c->incl.p, V))) return rc;
    rec<d_segstart>(c, grid_for(V, d_segstart::BLOCK), 0u, c->cks, c->flags.p, c->incl.p, V, climit, cell_start, &c->d_dc->n_cells, &c->d_dc->seg_count, 0);
    return F3DS_OK;
}
// stage 2c: nearest voxel per cell, radius filter, kept seeds
int seg_seeds(f3ds_ctx* c) {
    const uint32_t V = c->V, C = c->C;
    uint32_t *sorted_vox, *chvals, *keep; uint64_t* chk; int *seed_orig, *seed_kept;
    const uint32_t ccap = pow2_ge((size_t)C * 2 + 16);
    ENSURE(c->chv, V, sorted_vox); ENSURE(c->chk, ccap, chk); ENSURE(c->chvals, ccap, chvals);
    ENSURE(c->seed_orig, C, seed_orig); ENSURE(c->seed_kept, C, seed_kept); ENSURE(c->keep, C, keep);
    rec_copy(c, sorted_vox, c->cvs, (size_t)V * 4);      // the sort buffers are reused later
    rec_fill(c, chk, 0xFFFFFFFFu, (size_t)ccap * 8);
    const uint32_t* ckey = c->ckey.p; const uint32_t* cell_start = c->cell_start.p; const float* vf = c->vf.p;
    rec<d_cell_hash>(c, grid_for(C, d_cell_hash::BLOCK), 0u, ckey, sorted_vox, cell_start, c->d_dc, chk, chvals, ccap - 1);
    rec<d_seed_nn>(c, seed_cell_grid(C), 0u, vf, ckey, sorted_vox, cell_start, c->d_dc, c->d_sgrid, chk, chvals, ccap - 1, seed_orig);
    rec<d_seed_filter>(c, seed_cell_grid(C), 0u, vf, ckey, sorted_vox, cell_start, c->d_dc, c->d_sgrid, chk, chvals, ccap - 1, seed_orig, a_radius_sq(c->prm.seed_res), a_min_points(c->prm.seed_res, c->prm.voxel_res), keep);
    int rc = scan_u32(c, keep, c->incl.p, C);
    if (rc) return rc;
    rec<d_seed_compact>(c, grid_for(C, d_seed_compact::BLOCK), 0u, seed_orig, keep, c->incl.p, c->d_dc, seed_kept);
    return F3DS_OK;
}
// stage 3: helpers and all label-propagation sweeps
// The state a run of sweeps works on: extract's own (ctx members) or the copy refineSupervoxels continues from
struct SweepBufs {
    Scratch<uint32_t> *owner; Scratch<float> *dist, *hc; Scratch<uint32_t> *hcount, *hlo, *hhi; Scratch<int>* ghost_vox; Scratch<unsigned char> *ghost_active, *ghost_done; Scratch<uint32_t> *ghost_head, *ghost_next, *htiles, *htcnt;
    const float* vf;        // voxel features (refine: the copy with the refined normals)
    const int* seeds;       // S0 seed voxels (refine: -1 for helpers erased earlier)
    bool reseed;            // refine: centroids are kept, helpers without a seed stay empty
};
int seg_sweeps_on(f3ds_ctx* c, const SweepBufs& sb) {
    const uint32_t V = c->V, S0 = c->S0;
    const f3ds_params& prm = c->prm;
    uint32_t *owner0, *ownR, *hcount, *hlo, *hhi, *ghost_head, *ghost_next; float *dist0, *hc; unsigned char *R, *ghost_active, *ghost_done; int* ghost_vox;
    ENSURE(*sb.owner, V, owner0); ENSURE(c->ownR, V, ownR); ENSURE(*sb.dist, V, dist0);
    ENSURE(c->R, V, R); ENSURE(*sb.hc, (size_t)(S0 + 1) * 12, hc); ENSURE(*sb.hcount, S0 + 1, hcount);
    ENSURE(*sb.hlo, S0 + 1, hlo); ENSURE(*sb.hhi, S0 + 1, hhi); ENSURE(*sb.ghost_vox, S0 + 1, ghost_vox);
    ENSURE(*sb.ghost_active, S0 + 1, ghost_active); ENSURE(*sb.ghost_done, S0 + 1, ghost_done);
    ENSURE(*sb.ghost_head, V, ghost_head); ENSURE(*sb.ghost_next, S0 + 1, ghost_next);
    const uint32_t T = (V + 63u) / 64u;
    uint32_t *tiles4, *trr, *hD;
    ENSURE(c->tstamp, (size_t)4 * T, tiles4); ENSURE(c->tround, (size_t)(F3DS_R_ROUNDS - 1) * T, trr); ENSURE(c->hdirty, S0 + 1, hD);
    uint32_t *tl, *tcnt; ENSURE(*sb.htiles, (size_t)(S0 + 1) * HT_CAP, tl); ENSURE(*sb.htcnt, S0 + 1, tcnt);
    uint32_t *wl, *wl2, *tmask; ENSURE(c->vwl, V, wl); ENSURE(c->vwl2, V, wl2); ENSURE(c->vtmask, V, tmask);
    rec_fill(c, tiles4, 0u, (size_t)4 * T * 4);
    rec_fill(c, trr, 0u, (size_t)(F3DS_R_ROUNDS - 1) * T * 4);
    rec_fill(c, hD, 0u, (size_t)(S0 + 1) * 4);
    rec_fill(c, owner0, 0u, (size_t)V * 4);
    rec_fill(c, ghost_head, 0u, (size_t)V * 4);
    rec_fill(c, ghost_next, 0u, (size_t)(S0 + 1) * 4);
    { const float fmax = F3DS_FLT_MAX; uint32_t bits; memcpy(&bits, &fmax, 4); rec_fill(c, dist0, bits, (size_t)V * 4); }
    if (sb.reseed) {
        rec<d_reseed_own>(c, grid_for(S0, d_reseed_own::BLOCK), 0u, sb.seeds, S0, owner0);
        rec<d_reseed_init>(c, grid_for(S0 + 1, d_reseed_init::BLOCK), 0u, sb.seeds, S0, owner0, ghost_vox, ghost_active, ghost_done, hlo, hhi, hcount, tl, tcnt);
    } else {
        rec<d_helper_own>(c, grid_for(S0, d_helper_own::BLOCK), 0u, sb.seeds, S0, owner0);
        rec<d_helper_init>(c, grid_for(S0 + 1, d_helper_init::BLOCK), 0u, sb.seeds, S0, owner0, ghost_vox, ghost_active, ghost_done, hlo, hhi, hcount, hc, tl, tcnt);
    }
    const int* nbrT = c->nbrT.p; const float* vf = sb.vf;
    SweepFrame a;
    a.sv = SweepView{(int)V, nbrT, vf, owner0, dist0, hc, ghost_head, ghost_next, &c->d_dc->n_ghosts, prm.seed_res, prm.w_normal, prm.w_color, prm.w_spatial, c->nbr.p};
    a.R = R; a.ownR = ownR; a.owner_out = owner0; a.dist_out = dist0;
    a.ghost_done = ghost_done; a.ghost_active = ghost_active; a.ghost_vox = ghost_vox; a.ghost_head = ghost_head; a.ghost_next = ghost_next;
    a.hlo = hlo; a.hhi = hhi; a.hcount = hcount; a.hc = hc; a.dc = c->d_dc; a.S0 = S0;
    a.tR0 = tiles4; a.tR1 = tiles4 + T; a.tC0 = tiles4 + 2 * (size_t)T; a.tC1 = tiles4 + 3 * (size_t)T; a.tRr = trr; a.hD = hD; a.T = T; a.tl = tl; a.tcnt = tcnt; a.wl = wl; a.wl2 = wl2; a.tmask = tmask;
    a.thr = a_sweep_thr(V, g_inc_shift);
    if (!g_sw.sweep_tiles) a.tile_n1 = nullptr;      // development: F3DS_SWEEP_TILES=0 keeps the sweeps on their global-gather path (A/B, tests)
    else a.tile_n1 = c->tile_n1.p;
    a.tile_ord = c->tile_ord.p; a.tile_slots = c->tile_slots.p;
    for (uint32_t t = 0; t < c->res.sweeps; ++t) {
        if (a_sweep_needs_clear(t)) rec_fill(c, R, 0u, V);
        rec<d_sweep_begin>(c, 1u, 0u, a, t);
        // (sweeps 0 and 1 are full by construction -- d_sweep_begin: marking starts after a sweep t >= 1 at the earliest, and a sweep skips tiles only if the one
        // before it was marking --, so their incremental launches would be no-ops on every frame: not recorded)
        const bool can_skip = t >= 2u;
        const bool rounds = g_inc_shift >= 0 && can_skip;
        const uint32_t nrounds = rounds ? g_sw.r_rounds : 0u;      // (F3DS_R_ROUNDS; F3DS_R_ROUNDS_RUN=1|2 lets tests reach the non-convergence fallback of d_sweep_R)
        rec<d_sweep_R_first>(c, grid_for(V, d_sweep_R_first::BLOCK), 0u, a, a_sweep_tag(t), t, nrounds);      // pre-pass of a full sweep | round 0 of an incremental one
        for (uint32_t r = 1; r < nrounds; ++r) rec<d_sweep_R_round>(c, grid_for(V, d_sweep_R_round::BLOCK), 0u, a, t, r, nrounds);
        for (uint32_t pass = 0; pass < F3DS_R_PASSES; ++pass) rec<d_sweep_R>(c, pass == 0 ? grid_for(V, d_sweep_R::BLOCK) : 64u, 0u, a, a_sweep_tag(t), t, pass);
        rec<d_sweep_R_tail>(c, 1u, 0u, a, a_sweep_tag(t), t);
        rec<d_sweep_claim>(c, grid_for(V, d_sweep_claim::BLOCK), 0u, a, t);
        rec<d_centroid>(c, grid_for((size_t)S0 * 64u, d_centroid::BLOCK), 0u, a, t);
    }
    return F3DS_OK;
}
int seg_sweeps(f3ds_ctx* c) {
    SweepBufs sb{&c->owner0, &c->dist0, &c->hc, &c->hcount, &c->hlo, &c->hhi, &c->ghost_vox, &c->ghost_active, &c->ghost_done, &c->ghost_head, &c->ghost_next, &c->htiles, &c->htcnt, c->vf.p, c->seed_kept.p, false};
    return seg_sweeps_on(c, sb);
}
// stage 4a: supervoxel payload rows, adjacency set
int seg_supervoxels(f3ds_ctx* c) {
    const uint32_t V = c->V, S0 = c->S0;
    uint32_t *loff, *rcnt0, *ev0, *ev1; float *rows, *racc0, *rrec0; int* row_voxel; unsigned char* ralive0; uint64_t *ehk, *ek0, *ek1;
    ENSURE(c->loff, S0 + 2, loff);
    int rc = scan_u32(c, c->hcount.p, loff + 1, S0 + 1);     // loff[h+1] = inclusive => loff[h] = exclusive
    if (rc) return rc;
    rec_fill(c, loff, 0u, 4);
    ENSURE(c->rows, ((size_t)V + S0 + 1) * 12, rows); ENSURE(c->row_voxel, (size_t)V + S0 + 1, row_voxel);      // ghosts add at most S0 rows
    ENSURE(c->racc0, (size_t)(S0 + 1) * 12, racc0); ENSURE(c->rcnt0, S0 + 1, rcnt0); ENSURE(c->rrec0, (size_t)(S0 + 1) * 16, rrec0);
    ENSURE(c->ralive0, S0 + 1, ralive0);
    rec_fill(c, ralive0, 0u, S0 + 1);
    rec_fill(c, rcnt0, 0u, (size_t)(S0 + 1) * 4);
    rec<d_sv_fill>(c, S0 ? (S0 + 3u) / 4u : 1u, 0u,      // (four helpers per workgroup, one per row of its wave)
                   c->vf.p, c->owner0.p, S0, c->hlo.p, c->hhi.p, c->ghost_vox.p, c->ghost_active.p, c->hcount.p, loff, c->hc.p, rows, row_voxel, racc0, rcnt0, rrec0, ralive0, c->d_dc, c->htiles.p, c->htcnt.p, V);
    const uint32_t ecap = f3ds_policy::edge_capacity(S0, c->edge_mult);
    const uint32_t ehcap = pow2_ge((size_t)ecap * 2);
    ENSURE(c->ehk, ehcap, ehk);
    ENSURE(c->ekeys0, ecap, ek0); ENSURE(c->ekeys1, ecap, ek1); ENSURE(c->evals0, ecap, ev0); ENSURE(c->evals1, ecap, ev1);
    rec_fill(c, ehk, 0xFFFFFFFFu, (size_t)ehcap * 8);
    rec<d_edges>(c, grid_for(V, d_edges::BLOCK), 0u, V, S0, c->nbrT.p, c->owner0.p, ehk, ehcap - 1, ek0, ecap, c->d_dc);
    rec<d_edges_ghost>(c, grid_for(S0, d_edges_ghost::BLOCK), 0u, V, S0, c->ghost_vox.p, c->ghost_active.p, c->nbrT.p, c->owner0.p, ehk, ehcap - 1, ek0, ecap, c->d_dc);
    return F3DS_OK;
}
// stage 4b: sorted edge list
int seg_edge_sort(f3ds_ctx* c, int sort_bits) {
    const uint32_t E = c->E, S0 = c->S0;
    uint32_t *ea0, *eb0; ENSURE(c->ea0, E, ea0); ENSURE(c->eb0, E, eb0);
    uint32_t* evs;
    { uint32_t* h; ENSURE(c->hist, (size_t)RS_BINS * (((size_t)E * 2 + RS_TILE - 1) / RS_TILE + 1), h); }      // also holds the 2E-delta sort of seg_cluster_front, recorded before this one is flushed
    rec<d_iota>(c, grid_for(E, d_iota::BLOCK), 0u, c->evals0.p, E);
    int rc = radix_sort(c, c->ekeys0.p, c->evals0.p, c->ekeys1.p, c->evals1.p, E, sort_bits, &c->eks, &evs);
    if (rc) return rc;
    rec<d_edge_init>(c, grid_for(E, d_edge_init::BLOCK), 0u, c->eks, E, S0, ea0, eb0);
    return F3DS_OK;
}
// d_merge_il_t<NW, RES>: LDS a frame with E adjacencies needs (merge_il_offsets, f3ds_kernels.inc) and whether the kernel can take it
bool merge_il_layout(uint32_t E, uint32_t S0, int nw, int res, MergeLds* xl) {      // res: 2 = endpoints + keys in LDS, 0 = both in global memory
    memset(xl, 0, sizeof *xl);
    if ((uint64_t)E * (res == 2 ? 10u : 2u) > (1u << 22)) return false;              // (far beyond what fits: keep the 32-bit offsets below honest)
    const MergeIlLayout L = merge_il_offsets(E, nw, res);
    xl->Ecap = L.Ecap; xl->NGcap = L.NGcap; xl->lds_bytes = L.total; xl->keys_in_lds = res;
    xl->spec = g_sw.merge_spec ? 1 : 0;      // (the speculative second merge of an epoch; F3DS_MERGE_SPEC=0 switches it off)
    return L.total <= MC_LDS_LIMIT && S0 <= 65534u;
}
// merge kernel of a batch: MK_GLOBAL (d_merge, everything in HBM: any size) or MK_IL + (8 waves ? 0 : 2) + (res == 2 ? 0 : 1)
enum MergeKind { MK_GLOBAL = 0, MK_IL = 1 };
inline int mk_waves(int kind) { return (kind - MK_IL) >= 2 ? 4 : 8; }
inline int mk_res(int kind) { return (kind - MK_IL) % 2 ? 0 : 2; }
// Which merge kernel a batch runs (one dispatch for all its frames): 8 waves per frame with keys and endpoints in LDS -- the shortest loop, what a lone frame or
// a lone call wants.  A call of 16 frames or more that shares the device with other batch calls takes the 4-wave layout instead: its loop is longer, but a
// workgroup holds one wave slot and 250 registers per SIMD instead of two and 500, and the other calls' wide kernels run on the units the merge loops sit on
// (DESIGN.md 4i).  Results are identical whatever runs.  F3DS_MERGE_KEYS=lds|global says where the per-edge arrays live, F3DS_MERGE_NW=4|8 the width.
// A frame whose arrays fit neither way, or with more than 65534 seeds, takes d_merge.  F3DS_FORCE_GLOBAL_MERGE forces it (tests).
int choose_merge_kind(const std::vector<f3ds_ctx*>& fr, bool force_global) {
    if (force_global || g_sw.force_global_merge) return MK_GLOBAL;
    const bool e_keys = g_sw.merge_keys >= 0;
    const bool shared = fr.size() >= 16 && g_batch_calls[fr[0]->device & 15].load(std::memory_order_relaxed) >= 2;
    const int nw = g_sw.merge_nw ? (g_sw.merge_nw == 8 ? 8 : 4) : (shared ? 4 : 8);
    const int first = e_keys ? (g_sw.merge_keys == 2 ? 2 : 0) : (shared ? g_merge_shared_res : 2);
    for (int res = first; res >= (e_keys ? first : 0); res -= 2) {
        bool ok = true;
        for (f3ds_ctx* c : fr) { MergeLds t; if (!merge_il_layout(c->E, c->S0, nw, res, &t)) { ok = false; break; } }
        if (ok) return MK_IL + (nw == 8 ? 0 : 2) + (res == 2 ? 0 : 1);
    }
    return MK_GLOBAL;
}
// stage 4c: Clustering::cluster(threshold) up to the merge loop: working copies, deltas, lambda / cdf, weights
int seg_cluster_front(f3ds_ctx* c, const f3ds_params* prm, int kind) {
    const bool use_lds = kind != MK_GLOBAL;
    const uint32_t S0 = c->S0, E = c->E;
    // main(): set_merging / set_lambda / set_bins_num (src/supervoxel_clustering.cpp:415-423)
    float lambda = 0.5f; int bins = 500;
    if (prm->merging == F3DS_MANUAL_LAMBDA && prm->lambda != 0) { if (prm->lambda < 0 || prm->lambda > 1) return F3DS_ERR_RANGE; lambda = prm->lambda; }
    if (prm->merging == F3DS_EQUALIZATION && prm->bins != 0) { if (prm->bins < 0) return F3DS_ERR_RANGE; bins = (short)prm->bins; }
    if (prm->merging < 0 || prm->merging > 2 || prm->color_metric < 0 || prm->color_metric > 1 || prm->geom_metric < 0 || prm->geom_metric > 1) return F3DS_ERR_ARG;
    MergeDev m;
    memset(&m, 0, sizeof m);
    m.E = E; m.S0 = S0; m.threshold = prm->threshold; m.dc = c->d_dc;
    m.ev_cap = f3ds_policy::event_capacity(E, c->ev_mult);      // weight-history events: grown on demand (run_cluster)
    ENSURE(c->ea, E, m.ea); ENSURE(c->eb, E, m.eb); ENSURE(c->ew, ((size_t)E + 2047) & ~(size_t)2047, m.ew); /* d_merge: weights; d_merge_cw_t<., 0>: endpoints */ ENSURE(c->eku, ((size_t)E + 2047) & ~(size_t)2047, m.eku);      // (Ecap of the widest merge kernel)
    ENSURE(c->ehist, E, m.ehist); ENSURE(c->ealive, E, m.ealive);
    ENSURE(c->ev_epoch, m.ev_cap, m.ev_epoch); ENSURE(c->ev_key, m.ev_cap, m.ev_key); ENSURE(c->ev_prev, m.ev_cap, m.ev_prev);
    ENSURE(c->racc, (size_t)(S0 + 1) * 12, m.racc); ENSURE(c->rrec, (size_t)(S0 + 1) * 16, m.rrec);
    ENSURE(c->rcnt, S0 + 1, m.rcnt); ENSURE(c->ralive, S0 + 1, m.ralive);
    ENSURE(c->rhead, S0 + 1, m.rhead); ENSURE(c->rtail, S0 + 1, m.rtail); ENSURE(c->lnext, S0 + 1, m.lnext);
    ENSURE(c->parent, S0 + 1, m.parent); ENSURE(c->markA, S0 + 1, m.markA); ENSURE(c->markB, S0 + 1, m.markB);
    ENSURE(c->tl, E, m.tl); ENSURE(c->merges, (size_t)(S0 + 1) * 3, m.merges);
    m.loff = c->loff.p; m.llen = c->hcount.p; m.rows = c->rows.p;
    float* deltas; ENSURE(c->deltas, (size_t)E * 2, deltas);
    // working copies of the supervoxel state (a second cluster() call starts from the same initial state)
    rec_copy(c, m.racc, c->racc0.p, (size_t)(S0 + 1) * 12 * 4);
    rec_copy(c, m.rrec, c->rrec0.p, (size_t)(S0 + 1) * 16 * 4);
    rec_copy(c, m.rcnt, c->rcnt0.p, (size_t)(S0 + 1) * 4);
    rec_copy(c, m.ralive, c->ralive0.p, (size_t)(S0 + 1));
    rec_copy(c, m.ea, c->ea0.p, (size_t)E * 4);
    rec_copy(c, m.eb, c->eb0.p, (size_t)E * 4);
    MergeLds xl;
    merge_il_layout(E, S0, use_lds ? mk_waves(kind) : 8, use_lds ? mk_res(kind) : 0, &xl);
    xl.pool_cap = f3ds_policy::leaf_pool_capacity(S0, c->pool_mult);
    ENSURE(c->pool, xl.pool_cap, xl.pool); ENSURE(c->rstart, S0 + 1, xl.rstart); ENSURE(c->rnleaf, S0 + 1, xl.rnleaf);
    ENSURE(c->rcap, S0 + 1, xl.rcap);
    // incident-edge lists of the regions (d_inc_build): the initial lists take 2 E entries, a merge whose touched list outgrows a's segment takes a fresh one
    // (only the incident-list kernels have them: d_merge, the all-global fallback of the large-E scenes, scans the edge arrays)
    if (use_lds) {
        xl.ilist_cap = f3ds_policy::ilist_capacity(E, S0, g_sw.ilist_slack, c->ilist_mult, MC_TL_CAP);
        ENSURE(c->ilist, xl.ilist_cap, xl.ilist); ENSURE(c->istart, S0 + 1, xl.istart); ENSURE(c->ilen, S0 + 1, xl.ilen); ENSURE(c->icap, S0 + 1, xl.icap);
    }
    if (use_lds) rec<d_inc_build>(c, 1u, 0u, E, S0, m.ea, m.eb, xl.istart, xl.ilen, xl.icap, xl.ilist);
    xl.stop_key = (prm->threshold != prm->threshold) ? 0u : n_weight_key(prm->threshold);
    c->merge_in_lds = use_lds; c->merge_kind = kind;
    rec<d_region_reset>(c, grid_for(S0 + 1, d_region_reset::BLOCK), 0u, S0, c->hcount.p, m.rhead, m.rtail, m.lnext, m.parent, m.markA, m.markB, xl.pool, xl.rstart, xl.rnleaf, xl.rcap, c->loff.p);
    m.mp.color_metric = prm->color_metric; m.mp.geom_metric = prm->geom_metric; m.mp.merging = prm->merging; m.mp.lambda = lambda; m.mp.bins = bins;
    uint64_t *sk0 = nullptr, *sk1 = nullptr; uint32_t *sv0 = nullptr, *sv1 = nullptr;
    if (prm->merging == F3DS_ADAPTIVE_LAMBDA) {
        ENSURE(c->skeys0, (size_t)E * 2, sk0); ENSURE(c->skeys1, (size_t)E * 2, sk1);
        ENSURE(c->svals0, (size_t)E * 2, sv0); ENSURE(c->svals1, (size_t)E * 2, sv1);
    }
    rec<d_edge_deltas>(c, grid_for(E, d_edge_deltas::BLOCK), 0u, E, m.ea, m.eb, m.rrec, prm->color_metric, prm->geom_metric, deltas, sk0, sv0);
    if (prm->merging == F3DS_ADAPTIVE_LAMBDA) {
        uint64_t* ks; uint32_t* vs;
        int rc = radix_sort(c, sk0, sv0, sk1, sv1, E * 2u, 33, &ks, &vs);
        if (rc) return rc;
        rec<d_lambda>(c, 1u, 0u, E, deltas, vs, c->d_dc);
    } else if (prm->merging == F3DS_EQUALIZATION) {
        uint32_t* hist; float* cdf;
        ENSURE(c->cdf_hist, (size_t)2 * (bins > 0 ? bins : 1), hist); ENSURE(c->cdf, (size_t)2 * (bins > 0 ? bins : 1), cdf);
        rec_fill(c, hist, 0u, (size_t)2 * (bins > 0 ? bins : 1) * 4);
        rec<d_cdf_hist>(c, grid_for((size_t)E * 2, d_cdf_hist::BLOCK), 0u, E, deltas, bins, hist, c->d_dc);
        rec<d_cdf_scan>(c, 1u, 0u, E, bins, hist, cdf);
        m.mp.cdf_c = cdf; m.mp.cdf_g = cdf + bins;
    }
    rec<d_edge_weights>(c, grid_for(E, d_edge_weights::BLOCK), 0u, m, deltas);
    c->mdev = m; c->mlds = xl; c->host_lambda = lambda;
    return F3DS_OK;
}
// stage 5: the merge loop, one workgroup per frame
int seg_merge(f3ds_ctx* c) {
#ifdef F3DS_WHATIF      // make WHATIF=1 only: the stand-in changes the labels, so the default library does not contain it
    if (const char* e = dev_getenv("F3DS_FAKE_MERGE")) {      // experiment, timing only: see d_fake_merge
        unsigned us = 30000, waves = 1; sscanf(e, "%u,%u", &us, &waves);
        const char* l = dev_getenv("F3DS_FAKE_MERGE_LDS");
        rec<d_fake_merge>(c, 1u, l ? (uint32_t)atoi(l) * 1024u : c->mlds.lds_bytes, c->mdev, (uint32_t)us, (uint32_t)waves);
        return F3DS_OK;
    }
#endif
    switch (c->merge_kind) {
        case MK_IL + 0: rec<d_merge_il_t<8, 2>>(c, 1u, c->mlds.lds_bytes, c->mdev, c->mlds); break;
        case MK_IL + 1: rec<d_merge_il_t<8, 0>>(c, 1u, c->mlds.lds_bytes, c->mdev, c->mlds); break;
        case MK_IL + 2: rec<d_merge_il_t<4, 2>>(c, 1u, c->mlds.lds_bytes, c->mdev, c->mlds); break;
        case MK_IL + 3: rec<d_merge_il_t<4, 0>>(c, 1u, c->mlds.lds_bytes, c->mdev, c->mlds); break;
        default: rec<d_merge>(c, 1u, 0u, c->mdev);
    }
    return F3DS_OK;
}
// stage 6: region ids (ascending surviving label) and per-point labels: one kernel (rank table in LDS), or two when some frame of
// the batch has more supervoxels than the table holds (c->relabel_lds, decided for the whole batch in run_cluster)
int seg_labels(f3ds_ctx* c) {
    const uint32_t S0 = c->S0, n = c->n;
    const MergeDev& m = c->mdev;
    uint32_t *root, *rincl, *d_labels;
    ENSURE(c->root, S0 + 1, root); ENSURE(c->rincl, S0 + 1, rincl);
    if (c->user_labels) d_labels = c->user_labels;      // a device output buffer is written in place
    else ENSURE(c->labels, n, d_labels);
    if (c->relabel_lds) {
        // (every workgroup builds the table: a lone frame does not get more workgroups than it has 4096-point slices)
        const uint32_t gx = std::min(grid_for(n, d_relabel::BLOCK), grid_wide(n, 4096));
        rec<d_relabel>(c, gx, (S0 + 1u) * 4u, n, c->pt_voxel.p, c->owner0.p, S0, m.parent, m.ralive, root, rincl, d_labels, c->d_dc);
    } else {
        uint32_t* rank; ENSURE(c->rrank, S0 + 1, rank);
        rec<d_region_ids>(c, 1u, 0u, S0, m.parent, m.ralive, rank, root, rincl, c->d_dc);
        rec<d_point_labels>(c, grid_for(n, d_point_labels::BLOCK), 0u, n, c->pt_voxel.p, c->owner0.p, rank, d_labels);
    }
    return F3DS_OK;
}

// labels of a frame that has no voxels at all
int finish_empty(f3ds_ctx* c, hipStream_t st, uint32_t* point_labels, int labels_on_device) {
    uint32_t* d_labels;
    ENSURE(c->labels, c->n ? c->n : 1, d_labels);
    if (c->n) {
        HIPCHECK(hipMemsetAsync(d_labels, 0xFF, (size_t)c->n * 4, st));
        if (point_labels) HIPCHECK(hipMemcpyAsync(point_labels, d_labels, (size_t)c->n * 4, labels_on_device ? hipMemcpyDefault : hipMemcpyDeviceToHost, st));
    }
    c->have_frame = false; c->live = false;
    return F3DS_OK;
}

// Streams for batch calls.  HIP multiplexes streams onto a few hardware queues (4 by default) in creation order, and two
// batches whose streams share a hardware queue run one after the other (measured: with 576 contexts created in a row, two
// of bench.py's three concurrent batches landed in one queue).  A batch therefore does not run on its first context's
// stream but on one of four streams per device (GPU_MAX_HW_QUEUES of them if that is set) created back to back --
// different queues -- and held for the call.
// ONE stream per device for the host <-> device copies of ALL calls (F3DS_COPY_STREAM=0: every call copies on its own stream, as until round 4).  On this platform a
// host-to-device and a device-to-host copy that run at the same time get 16 GB/s each where either alone gets 55 (tools/pcie_bw.py); with six calls in flight the uploads of
// one call (16 MB per frame) kept meeting the label downloads of another (4 MB per frame).  Through one stream the link carries one copy at a time at full rate.  A call's
// downloads are queued only once its labels exist (the host thread waits for the event first), so the stream never sits blocked behind unfinished compute.
struct CopyStream { std::mutex m; hipStream_t s = nullptr; };
CopyStream g_copy_stream[16][2];      // [1]: a second stream for the downloads (development: F3DS_COPY_STREAM=2, both directions of the link at once)
hipStream_t copy_stream_of(int device, int which = 0) {
    CopyStream& c = g_copy_stream[device & 15][which & 1];
    std::lock_guard<std::mutex> lk(c.m);
    if (!c.s && hipStreamCreateWithFlags(&c.s, hipStreamNonBlocking) != hipSuccess) c.s = nullptr;
    return c.s;
}
struct BatchStreamPool { std::mutex m; hipStream_t s[8] = {}; bool busy[8] = {}; };
const int g_batch_stream_count = [] { const char* e = getenv("GPU_MAX_HW_QUEUES"); int n = e ? atoi(e) : 4; return n < 1 ? 1 : (n > 8 ? 8 : n); }();      // one per hardware queue HIP will use
BatchStreamPool g_batch_streams[16];
struct BatchStreamLease {
    int dev = -1, slot = -1;
    hipStream_t acquire(int device) {
        BatchStreamPool& p = g_batch_streams[device & 15];
        std::lock_guard<std::mutex> lk(p.m);
        if (!p.s[0]) for (int i = 0; i < g_batch_stream_count; ++i) if (hipStreamCreateWithFlags(&p.s[i], hipStreamNonBlocking) != hipSuccess) { p.s[i] = nullptr; return nullptr; }
        for (int i = 0; i < g_batch_stream_count; ++i) if (!p.busy[i] && p.s[i]) { p.busy[i] = true; dev = device & 15; slot = i; return p.s[i]; }
        return nullptr;      // more batches at once on this device than queues: the caller's own stream
    }
    ~BatchStreamLease() { if (slot >= 0) { std::lock_guard<std::mutex> lk(g_batch_streams[dev].m); g_batch_streams[dev].busy[slot] = false; } }
};

// run `fn` (a per-frame recorder) on every live frame; a failing frame fails the batch
template <class F>
int for_frames(Batch& b, F&& fn) {
    for (f3ds_ctx* c : b.fr) { int rc = fn(c); if (rc) return rc; }
    return F3DS_OK;
}
void stage_mark(Batch& b, int i) { (void)hipEventRecord(b.owner->ev[i], b.st); }
// device time of stages first ... last - 1 of a call whose stream has been waited for (HIP events on that stream): ms_stage[k] = from mark k to mark k + 1
void stage_times(const f3ds_ctx* owner, int first, int last, float* ms_stage) {
    for (int k = first; k < last; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, owner->ev[k], owner->ev[k + 1]) == hipSuccess) ms_stage[k] = ms; }
}

// The call's kernels wait for its uploads, which went through the device's copy stream `up` (the events of a call's copies are its owner's, made on first use)
int await_uploads(Batch& b, hipStream_t up) {
    hipEvent_t& ev = b.owner->ev_copy[0];
    if (!ev) HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(ev, up));
    HIPCHECK(hipStreamWaitEvent(b.st, ev, 0));
    return F3DS_OK;
}
// Host outputs leave through the device's download stream, and are queued there only once they exist: that stream must never sit blocked behind unfinished
// compute.  download_begin() waits for what the call's stream holds so far and gives the stream to copy on (nullptr with F3DS_COPY_STREAM=0: the call's own);
// download_queued() marks the end of the copies on that stream and download_wait() waits for the mark: work that need not wait for the copies goes between the two.
int download_begin(Batch& b, hipStream_t* dl) {
    *dl = g_sw.copy_stream ? copy_stream_of(b.owner->device, g_sw.copy_duplex ? 1 : 0) : nullptr;
    if (!*dl) return F3DS_OK;
    for (int k = 1; k < 3; ++k) if (!b.owner->ev_copy[k]) HIPCHECK(hipEventCreateWithFlags(&b.owner->ev_copy[k], hipEventDisableTiming));
    HIPCHECK(hipEventRecord(b.owner->ev_copy[1], b.st));
    HIPCHECK(timed_sync(b.owner->ev_copy[1]));
    return F3DS_OK;
}
int download_queued(Batch& b, hipStream_t dl) { if (dl) HIPCHECK(hipEventRecord(b.owner->ev_copy[2], dl)); return F3DS_OK; }
int download_wait(Batch& b, hipStream_t dl) { if (dl) HIPCHECK(timed_sync(b.owner->ev_copy[2])); return F3DS_OK; }

// ---- the label-image frame (f3ds_label_image.h, DESIGN.md "the label-image frame"): what the tracker update and the five region calls do alike.  A region call
// reads: check -> li_begin -> its staging (li_out_buffers) -> li_upload -> per frame its scratch, arguments and kernels -> flush -> li_download_heads -> deliver
// (li_rows_behind).  Every helper takes a batch of frames; a lone call is a batch of one. ----
// Start of a label-image call, after its checks: the switches, the device, the batch of the one context ...
int li_begin(f3ds_ctx* c, Batch* b) {
    g_sw.read();
    HIPCHECK(hipSetDevice(c->device));
    *b = batch_of(c);
    return F3DS_OK;
}
// ... or of ctxs[0 .. nctx) (distinct_contexts_on_one_device), on the first one's stream
int li_begin(f3ds_ctx** ctxs, int nctx, Batch* b) {
    g_sw.read();
    HIPCHECK(hipSetDevice(ctxs[0]->device));
    return batch_of(ctxs, nctx, *b);
}
// The images as the kernels read them: device inputs where they are; host inputs in the staging of the frame's own context, uploaded through the device's copy
// stream like those of f3ds_segment_rgbd -- the copies of all frames are queued there and awaited once.  color may be NULL (no frame has a colour image).
struct LiImages { const unsigned char* depth; const unsigned char* color; const uint32_t* labels; };
int li_upload(f3ds_ctx* const* ctxs, int nctx, Batch& b, const RgbdLayout& lay, const void* const* depth, const void* const* color, const uint32_t* const* labels, int inputs_on_device,
              LiImages* im) {
    for (int i = 0; i < nctx; ++i) im[i] = LiImages{static_cast<const unsigned char*>(depth[i]), color ? static_cast<const unsigned char*>(color[i]) : nullptr, labels[i]};
    if (inputs_on_device) return F3DS_OK;
    hipStream_t up = g_sw.copy_stream ? copy_stream_of(b.owner->device) : nullptr;
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        unsigned char *ud, *uc = nullptr; uint32_t* ul;
        ENSURE(c->li_depth, lay.depth_bytes, ud); ENSURE(c->li_lab, lay.n, ul);
        if (color) ENSURE(c->li_color, lay.color_bytes, uc);
        HIPCHECK(hipMemcpyAsync(ud, depth[i], lay.depth_bytes, hipMemcpyHostToDevice, up ? up : b.st));
        if (color) HIPCHECK(hipMemcpyAsync(uc, color[i], lay.color_bytes, hipMemcpyHostToDevice, up ? up : b.st));
        HIPCHECK(hipMemcpyAsync(ul, labels[i], lay.n * 4, hipMemcpyHostToDevice, up ? up : b.st));
        im[i] = LiImages{ud, uc, ul};
    }
    if (up) { if (const int urc = await_uploads(b, up)) return urc; }
    return F3DS_OK;
}
int li_upload(f3ds_ctx* c, Batch& b, const RgbdLayout& lay, const void* depth, const void* color, const uint32_t* labels, int inputs_on_device, LiImages* im) {
    return li_upload(&c, 1, b, lay, &depth, color ? &color : nullptr, &labels, inputs_on_device, im);
}
// Where a region call's kernels write what goes down: the staging of all frames is the OWNER's (li_stage_layout, f3ds_label_image.h: the heads first, the
// payloads of host callers behind them), device memory and the owner's one pinned buffer of the same layout, grown by a quarter beyond the request when it is
// too short (its contents are lost).  fixed / stage_rows: per frame, as li_stage_layout takes them.
struct LiStage {
    f3ds_ctx* o = nullptr; unsigned char* out = nullptr; std::vector<LiSlot> slot; size_t first_bytes = 0, total = 0;
    uint32_t* head(int i) const { return reinterpret_cast<uint32_t*>(out + (size_t)i * LI_HEAD_BYTES); }      // device
    const uint32_t* h_head(int i) const { return reinterpret_cast<const uint32_t*>(o->h_li + (size_t)i * LI_HEAD_BYTES); }      // after li_download_heads (8-byte aligned)
};
int li_out_buffers(f3ds_ctx* c, int nctx, const size_t* fixed, const size_t* stage_rows, size_t row_bytes, size_t first_rows, LiStage* s) {
    s->o = c; s->slot.resize((size_t)nctx);
    s->total = li_stage_layout((size_t)nctx, fixed, stage_rows, row_bytes, first_rows, s->slot.data(), &s->first_bytes);
    ENSURE(c->li_out, s->total, s->out);
    if (c->h_li_cap < s->total) {
        if (c->h_li) { HIPCHECK(hipHostFree(c->h_li)); c->h_li = nullptr; c->h_li_cap = 0; }
        HIPCHECK(hipHostMalloc(&c->h_li, s->total + s->total / 4, hipHostMallocDefault));
        c->h_li_cap = s->total + s->total / 4;
    }
    return F3DS_OK;
}
// ONE download, the call's only wait in the ordinary case: the heads of all frames and what li_stage_layout put into reach behind them (with device outputs
// the heads alone).  Word [1] of a frame's head says that one of its labels was >= n_regions: its kernels wrote nothing but the head then.
int li_download_heads(const LiStage& s, Batch& b) {
    HIPCHECK(hipMemcpyAsync(s.o->h_li, s.out, s.first_bytes, hipMemcpyDeviceToHost, b.st));
    HIPCHECK(timed_sync(b.st));
    HIPCHECK(hipGetLastError());
    return F3DS_OK;
}
// The rows of host callers whose count the device decided: frame i has count[i] rows to deliver into rows[i] (0: none -- no rows asked for, or the frame
// failed).  The first download brought slot[i].first of them; the frames with more (rare) get the rest in further copies, which are queued together and
// awaited once.
int li_rows_behind(const LiStage& s, Batch& b, int nctx, size_t row_bytes, const size_t* count, void* const* rows) {
    bool more = false;
    for (int i = 0; i < nctx; ++i) {
        const LiSlot& sl = s.slot[(size_t)i];
        if (count[i] <= sl.first) continue;
        const size_t off = sl.rows_at + sl.first * row_bytes;
        HIPCHECK(hipMemcpyAsync(s.o->h_li + off, s.out + off, (count[i] - sl.first) * row_bytes, hipMemcpyDeviceToHost, b.st));
        more = true;
    }
    if (more) HIPCHECK(timed_sync(b.st));
    for (int i = 0; i < nctx; ++i) if (count[i]) memcpy(rows[i], s.o->h_li + s.slot[(size_t)i].rows_at, count[i] * row_bytes);
    return F3DS_OK;
}
// Where the kernels write an output of frame i that has a fixed size: the caller's device array, or `off` bytes into the frame's slot of the staging
template <class T>
T* li_out_ptr(int on_device, T* caller, const LiStage& s, int i, size_t off = 0u) { return on_device ? caller : reinterpret_cast<T*>(s.out + s.slot[(size_t)i].at + off); }
// the end of a batch form: the frames' statuses to the caller, the lowest failing frame's as the call's
int li_statuses(const std::vector<int>& st, int* status) {
    int ret = F3DS_OK;
    for (size_t i = 0; i < st.size(); ++i) { if (status) status[i] = st[i]; if (st[i] && !ret) ret = st[i]; }
    return ret;
}
// The end of a call whose rows have a fixed size (one per region): the flush, the ONE download, and per frame its status -- F3DS_ERR_ARG where a label was
// >= n_regions: no finish kernel wrote a row --, its payloads out of the staging (bytes0[i] bytes at the start of the slot into out0[i], bytes1[i] behind
// them into out1[i]; 0 bytes: a device caller, or no such output; bytes1 may be NULL) and its result fields, fill(i, head).
template <class R0, class R1, class Fill>
int li_deliver_fixed(const LiStage& s, Batch& b, int nctx, const size_t* bytes0, R0* const* out0, const size_t* bytes1, R1* const* out1, int* status, const Fill& fill) {
    if (const int rc = flush(b)) return rc;
    if (const int rc = li_download_heads(s, b)) return rc;
    std::vector<int> st((size_t)nctx, F3DS_OK);
    for (int i = 0; i < nctx; ++i) {
        const uint32_t* h = s.h_head(i);
        if (h[1]) { st[i] = F3DS_ERR_ARG; continue; }
        const unsigned char* src = s.o->h_li + s.slot[(size_t)i].at;
        if (bytes0[i]) memcpy(out0[i], src, bytes0[i]);
        if (bytes1 && bytes1[i]) memcpy(out1[i], src + bytes0[i], bytes1[i]);
        fill(i, h);
    }
    return li_statuses(st, status);
}
// Start of every accessor: ARG for no context, LOGIC for a context that does not hold what the call needs -- both before any HIP call --, then the
// context's device and everything queued on its stream.
enum FrameNeed { NEED_NOTHING = 0, NEED_FRAME = 1, NEED_VOXEL_GRID = 2 /* not caller-supplied supervoxels */, NEED_REFINED = 4 };
int on_frame(f3ds_ctx* c, int need = NEED_FRAME) {
    if (!c) return F3DS_ERR_ARG;
    if (((need & NEED_FRAME) && !c->have_frame) || ((need & NEED_VOXEL_GRID) && c->user_mode) || ((need & NEED_REFINED) && c->refined_itr < 0)) return F3DS_ERR_LOGIC;
    HIPCHECK(hipSetDevice(c->device));
    HIPCHECK(hipStreamSynchronize(c->stream));
    return F3DS_OK;
}
// Output of an accessor that learns its entry count by walking the state: every entry is counted, those there is room() for are written, and
// finish() reports the count -- with F3DS_ERR_CAPACITY when an array was asked for (any) that did not hold them all: its first `cap` entries stand.
struct Capped {
    size_t cap; bool any; size_t k = 0;
    bool room() const { return k < cap; }
    void next() { ++k; }
    int finish(size_t* n_out) const { if (n_out) *n_out = k; return (k > cap && any) ? F3DS_ERR_CAPACITY : F3DS_OK; }
};
// ... and of one that knows its count n beforehand, all or nothing: n is reported; true = the caller's arrays take all n entries, go on and write
// them; false = *rc is the accessor's result (F3DS_OK without any array, F3DS_ERR_CAPACITY with too short a one: nothing is written)
inline bool all_fit(size_t n, size_t cap, bool any, size_t* n_out, int* rc) {
    if (n_out) *n_out = n;
    *rc = (any && cap < n) ? F3DS_ERR_CAPACITY : F3DS_OK;
    return any && cap >= n;
}
inline void put3(float* dst, size_t k, const float* src) { if (dst) { dst[3 * k] = src[0]; dst[3 * k + 1] = src[1]; dst[3 * k + 2] = src[2]; } }

// device address of a pinned host buffer (nullptr for pageable memory, which the device cannot reach)
static uint32_t* pinned_device_alias(uint32_t* host) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }      // (pageable memory: "invalid value", and the error must not stick)
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return nullptr;
    return static_cast<uint32_t*>(at.devicePointer);
}

// cluster stage for the live frames (also the whole of f3ds_recluster)
// The stage starts from the untouched supervoxel state, so a frame that ran out of room -- or whose merge did not fit the LDS kernel's lists -- makes it run again
// for all frames: the loop below goes round until neither happens.
int run_cluster(Batch& b, const f3ds_params* prm, uint32_t* const* labels_of, const std::vector<int>& index_of, int labels_on_device, bool force_global = false) {
    int rc;
    for (;;) {
        const int kind = choose_merge_kind(b.fr, force_global);      // one kernel for the whole batch
        const bool all_lds = kind != MK_GLOBAL;
        rc = for_frames(b, [&](f3ds_ctx* c) { return seg_cluster_front(c, prm, kind); });
        if (rc || (rc = flush(b))) return rc;
        stage_mark(b, 5);
        if ((rc = for_frames(b, seg_merge)) || (rc = flush(b))) return rc;
        stage_mark(b, 6);
        for (size_t i = 0; i < b.fr.size(); ++i) {
            uint32_t* out = labels_of ? labels_of[index_of[i]] : nullptr;
            // F3DS_DIRECT_LABELS=1 (experiment, measured and not the default): a host label buffer that is pinned (hipHostMalloc / hipHostRegister) is written by the relabel kernel
            // itself through its device address instead of a staging buffer + device-to-host copy.  With six calls in flight the pinned-host-in / host-out rate of bench.py
            // drops from 2 060 to 1 830 Mpoints/s: the kernel holds its workgroups while its stores trickle up the link.
            if (out && !labels_on_device && g_sw.direct_labels) out = pinned_device_alias(out);
            else if (!labels_on_device) out = nullptr;
            b.fr[i]->user_labels = out;
        }
        {
            const uint32_t cap = g_sw.relabel_lds_cap >= 0 ? (uint32_t)g_sw.relabel_lds_cap : RL_LDS_CAP;      // (tests: 0 forces the two-kernel form)
            bool fits = true;
            for (f3ds_ctx* c : b.fr) if (c->S0 + 1u > cap) fits = false;
            for (f3ds_ctx* c : b.fr) c->relabel_lds = fits;
        }
        if ((rc = for_frames(b, seg_labels)) || (rc = flush(b))) return rc;
        stage_mark(b, 7);
        {
            bool want = false;
            for (size_t i = 0; i < b.fr.size(); ++i) if (labels_of && labels_of[index_of[i]] && !b.fr[i]->user_labels && b.fr[i]->n) want = true;
            hipStream_t dl = nullptr;
            if (want && !labels_on_device && (rc = download_begin(b, &dl))) return rc;
            for (size_t i = 0; i < b.fr.size(); ++i) {
                f3ds_ctx* c = b.fr[i];
                uint32_t* out = labels_of ? labels_of[index_of[i]] : nullptr;
                if (out && !c->user_labels && c->n) HIPCHECK(hipMemcpyAsync(out, c->labels.p, (size_t)c->n * 4, hipMemcpyDeviceToHost, dl ? dl : b.st));
                c->user_labels = nullptr;
            }
            if ((rc = download_queued(b, dl)) || (rc = flush_sync(b)) || (rc = download_wait(b, dl))) return rc;      // (the frames' counters come to the host while the labels travel)
        }
        {
            // a frame whose merge loop re-weights more edges than its event arrays hold (huge regions of tiny supervoxels)
            // runs the stage again -- it starts from the untouched supervoxel state -- with four times the room
            bool again = false;
            for (f3ds_ctx* c : b.fr) {
                if (c->h_dc->ev_overflow == F3DS_OVF_EVENTS && f3ds_policy::grow(&c->ev_mult, f3ds_policy::EV_MULT_CAP)) again = true;
                if (c->h_dc->ev_overflow == F3DS_OVF_LEAF_POOL && f3ds_policy::grow(&c->pool_mult, f3ds_policy::POOL_MULT_CAP)) again = true;
                if (c->h_dc->ev_overflow == F3DS_OVF_ILIST_POOL && f3ds_policy::grow(&c->ilist_mult, f3ds_policy::ILIST_MULT_CAP)) again = true;
            }
            if (again) {
                if (g_sw.trace_err) fprintf(stderr, "f3ds: merge stage of %zu frames runs again with more history / leaf-pool room\n", b.fr.size());
                for (f3ds_ctx* c : b.fr) if ((rc = clear_counters(c, b.st, &DevCounters::error, &DevCounters::ev_overflow))) return rc;
                continue;
            }
        }
        if (all_lds) {
            // a merge whose two regions touch more than ML_TL_CAP edges does not fit the LDS kernel's lists: the stage
            // (it starts from the untouched supervoxel state) runs again with the global-memory kernel
            bool again = false;
            for (f3ds_ctx* c : b.fr) if (c->h_dc->error == F3DS_ERR_UNSUPPORTED) again = true;
            if (again) {
                if (g_sw.trace_err) fprintf(stderr, "f3ds: merge stage of %zu frames runs again with the global-memory kernel\n", b.fr.size());
                for (f3ds_ctx* c : b.fr) if ((rc = clear_counters(c, b.st, &DevCounters::error))) return rc;
                force_global = true;
                continue;
            }
        }
        break;
    }
    for (f3ds_ctx* c : b.fr) {
        if (c->h_dc->error) return trace_err(c->h_dc->error, "merge", c);
        c->res.n_merges = c->h_dc->n_merges; c->res.n_regions = c->h_dc->n_regions;
        c->res.lambda = prm->merging == F3DS_ADAPTIVE_LAMBDA ? (c->E ? c->h_dc->lambda : __builtin_nanf("")) : c->host_lambda;
        c->prm.color_metric = prm->color_metric; c->prm.geom_metric = prm->geom_metric; c->prm.merging = prm->merging;
        c->prm.lambda = prm->lambda; c->prm.bins = prm->bins; c->prm.threshold = prm->threshold;
        c->cluster_T = prm->threshold;
        c->have_frame = true;
    }
    return F3DS_OK;
}

}  // namespace

extern "C" {

const char* f3ds_last_hip_error(void) { return g_last_hip_error.c_str(); }

int f3ds_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int f3ds_create(int device, f3ds_ctx** out) {
    if (!out) return F3DS_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return F3DS_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return F3DS_ERR_ARG;
    HIPCHECK(hipSetDevice(device));
    f3ds_ctx* c = new f3ds_ctx;
    c->device = device;
    if (const char* e = dev_getenv("F3DS_EDGE_MULT")) { const int v = atoi(e); if (v >= 1 && v <= (int)f3ds_policy::EDGE_MULT) c->edge_mult = (uint32_t)v; }      // tests: start with a short adjacency list
    const int rc = [c]() -> int {
        HIPCHECK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
        c->stream = c->own_stream;
        for (auto& e : c->ev) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(hipMalloc(&c->d_dc, sizeof(DevCounters)));
        HIPCHECK(hipHostMalloc(&c->h_dc, sizeof(DevCounters), hipHostMallocDefault));
        HIPCHECK(hipMalloc(&c->d_grid, sizeof(GridInfo)));
        HIPCHECK(hipHostMalloc(&c->h_grid, sizeof(GridInfo), hipHostMallocDefault));
        HIPCHECK(hipMalloc(&c->d_sgrid, sizeof(SeedGrid)));
        return F3DS_OK;
    }();
    if (rc) { c->stream = c->own_stream; f3ds_destroy(c); return rc; }      // a half-built context is released, not leaked
    memset(c->h_grid, 0, sizeof(GridInfo));
    memset(&c->res, 0, sizeof c->res);
    *out = c;
    return F3DS_OK;
}

void f3ds_destroy(f3ds_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->each_scratch([](auto& b) { if (b.p) (void)hipFree(b.p); return 0; });
    if (c->d_dc) (void)hipFree(c->d_dc);
    if (c->h_dc) (void)hipHostFree(c->h_dc);
    if (c->d_grid) (void)hipFree(c->d_grid);
    if (c->h_grid) (void)hipHostFree(c->h_grid);
    if (c->d_sgrid) (void)hipFree(c->d_sgrid);
    for (int k = 0; k < 2; ++k) { if (c->h_args[k]) (void)hipHostFree(c->h_args[k]); if (c->d_args[k]) (void)hipFree(c->d_args[k]); if (c->ev_args[k]) (void)hipEventDestroy(c->ev_args[k]); }
    for (auto& e : c->ev_copy) if (e) (void)hipEventDestroy(e);
    if (c->d_dcblk) (void)hipFree(c->d_dcblk);
    if (c->h_dcblk) (void)hipHostFree(c->h_dcblk);
    if (c->h_li) (void)hipHostFree(c->h_li);
    for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int f3ds_set_stream(f3ds_ctx* c, void* hip_stream) {
    if (!c) return F3DS_ERR_ARG;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return F3DS_OK;
}

int f3ds_segment(f3ds_ctx* c, const void* points, size_t n_, int points_on_device, const f3ds_params* prm, uint32_t* point_labels,
                 int labels_on_device, f3ds_result* result) {
    const void* pp[1] = {points}; const size_t cnt[1] = {n_}; uint32_t* lp[1] = {point_labels};
    return f3ds_segment_batch(&c, 1, pp, cnt, points_on_device, prm, lp, labels_on_device, result);
}

// A batch of independent frames (BASELINE.json config 5: 8 frames per GPU) walks the stages in
// lockstep on the first context's stream: per stage every frame records its kernel calls, flush()
// turns them into batched dispatches (grid.y = frame), and the few host decisions (octree depth,
// voxel / seed / edge counts) are taken for all frames at one synchronisation point per stage.
}  // extern "C"
namespace {
// `source(c, i, copy, uploaded)` is where frame i's points come from: it sets c->n and c->d_pts, queues what it uploads on `copy` (the device's copy stream, or the
// call's own) and says so in `uploaded`, and may record kernels that build the records (they run first: stage 0 is recorded after them).  `sources_on_device`: nothing is uploaded.
template <class Source>
int segment_batch_from(f3ds_ctx** ctxs, int nctx, Source&& source, int sources_on_device, const f3ds_params* prm, uint32_t* const* point_labels, int labels_on_device,
                              f3ds_result* results) {
    const int points_on_device = sources_on_device;
    const auto t0 = std::chrono::steady_clock::now();
    g_t_wait = 0; g_t_launch = 0;
    g_sw.read();
    HIPCHECK(hipSetDevice(ctxs[0]->device));
    BatchCallCount in_flight(ctxs[0]->device);
    Batch b;
    b.owner = ctxs[0]; b.st = ctxs[0]->stream;
    BatchStreamLease lease;
    if (nctx > 1 && ctxs[0]->stream == ctxs[0]->own_stream && !g_sw.no_stream_pool) { hipStream_t ps = lease.acquire(ctxs[0]->device); if (ps) b.st = ps; }
    set_launch_shape(ctxs, nctx);
    std::vector<int> index_of;
    const int max_depth = (int)(1.8f * prm->seed_res / prm->voxel_res);      // [PCL-recall] SupervoxelClustering::extract
    const uint32_t sweeps = max_depth > 1 ? (uint32_t)(max_depth - 1) : 0u;
    stage_mark(b, 0);
    hipStream_t up_stream = (!points_on_device && g_sw.copy_stream) ? copy_stream_of(ctxs[0]->device) : nullptr;
    bool uploaded = false;
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        reset_recording(c);
        c->have_frame = false; c->live = true; c->rc = 0; c->refined_itr = -1;
        c->user_mode = false; c->user_label.clear(); c->user_row.clear();
        { const int prc = pregrow_scratch(c); if (prc) return prc; }
        c->prm = *prm; c->V = c->C = c->S0 = c->E = 0;
        c->fa = FrameArgs{prm->use_transform, prm->fold_negative_z, prm->leaf_order, prm->voxel_res, prm->seed_res, prm->w_color, prm->w_spatial, prm->w_normal};
        { const int src_rc = source(c, i, up_stream ? up_stream : b.st, uploaded); if (src_rc) return src_rc; }
        memset(&c->res, 0, sizeof c->res);
        c->res.n_points = c->n; c->res.sweeps = sweeps;
        b.fr.push_back(c); index_of.push_back(i);
    }
    if (up_stream && uploaded) { const int urc = await_uploads(b, up_stream); if (urc) return urc; }
    auto drop_dead = [&](auto&& dead) -> int {      // frames without voxels leave the batch with all labels = F3DS_NO_LABEL
        std::vector<f3ds_ctx*> keep; std::vector<int> keep_idx;
        for (size_t i = 0; i < b.fr.size(); ++i) {
            f3ds_ctx* c = b.fr[i];
            if (dead(c)) { int rc = finish_empty(c, b.st, point_labels ? point_labels[index_of[i]] : nullptr, labels_on_device); if (rc) return rc; }
            else { keep.push_back(c); keep_idx.push_back(index_of[i]); }
        }
        b.fr.swap(keep); index_of.swap(keep_idx);
        return F3DS_OK;
    };
    int rc;
    // ---- stage 0: voxelise
    if ((rc = for_frames(b, seg_bbox)) || (rc = flush_sync(b))) return rc;
    for (f3ds_ctx* c : b.fr) {
        c->res.n_finite = c->h_dc->n_finite;
        if (c->h_dc->error) return c->h_dc->error;
        c->res.octree_depth = (uint32_t)c->h_dc->depth;
    }
    if ((rc = drop_dead([](f3ds_ctx* c) { return c->h_dc->grid_empty || c->n == 0; }))) return rc;
    int maxd = 0;
    for (f3ds_ctx* c : b.fr) if (c->h_dc->depth > maxd) maxd = c->h_dc->depth;
    // Stage 0b/0c.  Default: the hash path (only the voxels are sorted).  The sort path (every point's key through a three-pass radix sort) remains for frames with
    // very dense voxels, for lone frames (below) and behind F3DS_VOX_TILES=0.
    // (a lone frame takes the sort path: two of the tile path's kernels are one workgroup per frame -- 2.4 ms on a lone frame's critical path, nothing in a batch)
    bool hashed = f3ds_policy::tile_path_wanted(nctx, g_sw.vox_hash, g_sw.vox_tiles_forced);
    for (f3ds_ctx* c : b.fr) {
        c->vox_hashed = false;
        if (c->vox_dense && hashed) { if (c->vox_dense_wait) c->vox_dense_wait--; else c->vox_dense = false; }      // (counted in calls that would have taken the tile path)
    }
    for (f3ds_ctx* c : b.fr) if (c->vox_dense) hashed = false;
    uint32_t maxn = 1;
    for (f3ds_ctx* c : b.fr) if (c->n > maxn) maxn = c->n;
    const f3ds_policy::Stage0Plan plan = f3ds_policy::stage0_plan(maxd, maxn, hashed, g_sw.sort_pairs, VT_LIMITS);
    if (hashed) {
        rc = plan.tiles ? for_frames(b, [&](f3ds_ctx* c) { return seg_vox_tiles(c, plan.code_bits, plan.tile_bits); }) : F3DS_ERR_UNSUPPORTED;
        if (rc == F3DS_ERR_UNSUPPORTED) {      // (a grid too deep / a frame too long for this path: nothing was flushed)
            for (f3ds_ctx* c : b.fr) { reset_recording(c); c->vox_hashed = false; }
            hashed = false;
        } else if (rc || (rc = flush_sync(b))) return rc;
        if (hashed && g_sw.trace_err) for (f3ds_ctx* c : b.fr) fprintf(stderr, "f3ds: tile path: most voxels in a tile %u, descriptors %u, leaves %u, lists sorted %u\n", c->h_dc->vox_max_tile, c->h_dc->seg_count, c->h_dc->n_voxels, c->h_dc->vox_disorder);
        if (hashed) for (f3ds_ctx* c : b.fr) if (c->h_dc->ev_overflow == F3DS_OVF_DENSE_VOXEL || c->h_dc->ev_overflow == F3DS_OVF_TILE_VOXELS) {
            if (g_sw.trace_err) fprintf(stderr, "f3ds: tile path refused a frame: %s (descriptors %u, leaves %u)\n", c->h_dc->ev_overflow == F3DS_OVF_DENSE_VOXEL ? "a voxel with too many points" : "a tile with too many voxels", c->h_dc->seg_count, c->h_dc->n_voxels);
            c->vox_dense = true; c->vox_dense_wait = c->vox_dense_penalty; c->vox_dense_penalty = f3ds_policy::next_dense_penalty(c->vox_dense_penalty); hashed = false;
        }
        if (!hashed) {
            if (g_sw.trace_err) fprintf(stderr, "f3ds: voxelisation of %zu frames runs again on the sort path (an unorganised cloud or dense voxels)\n", b.fr.size());
            for (f3ds_ctx* c : b.fr) {
                c->vox_hashed = false;
                if ((rc = clear_counters(c, b.st, &DevCounters::error, &DevCounters::ev_overflow, &DevCounters::n_voxels, &DevCounters::seg_count))) return rc;
            }
        }
    }
    if (!hashed) {
        if ((rc = for_frames(b, [&](f3ds_ctx* c) { return seg_sort(c, plan.sort_bits, plan.idxbits); })) || (rc = flush_sync(b))) return rc;
    }
    for (f3ds_ctx* c : b.fr) { if (c->h_dc->error) return trace_err(c->h_dc->error, "voxelisation", c); c->V = c->h_dc->n_voxels; c->res.n_voxels = c->V; }
    if ((rc = drop_dead([](f3ds_ctx* c) { return c->V == 0; }))) return rc;
    stage_mark(b, 1);
    // ---- stage 1 + 2: neighbours, normals, seeds
    if ((rc = for_frames(b, seg_voxels)) || (rc = flush(b))) return rc;
    if ((rc = for_frames(b, seg_normals)) || (rc = flush(b, b.owner->ev[9]))) return rc;      // (the event pair brackets the dispatch alone, not its argument upload)
    stage_mark(b, 10);
    if ((rc = for_frames(b, seg_seed_grid)) || (rc = flush(b))) return rc;
    stage_mark(b, 2);
    if ((rc = flush_sync(b))) return rc;
    int maxsd = 0;
    for (f3ds_ctx* c : b.fr) { if (c->h_dc->error) return c->h_dc->error; if (c->h_dc->sdepth > maxsd) maxsd = c->h_dc->sdepth; }
    if ((rc = for_frames(b, [&](f3ds_ctx* c) { return seg_seed_cells(c, 3 * maxsd, maxsd); })) || (rc = flush_sync(b))) return rc;
    for (f3ds_ctx* c : b.fr) { c->C = c->h_dc->n_cells; c->res.n_seed_cells = c->C; }
    if ((rc = for_frames(b, seg_seeds)) || (rc = flush_sync(b))) return rc;
    for (f3ds_ctx* c : b.fr) { c->S0 = c->h_dc->n_seeds; c->res.n_seeds = c->S0; if (c->S0 >= 0x3FFFFFFFu) return F3DS_ERR_UNSUPPORTED; }      // (labels below 2^30: f3ds_algo.h, a_next_label)
    stage_mark(b, 3);
    // ---- stage 3: sweeps
    if ((rc = for_frames(b, seg_sweeps)) || (rc = flush(b))) return rc;
    stage_mark(b, 4);
    // ---- stage 4: supervoxels, adjacency
    if ((rc = for_frames(b, seg_supervoxels)) || (rc = flush_sync(b))) return rc;
    for (int attempt = 0; attempt < 6; ++attempt) {
        // a frame with more adjacencies than its list holds (tiny supervoxels: 26 neighbours each and more) runs the pass again with four times the room
        bool again = false;
        for (f3ds_ctx* c : b.fr) if (c->h_dc->ev_overflow == F3DS_OVF_EDGE_LIST && f3ds_policy::grow(&c->edge_mult, f3ds_policy::EDGE_MULT_CAP)) again = true;
        if (!again) break;
        if (g_sw.trace_err) fprintf(stderr, "f3ds: adjacency pass of %zu frames runs again with more list room\n", b.fr.size());
        for (f3ds_ctx* c : b.fr) if ((rc = clear_counters(c, b.st, &DevCounters::error, &DevCounters::ev_overflow, &DevCounters::n_edges, &DevCounters::n_alive))) return rc;
        if ((rc = for_frames(b, seg_supervoxels)) || (rc = flush_sync(b))) return rc;
    }
    uint64_t maxkey = 1;
    for (f3ds_ctx* c : b.fr) {
        if (c->h_dc->error) return trace_err(c->h_dc->error, "supervoxels/adjacency", c);
        if (c->h_dc->r_overflow) return trace_err(F3DS_ERR_UNSUPPORTED, "sweeps (R chain)", c);
        c->E = c->h_dc->n_edges; c->res.n_edges = c->E; c->res.n_supervoxels = c->h_dc->n_alive;
        const uint64_t k = (uint64_t)(c->S0 + 1) * (c->S0 + 1);
        if (k > maxkey) maxkey = k;
    }
    if ((rc = for_frames(b, [&](f3ds_ctx* c) { return seg_edge_sort(c, bits_for(maxkey)); }))) return rc;
    // ---- stage 4c..6
    if ((rc = run_cluster(b, prm, point_labels, index_of, labels_on_device))) return rc;
    HIPCHECK(hipStreamSynchronize(b.st));
    float stage[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    stage_times(b.owner, 0, 7, stage);      // (of the whole batch)
    // the d_normals launch (inside stage 1): a HIP event pair around that one dispatch on the call's stream (the time it waits at the head of its queue
    // for a compute unit with room for its first workgroup + its execution)
    if (!b.fr.empty()) { float ms = 0; if (hipEventElapsedTime(&ms, b.owner->ev[9], b.owner->ev[10]) == hipSuccess) stage[7] = ms; }
    const float ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (g_sw.host_prof) fprintf(stderr, "batch of %d: %.1f ms total, %.1f waiting for the GPU, %.1f packing + launching, %.1f recording / host logic; stages %.0f %.0f %.0f %.0f %.0f %.0f %.0f ms; %llu scratch allocations so far\n", nctx, ms, g_t_wait, g_t_launch, ms - g_t_wait - g_t_launch, stage[0], stage[1], stage[2], stage[3], stage[4], stage[5], stage[6], g_scratch_allocs.load());
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        for (int k = 0; k < 8; ++k) c->res.ms_stage[k] = stage[k];
        c->res.ms_total = ms;
        if (results) results[i] = c->res;
    }
    return F3DS_OK;
}

}  // namespace
extern "C" {

int f3ds_segment_batch(f3ds_ctx** ctxs, int nctx, const void* const* points, const size_t* counts, int points_on_device, const f3ds_params* prm,
                       uint32_t* const* point_labels, int labels_on_device, f3ds_result* results) {
    if (!ctxs || nctx <= 0 || !points || !counts || !prm) return F3DS_ERR_ARG;
    if (!(prm->voxel_res > 0) || !(prm->seed_res > 0)) return F3DS_ERR_ARG;
    for (int i = 0; i < nctx; ++i) if (!ctxs[i] || (!points[i] && counts[i]) || counts[i] > 0x7fffffffull || ctxs[i]->device != ctxs[0]->device) return F3DS_ERR_ARG;
    auto source = [&](f3ds_ctx* c, int i, hipStream_t copy, bool& uploaded) -> int {
        c->n = (uint32_t)counts[i];
        if (points_on_device) c->d_pts = static_cast<const P16*>(points[i]);
        else {
            P16* up; ENSURE(c->pts, c->n ? c->n : 1, up);
            if (c->n) { HIPCHECK(hipMemcpyAsync(up, points[i], (size_t)c->n * 16, hipMemcpyHostToDevice, copy)); uploaded = true; }
            c->d_pts = up;
        }
        return F3DS_OK;
    };
    return segment_batch_from(ctxs, nctx, source, points_on_device, prm, point_labels, labels_on_device, results);
}

// RGB-D frames: the images are uploaded (5 to 8 bytes per pixel where the records take 16) or read where they are, and one d_deproject per frame writes the records into
// c->pts, in the same dispatch sequence as the bounding box that reads them.  From there on the call is f3ds_segment_batch on host points.
int f3ds_segment_rgbd_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt, const void* const* depth, const void* const* color, int images_on_device,
                            const f3ds_params* prm, uint32_t* const* point_labels, int labels_on_device, f3ds_result* results) {
    if (!ctxs || nctx <= 0 || !fmt || !depth || !color || !prm) return F3DS_ERR_ARG;
    if (!(prm->voxel_res > 0) || !(prm->seed_res > 0)) return F3DS_ERR_ARG;
    f3ds::RgbdLayout lay;
    if (const int rc = f3ds::rgbd_layout(fmt, &lay)) return rc;
    for (int i = 0; i < nctx; ++i) if (!ctxs[i] || !depth[i] || !color[i] || ctxs[i]->device != ctxs[0]->device) return F3DS_ERR_ARG;
    const RgbdArgs args{fmt->width, (uint32_t)lay.n, lay.depth_pitch, lay.color_pitch, fmt->depth_type == F3DS_DEPTH_F32 ? 1 : 0, fmt->color_format, fmt->depth_scale, fmt->fx, fmt->fy, fmt->cx, fmt->cy};
    auto source = [&](f3ds_ctx* c, int i, hipStream_t copy, bool& uploaded) -> int {
        c->n = (uint32_t)lay.n;
        P16* records; ENSURE(c->pts, c->n, records);
        const unsigned char* d_depth = static_cast<const unsigned char*>(depth[i]);
        const unsigned char* d_color = static_cast<const unsigned char*>(color[i]);
        if (!images_on_device) {
            unsigned char *ud, *uc; ENSURE(c->img_depth, lay.depth_bytes, ud); ENSURE(c->img_color, lay.color_bytes, uc);
            HIPCHECK(hipMemcpyAsync(ud, depth[i], lay.depth_bytes, hipMemcpyHostToDevice, copy));
            HIPCHECK(hipMemcpyAsync(uc, color[i], lay.color_bytes, hipMemcpyHostToDevice, copy));
            uploaded = true; d_depth = ud; d_color = uc;
        }
        rec<d_deproject>(c, grid_for(c->n, d_deproject::BLOCK), 0u, d_depth, d_color, args, records);
        c->d_pts = records;
        return F3DS_OK;
    };
    return segment_batch_from(ctxs, nctx, source, images_on_device, prm, point_labels, labels_on_device, results);
}
int f3ds_segment_rgbd(f3ds_ctx* c, const f3ds_rgbd_format* fmt, const void* depth, const void* color, int images_on_device, const f3ds_params* prm, uint32_t* point_labels,
                      int labels_on_device, f3ds_result* result) {
    const void* dp[1] = {depth}; const void* cp[1] = {color}; uint32_t* lp[1] = {point_labels};
    return f3ds_segment_rgbd_batch(&c, 1, fmt, dp, cp, images_on_device, prm, lp, labels_on_device, result);
}

// the records of the last segment call when they sit in the context's own buffer (uploaded host points, or built by d_deproject)
int f3ds_get_points(f3ds_ctx* c, void* points16, size_t cap, int dst_on_device, size_t* n_out) {
    if (!c || (!points16 && !n_out)) return F3DS_ERR_ARG;
    if (!c->d_pts || c->d_pts != c->pts.p) return F3DS_ERR_LOGIC;
    int rc;
    if (!all_fit(c->n, cap, points16 != nullptr, n_out, &rc)) return rc;
    HIPCHECK(hipSetDevice(c->device));
    if (c->n) HIPCHECK(hipMemcpy(points16, c->pts.p, (size_t)c->n * 16, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return F3DS_OK;
}

int f3ds_recluster(f3ds_ctx* c, const f3ds_params* prm, uint32_t* point_labels, int labels_on_device, f3ds_result* result) {
    if (!c || !prm) return F3DS_ERR_ARG;
    if (!c->have_frame) return F3DS_ERR_LOGIC;
    const auto t0 = std::chrono::steady_clock::now();
    g_sw.read();
    HIPCHECK(hipSetDevice(c->device));
    Batch b = batch_of(c);
    { const int crc = clear_counters(c, c->stream, &DevCounters::error); if (crc) return crc; }
    stage_mark(b, 4);
    std::vector<int> idx{0}; uint32_t* lp[1] = {point_labels};
    int rc = run_cluster(b, prm, lp, idx, labels_on_device);
    if (rc) return rc;
    HIPCHECK(hipStreamSynchronize(b.st));
    stage_times(c, 4, 7, c->res.ms_stage);
    c->res.ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (result) *result = c->res;
    return F3DS_OK;
}

// Clustering::set_initialstate(segm, adj) + cluster(threshold) on caller-supplied supervoxels (include/f3ds.h).  Host side: the std::map / std::multimap
// orders the reference iterates in (ascending key; adjacency rows by `first`, insertion order inside) become ranks and an edge list; device side: d_sv_user_fill
// builds what d_sv_fill builds for the library's own supervoxels, and stages 4c-6 run unchanged.
int f3ds_cluster_supervoxels(f3ds_ctx* c, const f3ds_supervoxel_set* sv, const uint32_t* pairs, size_t n_pairs, const f3ds_params* prm, uint32_t* region_of_sv,
                             uint32_t* voxel_labels, f3ds_result* result) {
    if (!c || !sv || !prm || (n_pairs && !pairs)) return F3DS_ERR_ARG;
    const uint32_t S = sv->n_supervoxels;
    if (S && (!sv->label || !sv->voxel_offset || !sv->voxel_xyz || !sv->voxel_rgba || !sv->centroid_xyz || !sv->normal)) return F3DS_ERR_ARG;
    if (S >= 0x3FFFFFFFu) return F3DS_ERR_UNSUPPORTED;
    const auto t0 = std::chrono::steady_clock::now();
    g_sw.read();
    HIPCHECK(hipSetDevice(c->device));
    // ---- std::map<uint32_t, Supervoxel::Ptr>: ascending key
    std::vector<uint32_t> row(S + 1u, 0u), lab(S + 1u, 0u), hof(S, 0u);      // row[h], label[h] of internal supervoxel h = rank + 1; hof[row] = h
    {
        std::vector<uint32_t> order(S);
        for (uint32_t i = 0; i < S; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sv->label[a] < sv->label[b]; });
        for (uint32_t r = 0; r < S; ++r) {
            if (r && sv->label[order[r]] == sv->label[order[r - 1]]) return F3DS_ERR_ARG;      // (a map holds a key once)
            row[r + 1] = order[r]; lab[r + 1] = sv->label[order[r]]; hof[order[r]] = r + 1u;
        }
    }
    if (S && sv->voxel_offset[0] != 0u) return F3DS_ERR_ARG;
    for (uint32_t i = 0; i < S; ++i) if (sv->voxel_offset[i + 1] <= sv->voxel_offset[i]) return F3DS_ERR_ARG;      // every supervoxel holds a voxel
    const uint32_t Vt = S ? sv->voxel_offset[S] : 0u;
    if ((uint64_t)Vt + S + 1u > 0x7fffffffull) return F3DS_ERR_UNSUPPORTED;
    // ---- clear_adjacency + adj2weight: rows with first <= second, multimap order
    std::vector<uint32_t> ea, eb;
    {
        std::vector<std::pair<uint32_t, uint32_t>> ed;      // (h_first, h_second)
        std::set<std::pair<uint32_t, uint32_t>> seen;
        for (size_t k = 0; k < n_pairs; ++k) {
            const uint32_t p = pairs[2 * k], q = pairs[2 * k + 1];
            if (p > q) continue;
            uint32_t hh[2];
            for (int w = 0; w < 2; ++w) {
                const uint32_t l = w ? q : p;
                const auto it = std::lower_bound(lab.begin() + 1, lab.end(), l);
                if (it == lab.end() || *it != l) return F3DS_ERR_OUT_OF_RANGE;
                hh[w] = (uint32_t)(it - lab.begin());
            }
            // (defects are reported in pair order, like the map::at / dereference the reference would meet first: an unknown label of pair k wins over a
            // duplicate or self-adjacency of a later pair and the other way round -- the oracle checks in the same order)
            if (hh[0] == hh[1] || !seen.insert({hh[0], hh[1]}).second) return F3DS_ERR_ARG;
            ed.push_back({hh[0], hh[1]});
        }
        std::stable_sort(ed.begin(), ed.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
        if (ed.size() > 0x7fffffffull) return F3DS_ERR_UNSUPPORTED;
        ea.resize(ed.size()); eb.resize(ed.size());
        for (size_t k = 0; k < ed.size(); ++k) { ea[k] = ed[k].first; eb[k] = ed[k].second; }
    }
    const uint32_t E = (uint32_t)ea.size();
    // ---- frame state
    reset_recording(c);
    c->have_frame = false; c->live = true; c->rc = 0; c->refined_itr = -1;
    { const int prc = pregrow_scratch(c); if (prc) return prc; }
    c->prm = *prm; c->n = Vt; c->V = c->C = 0; c->S0 = S; c->E = E; c->d_pts = nullptr;
    memset(&c->res, 0, sizeof c->res);
    c->res.n_voxels = Vt; c->res.n_seeds = S; c->res.n_supervoxels = S; c->res.n_edges = E;
    c->user_mode = true; c->user_label = lab; c->user_row = row;
    if (S == 0) {      // an empty map: cluster() finds an empty weight map and returns (src/clustering.cpp:387)
        c->user_mode = false; c->user_label.clear(); c->user_row.clear(); c->live = false;
        if (result) *result = c->res;
        return F3DS_OK;
    }
    Batch b = batch_of(c);      // (clears the recording once more: nothing was recorded since)
    uint32_t *d_src, *d_voff, *d_rgba, *loff, *hcount, *owner, *rcnt0, *ea0, *eb0; float *d_xyz, *d_cent, *d_nrm, *rows, *racc0, *rrec0, *hc; int *row_voxel, *pt_voxel; unsigned char* ralive0;
    ENSURE(c->u_src, S + 1u, d_src); ENSURE(c->u_voff, S + 1u, d_voff); ENSURE(c->u_xyz, (size_t)Vt * 3, d_xyz); ENSURE(c->u_rgba, Vt, d_rgba);
    ENSURE(c->u_cent, (size_t)S * 3, d_cent); ENSURE(c->u_nrm, (size_t)S * 3, d_nrm);
    ENSURE(c->loff, S + 2u, loff); ENSURE(c->hcount, S + 1u, hcount); ENSURE(c->owner0, Vt, owner); ENSURE(c->pt_voxel, Vt, pt_voxel);
    ENSURE(c->rows, ((size_t)Vt + S + 1) * 12, rows); ENSURE(c->row_voxel, (size_t)Vt + S + 1, row_voxel);
    ENSURE(c->racc0, (size_t)(S + 1) * 12, racc0); ENSURE(c->rcnt0, S + 1u, rcnt0); ENSURE(c->rrec0, (size_t)(S + 1) * 16, rrec0);
    ENSURE(c->ralive0, S + 1u, ralive0); ENSURE(c->hc, (size_t)(S + 1) * 12, hc);
    ENSURE(c->ea0, E, ea0); ENSURE(c->eb0, E, eb0);
    std::vector<uint32_t> h_loff(S + 2u, 0u), h_cnt(S + 1u, 0u);
    for (uint32_t h = 1; h <= S; ++h) { h_loff[h] = sv->voxel_offset[row[h]]; h_cnt[h] = sv->voxel_offset[row[h] + 1] - sv->voxel_offset[row[h]]; }
    h_loff[S + 1] = Vt;      // (rows in use: f3ds_get_voxel_cloud)
    const hipStream_t st = b.st;
    HIPCHECK(hipMemcpyAsync(d_src, row.data(), (size_t)(S + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_voff, sv->voxel_offset, (size_t)(S + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_xyz, sv->voxel_xyz, (size_t)Vt * 12, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_rgba, sv->voxel_rgba, (size_t)Vt * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_cent, sv->centroid_xyz, (size_t)S * 12, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(d_nrm, sv->normal, (size_t)S * 12, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(loff, h_loff.data(), (size_t)(S + 2) * 4, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(hcount, h_cnt.data(), (size_t)(S + 1) * 4, hipMemcpyHostToDevice, st));
    if (E) { HIPCHECK(hipMemcpyAsync(ea0, ea.data(), (size_t)E * 4, hipMemcpyHostToDevice, st)); HIPCHECK(hipMemcpyAsync(eb0, eb.data(), (size_t)E * 4, hipMemcpyHostToDevice, st)); }
    stage_mark(b, 4);
    rec<d_init_counters>(c, 1u, 0u, c->d_dc);
    rec_fill(c, ralive0, 0u, S + 1u);
    rec_fill(c, rcnt0, 0u, (size_t)(S + 1) * 4);
    rec_fill(c, racc0, 0u, 48); rec_fill(c, rrec0, 0u, 64); rec_fill(c, hc, 0u, 48);
    rec<d_iota>(c, grid_for(Vt, d_iota::BLOCK), 0u, reinterpret_cast<uint32_t*>(pt_voxel), Vt);      // (the caller's voxels are their own "points": ordinal v >= 0 as int, written through the kernel's uint32 view)
    rec<d_sv_user_fill>(c, S, 0u, S, d_src, d_voff, d_xyz, d_rgba, d_cent, d_nrm, rows, row_voxel, owner, racc0, rcnt0, rrec0, ralive0, hc, c->d_dc);
    int rc = flush(b);
    if (rc) return rc;
    uint32_t* lp[1] = {voxel_labels}; std::vector<int> idx{0};
    if ((rc = run_cluster(b, prm, lp, idx, 0))) return rc;
    HIPCHECK(hipStreamSynchronize(b.st));
    stage_times(c, 4, 7, c->res.ms_stage);
    if (region_of_sv) {
        std::vector<uint32_t> root(S + 1u);
        HIPCHECK(hipMemcpy(root.data(), c->root.p, (size_t)(S + 1) * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < S; ++i) region_of_sv[i] = lab[root[hof[i]]];
    }
    c->live = false;
    c->res.ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (result) *result = c->res;
    return F3DS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// accessors (not on the hot path): copy device state to the host and repack
// ------------------------------------------------------------------------------------------------
namespace {
template <class T>
int fetch(f3ds_ctx* c, const Scratch<T>& b, size_t count, std::vector<T>& out) {
    out.resize(count);
    if (count) HIPCHECK(hipMemcpy(out.data(), b.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return F3DS_OK;
}
// label of internal supervoxel h as the caller knows it: h itself after f3ds_segment (helper labels 1..S0), the caller's own after f3ds_cluster_supervoxels
inline uint32_t label_out(const f3ds_ctx* c, uint32_t h) { return c->user_mode && h < c->user_label.size() ? c->user_label[h] : h; }
// the leaves of every alive region, in voxels_ concatenation order, as (first payload row, rows)
int region_leaves(f3ds_ctx* c, std::vector<unsigned char>& ralive, std::vector<std::vector<uint2>>& leaves) {
    const uint32_t S0 = c->S0;
    std::vector<uint32_t> rhead, lnext, loff, llen, rstart, rnleaf; std::vector<uint2> pool;
    int rc;
    if ((rc = fetch(c, c->ralive, S0 + 1, ralive)) || (rc = fetch(c, c->rhead, S0 + 1, rhead)) || (rc = fetch(c, c->lnext, S0 + 1, lnext)) ||
        (rc = fetch(c, c->loff, S0 + 2, loff)) || (rc = fetch(c, c->hcount, S0 + 1, llen)))
        return rc;
    if (c->merge_in_lds && ((rc = fetch(c, c->pool, c->pool.cap / 8, pool)) || (rc = fetch(c, c->rstart, S0 + 1, rstart)) || (rc = fetch(c, c->rnleaf, S0 + 1, rnleaf)))) return rc;
    leaves.assign(S0 + 1, {});
    for (uint32_t h = 1; h <= S0; ++h) {
        if (!ralive[h]) continue;
        if (c->merge_in_lds) leaves[h].assign(pool.begin() + rstart[h], pool.begin() + rstart[h] + rnleaf[h]);
        else for (uint32_t leaf = rhead[h]; leaf; leaf = lnext[leaf]) leaves[h].push_back(make_uint2(loff[leaf], llen[leaf]));
    }
    return F3DS_OK;
}
// payload rows in use: the library's own supervoxels are packed (loff[S0 + 1] = total); a caller's keep the caller's layout
inline size_t rows_in_use(const f3ds_ctx* c, const std::vector<uint32_t>& loff) { return c->user_mode ? c->n : loff[c->S0 + 1]; }
}  // namespace

// get_currentstate().first: the merged regions in ascending key (include/f3ds.h)
extern "C" int f3ds_get_regions(f3ds_ctx* c, uint32_t* label, uint32_t* n_voxels, float* centroid_xyz, float* normal, float* mean_rgb, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c)) return frc;
    const uint32_t S0 = c->S0;
    std::vector<unsigned char> ralive; std::vector<uint32_t> rcnt; std::vector<float> rrec;
    int rc;
    if ((rc = fetch(c, c->ralive, S0 + 1, ralive)) || (rc = fetch(c, c->rcnt, S0 + 1, rcnt)) || (rc = fetch(c, c->rrec, (size_t)(S0 + 1) * 16, rrec))) return rc;
    Capped out{cap, label || n_voxels || centroid_xyz || normal || mean_rgb};
    for (uint32_t h = 1; h <= S0; ++h) {
        if (!ralive[h]) continue;
        if (out.room()) {
            const float* r = &rrec[(size_t)h * 16];
            if (label) label[out.k] = label_out(c, h);
            if (n_voxels) n_voxels[out.k] = rcnt[h];
            put3(centroid_xyz, out.k, r); put3(normal, out.k, r + 3); put3(mean_rgb, out.k, r + 6);
        }
        out.next();
    }
    return out.finish(n_out);
}

extern "C" int f3ds_get_region_voxels(f3ds_ctx* c, float* xyz, uint32_t* rgba, uint32_t* voxel_index, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c)) return frc;
    std::vector<unsigned char> ralive; std::vector<std::vector<uint2>> leaves; std::vector<float> rows; std::vector<int> rv; std::vector<uint32_t> loff;
    int rc;
    if ((rc = region_leaves(c, ralive, leaves)) || (rc = fetch(c, c->loff, c->S0 + 2, loff))) return rc;
    const size_t nrows = rows_in_use(c, loff);
    if ((rc = fetch(c, c->rows, nrows * 12, rows)) || (rc = fetch(c, c->row_voxel, nrows, rv))) return rc;
    Capped out{cap, xyz || rgba || voxel_index};
    for (uint32_t h = 1; h <= c->S0; ++h)
        for (const uint2& leaf : leaves[h])
            for (uint32_t j = 0; j < leaf.y; ++j) {
                if (out.room()) {
                    const float* r = &rows[(size_t)(leaf.x + j) * 12];
                    put3(xyz, out.k, r + 6);
                    if (rgba) rgba[out.k] = (uint32_t)r[9] << 16 | (uint32_t)r[10] << 8 | (uint32_t)r[11];
                    if (voxel_index) voxel_index[out.k] = (uint32_t)rv[leaf.x + j];
                }
                out.next();
            }
    return out.finish(n_out);
}

extern "C" int f3ds_get_voxel_cloud(f3ds_ctx* c, float* xyz, uint32_t* label, uint32_t* rgba, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c)) return frc;
    const uint32_t S0 = c->S0;
    std::vector<unsigned char> ralive; std::vector<std::vector<uint2>> all_leaves; std::vector<uint32_t> loff; std::vector<float> rows;
    int rc;
    if ((rc = region_leaves(c, ralive, all_leaves)) || (rc = fetch(c, c->loff, S0 + 2, loff))) return rc;
    if ((rc = fetch(c, c->rows, rows_in_use(c, loff) * 12, rows))) return rc;
    Capped out{cap, xyz || label || rgba}; uint32_t cur = 0;
    for (uint32_t h = 1; h <= S0; ++h) {
        if (!ralive[h]) continue;
        const std::vector<uint2>& leaves = all_leaves[h];      // the region's leaves (first payload row, rows) in voxels_ concatenation order
        for (const uint2& leaf : leaves)
            for (uint32_t j = 0; j < leaf.y; ++j) {
                if (out.room()) {
                    put3(xyz, out.k, &rows[(size_t)(leaf.x + j) * 12 + 6]);
                    if (label) label[out.k] = cur;
                    if (rgba) rgba[out.k] = f3ds_glasbey_256[cur % 256u];
                }
                out.next();
            }
        cur++;
    }
    return out.finish(n_out);
}

extern "C" int f3ds_get_voxel_centroid_cloud(f3ds_ctx* c, float* xyz, uint32_t* rgba, uint32_t* sv_label, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c, NEED_FRAME | NEED_VOXEL_GRID)) return frc;
    const uint32_t V = c->V;
    int rc;
    if (!all_fit(V, cap, xyz || rgba || sv_label, n_out, &rc)) return rc;
    std::vector<float> f; std::vector<uint32_t> o;
    if ((rc = fetch(c, c->vf, (size_t)V * 12, f)) || (rc = fetch(c, c->owner0, V, o))) return rc;
    for (uint32_t v = 0; v < V; ++v) {
        const float* r = &f[(size_t)v * 12];
        put3(xyz, v, r);
        if (rgba) rgba[v] = ((uint32_t)r[3] & 255u) << 16 | ((uint32_t)r[4] & 255u) << 8 | ((uint32_t)r[5] & 255u);
        if (sv_label) sv_label[v] = o[v];
    }
    return F3DS_OK;
}

extern "C" int f3ds_get_supervoxels(f3ds_ctx* c, uint32_t* label, float* xyz, float* rgb, float* normal, uint32_t* n_voxels, size_t cap, size_t* n_out);

// SupervoxelClustering::refineSupervoxels(num_itr, refined) [PCL-recall], called at src/supervoxel_clustering.cpp:371: on copies of
// the sweep state (main() goes on clustering the unrefined supervoxels), num_itr x { refineNormals on every helper's leaves;
// reseedSupervoxels; expandSupervoxels(max_depth) }.
extern "C" int f3ds_refine_supervoxels(f3ds_ctx* c, int num_itr) {
    if (!c || num_itr < 0) return F3DS_ERR_ARG;
    if (!c->have_frame || c->user_mode) return F3DS_ERR_LOGIC;
    g_sw.read();
    HIPCHECK(hipSetDevice(c->device));
    Batch b = batch_of(c);
    c->refined_itr = -1;
    const uint32_t V = c->V, S0 = c->S0;
    float *r_vf, *r_hc; uint32_t *r_owner, *r_hcount, *L; int *r_gvox, *seed; unsigned char* r_gact;
    ENSURE(c->r_vf, (size_t)V * 12, r_vf); ENSURE(c->r_owner, V, r_owner); ENSURE(c->r_hc, (size_t)(S0 + 1) * 12, r_hc);
    ENSURE(c->r_hcount, S0 + 1, r_hcount); ENSURE(c->r_gvox, S0 + 1, r_gvox); ENSURE(c->r_gact, S0 + 1, r_gact);
    ENSURE(c->r_seed, S0 + 1, seed); ENSURE(c->r_L, V, L);
    rec_copy(c, r_vf, c->vf.p, (size_t)V * 48); rec_copy(c, r_owner, c->owner0.p, (size_t)V * 4); rec_copy(c, r_hc, c->hc.p, (size_t)(S0 + 1) * 48);
    rec_copy(c, r_hcount, c->hcount.p, (size_t)(S0 + 1) * 4); rec_copy(c, r_gvox, c->ghost_vox.p, (size_t)(S0 + 1) * 4); rec_copy(c, r_gact, c->ghost_active.p, S0 + 1);
    SweepBufs sb{&c->r_owner, &c->r_dist, &c->r_hc, &c->r_hcount, &c->r_hlo, &c->r_hhi, &c->r_gvox, &c->r_gact, &c->r_gdone, &c->r_ghead, &c->r_gnext, &c->r_tl, &c->r_tcnt, r_vf, seed, true};
    int rc;
    for (int it = 0; it < num_itr; ++it) {
        rec_copy(c, L, r_owner, (size_t)V * 4);
        rec<d_refine_ghost_L>(c, grid_for(S0, d_refine_ghost_L::BLOCK), 0u, S0, r_gvox, r_gact, L);
        rec<d_refine_normals>(c, grid_for(V, d_refine_normals::BLOCK), 0u, r_vf, c->nbr.p, r_owner, L, V);
        rec<d_reseed>(c, S0 ? S0 : 1u, 0u, r_vf, V, S0, r_hcount, r_hc, seed);
        if ((rc = seg_sweeps_on(c, sb)) || (rc = flush_sync(b))) return rc;
        if (c->h_dc->error) return trace_err(c->h_dc->error, "refine", c);
    }
    if ((rc = flush_sync(b))) return rc;
    c->refined_itr = num_itr;
    return F3DS_OK;
}

// the refined state: per voxel (leaf order) its supervoxel label (0 = none) and normal
extern "C" int f3ds_get_refined_voxels(f3ds_ctx* c, uint32_t* sv_label, float* normal, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c, NEED_FRAME | NEED_REFINED)) return frc;
    const uint32_t V = c->V;
    int rc;
    if (!all_fit(V, cap, sv_label || normal, n_out, &rc)) return rc;
    std::vector<float> f; std::vector<uint32_t> o;
    if ((rc = fetch(c, c->r_vf, (size_t)V * 12, f)) || (rc = fetch(c, c->r_owner, V, o))) return rc;
    for (uint32_t v = 0; v < V; ++v) {
        if (sv_label) sv_label[v] = o[v];
        put3(normal, v, &f[(size_t)v * 12 + 6]);
    }
    return F3DS_OK;
}

namespace {
int supervoxels_of(f3ds_ctx* c, const Scratch<uint32_t>& hcount, const Scratch<float>& hcent, uint32_t* label, float* xyz, float* rgb, float* normal, uint32_t* n_voxels, size_t cap, size_t* n_out) {
    const uint32_t S0 = c->S0;
    std::vector<uint32_t> cnt; std::vector<float> hc;
    int rc;
    if ((rc = fetch(c, hcount, S0 + 1, cnt)) || (rc = fetch(c, hcent, (size_t)(S0 + 1) * 12, hc))) return rc;
    Capped out{cap, label || xyz || rgb || normal || n_voxels};
    for (uint32_t h = 1; h <= S0; ++h) {
        if (!cnt[h]) continue;
        if (out.room()) {
            const float* r = &hc[(size_t)h * 12];
            if (label) label[out.k] = label_out(c, h);
            put3(xyz, out.k, r); put3(rgb, out.k, r + 3); put3(normal, out.k, r + 6);
            if (n_voxels) n_voxels[out.k] = cnt[h];
        }
        out.next();
    }
    return out.finish(n_out);
}
}  // namespace

// the refined supervoxel map (refined_supervoxel_clusters): same layout as f3ds_get_supervoxels
extern "C" int f3ds_get_refined_supervoxels(f3ds_ctx* c, uint32_t* label, float* xyz, float* rgb, float* normal, uint32_t* n_voxels, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c, NEED_FRAME | NEED_REFINED)) return frc;
    return supervoxels_of(c, c->r_hcount, c->r_hc, label, xyz, rgb, normal, n_voxels, cap, n_out);
}

extern "C" int f3ds_get_supervoxels(f3ds_ctx* c, uint32_t* label, float* xyz, float* rgb, float* normal, uint32_t* n_voxels, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c)) return frc;
    return supervoxels_of(c, c->hcount, c->hc, label, xyz, rgb, normal, n_voxels, cap, n_out);
}

extern "C" int f3ds_get_supervoxel_adjacency(f3ds_ctx* c, uint32_t* pairs, size_t cap_pairs, size_t* n_out) {
    if (const int frc = on_frame(c)) return frc;
    const uint32_t E = c->E;
    int rc;
    if (!all_fit(E, cap_pairs, pairs != nullptr, n_out, &rc)) return rc;
    std::vector<uint32_t> a, b;
    if ((rc = fetch(c, c->ea0, E, a)) || (rc = fetch(c, c->eb0, E, b))) return rc;
    for (uint32_t e = 0; e < E; ++e) { pairs[2 * e] = label_out(c, a[e]); pairs[2 * e + 1] = label_out(c, b[e]); }
    return F3DS_OK;
}

// Clustering::get_currentstate().second after cluster(): the adjacency of the merged regions, as pairs (a < b) of the
// surviving supervoxel labels, sorted (src/supervoxel_clustering.cpp:444,465: what visualize() draws as the graph).  Every
// initial adjacency maps to the labels its two supervoxels ended in; merge() keeps one edge per pair (contains(), clustering.cpp:408-436).
extern "C" int f3ds_get_region_adjacency(f3ds_ctx* c, uint32_t* pairs, size_t cap_pairs, size_t* n_out) {
    if (const int frc = on_frame(c)) return frc;
    std::vector<uint32_t> a, b, root;
    int rc;
    if ((rc = fetch(c, c->ea0, c->E, a)) || (rc = fetch(c, c->eb0, c->E, b)) || (rc = fetch(c, c->root, c->S0 + 1, root))) return rc;
    std::vector<uint64_t> keys;
    for (uint32_t e = 0; e < c->E; ++e) {
        const uint32_t p = root[a[e]], q = root[b[e]];
        if (p != q) keys.push_back(((uint64_t)(p < q ? p : q) << 32) | (p < q ? q : p));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (!all_fit(keys.size(), cap_pairs, pairs != nullptr, n_out, &rc)) return rc;
    for (size_t k = 0; k < keys.size(); ++k) { pairs[2 * k] = label_out(c, (uint32_t)(keys[k] >> 32)); pairs[2 * k + 1] = label_out(c, (uint32_t)keys[k]); }
    return F3DS_OK;
}

extern "C" int f3ds_merge_layout_info(uint32_t n_edges, int waves, int keys_in_lds, uint32_t out[4]) {
    if (!out || (waves != 4 && waves != 8) || (keys_in_lds != 0 && keys_in_lds != 2)) return F3DS_ERR_ARG;
    const MergeIlLayout L = merge_il_offsets(n_edges, waves, keys_in_lds);
    out[0] = L.total; out[1] = L.sp_rows; out[2] = L.Ecap;
    out[3] = (L.total <= MC_LDS_LIMIT && (uint64_t)n_edges * (keys_in_lds == 2 ? 10u : 2u) <= (1u << 22)) ? 1u : 0u;
    return F3DS_OK;
}
extern "C" int f3ds_get_debug(f3ds_ctx* c, int what, void* dst, size_t cap_bytes, size_t* bytes_out) {
    if (const int frc = on_frame(c, NEED_NOTHING)) return frc;
    const uint32_t V = c->V, S0 = c->S0, E = c->E, n = c->n;
    std::vector<uint8_t> buf;
    auto put = [&](const void* src, size_t nb) { const uint8_t* b = static_cast<const uint8_t*>(src); buf.insert(buf.end(), b, b + nb); };
    int rc = F3DS_OK;
    std::vector<float> f; std::vector<uint32_t> u, u2, u3; std::vector<int> iv; std::vector<unsigned char> uc;
    if (what != F3DS_DBG_GRID && what != F3DS_DBG_LAUNCH_SHAPE && what != F3DS_DBG_CLOUD_PATH && !c->have_frame) return F3DS_ERR_LOGIC;      // (the launch shape describes the call: an empty frame of a batch has one too)
    switch (what) {
        case F3DS_DBG_GRID: { HIPCHECK(hipMemcpy(c->h_grid, c->d_grid, sizeof(GridInfo), hipMemcpyDeviceToHost)); double g[5] = {c->h_grid->min[0], c->h_grid->min[1], c->h_grid->min[2], c->h_grid->res, (double)c->h_grid->depth}; put(g, sizeof g); break; }
        case F3DS_DBG_TILE_LIST_LEN: if ((rc = fetch(c, c->tile_n1, (size_t)(V + NT_TILE - 1) / NT_TILE, u))) return rc; put(u.data(), u.size() * 4); break;
        case F3DS_DBG_LAUNCH_SHAPE: put(c->launch_shape, 12); break;
        case F3DS_DBG_CLOUD_PATH: put(&c->cloud_path, 4); break;
        case F3DS_DBG_STAGE0_PATH: { const uint32_t w = c->vox_hashed ? 1u : 0u; put(&w, 4); break; }
        case F3DS_DBG_SWEEP_STATS: {
            DevCounters dcs;
            HIPCHECK(hipMemcpy(&dcs, c->d_dc, sizeof dcs, hipMemcpyDeviceToHost));
            put(dcs.sweep_stats, 16);
#ifdef F3DS_CEN_STATS
            fprintf(stderr, "d_centroid: quads %u, live rows %u, to the wave path: list %u, leaves %u; per quad ndmax %.2f, max leaves %.1f; per row nd %.2f, leaves %.1f\n", dcs.cen_stats[0], dcs.cen_stats[1], dcs.cen_stats[2],
                    dcs.cen_stats[3], dcs.cen_stats[4] / (double)dcs.cen_stats[0], dcs.cen_stats[7] / (double)dcs.cen_stats[0], dcs.cen_stats[5] / (double)dcs.cen_stats[1], dcs.cen_stats[6] / (double)dcs.cen_stats[1]);
#endif
            break;
        }
        case F3DS_DBG_MERGE_LAYOUT: { const uint32_t w[2] = {c->merge_kind == MK_GLOBAL ? 0u : (uint32_t)mk_waves(c->merge_kind), c->merge_kind == MK_GLOBAL ? 0u : (uint32_t)mk_res(c->merge_kind)}; put(w, 8); break; }
        case F3DS_DBG_VOXEL_KEYS: if ((rc = fetch(c, c->vkey, (size_t)V * 3, u))) return rc; put(u.data(), u.size() * 4); break;
        case F3DS_DBG_VOXEL_COUNT: if ((rc = fetch(c, c->vcount, V, u))) return rc; put(u.data(), u.size() * 4); break;
        case F3DS_DBG_VOXEL_XYZ: case F3DS_DBG_VOXEL_RGB: case F3DS_DBG_VOXEL_NORMAL:
            if ((rc = fetch(c, c->vf, (size_t)V * 12, f))) return rc;
            for (uint32_t v = 0; v < V; ++v) {
                if (what == F3DS_DBG_VOXEL_XYZ) put(&f[(size_t)v * 12], 12);
                else if (what == F3DS_DBG_VOXEL_RGB) put(&f[(size_t)v * 12 + 3], 12);
                else { float n4[4] = {f[(size_t)v * 12 + 6], f[(size_t)v * 12 + 7], f[(size_t)v * 12 + 8], 0.0f}; put(n4, 16); }
            }
            break;
        case F3DS_DBG_VOXEL_NEIGHBORS: if ((rc = fetch(c, c->nbr, (size_t)V * 27, iv))) return rc; put(iv.data(), iv.size() * 4); break;
        case F3DS_DBG_POINT_VOXEL: if ((rc = fetch(c, c->pt_voxel, n, iv))) return rc; put(iv.data(), iv.size() * 4); break;
        case F3DS_DBG_SEED_ORIG: if ((rc = fetch(c, c->seed_orig, c->C, iv))) return rc; put(iv.data(), iv.size() * 4); break;
        case F3DS_DBG_SEED_KEPT: if ((rc = fetch(c, c->seed_kept, S0, iv))) return rc; put(iv.data(), iv.size() * 4); break;
        case F3DS_DBG_VOXEL_SVLABEL: if ((rc = fetch(c, c->owner0, V, u))) return rc; put(u.data(), u.size() * 4); break;
        case F3DS_DBG_VOXEL_DIST: if ((rc = fetch(c, c->dist0, V, f))) return rc; put(f.data(), f.size() * 4); break;
        case F3DS_DBG_SV_LABELS: case F3DS_DBG_SV_CENTROID: case F3DS_DBG_SV_REGION:
            if ((rc = fetch(c, c->hcount, S0 + 1, u)) || (rc = fetch(c, c->hc, (size_t)(S0 + 1) * 12, f)) || (rc = fetch(c, c->root, S0 + 1, u2))) return rc;
            for (uint32_t h = 1; h <= S0; ++h) {
                if (!u[h]) continue;
                const uint32_t lh = label_out(c, h), lr = label_out(c, u2[h]);
                if (what == F3DS_DBG_SV_LABELS) put(&lh, 4);
                else if (what == F3DS_DBG_SV_REGION) put(&lr, 4);
                else { float r[10]; for (int k = 0; k < 9; ++k) r[k] = f[(size_t)h * 12 + k]; r[9] = 0.0f; put(r, 40); }
            }
            break;
        case F3DS_DBG_EDGES:
            if ((rc = fetch(c, c->ea0, E, u)) || (rc = fetch(c, c->eb0, E, u2))) return rc;
            for (uint32_t e = 0; e < E; ++e) { const uint32_t la = label_out(c, u[e]), lb = label_out(c, u2[e]); put(&la, 4); put(&lb, 4); }
            break;
        case F3DS_DBG_EDGE_DELTAS: if ((rc = fetch(c, c->deltas, (size_t)E * 2, f))) return rc; put(f.data(), f.size() * 4); break;
        case F3DS_DBG_EDGE_WEIGHTS: {
            // initial weights = the epoch-0 history events, decoded back from their keys would lose NaN payloads:
            // recompute from deltas on the host with the same arithmetic
            if ((rc = fetch(c, c->deltas, (size_t)E * 2, f))) return rc;
            MergeParams mp; mp.color_metric = c->prm.color_metric; mp.geom_metric = c->prm.geom_metric; mp.merging = c->prm.merging;
            mp.lambda = c->res.lambda; mp.bins = (c->prm.merging == F3DS_EQUALIZATION && c->prm.bins != 0) ? (short)c->prm.bins : 500;
            std::vector<float> cdf;
            if (c->prm.merging == F3DS_EQUALIZATION) { if ((rc = fetch(c, c->cdf, (size_t)2 * mp.bins, cdf))) return rc; mp.cdf_c = cdf.data(); mp.cdf_g = cdf.data() + mp.bins; }
            else { mp.cdf_c = mp.cdf_g = nullptr; }
            for (uint32_t e = 0; e < E; ++e) { int err = 0; float w = a_tc(mp, f[e * 2], &err) + a_tg(mp, f[e * 2 + 1], &err); put(&w, 4); }
            break;
        }
        case F3DS_DBG_MERGES:
            if ((rc = fetch(c, c->merges, (size_t)c->res.n_merges * 3, u))) return rc;
            if (c->user_mode) for (size_t k = 0; k + 2 < u.size(); k += 3) { u[k] = label_out(c, u[k]); u[k + 1] = label_out(c, u[k + 1]); }
            put(u.data(), u.size() * 4); break;
        case F3DS_DBG_VOXEL_REGION:
            if ((rc = fetch(c, c->owner0, V, u)) || (rc = fetch(c, c->root, S0 + 1, u2)) || (rc = fetch(c, c->rincl, S0 + 1, u3))) return rc;
            for (uint32_t v = 0; v < V; ++v) { uint32_t l = u[v] ? u3[u2[u[v]]] - 1u : F3DS_NO_LABEL; put(&l, 4); }
            break;
        default: return F3DS_ERR_ARG;
    }
    if (!all_fit(buf.size(), cap_bytes, dst != nullptr, bytes_out, &rc)) return rc;
    if (!buf.empty()) memcpy(dst, buf.data(), buf.size());
    return F3DS_OK;
}

// ------------------------------------------------------------------------------------------------
// ground-truth evaluation and the automatic threshold (reference main():387-447, Clustering::all_thresh
// / best_thresh clustering.cpp:691-774, Testing src/testing.cpp).  Not on the per-frame hot path.
// ------------------------------------------------------------------------------------------------
namespace {
// color2label (clustering.cpp:823-846): the distinct colours of col[] are numbered in order of first appearance; col[] becomes the labels, tsize[l] the voxels of label l
void number_truth_colours(std::vector<uint32_t>& col, std::vector<uint32_t>& tsize) {
    std::map<uint32_t, uint32_t> ids;
    tsize.clear();
    for (uint32_t& cv : col) {
        const auto it = ids.find(cv);
        uint32_t l;
        if (it == ids.end()) { l = (uint32_t)tsize.size(); ids.insert({cv, l}); tsize.push_back(0); } else l = it->second;
        cv = l; tsize[l]++;
    }
}
// truth label of every voxel: label colours averaged per voxel on the GPU, distinct colours numbered
// in first-appearance (leaf) order on the host
int eval_truth(f3ds_ctx* c, const uint32_t* truth_point_labels) {
    const uint32_t n = c->n, V = c->V;
    uint32_t *lut, *tp, *tsum, *tcol, *tlab;
    ENSURE(c->glut, 256, lut); ENSURE(c->truth_pts, n, tp); ENSURE(c->tsum, (size_t)V * 3, tsum);
    ENSURE(c->tcol, V, tcol); ENSURE(c->tlab, V, tlab);
    HIPCHECK(hipMemcpyAsync(lut, f3ds_glasbey_256, 1024, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemcpyAsync(tp, truth_point_labels, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHECK(hipMemsetAsync(tsum, 0, (size_t)V * 12, c->stream));
    Batch b = batch_of(c);
    rec<d_truth_accum>(c, grid_for(n, d_truth_accum::BLOCK), 0u, n, c->pt_voxel.p, tp, lut, tsum);
    rec<d_truth_color>(c, grid_for(V, d_truth_color::BLOCK), 0u, V, tsum, c->vcount.p, tcol);
    int rc = flush_sync(b);
    if (rc) return rc;
    std::vector<uint32_t> col;
    if ((rc = fetch(c, c->tcol, V, col))) return rc;
    number_truth_colours(col, c->tsize);
    HIPCHECK(hipMemcpy(tlab, col.data(), (size_t)V * 4, hipMemcpyHostToDevice));
    return F3DS_OK;
}
// scores of the segmentation described by (root, incl): incl[root[h]]-1 is the segment of supervoxel h
int eval_scores(f3ds_ctx* c, const uint32_t* d_root, const uint32_t* d_incl, uint32_t K, f3ds_performance* out) {
    const uint32_t V = c->V, M = (uint32_t)c->tsize.size();
    if (K == 0 || M == 0) return F3DS_ERR_ARG;                         // std::invalid_argument, testing.cpp:414,431
    if ((uint64_t)K * M > (1ull << 26)) return F3DS_ERR_UNSUPPORTED;
    uint32_t *tab, *ssz;
    ENSURE(c->ctab, (size_t)K * M, tab); ENSURE(c->csize, K, ssz);
    HIPCHECK(hipMemsetAsync(tab, 0, (size_t)K * M * 4, c->stream));
    HIPCHECK(hipMemsetAsync(ssz, 0, (size_t)K * 4, c->stream));
    Batch b = batch_of(c);
    rec<d_contingency>(c, grid_for(V, d_contingency::BLOCK), 0u, V, M, c->owner0.p, d_root, d_incl, c->tlab.p, tab, ssz);
    rec<d_contingency_ghost>(c, grid_for(c->S0, d_contingency_ghost::BLOCK), 0u, c->S0, M, c->ghost_vox.p, c->ghost_active.p, c->owner0.p, d_root, d_incl, c->tlab.p, tab, ssz);
    int rc = flush_sync(b);
    if (rc) return rc;
    std::vector<uint32_t> table, ssize;
    if ((rc = fetch(c, c->ctab, (size_t)K * M, table)) || (rc = fetch(c, c->csize, K, ssize))) return rc;
    *out = f3ds_scores_from_table(table, ssize, c->tsize, V);
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_evaluate(f3ds_ctx* c, const uint32_t* truth_point_labels, f3ds_performance* out) {
    if (!truth_point_labels || !out) return F3DS_ERR_ARG;
    int rc = on_frame(c, NEED_FRAME | NEED_VOXEL_GRID);
    if (rc) return rc;
    g_sw.read();      // (eval_truth / eval_scores size their launches by the switches; f3ds_auto_threshold reads them in f3ds_recluster)
    rc = eval_truth(c, truth_point_labels);
    if (rc) return rc;
    return eval_scores(c, c->root.p, c->rincl.p, c->res.n_regions, out);
}

extern "C" int f3ds_auto_threshold(f3ds_ctx* c, const f3ds_params* prm, const uint32_t* truth_point_labels, float start, float end, float step,
                                   float* thresholds, f3ds_performance* scores, size_t cap, size_t* n_out, float* best_threshold,
                                   f3ds_performance* best_score, uint32_t* point_labels, int labels_on_device, f3ds_result* result) {
    if (!c || !prm || !truth_point_labels) return F3DS_ERR_ARG;
    if (!c->have_frame || c->user_mode) return F3DS_ERR_LOGIC;
    if (start < 0 || start > 1 || end < 0 || end > 1 || !(step > 0) || step > 1) return F3DS_ERR_OUT_OF_RANGE;   // std::out_of_range, clustering.cpp:694-698 (step 0 never ends there)
    if (start > end) { float t = start; start = end; end = t; }
    std::vector<float> ts{start};
    for (float t = start + step; t <= end; t += step) ts.push_back(t);
    // Clustering::cluster(state, t) continues one merge sequence, so every threshold's segmentation is a
    // prefix of the merges done at the largest one: merge once, then replay the log on the host
    f3ds_params p = *prm;
    p.threshold = ts.back();
    int rc = f3ds_recluster(c, &p, nullptr, 0, nullptr);
    if (rc) return rc;
    const uint32_t S0 = c->S0, nm = c->res.n_merges;
    std::vector<uint32_t> log, hcount;
    if ((rc = fetch(c, c->merges, (size_t)nm * 3, log)) || (rc = fetch(c, c->hcount, S0 + 1, hcount))) return rc;
    if ((rc = eval_truth(c, truth_point_labels))) return rc;
    uint32_t *d_root, *d_incl;
    ENSURE(c->eroot, S0 + 1, d_root); ENSURE(c->eincl, S0 + 1, d_incl);
    std::vector<uint32_t> parent(S0 + 1), root(S0 + 1), incl(S0 + 1);
    for (uint32_t h = 0; h <= S0; ++h) parent[h] = h;
    std::map<float, f3ds_performance> all;
    uint32_t done = 0;
    for (float t : ts) {
        while (done < nm) {
            float w; memcpy(&w, &log[(size_t)done * 3 + 2], 4);
            if (!(w < t)) break;
            parent[log[(size_t)done * 3 + 1]] = log[(size_t)done * 3];
            done++;
        }
        uint32_t K = 0;
        for (uint32_t h = 0; h <= S0; ++h) {
            uint32_t r = h;
            while (parent[r] != r) r = parent[r];
            root[h] = r;
            if (h > 0 && hcount[h] && r == h) K++;
            incl[h] = K;
        }
        HIPCHECK(hipMemcpy(d_root, root.data(), (size_t)(S0 + 1) * 4, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_incl, incl.data(), (size_t)(S0 + 1) * 4, hipMemcpyHostToDevice));
        f3ds_performance pf;
        if ((rc = eval_scores(c, d_root, d_incl, K, &pf))) return rc;
        all.insert({t, pf});
    }
    float bt = 0; f3ds_performance bp; memset(&bp, 0, sizeof bp);
    for (auto& kv : all) if (kv.second.fscore > bp.fscore) { bp = kv.second; bt = kv.first; }     // best_thresh, :748-774
    size_t k = 0;
    for (auto& kv : all) { if (k < cap) { if (thresholds) thresholds[k] = kv.first; if (scores) scores[k] = kv.second; } k++; }
    if (n_out) *n_out = k;
    if (best_threshold) *best_threshold = bt;
    if (best_score) *best_score = bp;
    p.threshold = bt;
    return f3ds_recluster(c, &p, point_labels, labels_on_device, result);
}

// ------------------------------------------------------------------------------------------------
// hierarchy levels: the labels of K thresholds t_l <= T from the merge log of the last cluster run to T (f3ds_levels.h / .inc).  Reads
// the frame state and leaves it as it was: only the lv_* scratch is written.
// ------------------------------------------------------------------------------------------------
namespace {
// a batch call's contexts: all there, on one device, no context twice (one context holds one frame's scratch)
bool distinct_contexts_on_one_device(f3ds_ctx* const* ctxs, int nctx) {
    for (int i = 0; i < nctx; ++i) {
        if (!ctxs[i] || ctxs[i]->device != ctxs[0]->device) return false;
        for (int j = 0; j < i; ++j) if (ctxs[j] == ctxs[i]) return false;
    }
    return true;
}
bool any_nan(const float* thr, int K) { for (int l = 0; l < K; ++l) if (thr[l] != thr[l]) return true; return false; }
int check_levels(const f3ds_ctx* c, const float* thr, int K) {
    if (!c->have_frame) return F3DS_ERR_LOGIC;
    for (int l = 0; l < K; ++l) if (thr[l] > c->cluster_T) return F3DS_ERR_OUT_OF_RANGE;
    for (int l = 0; l < K; ++l) if (!std::isfinite(thr[l])) return F3DS_ERR_ARG;      // (-inf; NaN is refused before)
    return F3DS_OK;
}
int levels_record(f3ds_ctx* c, const float* d_thr, uint32_t K, bool lds_form, uint32_t* d_out, uint32_t* nreg) {
    const uint32_t S0 = c->S0, n = c->n, nm = c->res.n_merges, Kp = (K + 3u) & ~3u;
    uint32_t *into, *at, *pfx;
    ENSURE(c->lv_into, S0 + 1, into); ENSURE(c->lv_at, S0 + 1, at); ENSURE(c->lv_pfx, (size_t)K * 2, pfx);      // (prefixes, then their order)
    const uint32_t* ord = pfx + K;
    const uint32_t* merges = c->merges.p;
    rec_fill(c, at, LV_NOT_ABSORBED, (size_t)(S0 + 1) * 4);
    rec<d_level_log>(c, grid_for(nm, d_level_log::BLOCK), 0u, nm, S0, merges, into, at);
    rec<d_level_prefix>(c, 1u, 0u, nm, merges, K, d_thr, pfx, pfx + K);
    const unsigned char* alive0 = c->ralive0.p;
    const int* pt_voxel = c->pt_voxel.p; const uint32_t* owner = c->owner0.p;
    if (lds_form) {
        const uint32_t gx = std::min(grid_for(n, d_level_labels::BLOCK), grid_wide(n, 4096));      // (every workgroup builds the tables: as d_relabel)
        rec<d_level_labels>(c, gx, (S0 + 1u) * Kp * 4u, n, pt_voxel, owner, S0, K, Kp, alive0, into, at, pfx, ord, d_out, nreg);
    } else {
        uint32_t* tab; ENSURE(c->lv_tab, (size_t)(S0 + 1) * Kp, tab);
        rec<d_level_tables>(c, 1u, 0u, S0, K, Kp, alive0, into, at, pfx, ord, tab, nreg);
        rec<d_level_points>(c, grid_for(n, d_level_points::BLOCK), 0u, n, K, Kp, pt_voxel, owner, tab, d_out);
    }
    return F3DS_OK;
}
// all contexts on one device, one dispatch per kernel for the batch (grid.y = frame)
int run_levels(f3ds_ctx** ctxs, int nctx, const float* thr, int K, uint32_t* const* point_labels, int labels_on_device, uint32_t* n_regions) {
    g_sw.read();
    f3ds_ctx* o = ctxs[0];
    HIPCHECK(hipSetDevice(o->device));
    Batch b;
    if (const int brc = batch_of(ctxs, nctx, b)) return brc;
    // the thresholds (shared by every frame) go up once, the region counts of all frames come back in one copy: both in the owner's scratch
    float* d_thr; uint32_t* d_nreg;
    { int rc = ensure(o, o->lv_thr, (size_t)K, &d_thr); if (rc) return rc; rc = ensure(o, o->lv_nreg, (size_t)nctx * K, &d_nreg); if (rc) return rc; }
    HIPCHECK(hipMemcpyAsync(d_thr, thr, (size_t)K * 4, hipMemcpyHostToDevice, b.st));
    const uint32_t Kp = ((uint32_t)K + 3u) & ~3u;
    bool lds_form = !g_sw.levels_global;      // one form for the whole batch: its frames record identical command shapes
    for (f3ds_ctx* c : b.fr) if ((uint64_t)(c->S0 + 1u) * Kp * 4u > LV_LDS_BYTES) lds_form = false;
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        uint32_t* d_out;
        if (labels_on_device) d_out = point_labels[i];
        else ENSURE(c->lv_out, (size_t)c->n * K, d_out);
        const int rc = levels_record(c, d_thr, (uint32_t)K, lds_form, d_out, d_nreg + (size_t)i * K);
        if (rc) return rc;
    }
    int rc = flush(b);
    if (rc) return rc;
    std::vector<uint32_t> nreg((size_t)nctx * K);
    HIPCHECK(hipMemcpyAsync(nreg.data(), d_nreg, nreg.size() * 4, hipMemcpyDeviceToHost, b.st));
    if (!labels_on_device) {
        // host outputs as run_cluster copies labels: through the device's copy stream once the labels exist (async into pinned memory), done before the call returns
        hipStream_t dl;
        if ((rc = download_begin(b, &dl))) return rc;
        for (int i = 0; i < nctx; ++i)
            if (ctxs[i]->n) HIPCHECK(hipMemcpyAsync(point_labels[i], ctxs[i]->lv_out.p, (size_t)ctxs[i]->n * K * 4, hipMemcpyDeviceToHost, dl ? dl : b.st));
        if ((rc = download_queued(b, dl)) || (rc = download_wait(b, dl))) return rc;
    }
    HIPCHECK(hipStreamSynchronize(b.st));
    HIPCHECK(hipGetLastError());
    if (n_regions) memcpy(n_regions, nreg.data(), nreg.size() * 4);
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_labels_at_thresholds(f3ds_ctx* c, const float* thresholds, int k, uint32_t* point_labels, int labels_on_device, uint32_t* n_regions) {
    uint32_t* lp[1] = {point_labels};
    return f3ds_labels_at_thresholds_batch(&c, 1, thresholds, k, lp, labels_on_device, n_regions);
}

extern "C" int f3ds_labels_at_thresholds_batch(f3ds_ctx** ctxs, int nctx, const float* thresholds, int k, uint32_t* const* point_labels, int labels_on_device,
                                               uint32_t* n_regions) {
    if (!ctxs || nctx < 1 || !thresholds || k < 1 || !point_labels) return F3DS_ERR_ARG;
    if (any_nan(thresholds, k) || !distinct_contexts_on_one_device(ctxs, nctx)) return F3DS_ERR_ARG;
    for (int i = 0; i < nctx; ++i) if (!point_labels[i]) return F3DS_ERR_ARG;
    for (int i = 0; i < nctx; ++i) { const int rc = check_levels(ctxs[i], thresholds, k); if (rc) return rc; }
    return run_levels(ctxs, nctx, thresholds, k, point_labels, labels_on_device, n_regions);
}

// ------------------------------------------------------------------------------------------------
// scores of hierarchy levels (f3ds_eval_levels.h / .inc): f3ds_evaluate's seven scores for K thresholds of the last
// cluster run, for every frame of a batch.  Reads the frame state and leaves it as it was: only the evaluation scratch (truth_pts ... tlab, which
// every f3ds_evaluate fills anew), the lv_* and the evl_* scratch are written.  Three waits per batch whatever k and nctx are: the truth
// colours (the first-appearance numbering is the host's, as in eval_truth), the base-table sizes, the results.
// ------------------------------------------------------------------------------------------------
namespace {
struct EvlTruth { std::vector<uint32_t> col, tsize, order; uint32_t M = 0, nvis = 0, Eb = 0, G = 0; };
// sorted (key, value) pairs -> the distinct keys below `limit` with summed values and their count
int evl_reduce_record(f3ds_ctx* c, const uint64_t* keys, const uint32_t* vals, uint32_t n, uint64_t limit, uint64_t* ukey, uint32_t* ucnt, uint32_t* total) {
    uint32_t* flag = c->evl_flag.p;
    rec_fill(c, ucnt, 0u, (size_t)n * 4);
    rec<d_evl_heads>(c, grid_for(n, d_evl_heads::BLOCK), 0u, keys, n, limit, flag);
    if (const int rc = scan_u32(c, flag, flag, n)) return rc;
    rec<d_evl_reduce>(c, grid_for(n, d_evl_reduce::BLOCK), 0u, keys, vals, n, limit, flag, ukey, ucnt, total);
    return F3DS_OK;
}
int run_eval_levels(f3ds_ctx** ctxs, int nctx, const uint32_t* const* truth, int truth_on_device, const float* thr, int K_, f3ds_performance* scores, uint32_t* n_regions) {
    g_sw.read();
    f3ds_ctx* o = ctxs[0];
    const uint32_t K = (uint32_t)K_, Kp = (K + 3u) & ~3u;
    HIPCHECK(hipSetDevice(o->device));
    for (int i = 0; i < nctx; ++i) if ((uint64_t)ctxs[i]->V + ctxs[i]->S0 >= (1u << 24)) return F3DS_ERR_UNSUPPORTED;      // (d_evl_score adds sizes as integers: exact in float below 2^24)
    Batch b;
    if (const int brc = batch_of(ctxs, nctx, b)) return brc;
    float* d_thr; uint32_t *d_nreg, *d_counts, *d_out;
    { int rc; if ((rc = ensure(o, o->lv_thr, (size_t)K, &d_thr)) || (rc = ensure(o, o->lv_nreg, (size_t)nctx * K, &d_nreg)) || (rc = ensure(o, o->evl_counts, (size_t)nctx * 4, &d_counts)) ||
                  (rc = ensure(o, o->evl_out, (size_t)nctx * K * 8, &d_out))) return rc; }
    HIPCHECK(hipMemcpyAsync(d_thr, thr, (size_t)K * 4, hipMemcpyHostToDevice, b.st));
    HIPCHECK(hipMemsetAsync(d_counts, 0, (size_t)nctx * 16, b.st));
    // 1. truth colours per voxel, the level tables (they do not depend on the truth) and the ghost list: one flush for all frames
    std::vector<EvlTruth> tr((size_t)nctx);
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        const uint32_t n = c->n, V = c->V, S0 = c->S0, nm = c->res.n_merges;
        uint32_t *lut, *tp = nullptr, *tsum, *tcol, *into, *at, *pfx, *tab, *glist;
        ENSURE(c->glut, 256, lut); ENSURE(c->tsum, (size_t)V * 3, tsum); ENSURE(c->tcol, V, tcol);
        ENSURE(c->lv_into, S0 + 1, into); ENSURE(c->lv_at, S0 + 1, at); ENSURE(c->lv_pfx, (size_t)K * 2, pfx); ENSURE(c->lv_tab, (size_t)(S0 + 1) * Kp, tab); ENSURE(c->evl_glist, S0 + 1, glist);
        HIPCHECK(hipMemcpyAsync(lut, f3ds_glasbey_256, 1024, hipMemcpyHostToDevice, b.st));
        const uint32_t* d_truth = truth[i];
        if (!truth_on_device) { ENSURE(c->truth_pts, n, tp); HIPCHECK(hipMemcpyAsync(tp, truth[i], (size_t)n * 4, hipMemcpyHostToDevice, b.st)); d_truth = tp; }
        rec_fill(c, tsum, 0u, (size_t)V * 12);
        rec_fill(c, at, LV_NOT_ABSORBED, (size_t)(S0 + 1) * 4);
        rec<d_truth_accum>(c, grid_for(n, d_truth_accum::BLOCK), 0u, n, c->pt_voxel.p, d_truth, lut, tsum);
        rec<d_truth_color>(c, grid_for(V, d_truth_color::BLOCK), 0u, V, tsum, c->vcount.p, tcol);
        rec<d_level_log>(c, grid_for(nm, d_level_log::BLOCK), 0u, nm, S0, c->merges.p, into, at);
        rec<d_level_prefix>(c, 1u, 0u, nm, c->merges.p, K, d_thr, pfx, pfx + K);
        rec<d_level_tables>(c, 1u, 0u, S0, K, Kp, c->ralive0.p, into, at, pfx, pfx + K, tab, d_nreg + (size_t)i * K);
        rec<d_evl_ghosts>(c, grid_for(S0, d_evl_ghosts::BLOCK), 0u, S0, c->ghost_active.p, glist, d_counts + (size_t)i * 4 + 1);
    }
    int rc = flush(b);
    if (rc) return rc;
    for (int i = 0; i < nctx; ++i) { tr[i].col.resize(ctxs[i]->V); HIPCHECK(hipMemcpyAsync(tr[i].col.data(), ctxs[i]->tcol.p, (size_t)ctxs[i]->V * 4, hipMemcpyDeviceToHost, b.st)); }
    HIPCHECK(timed_sync(b.st));
    // 2. truth labels in first-appearance order (color2label, as eval_truth), their sizes, the visiting order (evl_visit_order); then the base table
    uint32_t maxM = 1, maxS0 = 1;
    for (int i = 0; i < nctx; ++i) {
        EvlTruth& t = tr[i];
        number_truth_colours(t.col, t.tsize);
        t.M = (uint32_t)t.tsize.size();
        if (t.M == 0) return F3DS_ERR_ARG;      // (std::invalid_argument, testing.cpp:414,431, as eval_scores; a level has K >= 1 whenever the frame has a voxel)
        t.order.resize((size_t)t.M * 3);      // order, rank, then the visited labels ascending
        t.nvis = evl_visit_order_sorted(t.M, t.tsize.data(), t.order.data(), t.order.data() + t.M);
        for (uint32_t k = 0; k < t.nvis; ++k) { t.order[t.nvis + k] = t.order[t.M + k]; }
        for (uint32_t k = 0; k < t.nvis; ++k) t.order[2 * (size_t)t.nvis + t.order[t.nvis + k]] = t.order[k];
        t.order.resize((size_t)t.nvis * 3);
        maxM = std::max(maxM, t.M); maxS0 = std::max(maxS0, ctxs[i]->S0);
    }
    const int jb = bits_for(maxM - 1u), hb = bits_for((uint64_t)maxS0 + 1u), ib = bits_for(maxS0), lb = bits_for(K);
    if (lb + ib + jb > 64) return F3DS_ERR_UNSUPPORTED;
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        EvlTruth& t = tr[i];
        const uint32_t V = c->V, S0 = c->S0;
        uint64_t *k0, *k1, *bkey; uint32_t *v0, *v1, *flag, *bcnt, *tlab, *tsz, *ord, *hist, *tiles;
        ENSURE(c->tlab, V, tlab); ENSURE(c->evl_tsize, t.M, tsz); ENSURE(c->evl_order, t.order.size(), ord);
        ENSURE(c->evl_k0, V, k0); ENSURE(c->evl_k1, V, k1); ENSURE(c->evl_v0, V, v0); ENSURE(c->evl_v1, V, v1); ENSURE(c->evl_flag, V, flag); ENSURE(c->evl_bkey, V, bkey); ENSURE(c->evl_bcnt, V, bcnt);
        ENSURE(c->hist, (size_t)RS_BINS * ((V + RS_TILE - 1) / RS_TILE + 1), hist); ENSURE(c->tiles, (V + SCAN_TILE - 1) / SCAN_TILE + 1, tiles);
        HIPCHECK(hipMemcpyAsync(tlab, t.col.data(), (size_t)V * 4, hipMemcpyHostToDevice, b.st));
        HIPCHECK(hipMemcpyAsync(tsz, t.tsize.data(), (size_t)t.M * 4, hipMemcpyHostToDevice, b.st));
        HIPCHECK(hipMemcpyAsync(ord, t.order.data(), t.order.size() * 4, hipMemcpyHostToDevice, b.st));
        rec<d_evl_base_keys>(c, grid_for(V, d_evl_base_keys::BLOCK), 0u, V, S0, t.M, c->owner0.p, tlab, jb, k0, v0);
        uint64_t* ks; uint32_t* vs;
        if ((rc = radix_sort(c, k0, v0, k1, v1, V, hb + jb, &ks, &vs))) return rc;
        if ((rc = evl_reduce_record(c, ks, vs, V, (uint64_t)(S0 + 1u) << jb, bkey, bcnt, d_counts + (size_t)i * 4))) return rc;
    }
    if ((rc = flush(b))) return rc;
    std::vector<uint32_t> counts((size_t)nctx * 4);
    HIPCHECK(hipMemcpyAsync(counts.data(), d_counts, counts.size() * 4, hipMemcpyDeviceToHost, b.st));
    HIPCHECK(timed_sync(b.st));
    // 3. every level's table, the matching and the scores
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        EvlTruth& t = tr[i];
        t.Eb = counts[(size_t)i * 4]; t.G = counts[(size_t)i * 4 + 1];
        const uint32_t V = c->V, S0 = c->S0, ne = t.Eb + t.G;
        const uint64_t n64 = (uint64_t)K * ne;
        if (t.Eb > V || t.G > S0 || n64 == 0 || n64 >= (1ull << 31)) return n64 >= (1ull << 31) ? F3DS_ERR_UNSUPPORTED : F3DS_ERR_ARG;
        const uint32_t n = (uint32_t)n64;
        uint64_t *k0, *k1, *ukey; uint32_t *v0, *v1, *flag, *ucnt, *ssize, *slot, *hist, *tiles; unsigned char* used; float *hterm, *mterm, *tterm;
        ENSURE(c->evl_k0, n, k0); ENSURE(c->evl_k1, n, k1); ENSURE(c->evl_v0, n, v0); ENSURE(c->evl_v1, n, v1); ENSURE(c->evl_flag, n, flag); ENSURE(c->evl_ukey, n, ukey); ENSURE(c->evl_ucnt, n, ucnt);
        ENSURE(c->evl_ssize, (size_t)K * (S0 + 1), ssize); ENSURE(c->evl_used, (size_t)K * (S0 + 1), used); ENSURE(c->evl_hterm, (size_t)K * (S0 + 1), hterm); ENSURE(c->evl_mterm, n, mterm);
        ENSURE(c->evl_tterm, (size_t)t.M + 1, tterm); ENSURE(c->evl_slot, (size_t)K * t.nvis * 4 + 1, slot);
        ENSURE(c->hist, (size_t)RS_BINS * ((n + RS_TILE - 1) / RS_TILE + 1), hist); ENSURE(c->tiles, (n + SCAN_TILE - 1) / SCAN_TILE + 1, tiles);
        uint32_t* d_total = d_counts + (size_t)i * 4 + 2;
        const uint32_t* ord = c->evl_order.p;
        rec_fill(c, ssize, 0u, (size_t)K * (S0 + 1) * 4);
        rec_fill(c, used, 0u, (size_t)K * (S0 + 1));
        rec<d_evl_level_keys>(c, grid_for(ne, d_evl_level_keys::BLOCK), 0u, t.Eb, t.G, K, Kp, S0, t.M, V, c->evl_bkey.p, c->evl_bcnt.p, c->evl_glist.p, c->ghost_vox.p, c->owner0.p, c->tlab.p, c->lv_tab.p, ib, jb, k0, v0, ssize);
        uint64_t* ks; uint32_t* vs;
        if ((rc = radix_sort(c, k0, v0, k1, v1, n, lb + ib + jb, &ks, &vs))) return rc;
        if ((rc = evl_reduce_record(c, ks, vs, n, (uint64_t)K << (ib + jb), ukey, ucnt, d_total))) return rc;
        rec<d_evl_col_keys>(c, grid_for(n, d_evl_col_keys::BLOCK), 0u, ukey, ucnt, d_total, ib, jb, k0, v0);
        if ((rc = radix_sort(c, k0, v0, k1, v1, n, lb + jb, &ks, &vs, ib, d_total))) return rc;
        rec<d_evl_ht>(c, 1u, 0u, t.M, c->evl_tsize.p, V, tterm, tterm + t.M);
        rec<d_evl_score>(c, K, 0u, K, S0, V, d_nreg + (size_t)i * K, ssize, c->evl_tsize.p, ukey, ucnt, ks, vs, d_total, ib, jb, ord, ord + t.nvis, ord + 2 * (size_t)t.nvis, t.nvis,
                         tterm + t.M, used, hterm, mterm, slot, d_out + (size_t)i * K * 8);
    }
    if ((rc = flush(b))) return rc;
    std::vector<uint32_t> out((size_t)nctx * K * 8);
    HIPCHECK(hipMemcpyAsync(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost, b.st));
    if (g_sw.host_prof) HIPCHECK(hipMemcpyAsync(counts.data(), d_counts, counts.size() * 4, hipMemcpyDeviceToHost, b.st));
    HIPCHECK(timed_sync(b.st));
    HIPCHECK(hipGetLastError());
    if (g_sw.host_prof) {      // F3DS_HOST_PROF: the sizes the scratch follows, per frame (min / mean / max over the batch)
        auto line = [&](const char* what, auto get) {
            double lo = 1e300, hi = 0, sum = 0;
            for (int i = 0; i < nctx; ++i) { const double v = get(i); lo = std::min(lo, v); hi = std::max(hi, v); sum += v; }
            fprintf(stderr, " %s %.0f / %.0f / %.0f;", what, lo, sum / nctx, hi);
        };
        fprintf(stderr, "f3ds_evaluate_levels: %d frames x %u levels, global-memory tables:", nctx, K);
        line("truth labels M", [&](int i) { return (double)tr[i].M; }); line("visited labels", [&](int i) { return (double)tr[i].nvis; });
        line("base entries", [&](int i) { return (double)tr[i].Eb; }); line("live ghost leaves", [&](int i) { return (double)tr[i].G; });
        line("entries per level (mean over the levels)", [&](int i) { return (double)counts[(size_t)i * 4 + 2] / K; });
        fprintf(stderr, " key bits %d + %d + %d\n", lb, ib, jb);
    }
    for (size_t q = 0; q < (size_t)nctx * K; ++q) {
        if (out[q * 8 + 7] == 0u) return F3DS_ERR_ARG;      // (a level without regions: std::invalid_argument, as eval_scores)
        memcpy(&scores[q], &out[q * 8], sizeof(f3ds_performance));
        if (n_regions) n_regions[q] = out[q * 8 + 7];
    }
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_evaluate_levels(f3ds_ctx* c, const uint32_t* truth_point_labels, int truth_on_device, const float* thresholds, int k, f3ds_performance* scores,
                                    uint32_t* n_regions) {
    const uint32_t* tp[1] = {truth_point_labels};
    return f3ds_evaluate_levels_batch(&c, 1, tp, truth_on_device, thresholds, k, scores, n_regions);
}

extern "C" int f3ds_evaluate_levels_batch(f3ds_ctx** ctxs, int nctx, const uint32_t* const* truth_point_labels, int truth_on_device, const float* thresholds, int k,
                                          f3ds_performance* scores, uint32_t* n_regions) {
    if (!ctxs || nctx < 1 || !truth_point_labels || !thresholds || k < 1 || !scores) return F3DS_ERR_ARG;
    if (any_nan(thresholds, k) || !distinct_contexts_on_one_device(ctxs, nctx)) return F3DS_ERR_ARG;
    for (int i = 0; i < nctx; ++i) if (!truth_point_labels[i]) return F3DS_ERR_ARG;
    for (int i = 0; i < nctx; ++i) {
        if (ctxs[i]->have_frame && (ctxs[i]->user_mode || ctxs[i]->V == 0)) return F3DS_ERR_LOGIC;      // (as f3ds_evaluate; no voxel: nothing to score)
        const int rc = check_levels(ctxs[i], thresholds, k);
        if (rc) return rc;
    }
    return run_eval_levels(ctxs, nctx, truth_point_labels, truth_on_device, thresholds, k, scores, n_regions);
}

extern "C" int f3ds_best_level(const float* thresholds, const f3ds_performance* scores, int k, int* best_index) {
    if (!thresholds || !scores || !best_index || k < 1 || any_nan(thresholds, k)) return F3DS_ERR_ARG;
    std::vector<int> idx((size_t)k);
    for (int l = 0; l < k; ++l) idx[l] = l;
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return thresholds[a] < thresholds[b]; });
    int best = -1; float bf = 0.0f;
    for (int q = 0; q < k; ++q) {
        const int l = idx[q];
        if (q > 0 && thresholds[idx[q - 1]] == thresholds[l]) continue;      // (std::map::insert keeps the first of equal thresholds)
        if (scores[l].fscore > bf) { bf = scores[l].fscore; best = l; }       // best_thresh, clustering.cpp:759-774
    }
    *best_index = best;
    return F3DS_OK;
}

extern "C" int f3ds_get_merge_tree(f3ds_ctx* c, uint32_t* survivor, uint32_t* absorbed, float* weight, size_t cap, size_t* n_out) {
    if (const int frc = on_frame(c)) return frc;
    const size_t nm = c->res.n_merges;
    int rc;
    if (!all_fit(nm, cap, survivor || absorbed || weight, n_out, &rc)) return rc;
    std::vector<uint32_t> u;
    if ((rc = fetch(c, c->merges, nm * 3, u))) return rc;
    for (size_t i = 0; i < nm; ++i) {
        if (survivor) survivor[i] = label_out(c, u[i * 3]);
        if (absorbed) absorbed[i] = label_out(c, u[i * 3 + 1]);
        if (weight) memcpy(&weight[i], &u[i * 3 + 2], 4);
    }
    return F3DS_OK;
}

// ------------------------------------------------------------------------------------------------
// label tracker (f3ds_track.h / .inc): persistent ids for the regions of consecutive RGB-D frames.  The tracker owns a
// private context for its stream, scratch and copy-stream plumbing, and two state buffers (slot and depth per pixel of the previous frame) that
// it swaps: an update reads one and writes the other.  Per update: d_track_keys, the stage-0 radix sort on the keys alone, d_evl_heads / scan,
// d_track_runs, d_track_pack; ONE download (entries, their count, the bad-label flag) and the update's only wait before the output; the
// assignment on the host (f3ds_track_assign: the entries number thousands, not pixels); one upload of id[]; d_track_apply.
// ------------------------------------------------------------------------------------------------
struct f3ds_tracker {
    f3ds_ctx* c = nullptr;
    f3ds_track_params prm;
    uint32_t* slot[2] = {nullptr, nullptr}; float* z[2] = {nullptr, nullptr}; size_t state_n = 0;      // pixels a state buffer holds
    int cur = 0;                            // slot[cur] / z[cur]: the previous frame
    bool have_prev = false, have_fmt = false, have_ids = false;
    f3ds_rgbd_format fmt;                   // remembered with the state: width, height and intrinsics must not change under it
    std::vector<uint32_t> prev_id, ids;     // prev_id[slot]: persistent id of the previous frame's regions; ids: id[] of the last update
    uint32_t next_id = 0;
    uint32_t* h_out = nullptr; size_t out_cap = 0;      // pinned: TRK_HEAD words + out_cap (i, j, c) triples
    uint32_t* h_id = nullptr; size_t id_cap = 0;        // pinned: id[] on its way up
};

namespace {
static_assert(TK_MAX_REGIONS == LI_MAX_REGIONS, "li_check applies the tracker's cap");
constexpr size_t TRK_FIRST_CAP = 1024;     // entries the first download has room for; a frame with more is packed again with room for twice its count
int trk_pinned(uint32_t** p, size_t* cap, size_t want) {
    if (*cap >= want && *p) return F3DS_OK;
    if (*p) { HIPCHECK(hipHostFree(*p)); *p = nullptr; *cap = 0; }
    HIPCHECK(hipHostMalloc(p, (want ? want : 1) * sizeof(uint32_t), hipHostMallocDefault));
    *cap = want;
    return F3DS_OK;
}
int trk_state(f3ds_tracker* t, size_t n) {
    if (t->state_n == n && t->slot[0]) return F3DS_OK;      // (a remembered format fixes n: only a tracker without a previous frame gets here)
    for (int k = 0; k < 2; ++k) {
        if (t->slot[k]) HIPCHECK(hipFree(t->slot[k]));
        if (t->z[k]) HIPCHECK(hipFree(t->z[k]));
        t->slot[k] = nullptr; t->z[k] = nullptr;
    }
    t->state_n = 0;
    for (int k = 0; k < 2; ++k) { HIPCHECK(hipMalloc(&t->slot[k], n * 4)); HIPCHECK(hipMalloc(&t->z[k], n * 4)); }
    t->state_n = n;
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_tracker_create(int device, const f3ds_track_params* params, f3ds_tracker** out) {
    if (!out) return F3DS_ERR_ARG;
    *out = nullptr;
    f3ds_track_params prm;
    if (params) prm = *params; else f3ds_default_track_params(&prm);
    if (!tk_params_ok(prm.min_permille, prm.depth_tol)) return F3DS_ERR_ARG;
    f3ds_ctx* c = nullptr;
    if (const int rc = f3ds_create(device, &c)) return rc;
    f3ds_tracker* t = new f3ds_tracker;
    t->c = c; t->prm = prm;
    memset(&t->fmt, 0, sizeof t->fmt);
    *out = t;
    return F3DS_OK;
}

extern "C" void f3ds_tracker_destroy(f3ds_tracker* t) {
    if (!t) return;
    (void)hipSetDevice(t->c->device);
    if (t->c->stream) (void)hipStreamSynchronize(t->c->stream);
    for (int k = 0; k < 2; ++k) { if (t->slot[k]) (void)hipFree(t->slot[k]); if (t->z[k]) (void)hipFree(t->z[k]); }
    if (t->h_out) (void)hipHostFree(t->h_out);
    if (t->h_id) (void)hipHostFree(t->h_id);
    f3ds_destroy(t->c);
    delete t;
}

extern "C" int f3ds_tracker_set_stream(f3ds_tracker* t, void* hip_stream) {
    if (!t) return F3DS_ERR_ARG;
    return f3ds_set_stream(t->c, hip_stream);
}

extern "C" int f3ds_tracker_reset(f3ds_tracker* t) {
    if (!t) return F3DS_ERR_ARG;
    t->have_prev = false; t->have_fmt = false; t->prev_id.clear();
    return F3DS_OK;
}

extern "C" int f3ds_tracker_get_ids(f3ds_tracker* t, uint32_t* id_of_region, size_t cap, size_t* n_out) {
    if (!t || (!id_of_region && !n_out)) return F3DS_ERR_ARG;
    if (!t->have_ids) return F3DS_ERR_LOGIC;
    int rc;
    if (!all_fit(t->ids.size(), cap, id_of_region != nullptr, n_out, &rc)) return rc;
    if (!t->ids.empty()) memcpy(id_of_region, t->ids.data(), t->ids.size() * 4);
    return F3DS_OK;
}

extern "C" int f3ds_tracker_update(f3ds_tracker* t, const f3ds_rgbd_format* fmt_, const void* depth, const uint32_t* labels, uint32_t n_regions, int inputs_on_device,
                                   const float* pose12, uint32_t* track_ids, int ids_on_device, f3ds_track_result* result) {
    if (!t || !track_ids) return F3DS_ERR_ARG;
    f3ds_rgbd_format fmt; f3ds::RgbdLayout lay;
    const int crc = li_check(fmt_, depth, nullptr, labels, n_regions, &fmt, &lay);
    if (crc == F3DS_ERR_ARG) return crc;
    if (pose12) for (int k = 0; k < 12; ++k) if (!m_isfinitef(pose12[k])) return F3DS_ERR_ARG;
    if (t->have_fmt && (fmt.width != t->fmt.width || fmt.height != t->fmt.height || fmt.fx != t->fmt.fx || fmt.fy != t->fmt.fy || fmt.cx != t->fmt.cx || fmt.cy != t->fmt.cy))
        return F3DS_ERR_ARG;      // (the state is an image of the remembered camera: the caller resets first)
    if (crc) return crc;      // (more than TK_MAX_REGIONS regions)
    f3ds_ctx* c = t->c;
    Batch b;
    if (const int rc = li_begin(c, &b)) return rc;
    const uint32_t n = (uint32_t)lay.n, Kc = n_regions, Kp = t->have_prev ? (uint32_t)t->prev_id.size() : 0u;
    const int jb = tk_bits(Kp), sort_bits = tk_bits(Kc) + jb;
    if (const int rc = trk_state(t, n)) return rc;
    if (!t->h_out) { if (const int rc = trk_pinned(&t->h_out, &t->out_cap, TRK_HEAD + 3 * TRK_FIRST_CAP)) return rc; }
    size_t cap = (t->out_cap - TRK_HEAD) / 3;
    // every buffer of the update before anything is recorded
    uint64_t *k0, *k1, *ukey; uint32_t *flag, *ustart, *uend, *out, *d_id, *cnt, *hist, *tiles, *tid = nullptr;
    ENSURE(c->evl_k0, n, k0); ENSURE(c->evl_k1, n, k1); ENSURE(c->evl_flag, n, flag); ENSURE(c->evl_ukey, n, ukey); ENSURE(c->evl_ucnt, n, ustart); ENSURE(c->trk_end, n, uend);
    ENSURE(c->trk_out, TRK_HEAD + 3 * cap, out); ENSURE(c->trk_id, Kc ? Kc : 1u, d_id); ENSURE(c->evl_counts, 4, cnt);
    ENSURE(c->hist, (size_t)RS_BINS * ((n + RS_TILE - 1) / RS_TILE + 1), hist); ENSURE(c->tiles, (n + SCAN_TILE - 1) / SCAN_TILE + 1, tiles);
    if (!ids_on_device) ENSURE(c->trk_tid, n, tid);
    LiImages im;
    if (const int urc = li_upload(c, b, lay, depth, nullptr, labels, inputs_on_device, &im)) return urc;
    const unsigned char* d_depth = im.depth;
    const uint32_t* d_lab = im.labels;
    TrackArgs a;
    memset(&a, 0, sizeof a);
    a.width = fmt.width; a.height = fmt.height; a.n = n; a.depth_pitch = lay.depth_pitch; a.depth_f32 = fmt.depth_type == F3DS_DEPTH_F32 ? 1 : 0;
    a.has_pose = pose12 ? 1 : 0; a.has_prev = t->have_prev ? 1 : 0; a.Kc = Kc; a.Kp = Kp; a.jb = jb;
    a.depth_scale = fmt.depth_scale; a.fx = fmt.fx; a.fy = fmt.fy; a.cx = fmt.cx; a.cy = fmt.cy; a.depth_tol = t->prm.depth_tol;
    if (pose12) memcpy(a.pose, pose12, sizeof a.pose);
    const int nxt = t->cur ^ 1;
    int rc;
    HIPCHECK(hipMemsetAsync(cnt, 0, 16, b.st));      // [0] entries, [1] the bad-label flag
    rec<d_track_keys>(c, grid_for(n, d_track_keys::BLOCK), 0u, d_depth, d_lab, t->have_prev ? t->slot[t->cur] : nullptr, t->have_prev ? t->z[t->cur] : nullptr, a, k0, t->slot[nxt], t->z[nxt], cnt + 1);
    uint64_t* ks;
    if ((rc = radix_sort(c, k0, nullptr, k1, nullptr, n, sort_bits, &ks, nullptr))) return rc;
    rec<d_evl_heads>(c, grid_for(n, d_evl_heads::BLOCK), 0u, ks, n, tk_hole(Kc, jb), flag);
    if ((rc = scan_u32(c, flag, flag, n))) return rc;
    rec<d_track_runs>(c, grid_for(n, d_track_runs::BLOCK), 0u, ks, n, tk_hole(Kc, jb), flag, ukey, ustart, uend, cnt);
    rec<d_track_pack>(c, grid_for(cap, d_track_pack::BLOCK), 0u, ukey, ustart, uend, cnt, cnt + 1, jb, (uint32_t)cap, out);
    if ((rc = flush(b))) return rc;
    HIPCHECK(hipMemcpyAsync(t->h_out, out, (TRK_HEAD + 3 * cap) * 4, hipMemcpyDeviceToHost, b.st));
    HIPCHECK(timed_sync(b.st));
    HIPCHECK(hipGetLastError());
    if (t->h_out[1]) return F3DS_ERR_ARG;      // a label >= n_regions: the state buffers are not swapped, nothing of the tracker has changed
    const uint32_t total = t->h_out[0];
    if (total > n) return F3DS_ERR_LOGIC;
    if (total > cap) {      // (rare: more distinct (region, slot) pairs than the download had room for)
        cap = (size_t)total * 2;
        if ((rc = trk_pinned(&t->h_out, &t->out_cap, TRK_HEAD + 3 * cap))) return rc;
        ENSURE(c->trk_out, TRK_HEAD + 3 * cap, out);
        rec<d_track_pack>(c, grid_for(cap, d_track_pack::BLOCK), 0u, ukey, ustart, uend, cnt, cnt + 1, jb, (uint32_t)cap, out);
        if ((rc = flush(b))) return rc;
        HIPCHECK(hipMemcpyAsync(t->h_out, out, (TRK_HEAD + 3 * (size_t)total) * 4, hipMemcpyDeviceToHost, b.st));
        HIPCHECK(timed_sync(b.st));
    }
    // size[i] = the sum of region i's row, the no-vote column (j == Kp) included; the votes go to the assignment
    std::vector<uint32_t> size(Kc, 0u), votes, ids(Kc, F3DS_NO_LABEL);
    votes.reserve((size_t)total * 3);
    for (uint32_t e = 0; e < total; ++e) {
        const uint32_t* en = t->h_out + TRK_HEAD + (size_t)e * 3;
        if (en[0] >= Kc || en[1] > Kp) return F3DS_ERR_LOGIC;
        size[en[0]] += en[2];
        if (en[1] < Kp) votes.insert(votes.end(), en, en + 3);
    }
    uint32_t next = t->next_id;
    f3ds_track_result r;
    if ((rc = f3ds_track_assign(&t->prm, size.data(), Kc, votes.data(), votes.size() / 3, t->prev_id.data(), Kp, &next, ids.data(), &r))) return rc;
    r.first_frame = t->have_prev ? 0u : 1u;
    if ((rc = trk_pinned(&t->h_id, &t->id_cap, Kc))) return rc;
    if (Kc) { memcpy(t->h_id, ids.data(), (size_t)Kc * 4); HIPCHECK(hipMemcpyAsync(d_id, t->h_id, (size_t)Kc * 4, hipMemcpyHostToDevice, b.st)); }
    rec<d_track_apply>(c, grid_for(n, d_track_apply::BLOCK), 0u, d_lab, n, d_id, Kc, ids_on_device ? track_ids : tid);
    if ((rc = flush(b))) return rc;
    if (!ids_on_device) {
        hipStream_t dl;      // (queued on the copy stream only once the ids exist, as the labels of f3ds_segment_batch)
        if ((rc = download_begin(b, &dl))) return rc;
        HIPCHECK(hipMemcpyAsync(track_ids, tid, (size_t)n * 4, hipMemcpyDeviceToHost, dl ? dl : b.st));
        if ((rc = download_queued(b, dl)) || (rc = download_wait(b, dl))) return rc;
    }
    HIPCHECK(timed_sync(b.st));
    HIPCHECK(hipGetLastError());
    // the update stands: the buffer just written is the previous frame from now on
    t->cur = nxt; t->have_prev = true; t->have_fmt = true; t->fmt = fmt;
    t->prev_id = ids; t->ids.swap(ids); t->have_ids = true; t->next_id = next;
    if (result) *result = r;
    return F3DS_OK;
}

// ------------------------------------------------------------------------------------------------
// The five region calls share the label-image frame (li_begin ... li_rows_behind, above): the images of a host caller go up through the family's staging, the
// kernels of a call are recorded into one flush, and what goes down -- the heads and, for a host caller, what rides behind them on the call's stream, not through
// the copy stream -- is ONE download, the call's only wait in the ordinary case.  The staging (li_*) holds nothing once a call has returned; the working state
// between a call's kernels is the call's own (rgt_acc, rgc_*, rgs_acc, rgx_*, rgk_*; pass one of the boxes adds into rgs_acc, which both of its users zero first and
// which holds nothing between calls), so no call disturbs what another one of the context reads.
//
// Every call is written ONCE, for a batch of frames: f3ds_region_<x>_batch checks, stages, records every frame through <x>_record (one
// frame: its scratch, its argument struct, its rec<> lines), flushes -- one dispatch per kernel, grid.y = frame -- downloads once and delivers frame by frame;
// f3ds_region_<x> is that batch of one frame, with the same kernels, grids and waits as ever.  The staging of all frames and their uploads come before the first
// <x>_record; the scratch a frame's <x>_record ensures is its own context's, which only that context's recorded calls refer to (the regrow guard of ensure()).
// A frame's status is what the lone call returns once it has looked at pixels; the call returns the status of the lowest failing frame.
// ------------------------------------------------------------------------------------------------
namespace {
// what every batch form refuses first: no contexts, a NULL or repeated one, contexts on different devices
inline bool li_batch_ctxs(f3ds_ctx* const* ctxs, int nctx) { return ctxs && nctx >= 1 && distinct_contexts_on_one_device(ctxs, nctx); }

// region table (f3ds_regions.h / .inc): one row per region of a label image over an RGB-D frame.  Three kernels -- d_region_init,
// d_region_accum (the one read of the images), d_region_finish; behind the heads the rows of a host caller (72 B per region).
int rg_record(f3ds_ctx* c, const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, const LiImages& im, uint32_t K, uint32_t* head, f3ds_region_row* d_rows) {
    const uint32_t n = (uint32_t)lay.n, copies = rgt_copies(K);
    RgAcc* acc;
    ENSURE(c->rgt_acc, K ? (size_t)K * copies : 1u, acc);
    RegionArgs a;
    memset(&a, 0, sizeof a);
    a.width = fmt.width; a.n = n; a.depth_pitch = lay.depth_pitch; a.color_pitch = lay.color_pitch; a.depth_f32 = fmt.depth_type == F3DS_DEPTH_F32 ? 1 : 0;
    a.color_format = im.color ? fmt.color_format : -1; a.K = K; a.copies = copies;
    a.depth_scale = fmt.depth_scale; a.fx = fmt.fx; a.fy = fmt.fy; a.cx = fmt.cx; a.cy = fmt.cy;
    rec<d_region_init>(c, grid_for((size_t)K * copies * RG_WORDS, d_region_init::BLOCK), 0u, reinterpret_cast<uint32_t*>(acc), K * copies, head);
    rec<d_region_accum>(c, grid_for((n + LI_TRIPS - 1u) / LI_TRIPS, d_region_accum::BLOCK), 0u, im.depth, im.color, im.labels, a, acc, head);
    rec<d_region_finish>(c, grid_for(K, d_region_finish::BLOCK), 0u, acc, K, copies, head, d_rows);
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_region_table_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt_, const void* const* depth, const void* const* color, const uint32_t* const* labels,
                                       const uint32_t* n_regions, int inputs_on_device, f3ds_region_row* const* rows, int rows_on_device, f3ds_region_table_result* results,
                                       int* status) {
    if (!li_batch_ctxs(ctxs, nctx) || !depth || !labels || !n_regions || !rows) return F3DS_ERR_ARG;
    f3ds_rgbd_format fmt; f3ds::RgbdLayout lay;
    for (int i = 0; i < nctx; ++i) {
        if (color && !color[i]) return F3DS_ERR_ARG;      // (a colour image for every frame or for none: one command sequence)
        if (const int rc = rg_check(fmt_, depth[i], color ? color[i] : nullptr, labels[i], n_regions[i], rows[i], &fmt, &lay)) return rc;
    }
    Batch b;
    if (const int rc = li_begin(ctxs, nctx, &b)) return rc;
    std::vector<size_t> fixed((size_t)nctx);
    for (int i = 0; i < nctx; ++i) fixed[i] = rows_on_device ? 0u : (size_t)n_regions[i] * sizeof(f3ds_region_row);
    LiStage s; std::vector<LiImages> im((size_t)nctx);
    if (const int rc = li_out_buffers(ctxs[0], nctx, fixed.data(), nullptr, 0u, 0u, &s)) return rc;
    if (const int rc = li_upload(ctxs, nctx, b, lay, depth, color, labels, inputs_on_device, im.data())) return rc;
    for (int i = 0; i < nctx; ++i) if (const int rc = rg_record(ctxs[i], fmt, lay, im[i], n_regions[i], s.head(i), li_out_ptr(rows_on_device, rows[i], s, i))) return rc;
    return li_deliver_fixed(s, b, nctx, fixed.data(), rows, nullptr, static_cast<void* const*>(nullptr), status, [&](int i, const uint32_t* h) {
        if (!results) return;
        results[i].n_regions = n_regions[i]; results[i].n_nonempty = h[0];
        memcpy(&results[i].n_labelled, h + 2, 8); memcpy(&results[i].n_clamped, h + 4, 8);
    });
}
extern "C" int f3ds_region_table(f3ds_ctx* c, const f3ds_rgbd_format* fmt_, const void* depth, const void* color, const uint32_t* labels, uint32_t n_regions, int inputs_on_device,
                                 f3ds_region_row* rows, int rows_on_device, f3ds_region_table_result* result) {
    return f3ds_region_table_batch(&c, 1, fmt_, &depth, color ? &color : nullptr, &labels, &n_regions, inputs_on_device, &rows, rows_on_device, result, nullptr);
}

// ------------------------------------------------------------------------------------------------
// region contacts (f3ds_contacts.h / .inc): one row per pair of regions of a label image that touch.  d_pair_init, d_contact_accum
// (the one pass over the images: records of (pair, seven words)), the radix sort of the record keys, d_evl_heads / scan, d_track_runs, d_contact_finish; behind
// the head (row count, the bad-label flag, the records asked for, the sums) the first RGC_FIRST_ROWS rows of a host caller.  A frame with more records than the
// first buffer holds says so in the head and runs once more, alone, with room for all (every contact pair a record of its own: fewer than 2n) once the others
// have been delivered; a host caller with more rows gets the rest in a second download.  The frames of a batch share the record room (one n) and the sort
// width, the largest any frame needs (zero key bits above a frame's own sort to nothing).  Beside rgc_* the call uses the sort's histogram and the scan's
// tile sums, which hold nothing between calls.  All of this is the pair call's (pair_record, pair_run), which the joints share: a call is its scratch, its two
// kernels, its row and its result.
// ------------------------------------------------------------------------------------------------
namespace {
// The scratch of a pair call (the contacts over rgc_*, the joints over rgj_*): the records' keys and indices (twice: the sort), the records, the runs' flags,
// keys, starts and ends, the run count.
struct PairScratch {
    Scratch<uint64_t>&k0, &k1; Scratch<uint32_t>&v0, &v1, &rec, &flag; Scratch<uint64_t>& ukey; Scratch<uint32_t>&ustart, &uend, &cnt;
};
inline PairScratch rgc_scratch(f3ds_ctx* c) { return {c->rgc_k0, c->rgc_k1, c->rgc_v0, c->rgc_v1, c->rgc_rec, c->rgc_flag, c->rgc_ukey, c->rgc_ustart, c->rgc_uend, c->rgc_cnt}; }
inline PairScratch rgj_scratch(f3ds_ctx* c) { return {c->rgj_k0, c->rgj_k1, c->rgj_v0, c->rgj_v1, c->rgj_rec, c->rgj_flag, c->rgj_ukey, c->rgj_ustart, c->rgj_uend, c->rgj_cnt}; }
PairArgs pair_args(const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, uint32_t K, float depth_tol, uint32_t rec_cap) {
    PairArgs a;
    memset(&a, 0, sizeof a);
    a.width = fmt.width; a.height = fmt.height; a.n = (uint32_t)lay.n; a.depth_pitch = lay.depth_pitch; a.depth_f32 = fmt.depth_type == F3DS_DEPTH_F32 ? 1 : 0;
    a.K = K; a.kb = ct_bits(K); a.rec_cap = rec_cap; a.depth_scale = fmt.depth_scale; a.depth_tol = depth_tol; a.fx = fmt.fx; a.fy = fmt.fy; a.cx = fmt.cx; a.cy = fmt.cy;
    return a;
}
// One frame of a pair call: its scratch, d_pair_init, accum(keys, records) -- the call's own pass over the images --, the runs of equal keys (the radix sort of
// the record keys with the record index as value, d_evl_heads, the scan, d_track_runs), finish(run keys, starts, ends, run count, sorted indices, records) -- the
// call's own kernel that writes the rows.  Everything is ensured before the first of these kernels is recorded.
template <class Accum, class Finish>
int pair_record(f3ds_ctx* c, const PairScratch& s, size_t words, const PairArgs& a, int sort_bits, uint32_t* head, const Accum& accum, const Finish& finish) {
    const uint32_t rec_cap = a.rec_cap;
    uint64_t *k0, *k1, *ukey; uint32_t *v0, *v1, *rec_words, *flag, *ustart, *uend, *cnt, *hist, *tiles;
    ENSURE(s.k0, rec_cap, k0); ENSURE(s.k1, rec_cap, k1); ENSURE(s.v0, rec_cap, v0); ENSURE(s.v1, rec_cap, v1);
    ENSURE(s.rec, (size_t)rec_cap * words, rec_words); ENSURE(s.flag, rec_cap, flag); ENSURE(s.ukey, rec_cap, ukey);
    ENSURE(s.ustart, rec_cap, ustart); ENSURE(s.uend, rec_cap, uend); ENSURE(s.cnt, 4, cnt);
    ENSURE(c->hist, (size_t)RS_BINS * ((rec_cap + RS_TILE - 1) / RS_TILE + 1), hist); ENSURE(c->tiles, (rec_cap + SCAN_TILE - 1) / SCAN_TILE + 1, tiles);
    const uint64_t hole = ct_hole(a.K, a.kb);
    int rc;
    rec<d_pair_init>(c, grid_for(rec_cap, d_pair_init::BLOCK), 0u, k0, v0, rec_cap, head);
    accum(k0, rec_words);
    uint64_t* ks; uint32_t* vs;
    if ((rc = radix_sort(c, k0, v0, k1, v1, rec_cap, sort_bits, &ks, &vs))) return rc;
    rec<d_evl_heads>(c, grid_for(rec_cap, d_evl_heads::BLOCK), 0u, ks, rec_cap, hole, flag);
    if ((rc = scan_u32(c, flag, flag, rec_cap))) return rc;
    rec<d_track_runs>(c, grid_for(rec_cap, d_track_runs::BLOCK), 0u, ks, rec_cap, hole, flag, ukey, ustart, uend, cnt);
    finish(ukey, ustart, uend, cnt, vs, rec_words);
    return F3DS_OK;
}
// A pair call after its checks, with room for first_cap records (at most 2n) per frame: st[i] = frame i's status; the result is a failure of the call as a
// whole.  The call is its row and result types, first_rows (the rows of a host caller that ride with the head), record(context, images, K, rec_cap, sort_bits,
// head, device rows, row cap, device shapes) for one frame, and fill(head, K, result).  shapes: the joints' second output, a fixed payload in front of the rows
// (NULL: none, and always for the contacts).
template <class Row, class Result, class Record, class Fill>
int pair_run(f3ds_ctx** ctxs, int nctx, const f3ds::RgbdLayout& lay, const void* const* depth, const uint32_t* const* labels, const uint32_t* n_regions, int inputs_on_device,
             Row* const* rows, const size_t* caps, f3ds_region_shape* const* shapes, int rows_on_device, size_t* n_out, Result* results, size_t first_rows, uint32_t first_cap, int* st,
             const Record& record, const Fill& fill) {
    Batch b;
    if (const int rc = li_begin(ctxs, nctx, &b)) return rc;
    const uint32_t n = (uint32_t)lay.n;
    const uint32_t rec_all = 2u * n;      // (n < 2^31: rgbd_layout)  every contact pair a record of its own is fewer than this
    const uint32_t rec_cap = first_cap < rec_all ? first_cap : rec_all;
    int sort_bits = 0;
    for (int i = 0; i < nctx; ++i) sort_bits = std::max(sort_bits, ct_sort_bits(n_regions[i]));
    std::vector<size_t> fixed((size_t)nctx, 0u), stage_rows((size_t)nctx, 0u), count((size_t)nctx, 0u);
    std::vector<void*> dst((size_t)nctx, nullptr);
    for (int i = 0; i < nctx; ++i) {
        if (shapes && shapes[i] && !rows_on_device) fixed[i] = (size_t)n_regions[i] * sizeof(f3ds_region_shape);      // (84 B a row: li_stage_layout aligns what follows)
        if (rows && rows[i] && !rows_on_device) stage_rows[i] = caps[i] < rec_cap ? caps[i] : (size_t)rec_cap;      // (rows <= records <= rec_cap)
    }
    LiStage s; std::vector<LiImages> im((size_t)nctx);
    if (const int rc = li_out_buffers(ctxs[0], nctx, fixed.data(), stage_rows.data(), sizeof(Row), first_rows, &s)) return rc;
    if (const int rc = li_upload(ctxs, nctx, b, lay, depth, nullptr, labels, inputs_on_device, im.data())) return rc;
    for (int i = 0; i < nctx; ++i) {
        Row* const r = rows ? rows[i] : nullptr;
        Row* d_rows = !r ? nullptr : (rows_on_device ? r : reinterpret_cast<Row*>(s.out + s.slot[i].rows_at));
        f3ds_region_shape* d_shapes = !shapes || !shapes[i] ? nullptr : li_out_ptr(rows_on_device, shapes[i], s, i);
        if (const int rc = record(ctxs[i], im[i], n_regions[i], rec_cap, sort_bits, s.head(i), d_rows, r ? caps[i] : 0u, d_shapes)) return rc;
    }
    if (const int rc = flush(b)) return rc;
    if (const int rc = li_download_heads(s, b)) return rc;
    std::vector<int> again;
    for (int i = 0; i < nctx; ++i) {
        const uint32_t* h = s.h_head(i);
        st[i] = F3DS_OK;
        if (h[1]) { st[i] = F3DS_ERR_ARG; continue; }      // (a label >= n_regions: no finish kernel wrote a row)
        if (h[2] > rec_cap) {      // (rare: more records than the first buffer holds)
            if (rec_cap >= rec_all) return F3DS_ERR_LOGIC;
            again.push_back(i); continue;
        }
        const size_t cnt = h[0];
        if (cnt > rec_cap) return F3DS_ERR_LOGIC;
        n_out[i] = cnt;
        if (fixed[i]) memcpy(shapes[i], s.o->h_li + s.slot[i].at, fixed[i]);
        if (results) fill(h, n_regions[i], results[i]);
        if (!rows || !rows[i]) continue;
        if (caps[i] < cnt) { st[i] = F3DS_ERR_CAPACITY; continue; }
        if (!rows_on_device) { count[i] = cnt; dst[i] = rows[i]; }
    }
    if (const int rc = li_rows_behind(s, b, nctx, sizeof(Row), count.data(), dst.data())) return rc;
    for (const int i : again) {      // (the owner's staging is free again: everything else has been delivered)
        if (const int rc = pair_run(ctxs + i, 1, lay, depth + i, labels + i, n_regions + i, inputs_on_device, rows ? rows + i : nullptr, caps ? caps + i : nullptr,
                                    shapes ? shapes + i : nullptr, rows_on_device, n_out + i, results ? results + i : nullptr, first_rows, rec_all, &st[i], record, fill)) return rc;
    }
    return F3DS_OK;
}
int ct_record(f3ds_ctx* c, const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, const LiImages& im, uint32_t K, float depth_tol, uint32_t rec_cap, int sort_bits, uint32_t* head,
              f3ds_region_contact* d_rows, size_t cap) {
    const PairArgs a = pair_args(fmt, lay, K, depth_tol, rec_cap);
    const uint32_t n = a.n;
    return pair_record(c, rgc_scratch(c), CT_WORDS, a, sort_bits, head,
        [&](uint64_t* k0, uint32_t* rec_words) { rec<d_contact_accum>(c, grid_for((n + RGC_TRIPS - 1u) / RGC_TRIPS, d_contact_accum::BLOCK), 0u, im.depth, im.labels, a, k0, rec_words, head); },
        [&](uint64_t* ukey, uint32_t* ustart, uint32_t* uend, uint32_t* cnt, uint32_t* vs, uint32_t* rec_words) {
            rec<d_contact_finish>(c, grid_for((size_t)(rec_cap < 8192u ? rec_cap : 8192u) * 64u, d_contact_finish::BLOCK), 0u, ukey, ustart, uend, cnt, vs, rec_words, a.kb, rec_cap, head, d_rows, (uint64_t)cap);
        });
}
}  // namespace

extern "C" int f3ds_region_contacts_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt_, const void* const* depth, const uint32_t* const* labels, const uint32_t* n_regions,
                                          float depth_tol, int inputs_on_device, f3ds_region_contact* const* rows, const size_t* caps, int rows_on_device, size_t* n_out,
                                          f3ds_region_contacts_result* results, int* status) {
    if (!li_batch_ctxs(ctxs, nctx) || !depth || !labels || !n_regions || (rows && !caps)) return F3DS_ERR_ARG;
    f3ds_rgbd_format fmt; f3ds::RgbdLayout lay;
    for (int i = 0; i < nctx; ++i) if (const int rc = ct_check(fmt_, depth[i], labels[i], n_regions[i], depth_tol, n_out, &fmt, &lay)) return rc;
    std::vector<int> st((size_t)nctx, F3DS_OK);
    g_sw.read();
    const uint32_t first = g_sw.rgc_first_cap ? g_sw.rgc_first_cap : RGC_FIRST_CAP;
    const auto record = [&](f3ds_ctx* c, const LiImages& im, uint32_t K, uint32_t rec_cap, int sort_bits, uint32_t* head, f3ds_region_contact* d_rows, size_t cap, f3ds_region_shape*) {
        return ct_record(c, fmt, lay, im, K, depth_tol, rec_cap, sort_bits, head, d_rows, cap);
    };
    const auto fill = [](const uint32_t* h, uint32_t K, f3ds_region_contacts_result& r) { r.n_regions = K; r.n_contacts = h[0]; memcpy(&r.n_pairs, h + 4, 8); memcpy(&r.n_close, h + 6, 8); };
    if (const int rc = pair_run(ctxs, nctx, lay, depth, labels, n_regions, inputs_on_device, rows, caps, nullptr, rows_on_device, n_out, results, RGC_FIRST_ROWS, first, st.data(), record,
                                fill)) return rc;
    return li_statuses(st, status);
}
extern "C" int f3ds_region_contacts(f3ds_ctx* c, const f3ds_rgbd_format* fmt_, const void* depth, const uint32_t* labels, uint32_t n_regions, float depth_tol,
                                    int inputs_on_device, f3ds_region_contact* rows, size_t cap, int rows_on_device, size_t* n_out, f3ds_region_contacts_result* result) {
    return f3ds_region_contacts_batch(&c, 1, fmt_, &depth, &labels, &n_regions, depth_tol, inputs_on_device, rows ? &rows : nullptr, &cap, rows_on_device, n_out, result, nullptr);
}

// ------------------------------------------------------------------------------------------------
// region shapes (f3ds_shapes.h / .inc): one row per region of a label image over a depth image -- covariance, eigenvalues, plane and long
// axis.  The call has the region table's shape: d_shape_init, d_shape_accum (the one read of the image and the labels), d_shape_finish; behind the heads the
// rows of a host caller (84 B per region).  sh_record is also pass one of the boxes and the first step of the joints.
// ------------------------------------------------------------------------------------------------
namespace {
ShapeArgs sh_args(const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, uint32_t K) {
    ShapeArgs a;
    memset(&a, 0, sizeof a);
    a.width = fmt.width; a.n = (uint32_t)lay.n; a.depth_pitch = lay.depth_pitch; a.depth_f32 = fmt.depth_type == F3DS_DEPTH_F32 ? 1 : 0;
    a.K = K; a.copies = rgt_copies(K);
    a.depth_scale = fmt.depth_scale; a.fx = fmt.fx; a.fy = fmt.fy; a.cx = fmt.cx; a.cy = fmt.cy;
    return a;
}
// accs: the accumulators' scratch -- rgs_acc for the shapes and the boxes, the joints' own for the joints
int sh_record(f3ds_ctx* c, const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, const LiImages& im, uint32_t K, uint32_t* head, f3ds_region_shape* d_rows, Scratch<ShAcc>& accs) {
    const ShapeArgs a = sh_args(fmt, lay, K);
    const uint32_t n = a.n;
    ShAcc* acc;
    ENSURE(accs, K ? (size_t)K * a.copies : 1u, acc);
    rec<d_shape_init>(c, grid_for((size_t)K * a.copies * SH_WORDS, d_shape_init::BLOCK), 0u, reinterpret_cast<uint32_t*>(acc), K * a.copies, head);
    rec<d_shape_accum>(c, grid_for((n + LI_TRIPS - 1u) / LI_TRIPS, d_shape_accum::BLOCK), 0u, im.depth, im.labels, a, acc, head);
    rec<d_shape_finish>(c, grid_for(K, d_shape_finish::BLOCK), 0u, acc, K, a.copies, head, d_rows);
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_region_shapes_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt_, const void* const* depth, const uint32_t* const* labels, const uint32_t* n_regions,
                                        int inputs_on_device, f3ds_region_shape* const* rows, int rows_on_device, f3ds_region_shapes_result* results, int* status) {
    if (!li_batch_ctxs(ctxs, nctx) || !depth || !labels || !n_regions || !rows) return F3DS_ERR_ARG;
    f3ds_rgbd_format fmt; f3ds::RgbdLayout lay;
    for (int i = 0; i < nctx; ++i) if (const int rc = sh_check(fmt_, depth[i], labels[i], n_regions[i], rows[i], &fmt, &lay)) return rc;
    Batch b;
    if (const int rc = li_begin(ctxs, nctx, &b)) return rc;
    std::vector<size_t> fixed((size_t)nctx);
    for (int i = 0; i < nctx; ++i) fixed[i] = rows_on_device ? 0u : (size_t)n_regions[i] * sizeof(f3ds_region_shape);
    LiStage s; std::vector<LiImages> im((size_t)nctx);
    if (const int rc = li_out_buffers(ctxs[0], nctx, fixed.data(), nullptr, 0u, 0u, &s)) return rc;
    if (const int rc = li_upload(ctxs, nctx, b, lay, depth, nullptr, labels, inputs_on_device, im.data())) return rc;
    for (int i = 0; i < nctx; ++i) {
        if (const int rc = sh_record(ctxs[i], fmt, lay, im[i], n_regions[i], s.head(i), li_out_ptr(rows_on_device, rows[i], s, i), ctxs[i]->rgs_acc)) return rc;
    }
    return li_deliver_fixed(s, b, nctx, fixed.data(), rows, nullptr, static_cast<void* const*>(nullptr), status, [&](int i, const uint32_t* h) {
        if (!results) return;
        results[i].n_regions = n_regions[i]; results[i].n_nonempty = h[0];
        memcpy(&results[i].n_labelled, h + 2, 8); memcpy(&results[i].n_clamped, h + 4, 8);
    });
}
extern "C" int f3ds_region_shapes(f3ds_ctx* c, const f3ds_rgbd_format* fmt_, const void* depth, const uint32_t* labels, uint32_t n_regions, int inputs_on_device,
                                  f3ds_region_shape* rows, int rows_on_device, f3ds_region_shapes_result* result) {
    return f3ds_region_shapes_batch(&c, 1, fmt_, &depth, &labels, &n_regions, inputs_on_device, &rows, rows_on_device, result, nullptr);
}

// ------------------------------------------------------------------------------------------------
// region boxes (f3ds_boxes.h / .inc): one row per region of a label image over a depth image -- the box along the region's own axes and
// its plane residuals.  The family's first call with TWO reads of the images, the second depending on the finish of the first; both are recorded into the one
// flush: d_shape_init, d_shape_accum, d_shape_finish as they are (sh_record, into rgs_acc, which holds nothing between calls), d_box_frame (a frame per region
// from its shape row), d_box_accum (the second read, every pixel in the frame of its label), d_box_finish.  Behind the heads the box rows of a host caller (96 B
// per region) and behind them the shape rows (84 B) if they were asked for; the shape rows of a caller who wants none stay in scratch.
// ------------------------------------------------------------------------------------------------
namespace {
int bx_record(f3ds_ctx* c, const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, const LiImages& im, uint32_t K, float plane_tol, uint32_t* head, f3ds_region_box* d_rows,
              f3ds_region_shape* d_shapes /* NULL: the context's scratch */) {
    const ShapeArgs a = sh_args(fmt, lay, K);
    const uint32_t n = a.n;
    const uint32_t accum_grid = grid_for((n + LI_TRIPS - 1u) / LI_TRIPS, d_box_accum::BLOCK);      // (pass one, sh_record, asks for the same)
    BxAcc* acc2; BxFrame* frames; uint32_t* head2;
    ENSURE(c->rgx_acc, K ? (size_t)K * a.copies : 1u, acc2);
    ENSURE(c->rgx_frame, K ? K : 1u, frames);
    ENSURE(c->rgx_head, LI_HEAD_WORDS, head2);
    if (!d_shapes) ENSURE(c->rgx_shape, K ? K : 1u, d_shapes);
    if (const int rc = sh_record(c, fmt, lay, im, K, head, d_shapes, c->rgs_acc)) return rc;      // (rgs_acc is ensured before its first rec<>, and nothing recorded refers to it yet)
    rec<d_box_frame>(c, grid_for(K, d_box_frame::BLOCK), 0u, d_shapes, K, a.copies, plane_tol, head, frames, acc2, head2);
    rec<d_box_accum>(c, accum_grid, 0u, im.depth, im.labels, a, frames, acc2, head, head2);
    rec<d_box_finish>(c, grid_for(K, d_box_finish::BLOCK), 0u, acc2, frames, K, a.copies, head, d_rows);
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_region_boxes_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt_, const void* const* depth, const uint32_t* const* labels, const uint32_t* n_regions,
                                       float plane_tol, int inputs_on_device, f3ds_region_box* const* rows, f3ds_region_shape* const* shapes, int rows_on_device,
                                       f3ds_region_boxes_result* results, int* status) {
    if (!li_batch_ctxs(ctxs, nctx) || !depth || !labels || !n_regions || !rows) return F3DS_ERR_ARG;
    f3ds_rgbd_format fmt; f3ds::RgbdLayout lay;
    for (int i = 0; i < nctx; ++i) {
        if (shapes && !shapes[i] && n_regions[i]) return F3DS_ERR_ARG;      // (shape rows for every frame or for none)
        if (const int rc = bx_check(fmt_, depth[i], labels[i], n_regions[i], plane_tol, rows[i], &fmt, &lay)) return rc;
    }
    Batch b;
    if (const int rc = li_begin(ctxs, nctx, &b)) return rc;
    std::vector<size_t> fixed((size_t)nctx), box_bytes((size_t)nctx), shape_bytes((size_t)nctx);
    for (int i = 0; i < nctx; ++i) {
        box_bytes[i] = rows_on_device ? 0u : (size_t)n_regions[i] * sizeof(f3ds_region_box);      // (a multiple of 8: the shape rows behind them are aligned)
        shape_bytes[i] = rows_on_device || !shapes || !shapes[i] ? 0u : (size_t)n_regions[i] * sizeof(f3ds_region_shape);
        fixed[i] = box_bytes[i] + shape_bytes[i];
    }
    LiStage s; std::vector<LiImages> im((size_t)nctx);
    if (const int rc = li_out_buffers(ctxs[0], nctx, fixed.data(), nullptr, 0u, 0u, &s)) return rc;
    if (const int rc = li_upload(ctxs, nctx, b, lay, depth, nullptr, labels, inputs_on_device, im.data())) return rc;
    for (int i = 0; i < nctx; ++i) {
        f3ds_region_shape* d_shapes = !shapes || !shapes[i] ? nullptr : li_out_ptr(rows_on_device, shapes[i], s, i, box_bytes[i]);
        if (const int rc = bx_record(ctxs[i], fmt, lay, im[i], n_regions[i], plane_tol, s.head(i), li_out_ptr(rows_on_device, rows[i], s, i), d_shapes)) return rc;
    }
    return li_deliver_fixed(s, b, nctx, box_bytes.data(), rows, shape_bytes.data(), shapes, status, [&](int i, const uint32_t* h) {
        if (!results) return;
        results[i].n_regions = n_regions[i]; results[i].n_nonempty = h[0];
        memcpy(&results[i].n_labelled, h + 2, 8); memcpy(&results[i].n_clamped, h + 4, 8); memcpy(&results[i].n_inliers, h + 6, 8);
    });
}
extern "C" int f3ds_region_boxes(f3ds_ctx* c, const f3ds_rgbd_format* fmt_, const void* depth, const uint32_t* labels, uint32_t n_regions, float plane_tol, int inputs_on_device,
                                 f3ds_region_box* rows, f3ds_region_shape* shapes, int rows_on_device, f3ds_region_boxes_result* result) {
    return f3ds_region_boxes_batch(&c, 1, fmt_, &depth, &labels, &n_regions, plane_tol, inputs_on_device, &rows, shapes ? &shapes : nullptr, rows_on_device, result, nullptr);
}

// ------------------------------------------------------------------------------------------------
// region joints (f3ds_joints.h / .inc): one row per pair of regions of a label image that touch -- the border in space and the join of the
// two regions' shape rows.  One flush: the three kernels of the shapes as they are (sh_record, into the joints' own accumulators and a head of their own: the
// call's head is the contacts'), d_pair_init, d_joint_accum (the pass over the borders: records of (pair, 34 words)), the radix sort of the record keys,
// d_evl_heads / scan, d_track_runs, d_joint_finish.  Behind the head the shape rows of a host caller who asked for them (84 B per region), then the first
// RGJ_FIRST_ROWS rows.  Records that do not fit, long row arrays and the frames of a batch: as the contacts (pair_run).  Beside rgj_* the call uses the sort's
// histogram and the scan's tile sums, which hold nothing between calls.
// ------------------------------------------------------------------------------------------------
namespace {
int jt_record(f3ds_ctx* c, const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, const LiImages& im, uint32_t K, const f3ds_joint_params& prm, uint32_t rec_cap, int sort_bits,
              uint32_t* head, f3ds_region_joint* d_rows, size_t cap, f3ds_region_shape* d_shapes /* NULL: the context's scratch */) {
    const PairArgs a = pair_args(fmt, lay, K, prm.depth_tol, rec_cap);
    const uint32_t n = a.n;
    uint32_t* shead;
    ENSURE(c->rgj_shead, LI_HEAD_WORDS, shead);
    if (!d_shapes) ENSURE(c->rgj_shape, K ? K : 1u, d_shapes);
    // (the scratch of the pair kernels is ensured behind the shapes' kernels: none of them refers to it, nor to the sort's histogram or the scan's tile sums)
    if (const int rc = sh_record(c, fmt, lay, im, K, shead, d_shapes, c->rgj_sacc)) return rc;      // (rgj_sacc is ensured before its first rec<>, and nothing recorded refers to it yet)
    return pair_record(c, rgj_scratch(c), JT_WORDS, a, sort_bits, head,
        [&](uint64_t* k0, uint32_t* rec_words) { rec<d_joint_accum>(c, grid_for((n + RGJ_TRIPS - 1u) / RGJ_TRIPS, RGJ_BLOCK), 0u, im.depth, im.labels, a, k0, rec_words, head); },
        [&](uint64_t* ukey, uint32_t* ustart, uint32_t* uend, uint32_t* cnt, uint32_t* vs, uint32_t* rec_words) {
            rec<d_joint_finish>(c, grid_for((size_t)(rec_cap < 8192u ? rec_cap : 8192u) * 64u, d_joint_finish::BLOCK), 0u, ukey, ustart, uend, cnt, vs, rec_words, d_shapes, prm, a.kb, rec_cap, head, d_rows,
                                (uint64_t)cap);
        });
}
}  // namespace

extern "C" int f3ds_region_joints_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt_, const void* const* depth, const uint32_t* const* labels, const uint32_t* n_regions,
                                        const f3ds_joint_params* params, int inputs_on_device, f3ds_region_joint* const* rows, const size_t* caps, f3ds_region_shape* const* shapes,
                                        int rows_on_device, size_t* n_out, f3ds_region_joints_result* results, int* status) {
    if (!li_batch_ctxs(ctxs, nctx) || !depth || !labels || !n_regions || (rows && !caps)) return F3DS_ERR_ARG;
    f3ds_rgbd_format fmt; f3ds::RgbdLayout lay; f3ds_joint_params prm;
    for (int i = 0; i < nctx; ++i) {
        if (shapes && !shapes[i] && n_regions[i]) return F3DS_ERR_ARG;      // (shape rows for every frame or for none)
        if (const int rc = jt_check(fmt_, depth[i], labels[i], n_regions[i], params, n_out, &fmt, &lay, &prm)) return rc;
    }
    std::vector<int> st((size_t)nctx, F3DS_OK);
    g_sw.read();
    const uint32_t first = g_sw.rgj_first_cap ? g_sw.rgj_first_cap : RGJ_FIRST_CAP;
    const auto record = [&](f3ds_ctx* c, const LiImages& im, uint32_t K, uint32_t rec_cap, int sort_bits, uint32_t* head, f3ds_region_joint* d_rows, size_t cap, f3ds_region_shape* d_shapes) {
        return jt_record(c, fmt, lay, im, K, prm, rec_cap, sort_bits, head, d_rows, cap, d_shapes);
    };
    const auto fill = [](const uint32_t* h, uint32_t K, f3ds_region_joints_result& r) {
        r.n_regions = K; r.n_joints = h[0]; r.n_surface = h[3]; r.reserved = 0u;
        memcpy(&r.n_pairs, h + 4, 8); memcpy(&r.n_close, h + 6, 8);
    };
    if (const int rc = pair_run(ctxs, nctx, lay, depth, labels, n_regions, inputs_on_device, rows, caps, shapes, rows_on_device, n_out, results, RGJ_FIRST_ROWS, first, st.data(), record,
                                fill)) return rc;
    return li_statuses(st, status);
}
extern "C" int f3ds_region_joints(f3ds_ctx* c, const f3ds_rgbd_format* fmt_, const void* depth, const uint32_t* labels, uint32_t n_regions, const f3ds_joint_params* params,
                                  int inputs_on_device, f3ds_region_joint* rows, size_t cap, f3ds_region_shape* shapes, int rows_on_device, size_t* n_out,
                                  f3ds_region_joints_result* result) {
    return f3ds_region_joints_batch(&c, 1, fmt_, &depth, &labels, &n_regions, params, inputs_on_device, rows ? &rows : nullptr, &cap, shapes ? &shapes : nullptr, rows_on_device, n_out,
                                    result, nullptr);
}

// ------------------------------------------------------------------------------------------------
// region components (f3ds_components.h / .inc): the connected components of a label image over a depth image, as a label image and one
// row per component.  The head's zeros, d_comp_local (the one read of the images: tiles resolved in LDS), d_comp_seam, d_comp_flatten, d_comp_flag, the scan
// of the flags, d_comp_write; behind the heads the image and the first RGK_FIRST_ROWS rows of a host caller, who gets further rows in a second download.
// Beside rgk_* (twelve bytes per pixel) the call uses the scan's tile sums, which hold nothing between calls.
// ------------------------------------------------------------------------------------------------
namespace {
int cc_record(f3ds_ctx* c, const f3ds_rgbd_format& fmt, const f3ds::RgbdLayout& lay, const f3ds_component_params& prm, const LiImages& im, uint32_t K, uint32_t* head, uint32_t* d_comp,
              f3ds_region_component* d_rows, size_t cap) {
    const uint32_t n = (uint32_t)lay.n;
    uint32_t *parent, *cnt, *flag;
    ENSURE(c->rgk_parent, n, parent); ENSURE(c->rgk_cnt, n, cnt); ENSURE(c->rgk_flag, n, flag);
    CompArgs a;
    memset(&a, 0, sizeof a);
    a.width = fmt.width; a.height = fmt.height; a.n = n; a.depth_pitch = lay.depth_pitch; a.depth_f32 = fmt.depth_type == F3DS_DEPTH_F32 ? 1 : 0;
    a.K = K; a.min_pixels = prm.min_pixels; a.tiles_x = (fmt.width + CC_TILE_W - 1u) / CC_TILE_W; a.tiles_y = (fmt.height + CC_TILE_H - 1u) / CC_TILE_H;
    a.depth_scale = fmt.depth_scale; a.depth_tol = prm.depth_tol;
    const size_t seams = (size_t)(a.tiles_x - 1u) * fmt.height + (size_t)(a.tiles_y - 1u) * fmt.width;
    rec_fill(c, head, 0u, LI_HEAD_BYTES);
    rec<d_comp_local>(c, grid_for((size_t)a.tiles_x * a.tiles_y, CC_TILES_PER_WG), 0u, im.depth, im.labels, a, parent, cnt, head);
    rec<d_comp_seam>(c, grid_for(seams, d_comp_seam::BLOCK), 0u, im.depth, im.labels, a, parent);
    rec<d_comp_flatten>(c, grid_for(n, d_comp_flatten::BLOCK), 0u, n, parent, cnt);
    rec<d_comp_flag>(c, grid_for(n, d_comp_flag::BLOCK), 0u, n, parent, cnt, a.min_pixels, flag, head);
    if (const int rc = scan_u32(c, flag, flag, n)) return rc;
    rec<d_comp_write>(c, grid_for(n, d_comp_write::BLOCK), 0u, n, im.labels, parent, cnt, flag, a.min_pixels, head, d_comp, d_rows, (uint64_t)cap);
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_region_components_batch(f3ds_ctx** ctxs, int nctx, const f3ds_rgbd_format* fmt_, const void* const* depth, const uint32_t* const* labels, const uint32_t* n_regions,
                                            const f3ds_component_params* params, int inputs_on_device, uint32_t* const* comp_labels, f3ds_region_component* const* rows,
                                            const size_t* caps, int outputs_on_device, size_t* n_out, f3ds_region_components_result* results, int* status) {
    if (!li_batch_ctxs(ctxs, nctx) || !depth || !labels || !n_regions || !comp_labels || (rows && !caps)) return F3DS_ERR_ARG;
    f3ds_rgbd_format fmt; f3ds::RgbdLayout lay; f3ds_component_params prm;
    for (int i = 0; i < nctx; ++i) if (const int rc = cc_check(fmt_, depth[i], labels[i], n_regions[i], params, comp_labels[i], n_out, &fmt, &lay, &prm)) return rc;
    Batch b;
    if (const int rc = li_begin(ctxs, nctx, &b)) return rc;
    const uint32_t n = (uint32_t)lay.n;
    const bool host_out = !outputs_on_device;
    const size_t image_bytes = host_out ? (size_t)n * 4 : 0u;
    std::vector<size_t> fixed((size_t)nctx, image_bytes), stage_rows((size_t)nctx, 0u), count((size_t)nctx, 0u);
    std::vector<void*> dst((size_t)nctx, nullptr);
    for (int i = 0; i < nctx; ++i) if (rows && rows[i] && host_out) stage_rows[i] = caps[i] < n ? caps[i] : (size_t)n;      // (components <= pixels)
    LiStage s; std::vector<LiImages> im((size_t)nctx);
    if (const int rc = li_out_buffers(ctxs[0], nctx, fixed.data(), stage_rows.data(), sizeof(f3ds_region_component), RGK_FIRST_ROWS, &s)) return rc;
    if (const int rc = li_upload(ctxs, nctx, b, lay, depth, nullptr, labels, inputs_on_device, im.data())) return rc;
    for (int i = 0; i < nctx; ++i) {
        f3ds_region_component* const r = rows ? rows[i] : nullptr;
        uint32_t* d_comp = li_out_ptr(outputs_on_device, comp_labels[i], s, i);
        f3ds_region_component* d_rows = !r ? nullptr : (host_out ? reinterpret_cast<f3ds_region_component*>(s.out + s.slot[i].rows_at) : r);
        if (const int rc = cc_record(ctxs[i], fmt, lay, prm, im[i], n_regions[i], s.head(i), d_comp, d_rows, r ? caps[i] : 0u)) return rc;
    }
    if (const int rc = flush(b)) return rc;
    if (const int rc = li_download_heads(s, b)) return rc;
    std::vector<int> st((size_t)nctx, F3DS_OK);
    for (int i = 0; i < nctx; ++i) {
        const uint32_t* h = s.h_head(i);
        if (h[1]) { st[i] = F3DS_ERR_ARG; continue; }      // (a label >= n_regions: d_comp_write wrote nothing)
        const size_t cnt = h[0];
        if (cnt > n) return F3DS_ERR_LOGIC;
        if (host_out) memcpy(comp_labels[i], s.o->h_li + s.slot[i].at, image_bytes);
        n_out[i] = cnt;
        if (results) {
            results[i].n_regions = n_regions[i]; results[i].n_components = h[0]; results[i].n_dropped = h[2]; results[i].reserved = 0u;
            memcpy(&results[i].n_labelled, h + 4, 8); memcpy(&results[i].n_kept, h + 6, 8);
        }
        if (!rows || !rows[i]) continue;
        if (caps[i] < cnt) { st[i] = F3DS_ERR_CAPACITY; continue; }
        if (host_out) { count[i] = cnt; dst[i] = rows[i]; }
    }
    if (const int rc = li_rows_behind(s, b, nctx, sizeof(f3ds_region_component), count.data(), dst.data())) return rc;
    return li_statuses(st, status);
}
extern "C" int f3ds_region_components(f3ds_ctx* c, const f3ds_rgbd_format* fmt_, const void* depth, const uint32_t* labels, uint32_t n_regions, const f3ds_component_params* params,
                                      int inputs_on_device, uint32_t* comp_labels, f3ds_region_component* rows, size_t cap, int outputs_on_device, size_t* n_out,
                                      f3ds_region_components_result* result) {
    return f3ds_region_components_batch(&c, 1, fmt_, &depth, &labels, &n_regions, params, inputs_on_device, &comp_labels, rows ? &rows : nullptr, &cap, outputs_on_device, n_out, result,
                                        nullptr);
}

// ------------------------------------------------------------------------------------------------
// region rows of a point cloud (f3ds_cloud.h / .inc): one row per region of n labelled records, and optionally the region boxes.  The
// call has the shape of the family's batch forms -- checks, staging, uploads, one record per frame, one flush, one download, one wait -- over points, not
// images: every frame has its own n.  What every frame of a batch must agree on is decided for the batch: the walk (ordered if any frame's K asks for it, or
// what F3DS_CLOUD_PATH says), the key layout (index bits of the longest frame, label bits of the largest K: the same sort passes for all) and whether there
// are boxes.  Kernels: d_cloud_init, [d_cloud_keys, the stage-0 radix sort on the label bits,] d_cloud_accum, d_cloud_finish, [d_box_frame, d_cloud_box_accum,
// d_box_finish].  Behind the heads the rows of a host caller (128 B per region) and behind them its boxes (96 B).  Beside rgp_* the call uses the sort's
// histogram, which holds nothing between calls, and li_lab for a host caller's labels.
// ------------------------------------------------------------------------------------------------
namespace {
int cd_record(f3ds_ctx* c, const P16* pts, const uint32_t* labels, uint32_t n, uint32_t K, const f3ds_cloud_params& prm, bool ordered, uint32_t idx_bits, int label_bits, uint32_t* head,
              f3ds_cloud_region* d_rows, f3ds_region_box* d_boxes /* NULL: none */) {
    CloudArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.K = K; a.copies = rgt_copies(K); a.idx_bits = idx_bits; a.fold_negative_z = prm.fold_negative_z; a.ordered = ordered ? 1 : 0;
    static_assert(d_cloud_accum::BLOCK == d_cloud_box_accum::BLOCK, "one grid for both walks");
    const uint32_t walk_grid = grid_for(((size_t)n + LI_TRIPS - 1u) / LI_TRIPS, d_cloud_accum::BLOCK);      // (both walks, both passes: LI_TRIPS trips a workgroup, as the image family)
    CdAcc* acc; uint64_t *k0 = nullptr, *k1 = nullptr, *ks = nullptr;
    f3ds_region_shape* shapes = nullptr; BxFrame* frames = nullptr; BxAcc* acc2 = nullptr; uint32_t* head2 = nullptr;
    ENSURE(c->rgp_acc, K ? (size_t)K * a.copies : 1u, acc);
    if (ordered) { ENSURE(c->rgp_k0, n ? n : 1u, k0); ENSURE(c->rgp_k1, n ? n : 1u, k1); }
    if (d_boxes) {
        ENSURE(c->rgp_shape, K ? K : 1u, shapes); ENSURE(c->rgp_frame, K ? K : 1u, frames);
        ENSURE(c->rgp_bacc, K ? (size_t)K * a.copies : 1u, acc2); ENSURE(c->rgp_head, LI_HEAD_WORDS, head2);
    }
    rec<d_cloud_init>(c, grid_for((size_t)K * a.copies * CD_WORDS, d_cloud_init::BLOCK), 0u, reinterpret_cast<uint32_t*>(acc), K * a.copies, head);
    if (ordered) {
        rec<d_cloud_keys>(c, grid_for(n, d_cloud_keys::BLOCK), 0u, labels, a, k0, head);
        if (const int rc = radix_sort(c, k0, nullptr, k1, nullptr, n, label_bits, &ks, nullptr, (int)idx_bits)) return rc;
    }
    rec<d_cloud_accum>(c, walk_grid, 0u, pts, labels, ks, a, acc, head);
    rec<d_cloud_finish>(c, grid_for(K, d_cloud_finish::BLOCK), 0u, acc, K, a.copies, head, d_rows, shapes);
    if (d_boxes) {
        rec<d_box_frame>(c, grid_for(K, d_box_frame::BLOCK), 0u, shapes, K, a.copies, prm.plane_tol, head, frames, acc2, head2);
        rec<d_cloud_box_accum>(c, walk_grid, 0u, pts, labels, ks, a, frames, acc2, head, head2);
        rec<d_box_finish>(c, grid_for(K, d_box_finish::BLOCK), 0u, acc2, frames, K, a.copies, head, d_boxes);
    }
    c->cloud_path = ordered ? CD_PATH_ORDERED : CD_PATH_DIRECT;
    return F3DS_OK;
}
}  // namespace

extern "C" int f3ds_cloud_regions_batch(f3ds_ctx** ctxs, int nctx, const void* const* points, const size_t* counts, const uint32_t* const* labels, const uint32_t* n_regions,
                                        const f3ds_cloud_params* params, int inputs_on_device, f3ds_cloud_region* const* rows, f3ds_region_box* const* boxes, int rows_on_device,
                                        f3ds_cloud_regions_result* results, int* status) {
    if (!li_batch_ctxs(ctxs, nctx) || !points || !counts || !labels || !n_regions || !rows) return F3DS_ERR_ARG;
    f3ds_cloud_params prm;
    for (int i = 0; i < nctx; ++i) {
        if (boxes && !boxes[i] && n_regions[i]) return F3DS_ERR_ARG;      // (boxes for every frame or for none)
        if (const int rc = cd_check(points[i], counts[i], labels[i], n_regions[i], params, rows[i], true, &prm)) return rc;
    }
    for (int i = 0; i < nctx; ++i) {      // the context's own records, by the rule of f3ds_get_points
        if (points[i]) continue;
        if (!ctxs[i]->d_pts || ctxs[i]->d_pts != ctxs[i]->pts.p) return F3DS_ERR_LOGIC;
        if (counts[i] != ctxs[i]->n) return F3DS_ERR_ARG;
    }
    Batch b;
    if (const int rc = li_begin(ctxs, nctx, &b)) return rc;
    // the batch-wide decisions
    uint32_t maxn = 1, maxk = 0;
    bool ordered = false;
    for (int i = 0; i < nctx; ++i) {
        maxn = std::max(maxn, (uint32_t)counts[i]); maxk = std::max(maxk, n_regions[i]);
        ordered = ordered || cd_choose_path(n_regions[i]) == CD_PATH_ORDERED;
    }
    if (g_sw.cloud_path) ordered = g_sw.cloud_path == CD_PATH_ORDERED;
    const uint32_t idx_bits = (uint32_t)bits_for((uint64_t)maxn - 1u);
    const int label_bits = bits_for(maxk);      // (the key of a point without a label carries K itself)
    std::vector<size_t> fixed((size_t)nctx), row_bytes((size_t)nctx), box_bytes((size_t)nctx);
    for (int i = 0; i < nctx; ++i) {
        row_bytes[i] = rows_on_device ? 0u : (size_t)n_regions[i] * sizeof(f3ds_cloud_region);      // (a multiple of 8: the boxes behind them are aligned)
        box_bytes[i] = rows_on_device || !boxes ? 0u : (size_t)n_regions[i] * sizeof(f3ds_region_box);
        fixed[i] = row_bytes[i] + box_bytes[i];
    }
    LiStage s;
    if (const int rc = li_out_buffers(ctxs[0], nctx, fixed.data(), nullptr, 0u, 0u, &s)) return rc;
    // the inputs as the kernels read them: host records and labels go up through the device's copy stream, all frames' copies awaited once
    std::vector<const P16*> d_pts((size_t)nctx); std::vector<const uint32_t*> d_lab((size_t)nctx);
    hipStream_t up = (!inputs_on_device && g_sw.copy_stream) ? copy_stream_of(b.owner->device) : nullptr;
    for (int i = 0; i < nctx; ++i) {
        f3ds_ctx* c = ctxs[i];
        const size_t n = counts[i];
        d_pts[i] = points[i] ? static_cast<const P16*>(points[i]) : c->d_pts;
        d_lab[i] = labels[i];
        if (inputs_on_device) continue;
        uint32_t* ul;
        ENSURE(c->li_lab, n ? n : 1u, ul);
        if (n) HIPCHECK(hipMemcpyAsync(ul, labels[i], n * 4, hipMemcpyHostToDevice, up ? up : b.st));
        d_lab[i] = ul;
        if (points[i]) {
            P16* upts;
            ENSURE(c->rgp_pts, n ? n : 1u, upts);
            if (n) HIPCHECK(hipMemcpyAsync(upts, points[i], n * 16, hipMemcpyHostToDevice, up ? up : b.st));
            d_pts[i] = upts;
        }
    }
    if (up) { if (const int urc = await_uploads(b, up)) return urc; }
    for (int i = 0; i < nctx; ++i) {
        // (boxes for every frame: a frame without regions may come without an array and then has nothing to write, wherever its pointer goes)
        f3ds_region_box* d_boxes = !boxes ? nullptr : li_out_ptr(rows_on_device && boxes[i], boxes[i], s, i, row_bytes[i]);
        if (const int rc = cd_record(ctxs[i], d_pts[i], d_lab[i], (uint32_t)counts[i], n_regions[i], prm, ordered, idx_bits, label_bits, s.head(i),
                                     li_out_ptr(rows_on_device, rows[i], s, i), d_boxes)) return rc;
    }
    return li_deliver_fixed(s, b, nctx, row_bytes.data(), rows, box_bytes.data(), boxes, status, [&](int i, const uint32_t* h) {
        if (!results) return;
        results[i].n_regions = n_regions[i]; results[i].n_nonempty = h[0];
        memcpy(&results[i].n_labelled, h + 2, 8); memcpy(&results[i].n_clamped, h + 4, 8); memcpy(&results[i].n_inliers, h + 6, 8);
    });
}
extern "C" int f3ds_cloud_regions(f3ds_ctx* c, const void* points16, size_t n, const uint32_t* labels, uint32_t n_regions, const f3ds_cloud_params* params, int inputs_on_device,
                                  f3ds_cloud_region* rows, f3ds_region_box* boxes, int rows_on_device, f3ds_cloud_regions_result* result) {
    return f3ds_cloud_regions_batch(&c, 1, &points16, &n, &labels, &n_regions, params, inputs_on_device, &rows, boxes ? &boxes : nullptr, rows_on_device, result, nullptr);
}

// ---- The limits by name: every number a test is sized by, from the constant the code itself uses (kernel limits: f3ds_kernels.inc, f3ds_algo.h and the region
// includes; host policy: f3ds_batch_policy.h; a kernel's workgroup size under "<kernel>::BLOCK").  Host arithmetic only, no HIP call.  X(name, value), B(kernel).
#define F3DS_CONSTANTS(X, B) \
    X(NT_TILE, NT_TILE) X(NT_RING1, NT_RING1) X(NT_SLOTS, NT_SLOTS) X(VL_MAX_RUN, VL_MAX_RUN) X(VT_TILE, VT_TILE) X(VT_TAB, VT_TAB) X(VT_ENT_MAX, VT_ENT_MAX) \
    X(VT_CNT_BITS, VT_CNT_BITS) X(VG_CHUNK, VG_CHUNK) X(RL_LDS_CAP, RL_LDS_CAP) X(HT_CAP, HT_CAP) X(HT_ROW, HT_ROW) X(QL, QL) X(BY_WAVE_RATIO, BY_WAVE_RATIO) \
    X(SW_TILE_NONE, SW_TILE_NONE) X(N_BLOCK_DEPTH_MAX, N_BLOCK_DEPTH_MAX) X(R_STACK, F3DS_R_STACK) X(R_ROUNDS, F3DS_R_ROUNDS) X(TAG_PERIOD, A_TAG_PERIOD) \
    X(MAX_SEED_EVENTS, F3DS_MAX_SEED_EVENTS) X(SEED_CHUNK, SEED_CHUNK) X(SEED_CELLS_PER_WG, SEED_CELLS_PER_WG) X(SEED_CAND_STRIDE, SEED_CAND_STRIDE) \
    X(SEED_NN_MARGIN, double_bits(SEED_NN_MARGIN)) X(SEED_NN_ULP, double_bits(SEED_NN_ULP)) X(SEED_PRUNE_MARGIN, double_bits(SEED_PRUNE_MARGIN)) \
    X(MC_TL_CAP, MC_TL_CAP) X(MC_SP_TL, MC_SP_TL) X(MC_SP_LEAVES, MC_SP_LEAVES) X(MC_GROUP, MC_GROUP) X(MC_LDS_LIMIT, MC_LDS_LIMIT) X(MC_LDS_STATIC, MC_LDS_STATIC) \
    X(MC_CH_ROWS4, MC_CH_ROWS4) X(MC_CH_ROWS8, MC_CH_ROWS8) X(MC_SP_ROWS_MIN, MC_SP_ROWS_MIN) X(MC_SP_ROWS8, F3DS_SP_ROWS8) X(MC_SP_REST_TRIES, MC_SP_REST_TRIES) \
    X(MC_SP_REST_DIV, F3DS_SP_REST_DIV) X(MC_SP_REST_EPOCHS, MC_SP_REST_EPOCHS) \
    X(LI_SLOTS, LI_SLOTS) X(LI_PROBES, LI_PROBES) X(LI_TRIPS, LI_TRIPS) X(RGT_MAX_COPIES, RGT_MAX_COPIES) X(RGT_COPY_BUDGET, RGT_COPY_BUDGET) X(RGC_SLOTS, RGC_SLOTS) \
    X(RGC_TRIPS, RGC_TRIPS) X(CC_TILE_W, CC_TILE_W) X(CC_TILE_H, CC_TILE_H) X(CC_TILES_PER_WG, CC_TILES_PER_WG) \
    X(OVF_EVENTS, F3DS_OVF_EVENTS) X(OVF_LEAF_POOL, F3DS_OVF_LEAF_POOL) X(OVF_EDGE_LIST, F3DS_OVF_EDGE_LIST) X(OVF_ILIST_POOL, F3DS_OVF_ILIST_POOL) \
    X(OVF_DENSE_VOXEL, F3DS_OVF_DENSE_VOXEL) X(OVF_TILE_VOXELS, F3DS_OVF_TILE_VOXELS) \
    X(KEY_BITS, f3ds_policy::KEY_BITS) X(TILE_MIN_CONTEXTS, f3ds_policy::TILE_MIN_CONTEXTS) X(EV_MULT, f3ds_policy::EV_MULT) X(EV_EXTRA, f3ds_policy::EV_EXTRA) \
    X(EDGE_MULT, f3ds_policy::EDGE_MULT) X(EDGE_EXTRA, f3ds_policy::EDGE_EXTRA) X(GROW, f3ds_policy::GROW) X(EV_MULT_CAP, f3ds_policy::EV_MULT_CAP) \
    X(POOL_MULT_CAP, f3ds_policy::POOL_MULT_CAP) X(ILIST_MULT_CAP, f3ds_policy::ILIST_MULT_CAP) X(EDGE_MULT_CAP, f3ds_policy::EDGE_MULT_CAP) \
    X(ILIST_SLACK, f3ds_policy::ILIST_SLACK) X(ILIST_EXTRA_SHORT, f3ds_policy::ILIST_EXTRA_SHORT) X(ILIST_EXTRA, f3ds_policy::ILIST_EXTRA) \
    X(DENSE_PENALTY, f3ds_policy::DENSE_PENALTY) X(DENSE_PENALTY_STEP, f3ds_policy::DENSE_PENALTY_STEP) X(DENSE_PENALTY_CAP, f3ds_policy::DENSE_PENALTY_CAP) \
    X(NORMALS_256_FRAMES, f3ds_policy::NORMALS_256_FRAMES) X(GRID_TARGET, f3ds_policy::GRID_TARGET) X(GRID_MIN, f3ds_policy::GRID_MIN) X(WIDE_CAP, f3ds_policy::WIDE_CAP) \
    B(d_seed_grow) B(d_seed_nn) B(d_seed_filter) B(d_reseed) B(d_region_accum) B(d_shape_accum) B(d_box_accum) B(d_contact_accum) B(d_comp_local) B(d_comp_seam) B(d_track_keys)
namespace {
uint64_t double_bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
struct NamedConstant { const char* name; uint64_t value; };
const NamedConstant* constant_table(size_t* count) {
#define F3DS_X(name, value) {#name, (uint64_t)(value)},
#define F3DS_B(kernel) {#kernel "::BLOCK", (uint64_t)kernel::BLOCK},
    static const NamedConstant table[] = {F3DS_CONSTANTS(F3DS_X, F3DS_B)};
#undef F3DS_X
#undef F3DS_B
    *count = sizeof table / sizeof table[0];
    return table;
}
}  // namespace
extern "C" int f3ds_constant(const char* name, uint64_t* value) {
    size_t n; const NamedConstant* t = constant_table(&n);
    if (!name || !value) return F3DS_ERR_ARG;
    for (size_t i = 0; i < n; ++i) if (!strcmp(t[i].name, name)) { *value = t[i].value; return F3DS_OK; }
    return F3DS_ERR_ARG;
}
extern "C" const char* f3ds_constant_name(size_t index) {
    size_t n; const NamedConstant* t = constant_table(&n);
    return index < n ? t[index].name : nullptr;
}
extern "C" int f3ds_stage0_plan(int max_depth, uint32_t max_points, int n_contexts, int vox_tiles, int sort_pairs, int32_t out[4]) {
    if (!out || max_depth < 0 || max_depth > 21 || n_contexts < 1 || vox_tiles < 0 || vox_tiles > 2) return F3DS_ERR_ARG;
    const bool wanted = f3ds_policy::tile_path_wanted(n_contexts, vox_tiles != 0 && !sort_pairs, vox_tiles == 2);      // (Switches::read: F3DS_SORT_PAIRS implies the sort path)
    const f3ds_policy::Stage0Plan p = f3ds_policy::stage0_plan(max_depth, max_points, wanted, sort_pairs != 0, VT_LIMITS);
    out[0] = p.tiles ? 1 : 0; out[1] = p.tile_bits; out[2] = p.idxbits; out[3] = p.sort_bits;
    return F3DS_OK;
}
extern "C" int f3ds_policy_capacity(int what, uint32_t count, uint32_t n_seeds, uint32_t mult, uint32_t slack, uint32_t* out) {
    if (!out) return F3DS_ERR_ARG;
    switch (what) {
        case F3DS_CAP_EDGES: *out = f3ds_policy::edge_capacity(count, mult); return F3DS_OK;
        case F3DS_CAP_EVENTS: *out = f3ds_policy::event_capacity(count, mult); return F3DS_OK;
        case F3DS_CAP_LEAF_POOL: *out = f3ds_policy::leaf_pool_capacity(count, mult); return F3DS_OK;
        case F3DS_CAP_ILIST: *out = f3ds_policy::ilist_capacity(count, n_seeds, slack, mult, MC_TL_CAP); return F3DS_OK;
    }
    return F3DS_ERR_ARG;
}
extern "C" int f3ds_policy_grow(uint32_t mult, uint32_t cap, uint32_t* out) {
    if (!out) return F3DS_ERR_ARG;
    f3ds_policy::grow(&mult, cap);
    *out = mult;
    return F3DS_OK;
}
extern "C" int f3ds_policy_launch(int frames, int normals_forced, uint32_t grid_target, uint32_t grid_cap_forced, uint32_t out[3]) {
    if (!out) return F3DS_ERR_ARG;
    out[0] = (uint32_t)f3ds_policy::normals_threads(frames, normals_forced);
    out[1] = (uint32_t)f3ds_policy::grid_cap_for_batch(frames, grid_target, grid_cap_forced);
    out[2] = (uint32_t)f3ds_policy::wide_cap(grid_cap_forced);
    return F3DS_OK;
}
extern "C" uint32_t f3ds_policy_dense_penalty(uint32_t penalty) { return f3ds_policy::next_dense_penalty(penalty); }
extern "C" int f3ds_policy_stage_layout(size_t n_frames, const size_t* fixed_bytes, const size_t* stage_rows, size_t row_bytes, size_t first_rows, size_t* slots, size_t* first_bytes, size_t* total) {
    if (!n_frames || !fixed_bytes || !slots || !first_bytes || !total) return F3DS_ERR_ARG;
    static_assert(sizeof(LiSlot) == 3 * sizeof(size_t), "a slot is (at, rows_at, first)");
    std::vector<LiSlot> slot(n_frames);
    *total = li_stage_layout(n_frames, fixed_bytes, stage_rows, row_bytes, first_rows, slot.data(), first_bytes);
    memcpy(slots, slot.data(), n_frames * sizeof(LiSlot));
    return F3DS_OK;
}
