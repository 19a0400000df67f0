// f3ds_batch_policy.h -- the decisions the host takes once for all frames of a batch call, as functions of plain numbers: which path stage 0 takes and how wide its
// sort keys are, how much room the growing buffers get and how they grow after an overflow, and the launch widths.  Host only, plain C++17: no HIP, no f3ds_ctx.
// f3ds_hip.hip calls these functions and holds no copy of their arithmetic; the limits of the kernels they depend on (VT_TILE, MC_TL_CAP, ...) are passed in by
// it, since they live with the kernels.  f3ds_constant / f3ds_stage0_plan / f3ds_policy_capacity export all of it to tests that run without a GPU.
#ifndef F3DS_BATCH_POLICY_H_
#define F3DS_BATCH_POLICY_H_
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace f3ds_policy {

constexpr int KEY_BITS = 64;                    // a sort key is one 64-bit word
constexpr int TILE_MIN_CONTEXTS = 4;            // a call of fewer contexts takes the sort path (two of the tile path's kernels are one workgroup per frame)
// room of the growing buffers: count * multiplier + extra entries; a multiplier grows GROW-fold after an overflow while it is below its cap
constexpr uint32_t EV_MULT = 64, EV_EXTRA = 4096;             // weight-history events per initial edge
constexpr uint32_t EDGE_MULT = 32, EDGE_EXTRA = 1024;         // adjacency list entries per seed
constexpr uint32_t GROW = 4;
constexpr uint32_t EV_MULT_CAP = 16384, POOL_MULT_CAP = 64, ILIST_MULT_CAP = 4096, EDGE_MULT_CAP = 1u << 14;
constexpr uint32_t ILIST_SLACK = 32;                          // incident-list pool: 2 E + slack * E * ilist_mult + extra entries; F3DS_ILIST_SLACK below this: the short extra
constexpr uint32_t ILIST_EXTRA_SHORT = 16, ILIST_EXTRA = 1024;
constexpr uint32_t ENTRIES_MAX = 0x7fffffffu;                 // no buffer holds more entries than this
// a context the tile path refused stays off it for DENSE_PENALTY calls, DENSE_PENALTY_STEP times as many after every further refusal, up to DENSE_PENALTY_CAP
constexpr uint32_t DENSE_PENALTY = 8, DENSE_PENALTY_STEP = 2, DENSE_PENALTY_CAP = 1024;
constexpr int NORMALS_256_FRAMES = 16;          // d_normals_t<256> replaces <384> in calls of this many frames
constexpr size_t GRID_TARGET = 3072;            // workgroups of a streaming kernel for all frames of a call together ...
constexpr size_t GRID_MIN = 8, WIDE_CAP = 2048; // ... per frame no fewer than GRID_MIN and no more than WIDE_CAP, which is also the cap of a gathering kernel

inline int bits_for(uint64_t max_value) { int b = 0; while (b < 64 && (max_value >> b)) ++b; return b; }

// ---- stage 0
struct TileLimits { uint32_t tile, cnt_bits, ent_max, tab; };      // VT_TILE, VT_CNT_BITS, VT_ENT_MAX, VT_TAB of f3ds_kernels.inc
inline bool tile_path_wanted(int n_contexts, bool vox_hash, bool tiles_forced) { return vox_hash && (n_contexts >= TILE_MIN_CONTEXTS || tiles_forced); }
// whether a frame of n points fits the tile path: its descriptor keys in one word, its tables below 2^31 entries
inline bool tile_path_fits(int code_bits, int tile_bits, uint32_t n, const TileLimits& vt) {
    const uint32_t ntiles = (n + vt.tile - 1u) / vt.tile;
    const uint64_t dcap64 = (uint64_t)ntiles * vt.ent_max;
    if (code_bits + tile_bits + (int)vt.cnt_bits > KEY_BITS || dcap64 > 0x7fffffffull || (uint64_t)ntiles * vt.tab > 0x7fffffffull) return false;
    return true;
}
struct Stage0Plan {
    bool tiles;          // the tile path (false: the point sort)
    int code_bits;       // bits of a voxel's Morton code at the deepest grid of the call
    int tile_bits;       // bits of a tile's number in a descriptor key
    int idxbits;         // bits of a point's index in a one-word sort key; -1: the sort moves (key, index) pairs
    int sort_bits;       // width of the point sort's key without the index
};
// wanted: tile_path_wanted() and no context of the call is serving a refusal's penalty
inline Stage0Plan stage0_plan(int maxd, uint32_t maxn, bool wanted, bool sort_pairs, const TileLimits& vt) {
    Stage0Plan p;
    const uint32_t maxtiles = std::max(1u, (maxn + vt.tile - 1u) / vt.tile);
    p.tile_bits = bits_for((uint64_t)maxtiles - 1u);
    p.code_bits = 3 * maxd;
    p.tiles = wanted && tile_path_fits(p.code_bits, p.tile_bits, maxn, vt);
    // (Morton code << idxbits) | point index in one 64-bit word when both fit: the sort then moves 8 bytes per point and pass, not 12
    p.sort_bits = p.code_bits + 1;
    p.idxbits = bits_for((uint64_t)std::max(1u, maxn) - 1u);
    if (p.sort_bits + p.idxbits > KEY_BITS || sort_pairs) p.idxbits = -1;
    return p;
}

// ---- capacities and growth
inline uint32_t clamp_entries(uint64_t cap) { return cap > ENTRIES_MAX ? ENTRIES_MAX : (uint32_t)cap; }
inline uint32_t edge_capacity(uint32_t S0, uint32_t edge_mult) { return clamp_entries((uint64_t)S0 * edge_mult + EDGE_EXTRA); }
inline uint32_t event_capacity(uint32_t E, uint32_t ev_mult) { return clamp_entries((uint64_t)E * ev_mult + EV_EXTRA); }
inline uint32_t leaf_pool_capacity(uint32_t S0, uint32_t pool_mult) {
    uint32_t logS = 1; while ((1u << logS) < S0 + 2u) ++logS;
    return (S0 + 1u) * (4u * logS + 8u) * pool_mult;
}
// tl_cap: MC_TL_CAP.  What the loop can need is bounded: a merge that leaves its segment takes at most nt + nt / 2 + 4 fresh entries, nt <= tl_cap, and there
// are at most S0 - 1 merges
inline uint32_t ilist_capacity(uint32_t E, uint32_t S0, uint32_t slack, uint32_t ilist_mult, uint32_t tl_cap) {
    const uint64_t bound = 2ull * E + (uint64_t)(S0 ? S0 - 1u : 0u) * (tl_cap + tl_cap / 2u + 4u) + ILIST_EXTRA;
    uint64_t cap = 2ull * E + (uint64_t)slack * E * ilist_mult + (slack < ILIST_SLACK ? ILIST_EXTRA_SHORT : ILIST_EXTRA);
    if (cap > bound) cap = bound;
    return clamp_entries(cap);
}
// after an overflow: GROW times the room while the multiplier is below its cap (false: it stays, and the frame's error stands)
inline bool grow(uint32_t* mult, uint32_t cap) { if (*mult >= cap) return false; *mult *= GROW; return true; }
inline uint32_t next_dense_penalty(uint32_t penalty) { return std::min(DENSE_PENALTY_STEP * penalty, DENSE_PENALTY_CAP); }

// ---- launch shape
// threads of d_normals_t: forced: F3DS_NORMALS_THREADS (0: unset)
inline int normals_threads(int frames, int forced) { return (forced ? forced == 256 : frames >= NORMALS_256_FRAMES) ? 256 : 384; }
// workgroups per frame of a streaming kernel: target: F3DS_GRID_TARGET or GRID_TARGET (0: no sharing); forced: F3DS_GRID_CAP, which replaces both caps (0: unset)
inline size_t grid_cap_for_batch(int frames, size_t target, uint32_t forced) {
    if (forced) return (size_t)forced;
    if (!target) return WIDE_CAP;
    const size_t cap = target / (size_t)(frames > 0 ? frames : 1);
    return cap < GRID_MIN ? GRID_MIN : (cap > WIDE_CAP ? WIDE_CAP : cap);
}
// ... of a gathering kernel
inline size_t wide_cap(uint32_t forced) { return forced ? (size_t)forced : WIDE_CAP; }

}  // namespace f3ds_policy
#endif
