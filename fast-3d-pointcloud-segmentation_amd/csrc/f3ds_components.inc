// f3ds_components.inc -- the device path of the region components (f3ds_region_components, include/f3ds.h; the rules and the union-find steps are in
// f3ds_components.h; DESIGN.md section 21).  Included by f3ds_hip.hip after f3ds_shapes.inc.
//
//   d_comp_local    a workgroup takes tiles of 64 x 16 pixels in a grid-stride loop.  The tile's labels and depths go to LDS once; a row of the tile is one wave,
//                   and ONE ballot of "linked to my left neighbour" gives every lane its run head by bit arithmetic (cc_run_head): no union along a row.  Only
//                   where a run meets the row above for the first time (cc_joins) is it united with it, by atomic minima in LDS.  Then every pixel finds its
//                   root, the sizes are counted in LDS (one add per wave where the wave is of one component), and parent[p] = the global index of the tile's
//                   root, cnt[p] = the size at a root and 0 elsewhere are written.  A pixel that is not labelled gets CC_NONE.  A label out of range is flagged.
//   d_comp_seam     one lane per pixel of a tile's right column and bottom row: where the pair across the seam is a link that the pair before it does not
//                   already stand for (cc_joins again), the two sides are united in global memory (cc_unite: find both roots, atomicMin on the larger).
//   d_comp_flatten  every pixel finds its root and stores it; a pixel that was its tile's root adds the tile's size onto the root's: one atomic per tile
//                   component, not per pixel (DESIGN.md sections 17, 18).
//   d_comp_flag     flag[p] = 1 at the root of a kept component; the sums of the head, reduced in LDS, one atomic per workgroup that has any
//   (scan_u32 over the flags, in place)
//   d_comp_write    the image, the rows (region = label[root]) and the row count; nothing when a label was out of range, no row when they do not fit
// Termination is by construction: parent[x] <= x always, a stored parent only decreases, every walk goes down and every retry follows an atomic that lowered
// a word or saw a lower one (the comments at cc_find and cc_unite); no loop waits for another workgroup.  The root is the minimum index, so the result is the
// same under any schedule.

struct CompArgs {
    uint32_t width, height, n;         // n = width * height
    uint32_t depth_pitch;              // bytes per row (never 0 here)
    int depth_f32;
    uint32_t K;                        // regions
    uint32_t min_pixels;
    uint32_t tiles_x, tiles_y;
    float depth_scale, depth_tol;
};
// the head (LI_HEAD_WORDS, f3ds_label_image.h): [0] kept components, [1] 1 if a label was >= K, [2] dropped components, [3] spare, [4..5] labelled pixels (u64), [6..7] those in kept components (u64)
constexpr uint32_t RGK_FIRST_ROWS = 2048;      // rows of a host caller that ride with the head and the image; a frame with more gets a second download
constexpr uint32_t CC_TILE = CC_TILE_W * CC_TILE_H, CC_PER_THREAD = CC_TILE / 256u;
static_assert(CC_TILE_W == 64u && CC_TILE % 256u == 0u, "a tile row is a wave; a workgroup of 256 takes whole rows per trip");

// LDS and global memory for cc_find / cc_unite.  The loads are relaxed atomics so that a walk reads memory every step; a global one may still be served a word
// that another compute unit has lowered since -- an earlier parent, which is as good (cc_find).  What decides is the atomic minimum.
struct CcLds {
    uint32_t* p;
    __device__ uint32_t load(uint32_t i) const { return __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ uint32_t fetch_min(uint32_t i, uint32_t v) const { return atomicMin(&p[i], v); }
};
struct CcGlobal {
    uint32_t* p;
    __device__ uint32_t load(uint32_t i) const { return __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ uint32_t fetch_min(uint32_t i, uint32_t v) const { return atomicMin(&p[i], v); }
};
// a pixel as the rules see it: the label of a labelled pixel (CC_NONE for any other, one with a label out of range included) and its depth
template <bool DEPTH_F32>
struct CcImagePix {
    const unsigned char* depth; const uint32_t* label; uint32_t width, depth_pitch, K; float depth_scale;
    __device__ void operator()(uint32_t u, uint32_t v, uint32_t& lab, float& z) const {
        const uint32_t l = label[v * width + u];
        z = 0.0f;
        const bool valid = li_read_depth<DEPTH_F32>(depth, depth_pitch, depth_scale, u, v, z);
        lab = valid && l < K ? l : CC_NONE;      // (K <= CC_MAX_REGIONS: CC_NONE is never below it)
    }
};
struct CcTilePix {
    const uint32_t* lab; const float* z;
    __device__ void operator()(uint32_t c, uint32_t r, uint32_t& l, float& zz) const { l = lab[r * CC_TILE_W + c]; zz = z[r * CC_TILE_W + c]; }
};
struct CcTileLds { uint32_t lab[CC_TILE]; float z[CC_TILE]; uint32_t par[CC_TILE]; uint32_t cnt[CC_TILE]; };      // 16 KiB

// Thread t holds the pixels li = k * 256 + t, k = 0 ... 3, of the tile: row li >> 6 (wave + 4k), column li & 63 (its lane).  The tile loop and every barrier
// in it are uniform across the workgroup.
template <bool DEPTH_F32>
__device__ __forceinline__ void comp_local_tiles(const unsigned char* depth, const uint32_t* label, const CompArgs& a, uint32_t* parent, uint32_t* cnt, uint32_t* head, CcTileLds& t) {
    const CcImagePix<DEPTH_F32> image{depth, label, a.width, a.depth_pitch, a.K, a.depth_scale};
    const CcTilePix tile{t.lab, t.z};
    const CcLds mem{t.par};
    const uint32_t ntiles = a.tiles_x * a.tiles_y, c = threadIdx.x & 63u;
    bool bad = false;
    for (uint32_t ti = BIX; ti < ntiles; ti += gridDim.x) {
        const uint32_t ty = ti / a.tiles_x, tx = ti - ty * a.tiles_x, u0 = tx * CC_TILE_W, v0 = ty * CC_TILE_H;
        const bool in_u = u0 + c < a.width;
#pragma unroll
        for (uint32_t k = 0; k < CC_PER_THREAD; ++k) {      // the tile into LDS; outside the image nothing is labelled
            const uint32_t li = k * 256u + threadIdx.x, r = li >> 6;
            uint32_t l = CC_NONE; float z = 0.0f;
            if (in_u && v0 + r < a.height) {
                const uint32_t raw = label[(v0 + r) * a.width + u0 + c];
                bad = bad || (raw != CC_NONE && raw >= a.K);
                image(u0 + c, v0 + r, l, z);
            }
            t.lab[li] = l; t.z[li] = z; t.cnt[li] = 0u;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < CC_PER_THREAD; ++k) {      // run heads: one ballot per row
            const uint32_t li = k * 256u + threadIdx.x;
            const bool linked = c > 0u && cc_link(t.lab[li - 1u], t.z[li - 1u], t.lab[li], t.z[li], a.depth_tol);
            const uint64_t m = __ballot(linked);
            t.par[li] = (li & ~63u) + cc_run_head(m, c);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < CC_PER_THREAD; ++k) {      // the row above: where a run meets it for the first time
            const uint32_t li = k * 256u + threadIdx.x, r = li >> 6;
            if (r > 0u && cc_joins(tile, c, r - 1u, true, c != 0u, a.depth_tol)) cc_unite(mem, li, li - CC_TILE_W);      // (terminates: cc_unite)
        }
        __syncthreads();
        uint32_t root[CC_PER_THREAD];
#pragma unroll
        for (uint32_t k = 0; k < CC_PER_THREAD; ++k) {      // roots and sizes; nothing changes a parent any more
            const uint32_t li = k * 256u + threadIdx.x;
            const bool labelled = t.lab[li] != CC_NONE;
            root[k] = labelled ? cc_find(mem, li) : CC_NONE;      // (terminates: cc_find)
            const uint64_t m = __ballot(labelled);
            if (m != 0ull) {      // (wave-uniform)  a row of one component: one add for the wave
                const int first = (int)__builtin_ctzll(m);
                const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)root[k], first);
                if (__ballot(labelled && root[k] != r0) == 0ull) { if (lane_id() == first) atomicAdd(&t.cnt[r0], (uint32_t)__popcll(m)); }
                else if (labelled) atomicAdd(&t.cnt[root[k]], 1u);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < CC_PER_THREAD; ++k) {
            const uint32_t li = k * 256u + threadIdx.x, r = li >> 6;
            if (in_u && v0 + r < a.height) {
                const uint32_t p = (v0 + r) * a.width + u0 + c, rt = root[k];
                parent[p] = rt == CC_NONE ? CC_NONE : (v0 + (rt >> 6)) * a.width + u0 + (rt & 63u);      // (the tile's order of indices is the image's: the smallest stays the smallest)
                cnt[p] = rt == li ? t.cnt[li] : 0u;
            }
        }
        __syncthreads();      // (the next tile writes the same LDS)
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
}
constexpr int CC_TILES_PER_WG = 1;      // tiles a workgroup of d_comp_local takes per trip: what its launch divides the tile count by
struct d_comp_local {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, CompArgs a, uint32_t* parent, uint32_t* cnt, uint32_t* head) const {
        __shared__ CcTileLds t;      // (here and not in the template: one for the kernel, not one per instantiation)
        if (a.depth_f32) comp_local_tiles<true>(depth, label, a, parent, cnt, head, t);
        else comp_local_tiles<false>(depth, label, a, parent, cnt, head, t);
    }
};

// Seam pixels, numbered: first the right columns of the tile columns but the last ((tiles_x - 1) * height: pixel (64 (tx + 1) - 1, v) with its right neighbour),
// then the bottom rows of the tile rows but the last ((tiles_y - 1) * width: pixel (u, 16 (ty + 1) - 1) with its lower neighbour; lanes run along the row).
template <bool DEPTH_F32>
__device__ __forceinline__ void comp_seam_pixels(const unsigned char* depth, const uint32_t* label, const CompArgs& a, uint32_t* parent) {
    const CcImagePix<DEPTH_F32> image{depth, label, a.width, a.depth_pitch, a.K, a.depth_scale};
    const CcGlobal mem{parent};
    const uint32_t n_vert = (a.tiles_x - 1u) * a.height, total = n_vert + (a.tiles_y - 1u) * a.width;
    for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        uint32_t u, v; bool below;
        if (i < n_vert) { const uint32_t tx = i / a.height; v = i - tx * a.height; u = (tx + 1u) * CC_TILE_W - 1u; below = false; }      // (u + 1 < width: a tile column follows)
        else { const uint32_t j = i - n_vert, ty = j / a.width; u = j - ty * a.width; v = (ty + 1u) * CC_TILE_H - 1u; below = true; }      // (v + 1 < height likewise)
        const bool inner = below ? (u & (CC_TILE_W - 1u)) != 0u : (v & (CC_TILE_H - 1u)) != 0u;
        if (cc_joins(image, u, v, below, inner, a.depth_tol)) {
            const uint32_t p = v * a.width + u;
            cc_unite(mem, p, below ? p + a.width : p + 1u);      // (terminates: cc_unite; it waits for nobody)
        }
    }
}
struct d_comp_seam {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, CompArgs a, uint32_t* parent) const {
        if (a.depth_f32) comp_seam_pixels<true>(depth, label, a, parent);
        else comp_seam_pixels<false>(depth, label, a, parent);
    }
};

// No union runs any more: a root stays a root, and the only stores are roots into words of their own sets.
struct d_comp_flatten {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, uint32_t* parent, uint32_t* cnt) const {
        const CcGlobal mem{parent};
        for (uint32_t p = BIX * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
            const uint32_t q = parent[p];
            if (q == CC_NONE) continue;
            const uint32_t r = cc_find(mem, q);      // (terminates: cc_find)
            if (r != q) parent[p] = r;
            const uint32_t c = cnt[p];      // (nobody adds onto a word that is not a final root's)
            if (c != 0u && r != p) atomicAdd(&cnt[r], c);
        }
    }
};

struct d_comp_flag {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, const uint32_t* parent, const uint32_t* cnt, uint32_t min_pixels, uint32_t* flag, uint32_t* head) const {
        __shared__ rg_u64 s_sum[2];
        __shared__ uint32_t s_dropped;
        if (threadIdx.x < 2u) s_sum[threadIdx.x] = 0ull;
        if (threadIdx.x == 2u) s_dropped = 0u;
        __syncthreads();
        const uint32_t n_up = (n + blockDim.x - 1u) / blockDim.x * blockDim.x;      // (every lane makes the same trips: the ballot is of whole waves)
        for (uint32_t p = BIX * blockDim.x + threadIdx.x; p < n_up; p += gridDim.x * blockDim.x) {
            const bool root = p < n && parent[p] == p;
            if (__ballot(root) == 0ull) { if (p < n) flag[p] = 0u; continue; }      // (wave-uniform)  most waves hold no root
            const uint32_t c = root ? cnt[p] : 0u;
            const bool kept = root && cc_kept(c, min_pixels);
            if (p < n) flag[p] = kept ? 1u : 0u;
            if (root) {
                atomicAdd(&s_sum[0], (rg_u64)c);
                if (kept) atomicAdd(&s_sum[1], (rg_u64)c); else atomicAdd(&s_dropped, 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0u) {
            if (s_sum[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_sum[0]);
            if (s_sum[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 6), s_sum[1]);
            if (s_dropped) atomicAdd(&head[2], s_dropped);
        }
    }
};

// incl: the inclusive scan of the flags.  rows may be null (no rows asked for); more rows than row_cap: none is written.
struct d_comp_write {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, const uint32_t* label, const uint32_t* parent, const uint32_t* cnt, const uint32_t* incl, uint32_t min_pixels, uint32_t* head,
                               uint32_t* comp, f3ds_region_component* rows, uint64_t row_cap) const {
        if (head[1]) return;      // a label out of range: the image and the rows stay as they are
        const uint32_t total = n ? incl[n - 1u] : 0u;
        const bool write = rows != nullptr && (uint64_t)total <= row_cap;
        for (uint32_t p = BIX * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
            const uint32_t r = parent[p];
            uint32_t out = CC_NONE;
            if (r != CC_NONE) {
                const uint32_t c = cnt[r];
                if (cc_kept(c, min_pixels)) {
                    out = incl[r] - 1u;
                    if (r == p && write) { f3ds_region_component row; row.region = label[p]; row.first_pixel = p; row.n_pixels = c; rows[out] = row; }
                }
            }
            comp[p] = out;
        }
        if (BIX == 0u && threadIdx.x == 0u) head[0] = total;
    }
};
