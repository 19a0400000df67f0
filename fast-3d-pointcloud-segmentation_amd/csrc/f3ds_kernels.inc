// f3ds_kernels.inc -- every device kernel of the path as a functor `d_<name>` (operator() = the body
// for ONE frame; BLOCK = workgroup size).  f3ds_hip.hip launches them through k_batched<>, which adds
// the frame dimension: blockIdx.y selects the frame, so a batch of frames is one dispatch per kernel.
// Bodies keep using BIX / gridDim.x for their grid-stride loops.


namespace {

struct P16 { float x, y, z; uint32_t rgba; };

// small block of device scalars the host reads back at the few sync points
struct DevCounters {
    unsigned long long n_finite;
    uint32_t bbox[6];        // order-preserving encodings of min xyz, max xyz
    uint32_t bbox_any;
    uint32_t n_valid;        // points with a valid voxel key
    uint32_t n_voxels;
    uint32_t n_cells;
    uint32_t n_seeds;
    uint32_t n_edges;
    uint32_t n_alive;        // non-empty supervoxels
    uint32_t n_merges;
    uint32_t n_regions;
    uint32_t n_events;
    int error;               // first error raised on the device
    int r_overflow;
    float lambda;
    uint32_t seg_count;      // scratch for generic segmenting
    uint32_t n_ghosts;       // helpers that still hold a ghost leaf (sweeps)
    int depth;               // voxel grid depth (k_grid)
    int grid_empty;          // no point survived the bounding-box pass
    int sdepth;              // seed grid depth (k_seed_grow)
    uint32_t n_changed;      // voxels whose (owner, distance) changed in the current sweep
    uint32_t sweep_full;     // t+1 while sweep t has to evaluate every voxel (no dirty-tile skipping)
    uint32_t sweep_marks;    // t+1 while sweep t records which tiles the next sweep has to look at
    int ev_overflow;         // an F3dsOverflow (f3ds_algo.h): what the kernel that set error = F3DS_ERR_UNSUPPORTED ran out of; the host reruns the stage with more of it, or on another path
    uint32_t sweep_pre;      // t+1 when sweep t was full from its start, i.e. its R pre-pass ran (an incremental sweep whose rounds do not converge turns full later: d_sweep_R)
    uint32_t pad_to_line_[1];         // rq[] starts a 128-byte line of its own: the chain walker's list counters are bumped by atomics from every workgroup, as n_changed (above) is by the claim kernel
    uint32_t rq[F3DS_R_PASSES + 1];   // chain walker lists of a full sweep: rq[0] voxels from the pre-pass, rq[p] voxels whose
                                      // dependency chain was deeper than pass p-1 could follow (they are retried in pass p)
    uint32_t vox_disorder;            // stage 0, tile path: some leaf list may not be ascending (two runs of one voxel met in one 256-point step): d_voxel_list_accum sorts
    uint32_t vox_max_tile;            // ... most distinct voxels in a tile (diagnostics)
#ifdef F3DS_CEN_STATS
    uint32_t cen_stats[8];            // (measurement build) d_centroid: quads, live rows, rows sent to the wave-wide path for their list / for their leaves, sum of ndmax, of nd, of leaves, of max leaves
#endif
    uint32_t sweep_stats[4];          // sweeps of the last run that were full from their start / incremental (dirty tiles, R rounds) / incremental at first and sent to the chain
                                      // walker because their last R round still changed a word (the fallback of d_sweep_R) / skipped (sweep_idle): F3DS_DBG_SWEEP_STATS, diagnostics and tests
    uint32_t sweep_idle;              // t+1 while sweep t is known to change nothing (the sweep before it changed nothing and no ghost leaf is active): its kernels return at once
};

static_assert(offsetof(DevCounters, rq) == 128, "rq[] on a 128-byte line of its own");
// the sweep-control words as the shared protocol takes them (f3ds_algo.h: a_sweep_begin and its predicates)
__device__ inline SweepCtl sweep_ctl(DevCounters* dc) { return SweepCtl{&dc->n_changed, &dc->sweep_full, &dc->sweep_pre, &dc->sweep_marks, &dc->sweep_idle}; }
constexpr uint64_t HASH_EMPTY = 0xFFFFFFFFFFFFFFFFull;

__host__ __device__ inline uint64_t hash64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
__device__ inline uint32_t enc_f32(float f) {
    uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float dec_f32(uint32_t e) {
    uint32_t b = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
    float f; memcpy(&f, &b, 4); return f;
}

// XCD-aware block mapping for batched launches (grid = (width, frames)).  Workgroups are handed to
// the 8 XCDs round-robin in linear order, and each XCD has its own 4 MB L2; a frame's voxel table
// (3-4 MB) is gathered ~800 times per voxel by the normals / sweep kernels.  So the linear workgroup
// id is re-read as: 8 consecutive ids -> the same virtual block of 8 different frames.  All workgroups
// of one frame then sit on one XCD and hit that XCD's L2.  Frames beyond the last full group of 8
// keep the plain mapping.  BIX = virtual blockIdx.x, f3ds_frame() = virtual blockIdx.y.
__device__ __forceinline__ void f3ds_vblock(uint32_t* frame, uint32_t* vbx) {
    const uint32_t gx = gridDim.x, nf = gridDim.y;
    const uint32_t full = nf & ~7u;
    if (blockIdx.y < full) {
        const uint32_t lin = blockIdx.y * gx + blockIdx.x;
        const uint32_t g = lin / (8u * gx), r = lin - g * 8u * gx;
        *frame = g * 8u + (r & 7u); *vbx = r >> 3;
    } else { *frame = blockIdx.y; *vbx = blockIdx.x; }
}
__device__ __forceinline__ uint32_t f3ds_vbx() { uint32_t f, x; f3ds_vblock(&f, &x); return x; }
__device__ __forceinline__ uint32_t f3ds_frame() { uint32_t f, x; f3ds_vblock(&f, &x); return f; }
#define BIX (f3ds_vbx())

__device__ inline int lane_id() { return (int)(threadIdx.x & 63u); }
__device__ inline uint64_t lanemask_lt() { return (1ull << lane_id()) - 1ull; }
// LDS written by some lanes of a wave and read by others of the same wave (no workgroup barrier: the
// waves of a block work on different helpers and leave at different times)
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------
// generic inclusive scan of uint32 (three launches; any n)
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

__device__ inline uint32_t wave_incl_scan(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane_id() >= d) v += t;
    }
    return v;
}
// inclusive scan across a block of BLOCK threads (BLOCK multiple of 64, <= 1024); returns the
// inclusive prefix of `v`, *total gets the block sum
template <int BLOCK>
__device__ inline uint32_t block_incl_scan(uint32_t v, uint32_t* total) {
    __shared__ uint32_t wsum[BLOCK / 64];
    __shared__ uint32_t wtot;
    uint32_t inc = wave_incl_scan(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 63) wsum[w] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < BLOCK / 64; ++i) { uint32_t t = wsum[i]; wsum[i] = run; run += t; }
        wtot = run;
    }
    __syncthreads();
    *total = wtot;
    return inc + wsum[w];
}

// exclusive scan of m values in place by ONE workgroup of 256 threads: 4096 consecutive values per round (16 per thread, coalesced b128),
// carry across rounds.  256 threads and not 1024 (round 2): with other calls filling the chip a 1024-thread workgroup waited 0.6 ms on
// average (52 ms at worst) for a compute unit with sixteen free wave slots, 18 times per call, on the dependent chain of every radix pass.
// (Tried in round 3 and dropped: the LAST workgroup of the counting kernel scans on the spot -- no launch at all -- but the device-scope
// release/acquire fences every workgroup then needs write back and invalidate the XCD's L2 (buffer_wbl2 / buffer_inv): d_radix_hist
// went from 6 to 94 us per frame, d_seg_count from 1.9 to 43, the bench from 2 400 to 1 550 Mpoints/s.)
struct d_scan_single {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* data, uint32_t m) const {
        uint32_t carry = 0;
        for (uint32_t base = 0; base < m; base += 4096u) {
            const uint32_t i0 = base + threadIdx.x * 16u;
            uint32_t v[16];
            if (i0 + 15u < m) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { const uint4 x = *reinterpret_cast<const uint4*>(data + i0 + 4 * q); v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w; }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = i0 + k < m ? data[i0 + k] : 0u;
            }
            uint32_t sum = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) sum += v[k];
            uint32_t tot;
            const uint32_t inc = block_incl_scan<256>(sum, &tot);
            uint32_t run = carry + inc - sum;
            if (i0 + 15u < m) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint4 x; x.x = run; x.y = run + v[4 * q]; x.z = x.y + v[4 * q + 1]; x.w = x.z + v[4 * q + 2]; run = x.w + v[4 * q + 3];
                    *reinterpret_cast<uint4*>(data + i0 + 4 * q) = x;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) if (i0 + k < m) { data[i0 + k] = run; run += v[k]; }
            }
            carry += tot;
        }
    }
};
struct d_scan_tiles {
    static constexpr int BLOCK = SCAN_THREADS;
    __device__ void operator()(const uint32_t* in, uint32_t* out, uint32_t* tile_sums, uint32_t n) const {
        if (BIX > 0 && BIX * SCAN_TILE >= n) return;      // (a batched launch is as wide as its widest frame)
        const uint32_t base = BIX * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
        uint32_t v[SCAN_ITEMS];
        uint32_t s = 0;
    #pragma unroll
        for (int i = 0; i < SCAN_ITEMS; ++i) { v[i] = (base + i < n) ? in[base + i] : 0u; s += v[i]; }
        uint32_t tot;
        uint32_t inc = block_incl_scan<SCAN_THREADS>(s, &tot);
        uint32_t run = inc - s;
    #pragma unroll
        for (int i = 0; i < SCAN_ITEMS; ++i) { run += v[i]; if (base + i < n) out[base + i] = run; }
        if (threadIdx.x == 0) tile_sums[BIX] = tot;
    }
};
struct d_scan_add {
    static constexpr int BLOCK = SCAN_THREADS;
    __device__ void operator()(uint32_t* out, const uint32_t* tile_offsets, uint32_t n) const {
        if (BIX > 0 && BIX * SCAN_TILE >= n) return;
        const uint32_t base = BIX * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
        const uint32_t off = tile_offsets[BIX];
    #pragma unroll
        for (int i = 0; i < SCAN_ITEMS; ++i) if (base + i < n) out[base + i] += off;
    }
};

// ------------------------------------------------------------------------------------------------
// stable LSD radix sort of (uint64 key, uint32 value) pairs, up to RS_MAXBITS (9) bits per pass: the 25 code bits of a
// 1M-point frame are three passes (four with 8-bit digits: a quarter of the sort's traffic and launches).
// One workgroup owns a contiguous tile; inside the tile each wave owns a contiguous quarter and
// walks it in 64-element strips, so "earlier in memory" == "earlier in (wave, strip, lane)" and
// ranks from ballots are stable.
// ------------------------------------------------------------------------------------------------
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_STRIPS = 16;                         // strips of 64 per wave
constexpr int RS_TILE = RS_THREADS * RS_STRIPS;       // 4096 keys per workgroup
constexpr int RS_MAXBITS = 9;
constexpr int RS_BINS = 1 << RS_MAXBITS;

struct d_radix_hist {
    static constexpr int BLOCK = RS_THREADS;
    // n_dev != nullptr: the element count lives on the device (the voxel sort of the hash voxelisation: V is not known to the host yet); `n` then only bounds it
    __device__ void operator()(const uint64_t* keys, uint32_t n, int shift, int bits, uint32_t* hist,
                                                         uint32_t nblocks, const uint32_t* n_dev) const {
        if (BIX >= nblocks) return;
        if (n_dev) { const uint32_t nd = *n_dev; n = nd < n ? nd : n; }
        __shared__ uint32_t lh[RS_BINS];
        for (int i = threadIdx.x; i < RS_BINS; i += RS_THREADS) lh[i] = 0;
        __syncthreads();
        const uint32_t mask = (1u << bits) - 1u;
        const uint32_t wbase = BIX * RS_TILE + (threadIdx.x >> 6) * (64 * RS_STRIPS);
    #pragma unroll
        for (int s = 0; s < RS_STRIPS; ++s) {
            uint32_t i = wbase + s * 64 + lane_id();
            if (i < n) atomicAdd(&lh[(uint32_t)(keys[i] >> shift) & mask], 1u);
        }
        __syncthreads();
        for (uint32_t d = threadIdx.x; d < (1u << bits); d += RS_THREADS) hist[d * nblocks + BIX] = lh[d];
    }
};
struct d_radix_scatter {
    static constexpr int BLOCK = RS_THREADS;
    __device__ void operator()(const uint64_t* keys, const uint32_t* vals, uint64_t* keys_out,
                                                            uint32_t* vals_out, uint32_t n, int shift, int bits,
                                                            const uint32_t* hist_scanned, uint32_t nblocks, const uint32_t* n_dev) const {
        if (BIX >= nblocks) return;
        if (n_dev) { const uint32_t nd = *n_dev; n = nd < n ? nd : n; }
        __shared__ uint32_t wcount[RS_WAVES][RS_BINS];
        const uint32_t mask = (1u << bits) - 1u;
        const int w = threadIdx.x >> 6;
        for (int i = threadIdx.x; i < RS_WAVES * RS_BINS; i += RS_THREADS) (&wcount[0][0])[i] = 0;
        __syncthreads();
        const uint32_t wbase = BIX * RS_TILE + w * (64 * RS_STRIPS);
        uint64_t k[RS_STRIPS];
    #pragma unroll
        for (int s = 0; s < RS_STRIPS; ++s) {
            uint32_t i = wbase + s * 64 + lane_id();
            k[s] = i < n ? keys[i] : 0ull;
            if (i < n) atomicAdd(&wcount[w][(uint32_t)(k[s] >> shift) & mask], 1u);
        }
        __syncthreads();
        for (uint32_t d = threadIdx.x; d < (1u << bits); d += RS_THREADS) {   // digit d: global base of this tile, then per-wave starts
            uint32_t run = hist_scanned[d * nblocks + BIX];
            for (int ww = 0; ww < RS_WAVES; ++ww) { uint32_t t = wcount[ww][d]; wcount[ww][d] = run; run += t; }
        }
        __syncthreads();
    #pragma unroll
        for (int s = 0; s < RS_STRIPS; ++s) {
            uint32_t i = wbase + s * 64 + lane_id();
            const bool valid = i < n;
            const uint32_t d = (uint32_t)(k[s] >> shift) & mask;
            uint64_t peers = __ballot(valid);
            for (int b = 0; b < bits; ++b) {
                uint64_t m = __ballot(valid && ((d >> b) & 1u));
                peers &= ((d >> b) & 1u) ? m : ~m;
            }
            uint32_t pos = 0;
            if (valid) pos = wcount[w][d] + (uint32_t)__popcll(peers & lanemask_lt());
            __builtin_amdgcn_wave_barrier();
            if (valid && (peers & lanemask_lt()) == 0ull) wcount[w][d] += (uint32_t)__popcll(peers);   // lowest peer advances the cursor
            __builtin_amdgcn_wave_barrier();
            if (valid) { keys_out[pos] = k[s]; vals_out[pos] = vals[i]; }
        }
    }
};


// the same for keys that carry their payload in their own low bits (point sort: (Morton code << idxbits) | index)
struct d_radix_scatter_k {
    static constexpr int BLOCK = RS_THREADS;
    __device__ void operator()(const uint64_t* keys, uint64_t* keys_out, uint32_t n, int shift, int bits, const uint32_t* hist_scanned, uint32_t nblocks) const {
        if (BIX >= nblocks) return;
        __shared__ uint32_t wcount[RS_WAVES][RS_BINS];
        const uint32_t mask = (1u << bits) - 1u;
        const int w = threadIdx.x >> 6;
        for (int i = threadIdx.x; i < RS_WAVES * RS_BINS; i += RS_THREADS) (&wcount[0][0])[i] = 0;
        __syncthreads();
        const uint32_t wbase = BIX * RS_TILE + w * (64 * RS_STRIPS);
        uint64_t k[RS_STRIPS];
    #pragma unroll
        for (int s = 0; s < RS_STRIPS; ++s) {
            uint32_t i = wbase + s * 64 + lane_id();
            k[s] = i < n ? keys[i] : 0ull;
            if (i < n) atomicAdd(&wcount[w][(uint32_t)(k[s] >> shift) & mask], 1u);
        }
        __syncthreads();
        for (uint32_t d = threadIdx.x; d < (1u << bits); d += RS_THREADS) {
            uint32_t run = hist_scanned[d * nblocks + BIX];
            for (int ww = 0; ww < RS_WAVES; ++ww) { uint32_t t = wcount[ww][d]; wcount[ww][d] = run; run += t; }
        }
        __syncthreads();
    #pragma unroll
        for (int s = 0; s < RS_STRIPS; ++s) {
            uint32_t i = wbase + s * 64 + lane_id();
            const bool valid = i < n;
            const uint32_t d = (uint32_t)(k[s] >> shift) & mask;
            uint64_t peers = __ballot(valid);
            for (int b = 0; b < bits; ++b) {
                uint64_t m = __ballot(valid && ((d >> b) & 1u));
                peers &= ((d >> b) & 1u) ? m : ~m;
            }
            uint32_t pos = 0;
            if (valid) pos = wcount[w][d] + (uint32_t)__popcll(peers & lanemask_lt());
            __builtin_amdgcn_wave_barrier();
            if (valid && (peers & lanemask_lt()) == 0ull) wcount[w][d] += (uint32_t)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
            if (valid) keys_out[pos] = k[s];
        }
    }
};

// ------------------------------------------------------------------------------------------------
// stage 0: voxelise
// ------------------------------------------------------------------------------------------------
struct FrameArgs {
    int use_transform, fold_negative_z, leaf_order;
    float voxel_res, seed_res, w_color, w_spatial, w_normal;
};

__device__ inline P16 load_point(const P16* pts, size_t i) {
    const uint4 q = reinterpret_cast<const uint4*>(pts)[i];     // one global_load_dwordx4
    P16 p;
    p.x = __uint_as_float(q.x); p.y = __uint_as_float(q.y); p.z = __uint_as_float(q.z); p.rgba = q.w;
    return p;
}

// The voxel table of the neighbour search (cell key -> leaf ordinal), open addressing, built by d_vox_table after the host knows V and read by d_neighbors.  d_neighbors runs at the
// rate its address unit can touch lines (DESIGN.md 5) and nearly all its lines were probes: 27 per voxel into a table with an entry per voxel.  Grids of depth <= 12 (every BASELINE
// configuration) therefore keep an entry per 4x4x4 BLOCK of cells (f3ds_numerics.h, n_block_*): 16 bytes -- block key, ordinal of the block's first leaf, 64-bit mask of its EMPTY cells
// (stored complemented so that the all-ones fill is an empty entry and a build is atomic ANDs) -- read with one load.  A voxel's 27 cells lie in at most 8 blocks and the lanes of a wave
// ask for about ten blocks between them: lanes that want the same block read the same line, the rest is arithmetic.  A surface fills 10-16 cells of a block it crosses, so the table
// has a tenth of the entries.  Deeper grids keep an entry per voxel: 63-bit keys in hkeys, ordinals in hvals, two dependent loads per hit.
__device__ inline bool vt_blocks(int depth) { return depth <= N_BLOCK_DEPTH_MAX; }
constexpr uint32_t BT_EMPTY = 0xFFFFFFFFu;
struct __attribute__((aligned(16))) BtEntry { uint32_t key, base; unsigned long long vacant; };
static_assert(sizeof(BtEntry) == 16, "one 16-byte load per probe");
// The atomics of a table one workgroup builds are WORKGROUP-scope (resolved in the XCD's L2); several workgroups need agent scope (resolved beyond it: ~0.1 us of the chip per thousand).
template <class T> __device__ inline bool vt_cas(T* p, T* expect, T v, bool agent) {
    return agent ? __hip_atomic_compare_exchange_strong(p, expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                 : __hip_atomic_compare_exchange_strong(p, expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// general layout: keys are unique (one insert per leaf)
__device__ inline void vt_insert(uint64_t* hkeys, uint32_t* hvals, uint32_t hmask, bool agent, unsigned x, unsigned y, unsigned z, uint32_t v) {
    const unsigned long long pk = (unsigned long long)n_pack_key(x, y, z);
    uint32_t h = (uint32_t)hash64((uint64_t)pk) & hmask;
    for (;;) {
        unsigned long long expect = HASH_EMPTY;
        if (vt_cas((unsigned long long*)&hkeys[h], &expect, pk, agent) || expect == pk) { hvals[h] = v; return; }
        h = (h + 1u) & hmask;
    }
}
__device__ inline int vt_find(const uint64_t* hkeys, const uint32_t* hvals, uint32_t hmask, unsigned x, unsigned y, unsigned z) {
    const uint64_t pk = n_pack_key(x, y, z);
    uint32_t h = (uint32_t)hash64(pk) & hmask;
    for (;;) {
        const uint64_t k = hkeys[h];
        if (k == pk) return (int)hvals[h];
        if (k == HASH_EMPTY) return -1;
        h = (h + 1u) & hmask;
    }
}
// block layout: the entry of block `bk`, claimed on the way if no lane has asked for it yet (the heads of a block's run of leaves and the lanes that continue a run across a wave border)
__device__ inline BtEntry* bt_entry(BtEntry* tab, uint32_t tmask, bool agent, uint32_t bk) {
    uint32_t h = (uint32_t)hash64((uint64_t)bk) & tmask;
    for (;;) {
        uint32_t expect = BT_EMPTY;
        if (vt_cas(&tab[h].key, &expect, bk, agent) || expect == bk) return &tab[h];
        h = (h + 1u) & tmask;
    }
}
__device__ inline int bt_find(const BtEntry* tab, uint32_t tmask, int leaf_order, unsigned x, unsigned y, unsigned z) {
    const uint32_t bk = n_block_key(x, y, z);
    uint32_t h = (uint32_t)hash64((uint64_t)bk) & tmask;
    for (;;) {
        const uint4 e = reinterpret_cast<const uint4*>(tab)[h];      // one global_load_dwordx4
        if (e.x == bk) return n_block_ordinal(e.y, ~(((uint64_t)e.w << 32) | (uint64_t)e.z), n_block_cell(x, y, z), leaf_order);
        if (e.x == BT_EMPTY) return -1;
        h = (h + 1u) & tmask;
    }
}
// RGB-D frames (f3ds_segment_rgbd): the XYZRGBA records of a depth image + a colour image, pixel (u, v) -> record v * width + u.  One pixel per lane and trip,
// consecutive lanes on consecutive pixels: a wave reads 128 or 256 contiguous bytes of depth and 192 or 256 of colour (less where a row ends inside it) and writes
// 1 KiB of records, one 16-byte store per lane.  Rows are addressed through their pitches and nothing but byte alignment is assumed of a colour row (the loads are
// unaligned ones: RGB8 rows, and rows of any format behind an odd pitch); depth elements are aligned to their size.  The two formats are template parameters so that the
// loop holds no branch between its loads: both are in flight before the first is waited for.  The arithmetic is n_depth_to_z / n_deproject (f3ds_numerics.h), which
// f3ds_deproject runs on the host.
struct RgbdArgs {
    uint32_t width, n;                 // n = width * height
    uint32_t depth_pitch, color_pitch; // bytes per row (never 0 here: the host resolves "tightly packed")
    int depth_f32, color_format;       // depth elements are f32 (else u16); F3DS_COLOR_*
    float depth_scale, fx, fy, cx, cy;
};
template <class T> __device__ inline T load_unaligned(const unsigned char* p) { T t; __builtin_memcpy(&t, p, sizeof(T)); return t; }
template <bool DEPTH_F32, int COLOR>
__device__ inline void deproject_loop(const unsigned char* depth, const unsigned char* color, const RgbdArgs& a, P16* out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t sv = stride / a.width, su = stride - sv * a.width;      // a trip moves every lane this many rows and columns on
    uint32_t i = BIX * blockDim.x + threadIdx.x;
    uint32_t v = i / a.width, u = i - v * a.width;
    for (; i < a.n; i += stride) {
        const unsigned char* drow = depth + (size_t)v * a.depth_pitch;
        const unsigned char* crow = color + (size_t)v * a.color_pitch;
        float z = 0.0f;
        bool valid;
        if constexpr (DEPTH_F32) valid = n_depth_to_z(reinterpret_cast<const float*>(drow)[u], a.depth_scale, z);
        else valid = n_depth_to_z(reinterpret_cast<const uint16_t*>(drow)[u], a.depth_scale, z);
        uint32_t rgba;
        if constexpr (COLOR == 0) { const unsigned char* p = crow + 3u * (size_t)u; rgba = n_color_word(p[0], p[1], p[2], 255u); }
        else {
            const uint32_t w = load_unaligned<uint32_t>(crow + 4u * (size_t)u);      // bytes r, g, b, a in memory = a << 24 | b << 16 | g << 8 | r as a little-endian word
            rgba = COLOR == 1 ? n_color_word(w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, w >> 24) : w;
        }
        float x, y, zo;
        n_deproject(u, v, valid, z, a.fx, a.fy, a.cx, a.cy, x, y, zo);
        reinterpret_cast<uint4*>(out)[i] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(zo), rgba);      // one global_store_dwordx4
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
}
struct d_deproject {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const unsigned char* color, RgbdArgs a, P16* out) const {
        if (a.depth_f32) {
            if (a.color_format == 0) deproject_loop<true, 0>(depth, color, a, out);
            else if (a.color_format == 1) deproject_loop<true, 1>(depth, color, a, out);
            else deproject_loop<true, 2>(depth, color, a, out);
        } else {
            if (a.color_format == 0) deproject_loop<false, 0>(depth, color, a, out);
            else if (a.color_format == 1) deproject_loop<false, 1>(depth, color, a, out);
            else deproject_loop<false, 2>(depth, color, a, out);
        }
    }
};
// bounding box of the transformed finite points + count of finite input points
struct d_bbox {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* pts, uint32_t n, FrameArgs fa, DevCounters* dc) const {
        float mn[3] = {F3DS_FLT_MAX, F3DS_FLT_MAX, F3DS_FLT_MAX}, mx[3] = {-F3DS_FLT_MAX, -F3DS_FLT_MAX, -F3DS_FLT_MAX};
        uint32_t nfin = 0, any = 0;
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            P16 p = load_point(pts, i);
            float x = p.x, y = p.y, z = p.z;
            n_prelude(z, fa.fold_negative_z);
            if (n_finite3(x, y, z)) nfin++;
            n_transform(x, y, z, fa.use_transform);
            if (!n_finite3(x, y, z)) continue;
            any = 1;
            if (x < mn[0]) mn[0] = x;
            if (y < mn[1]) mn[1] = y;
            if (z < mn[2]) mn[2] = z;
            if (x > mx[0]) mx[0] = x;
            if (y > mx[1]) mx[1] = y;
            if (z > mx[2]) mx[2] = z;
        }
    #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            for (int a = 0; a < 3; ++a) {
                float t = __shfl_xor(mn[a], d, 64); if (t < mn[a]) mn[a] = t;
                t = __shfl_xor(mx[a], d, 64); if (t > mx[a]) mx[a] = t;
            }
            nfin += __shfl_xor(nfin, d, 64);
            any |= __shfl_xor(any, d, 64);
        }
        __shared__ float smn[4][3], smx[4][3];
        __shared__ uint32_t sfin[4], sany[4];
        const int w = threadIdx.x >> 6;
        if (lane_id() == 0) { for (int a = 0; a < 3; ++a) { smn[w][a] = mn[a]; smx[w][a] = mx[a]; } sfin[w] = nfin; sany[w] = any; }
        __syncthreads();
        if (threadIdx.x == 0) {      // one set of atomics per workgroup: ~13 ns each on one address
            for (int ww = 1; ww < 4; ++ww) {
                for (int a = 0; a < 3; ++a) { if (smn[ww][a] < mn[a]) mn[a] = smn[ww][a]; if (smx[ww][a] > mx[a]) mx[a] = smx[ww][a]; }
                nfin += sfin[ww]; any |= sany[ww];
            }
            if (any) {
                for (int a = 0; a < 3; ++a) { atomicMin(&dc->bbox[a], enc_f32(mn[a])); atomicMax(&dc->bbox[3 + a], enc_f32(mx[a])); }
                atomicOr(&dc->bbox_any, 1u);
            }
            if (nfin) atomicAdd(&dc->n_finite, (unsigned long long)nfin);
        }
    }
};
struct d_grid {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 64;
    __device__ void operator()(DevCounters* dc, float voxel_res, GridInfo* g) const {
        if (threadIdx.x || BIX) return;
        GridInfo t;
        if (!dc->bbox_any) {
            for (int a = 0; a < 3; ++a) { t.min[a] = 0; t.max[a] = 0; }
            t.res = (double)voxel_res; t.depth = 0; t.max_key = 0; t.error = 0; t.empty = 1;
        } else {
            float mn[3], mx[3];
            for (int a = 0; a < 3; ++a) { mn[a] = dec_f32(dc->bbox[a]); mx[a] = dec_f32(dc->bbox[3 + a]); }
            n_grid_from_bbox(mn, mx, voxel_res, t);
            if (t.error) dc->error = t.error;
        }
        *g = t;
        dc->depth = t.depth; dc->grid_empty = t.empty;
    }
};
// Morton key per point (leaf order), invalid points get the one key above every valid one
struct d_keys {
    static constexpr int BLOCK = 256;
    // vals == nullptr: the index goes into the low idxbits bits of the key (one 8-byte array to sort instead of 12 bytes in two)
    __device__ void operator()(const P16* pts, uint32_t n, FrameArgs fa, const GridInfo* gp, uint64_t* keys, uint32_t* vals, int idxbits) const {
        const GridInfo g = *gp;
        const uint64_t invalid = 1ull << (3 * g.depth);
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            P16 p = load_point(pts, i);
            float x = p.x, y = p.y, z = p.z;
            n_prelude(z, fa.fold_negative_z);
            uint64_t key = invalid;
            if (n_finite3(x, y, z) && !g.empty) {
                unsigned k[3];
                n_point_key(g, x, y, z, fa.use_transform, k);
                key = n_morton(k[0], k[1], k[2], g.depth);
                if (fa.leaf_order == 1) key = (~key) & (invalid - 1ull);
            }
            if (vals) { keys[i] = key; vals[i] = i; } else keys[i] = (key << idxbits) | (uint64_t)i;
        }
    }
};
// segment heads of a sorted key array; keys >= limit are "no segment"
struct d_heads {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* keys, uint32_t n, uint64_t limit, uint32_t* flags, int shift) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            uint64_t k = keys[i] >> shift;
            flags[i] = (k < limit && (i == 0 || (keys[i - 1] >> shift) != k)) ? 1u : 0u;
        }
    }
};
// seg_start[s] = first sorted position of segment s; seg_start[nseg] = number of valid keys
struct d_segstart {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* keys, const uint32_t* flags, const uint32_t* incl, uint32_t n, uint64_t limit,
                                                 uint32_t* seg_start, uint32_t* nseg_out, uint32_t* nvalid_out, int shift) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            if (flags[i]) seg_start[incl[i] - 1u] = i;
            if ((keys[i] >> shift) < limit && (i + 1 == n || (keys[i + 1] >> shift) >= limit)) { seg_start[incl[i]] = i + 1u; *nseg_out = incl[i]; *nvalid_out = i + 1u; }
        }
    }
};
// The same segment table without the per-position flag and rank arrays (nothing reads them once the voxel sums gather their points themselves):
// d_seg_count counts the segment heads of every SCAN_TILE sorted positions, d_scan_single turns the counts into offsets, d_seg_write finds the heads again
// and writes seg_start / n_voxels / n_valid.  16 bytes of key reads per point instead of the 44 bytes of d_heads + scan + d_segstart.
__device__ inline uint32_t seg_heads_of_thread(const uint64_t* keys, uint32_t n, uint64_t limit, int shift, uint32_t base, uint64_t k[SCAN_ITEMS + 1], uint32_t* head_mask) {
    // k[0..ITEMS-1] = codes of this thread's positions, k[ITEMS] = the code behind them (~0 = none); bit i of *head_mask: position base + i starts a segment
    uint64_t prev = (base > 0u && base - 1u < n) ? keys[base - 1u] >> shift : ~0ull;
    uint32_t cnt = 0, mask = 0;
#pragma unroll
    for (int i = 0; i <= SCAN_ITEMS; ++i) k[i] = base + (uint32_t)i < n ? keys[base + (uint32_t)i] >> shift : ~0ull;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        const bool head = base + (uint32_t)i < n && k[i] < limit && (base + (uint32_t)i == 0u || prev != k[i]);
        if (head) { cnt++; mask |= 1u << i; }
        prev = k[i];
    }
    *head_mask = mask;
    return cnt;
}
struct d_seg_count {
    static constexpr int BLOCK = SCAN_THREADS;
    __device__ void operator()(const uint64_t* keys, uint32_t n, uint64_t limit, int shift, uint32_t* tile_sums) const {
        if (BIX > 0 && BIX * SCAN_TILE >= n) return;
        uint64_t k[SCAN_ITEMS + 1]; uint32_t mask, tot;
        const uint32_t cnt = seg_heads_of_thread(keys, n, limit, shift, BIX * SCAN_TILE + threadIdx.x * SCAN_ITEMS, k, &mask);
        block_incl_scan<SCAN_THREADS>(cnt, &tot);
        if (threadIdx.x == 0) tile_sums[BIX] = tot;
    }
};
struct d_seg_write {
    static constexpr int BLOCK = SCAN_THREADS;
    __device__ void operator()(const uint64_t* keys, uint32_t n, uint64_t limit, int shift, const uint32_t* tile_offsets, uint32_t* seg_start, uint32_t* nseg_out, uint32_t* nvalid_out) const {
        if (BIX > 0 && BIX * SCAN_TILE >= n) return;
        const uint32_t base = BIX * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
        uint64_t k[SCAN_ITEMS + 1]; uint32_t mask, tot;
        const uint32_t cnt = seg_heads_of_thread(keys, n, limit, shift, base, k, &mask);
        uint32_t run = tile_offsets[BIX] + block_incl_scan<SCAN_THREADS>(cnt, &tot) - cnt;      // segments that start before this thread's first position
#pragma unroll
        for (int i = 0; i < SCAN_ITEMS; ++i) {
            const uint32_t pos = base + (uint32_t)i;
            if (mask & (1u << i)) seg_start[run++] = pos;
            if (pos < n && k[i] < limit && (pos + 1u == n || k[i + 1] >= limit)) { seg_start[run] = pos + 1u; *nseg_out = run; *nvalid_out = pos + 1u; }      // the last valid position closes the table
        }
    }
};
// one lane per sorted position: the point records in voxel order (the accumulation below then streams them instead
// of gathering 16-byte records all over the frame) and the voxel of every input point
struct d_point_gather {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* pts, const uint32_t* vals, const uint64_t* keys, int idxbits, const uint32_t* incl, uint32_t n, const DevCounters* dc, P16* spts,
                               int* pt_voxel) const {
        const uint32_t nv = dc->n_valid;
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const uint32_t idx = vals ? vals[i] : (uint32_t)(keys[i] & ((1ull << idxbits) - 1ull));
            if (i < nv) {
                const P16 p = load_point(pts, idx);
                *reinterpret_cast<float4*>(spts + i) = make_float4(p.x, p.y, p.z, __uint_as_float(p.rgba));
                pt_voxel[idx] = (int)(incl[i] - 1u);
            } else pt_voxel[idx] = -1;
        }
    }
};
// one lane per voxel: ordered sums over its points (input order), centroid, key
struct d_voxel_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* spts, const uint64_t* keys, int keyshift, const uint32_t* seg_start,
                                                    const DevCounters* dc, FrameArgs fa, const GridInfo* gp, uint32_t* vkey, uint32_t* vcount,
                                                    float* vf) const {
        const uint32_t V = dc->n_voxels;
        const int depth = gp->depth;
        for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
            const uint32_t s = seg_start[v], e = seg_start[v + 1];
            float sx = 0, sy = 0, sz = 0, sr = 0, sg = 0, sb = 0;
            for (uint32_t i = s; i < e; ++i) {
                P16 p = load_point(spts, i);
                float z = p.z; n_prelude(z, fa.fold_negative_z);
                sx += p.x; sy += p.y; sz += z;
                sr += (float)((p.rgba >> 16) & 255u); sg += (float)((p.rgba >> 8) & 255u); sb += (float)(p.rgba & 255u);
            }
            const uint32_t cnt = e - s;
            const float c = (float)cnt;
            float4* row = reinterpret_cast<float4*>(vf + (size_t)v * 12);
            row[0] = make_float4(sx / c, sy / c, sz / c, sr / c);
            row[1] = make_float4(sg / c, sb / c, 0.0f, 0.0f);
            row[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            vcount[v] = cnt;
            uint64_t code = keys[s] >> keyshift;
            if (fa.leaf_order == 1) code = (~code) & ((1ull << (3 * depth)) - 1ull);
            unsigned k[3];
            n_demorton(code, depth, k);
            vkey[v * 3] = k[0]; vkey[v * 3 + 1] = k[1]; vkey[v * 3 + 2] = k[2];
        }
    }
};
// d_point_gather + d_voxel_accum in one pass: a workgroup takes 256 consecutive voxels, whose points are one contiguous range of sorted positions; the
// range passes through LDS in chunks that all lanes gather together (one 16-byte record per lane and step, all in flight), then every lane continues
// the ordered sums of its voxel over the part of its segment that lies in the chunk.  Same additions in the same order as d_voxel_accum; the sorted
// copy of the frame (16 bytes per point written and read back) is gone.  The workgroups also mark the points behind the last valid one.
constexpr uint32_t VG_CHUNK = 1024;
struct d_voxel_gather_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* pts, const uint32_t* vals, const uint64_t* keys, int keyshift, const uint32_t* seg_start, uint32_t n,
                               const DevCounters* dc, FrameArgs fa, const GridInfo* gp, uint32_t* vkey, uint32_t* vcount,
                               float* vf, int* pt_voxel) const {
        __shared__ __attribute__((aligned(16))) uint4 buf[VG_CHUNK];
        __shared__ uint32_t ibuf[VG_CHUNK], vbuf[VG_CHUNK];
        const uint32_t V = dc->n_voxels, nv = dc->n_valid;
        const int depth = gp->depth;
        const uint64_t imask = (1ull << keyshift) - 1ull;
        const uint32_t tid = threadIdx.x;
        for (uint32_t i = nv + BIX * blockDim.x + tid; i < n; i += gridDim.x * blockDim.x) pt_voxel[vals ? vals[i] : (uint32_t)(keys[i] & imask)] = -1;
        for (uint32_t vb = BIX * 256u; vb < V; vb += gridDim.x * 256u) {
            const uint32_t v = vb + tid;
            const bool mine = v < V;
            const uint32_t s = mine ? seg_start[v] : 0u, e = mine ? seg_start[v + 1] : 0u;
            const uint32_t p0 = seg_start[vb], p1 = seg_start[vb + 256u < V ? vb + 256u : V];      // (uniform)
            float sx = 0, sy = 0, sz = 0, sr = 0, sg = 0, sb = 0;
            for (uint32_t c0 = p0; c0 < p1; c0 += VG_CHUNK) {
                const uint32_t c1 = p1 - c0 < VG_CHUNK ? p1 : c0 + VG_CHUNK;
                uint32_t idx[VG_CHUNK / 256];
        #pragma unroll
                for (uint32_t j = 0; j < VG_CHUNK / 256; ++j) { const uint32_t i = c0 + j * 256u + tid; const uint32_t ii = i < c1 ? i : c1 - 1u; idx[j] = vals ? vals[ii] : (uint32_t)(keys[ii] & imask); }
                uint4 q[VG_CHUNK / 256];
        #pragma unroll
                for (uint32_t j = 0; j < VG_CHUNK / 256; ++j) q[j] = reinterpret_cast<const uint4*>(pts)[idx[j]];
        #pragma unroll
                for (uint32_t j = 0; j < VG_CHUNK / 256; ++j) { buf[j * 256u + tid] = q[j]; ibuf[j * 256u + tid] = idx[j]; }
                __syncthreads();
                const uint32_t a = s > c0 ? s : c0, b = e < c1 ? e : c1;
                for (uint32_t i = a; i < b; ++i) {
                    const uint4 w = buf[i - c0];
                    float z = __uint_as_float(w.z); n_prelude(z, fa.fold_negative_z);
                    sx += __uint_as_float(w.x); sy += __uint_as_float(w.y); sz += z;
                    sr += (float)((w.w >> 16) & 255u); sg += (float)((w.w >> 8) & 255u); sb += (float)(w.w & 255u);
                    vbuf[i - c0] = v;
                }
                __syncthreads();
                // voxel-of-point: one lane per sorted POSITION, not per voxel -- the points of a voxel are short runs of consecutive input indices (a few pixels of a few
                // scanlines), so adjacent lanes store into the same lines; from the per-voxel loop above every lane of a store went to a line of its own (a scatter
                // costs the lines it touches: tools/ubench/ta_cost.hip)
        #pragma unroll
                for (uint32_t j = 0; j < VG_CHUNK / 256; ++j) { const uint32_t pp = j * 256u + tid; if (c0 + pp < c1) pt_voxel[ibuf[pp]] = (int)vbuf[pp]; }
                __syncthreads();
            }
            if (!mine) continue;
            const uint32_t cnt = e - s;
            const float c = (float)cnt;
            float4* row = reinterpret_cast<float4*>(vf + (size_t)v * 12);
            row[0] = make_float4(sx / c, sy / c, sz / c, sr / c);
            row[1] = make_float4(sg / c, sb / c, 0.0f, 0.0f);
            row[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            vcount[v] = cnt;
            uint64_t code = keys[s] >> keyshift;
            if (fa.leaf_order == 1) code = (~code) & ((1ull << (3 * depth)) - 1ull);
            unsigned k[3];
            n_demorton(code, depth, k);
            vkey[v * 3] = k[0]; vkey[v * 3 + 1] = k[1]; vkey[v * 3 + 2] = k[2];
        }
    }
};

// ------------------------------------------------------------------------------------------------
// stage 0 without sorting the points (round 5).  The stable radix sort above moves every point's 8-byte key through HBM six times (three passes) to
// make the points of a voxel contiguous.  What the leaf sums need is less -- which voxel a point falls into, the voxels in leaf (Morton) order, each
// voxel's points in input order -- and an RGB-D frame offers more: consecutive points are neighbouring pixels, so the 4096 points of a tile (four
// scanlines of a 1000-wide frame) fall into a few hundred voxels.  So the points are only grouped INSIDE a tile, in LDS, and what is sorted globally is the tiles' short lists:
//   d_tile_keys    one pass over the points, a workgroup per tile of VT_TILE consecutive points: cell key -> an LDS hash table of the tile's distinct
//                  voxels with their point counts (a run of equal keys inside a wave is one lookup by its first lane); per point the table entry and
//                  its rank among the tile's points of that entry; per distinct voxel of the tile one DESCRIPTOR (Morton code << tile bits | tile)
//   pair sort      of the descriptors (~450 per tile, ~110 k per 1M-point frame; the radix kernels above with the count on the device) on (code, tile): a voxel's
//                  descriptors end up in tile order, i.e. in input order
//   d_desc_part / d_desc_offsets / d_desc_apply   a new code starts a leaf (ordinal, key, seg_start); the running sum of the counts (they ride in the keys' low bits) is
//                  where a descriptor's points go: chunk totals, one workgroup's prefix over the chunks, per-descriptor results
//   d_tile_place   second pass over the per-point words: voxel of every point (pt_voxel) and the point's index into its leaf's list
//   d_voxel_list_accum   per leaf: the points gathered through LDS and added in list order -- the additions of d_voxel_accum, bit for bit
//   d_vox_table    the leaf keys into the voxel table of the neighbour search (after the host knows V; the sort path runs it too)
// No global atomic on the way (an agent-scope atomic is resolved beyond the XCD's L2: ~0.1 us of the chip per thousand -- the first version of this path,
// a global hash insert per run of points, spent 47 us per frame on them), 121-143 MB of HBM traffic per 1M-point frame where the sort path moves 185-200.
// Inside a tile the 256-point steps are separated by barriers, so a leaf's list comes out ascending except when two runs of one voxel meet in one
// step (a hole in a scanline, a surface that flips between two depth layers): d_tile_keys reports that per frame (vox_disorder), and the leaf kernel then
// passes an insertion sort over every list of the frame, in place.
// Falls back to the sort path, per context and sticky (the host reruns the stage): a tile with more than VT_ENT_MAX distinct voxels -- an unorganised
// cloud (BASELINE config 4) has no locality to use --, a leaf with more than VL_MAX_RUN points, a grid too deep for code + tile in 64 bits.
// ------------------------------------------------------------------------------------------------
#ifndef F3DS_VT_TILE
#define F3DS_VT_TILE 4096
#endif
constexpr uint32_t VT_TILE = F3DS_VT_TILE; // points per tile
constexpr uint32_t VT_TAB = VT_TILE / 2;   // LDS table entries per tile (12 bytes each)
constexpr int VT_CNT_BITS = 14;            // bits of a descriptor key that hold the entry's point count (<= VT_TILE)
static_assert(VT_TILE < (1u << VT_CNT_BITS), "a tile's point count must fit the count field");
constexpr uint32_t VT_ENT_MAX = VT_TAB * 5 / 8;      // distinct voxels a tile may hold (load factor 0.63).  The 1M-point bench frames: ~870 on average and ~1 300 at most per 8192 points, fewer per 4096
constexpr uint32_t VL_MAX_RUN = 256;       // points per leaf the per-lane insertion sort accepts
constexpr uint32_t VOX_NONE = 0xFFFFFFFFu;
// first lane of the run of equal, valid words that `lane` belongs to, and the run's length (uniform control flow: every lane calls this)
__device__ inline void run_of_lane(bool valid, uint32_t w0, uint32_t w1, bool* head, int* head_lane, uint32_t* run_len) {
    const int lane = lane_id();
    const uint32_t p0 = __shfl_up(w0, 1, 64), p1 = __shfl_up(w1, 1, 64);
    const bool pv = __shfl_up((int)valid, 1, 64) != 0;
    const bool h = valid && (lane == 0 || !pv || p0 != w0 || p1 != w1);
    const uint64_t hm = __ballot(h), vm = __ballot(valid);
    const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int hl = valid ? 63 - __builtin_clzll(hm & le) : lane;
    const uint64_t above = hl == 63 ? 0ull : ~((2ull << hl) - 1ull);
    const uint64_t stop = (hm | ~vm) & above;
    *head = h; *head_lane = hl; *run_len = (uint32_t)((stop ? __builtin_ctzll(stop) : 64) - hl);
}
struct d_tile_keys {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* pts, uint32_t n, FrameArgs fa, const GridInfo* gp, uint32_t* ploc, uint64_t* dkeys, uint32_t* dvals,
                               uint32_t dcap, int tile_bits, DevCounters* dc) const {
        __shared__ unsigned long long tkey[VT_TAB];
        __shared__ uint32_t tcnt[VT_TAB];
        __shared__ uint32_t tbits[2][VT_TAB / 32];      // entries touched in the current step (two bitmaps, used in turn)
        __shared__ uint32_t s_ent, s_base, s_over[2], s_dis;      // s_over: two flags used in turn (below)
        const GridInfo g = *gp;
        const uint64_t code_mask = (1ull << (3 * g.depth)) - 1ull;
        const int lane = lane_id();
        const uint32_t tid = threadIdx.x;
        const uint32_t ntiles = (n + VT_TILE - 1u) / VT_TILE;
        for (uint32_t tile = BIX; tile < ntiles; tile += gridDim.x) {
            for (uint32_t e = tid; e < VT_TAB; e += 256u) { tkey[e] = HASH_EMPTY; tcnt[e] = 0u; }
            if (tid < VT_TAB / 32u) { tbits[0][tid] = 0u; tbits[1][tid] = 0u; }
            if (tid == 0) { s_ent = 0u; s_over[0] = 0u; s_over[1] = 0u; s_dis = 0u; }
            __syncthreads();
            const uint32_t t0 = tile * VT_TILE, t1 = n - t0 < VT_TILE ? n : t0 + VT_TILE;
            // (the points of VT_PF steps are requested together: step by step the loop was one trip to memory per 256 points, 32 in a row per tile)
            constexpr uint32_t VT_PF = 4;
            // (the refusal flag the loop condition reads is the one the PREVIOUS iteration wrote -- complete behind that iteration's closing barrier; this iteration writes
            // the other one.  With one flag a fast wave could set it in the next iteration before a slow wave had evaluated the condition, and the slow wave would leave
            // the loop while the others wait at the step barrier: a divergent barrier.)
            uint32_t it4 = 0u;
            for (uint32_t base4 = t0; base4 < t1 && !s_over[(it4 + 1u) & 1u]; base4 += 256u * VT_PF, ++it4) {
              uint4 q[VT_PF];
        #pragma unroll
              for (uint32_t j = 0; j < VT_PF; ++j) { const uint32_t i = base4 + j * 256u + tid; q[j] = reinterpret_cast<const uint4*>(pts)[i < t1 ? i : t1 - 1u]; }
        #pragma unroll
              for (uint32_t j = 0; j < VT_PF; ++j) {
                const uint32_t base = base4 + j * 256u;
                if (base >= t1) break;      // (uniform)
                const uint32_t i = base + tid;
                const uint32_t step = (base - t0) >> 8;
                uint64_t pk = HASH_EMPTY;
                if (i < t1) {
                    float x = __uint_as_float(q[j].x), y = __uint_as_float(q[j].y), z = __uint_as_float(q[j].z);
                    n_prelude(z, fa.fold_negative_z);
                    if (n_finite3(x, y, z) && !g.empty) { unsigned k[3]; n_point_key(g, x, y, z, fa.use_transform, k); pk = n_pack_key(k[0], k[1], k[2]); }
                }
                const bool valid = pk != HASH_EMPTY;
                bool head; int hl; uint32_t len;
                run_of_lane(valid, (uint32_t)pk, (uint32_t)(pk >> 32), &head, &hl, &len);
                uint32_t ent = VOX_NONE, roff = 0;
                if (head) {
                    uint32_t e = (uint32_t)hash64(pk) & (VT_TAB - 1u);
                    for (uint32_t probes = 0; probes < VT_TAB; ++probes) {
                        const unsigned long long old = atomicCAS(&tkey[e], (unsigned long long)HASH_EMPTY, (unsigned long long)pk);
                        if (old == HASH_EMPTY) { if (atomicAdd(&s_ent, 1u) >= VT_ENT_MAX) s_over[it4 & 1u] = 1u; ent = e; break; }
                        if (old == pk) { ent = e; break; }
                        e = (e + 1u) & (VT_TAB - 1u);
                    }
                    if (ent != VOX_NONE) {
                        roff = atomicAdd(&tcnt[ent], len);
                        // a second run of this voxel in the SAME step may have taken its places before or after this one: the leaf's list is then no longer known to be ascending
                        const uint32_t bit = 1u << (ent & 31u);
                        if (atomicOr(&tbits[step & 1u][ent >> 5], bit) & bit) s_dis = 1u;
                    } else s_over[it4 & 1u] = 1u;
                }
                if (tid < VT_TAB / 32u) tbits[(step + 1u) & 1u][tid] = 0u;      // (the other step's bitmap: idle during this step)
                ent = __shfl(ent, hl, 64); roff = __shfl(roff, hl, 64);
                if (i < t1) ploc[i] = (valid && ent != VOX_NONE) ? (ent << 16) | (roff + (uint32_t)(lane - hl)) : VOX_NONE;
                __syncthreads();      // (steps in order: a leaf's list comes out ascending)
              }
            }
            __syncthreads();
            if (tid == 0) { atomicMax(&dc->vox_max_tile, s_ent); if (s_dis) dc->vox_disorder = 1u; }
            if (s_over[0] | s_over[1]) { if (tid == 0) { dc->error = F3DS_ERR_UNSUPPORTED; dc->ev_overflow = F3DS_OVF_TILE_VOXELS; } return; }
            // ---- one descriptor per live entry: (code << tile_bits | tile, tile * VT_TAB + entry), its count beside it
            if (tid == 0) s_base = s_ent ? atomicAdd(&dc->seg_count, s_ent) : 0u;      // (one atomic per tile on the frame's descriptor counter)
            __syncthreads();
            const uint32_t dbase = s_base;
            // (the order of a tile's descriptors among themselves is irrelevant -- their codes differ and the sort puts them where they belong --, so a wave takes
            // its places with one LDS atomic per round instead of a workgroup scan)
            if (tid == 0) s_ent = 0u;
            __syncthreads();
            for (uint32_t e0 = 0; e0 < VT_TAB; e0 += 256u) {
                const uint32_t e = e0 + tid;
                const unsigned long long pk = tkey[e];
                const bool live = pk != HASH_EMPTY;
                const uint64_t lm = __ballot(live);
                if (!lm) continue;
                uint32_t wb = 0;
                if (lane == __builtin_ctzll(lm)) wb = atomicAdd(&s_ent, (uint32_t)__popcll(lm));
                wb = __shfl(wb, __builtin_ctzll(lm), 64);
                if (live) {
                    const uint32_t d = dbase + wb + (uint32_t)__popcll(lm & lanemask_lt());
                    if (d < dcap) {
                        uint64_t code = n_morton((unsigned)(pk >> 42) & 0x1FFFFFu, (unsigned)(pk >> 21) & 0x1FFFFFu, (unsigned)pk & 0x1FFFFFu, g.depth);
                        if (fa.leaf_order == 1) code = (~code) & code_mask;
                        dkeys[d] = (((code << tile_bits) | (uint64_t)tile) << VT_CNT_BITS) | (uint64_t)tcnt[e];      // (the count rides below the sorted bits: the descriptor pass needs no second array)
                        dvals[d] = tile * VT_TAB + e;
                    } else { dc->error = F3DS_ERR_UNSUPPORTED; dc->ev_overflow = F3DS_OVF_TILE_VOXELS; }
                }
            }
            __syncthreads();
        }
    }
};
// The sorted descriptors: a new code starts a leaf (ordinal, key, seg_start); the running sum of the counts is where a descriptor's points go in the leaf lists.
// Per (tile, entry) both numbers for d_tile_place.  Three small launches -- per chunk of DS_CHUNK descriptors the number of leaf heads and of points (d_desc_part),
// one workgroup turns the chunk totals into offsets (d_desc_offsets), every chunk writes its descriptors' results (d_desc_apply) -- so that no frame waits for one
// workgroup to walk 110 k descriptors (1.3 ms on every call's critical path when this was one kernel).
constexpr uint32_t DS_IT = 8;                 // consecutive descriptors per thread
constexpr uint32_t DS_CHUNK = 256u * DS_IT;   // descriptors per workgroup
struct DescThread { uint64_t code[DS_IT]; uint32_t te[DS_IT], cnt[DS_IT]; uint32_t headmask, nheads, npts; };
__device__ inline void desc_load(const uint64_t* dkeys, const uint32_t* dvals, uint32_t D, int tile_bits, uint32_t db, DescThread& t, bool want_te) {
    const int sh = tile_bits + VT_CNT_BITS;
    uint64_t prev = (db > 0u && db - 1u < D) ? dkeys[db - 1u] >> sh : ~0ull;
#pragma unroll
    for (uint32_t k = 0; k < DS_IT; ++k) {
        const uint32_t d = db + k;
        const uint64_t key = d < D ? dkeys[d] : 0ull;
        t.code[k] = key >> sh; t.cnt[k] = d < D ? (uint32_t)key & ((1u << VT_CNT_BITS) - 1u) : 0u;
        t.te[k] = (want_te && d < D) ? dvals[d] : 0u;
    }
    t.headmask = 0u; t.nheads = 0u; t.npts = 0u;
#pragma unroll
    for (uint32_t k = 0; k < DS_IT; ++k) {
        const uint32_t d = db + k;
        const bool head = d < D && (d == 0u || prev != t.code[k]);
        prev = t.code[k];
        if (head) { t.headmask |= 1u << k; t.nheads++; }
        t.npts += t.cnt[k];
    }
}
// exclusive prefix of (a, b) over the 256 threads of the workgroup (two barriers)
__device__ inline void block_excl_scan2(uint32_t a, uint32_t b, uint32_t* ea, uint32_t* eb, uint32_t* ta, uint32_t* tb) {
    __shared__ uint32_t s_a[4], s_b[4];
    const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x >> 6;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) { const uint32_t x = __shfl_up(ia, k, 64), y = __shfl_up(ib, k, 64); if ((int)lane >= k) { ia += x; ib += y; } }
    __syncthreads();
    if (lane == 63u) { s_a[w] = ia; s_b[w] = ib; }
    __syncthreads();
    uint32_t ba = 0, bb = 0, sa = 0, sb = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) { if (k < w) { ba += s_a[k]; bb += s_b[k]; } sa += s_a[k]; sb += s_b[k]; }
    *ea = ba + ia - a; *eb = bb + ib - b; *ta = sa; *tb = sb;
}
struct d_desc_part {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* dkeys, uint32_t dcap, int tile_bits, uint32_t* part, const DevCounters* dc) const {
        if (dc->ev_overflow) return;
        const uint32_t D = dc->seg_count < dcap ? dc->seg_count : dcap;
        const uint32_t nchunks = (dcap + DS_CHUNK - 1u) / DS_CHUNK;
        for (uint32_t b = BIX; b < nchunks; b += gridDim.x) {
            DescThread t;
            desc_load(dkeys, nullptr, D, tile_bits, b * DS_CHUNK + threadIdx.x * DS_IT, t, false);
            uint32_t eh, ec, th, tc;
            block_excl_scan2(t.nheads, t.npts, &eh, &ec, &th, &tc);
            if (threadIdx.x == 0) { part[2u * b] = th; part[2u * b + 1u] = tc; }
            __syncthreads();
        }
    }
};
struct d_desc_offsets {
    static constexpr bool LATENCY_KERNEL = true;
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* part, uint32_t dcap, uint32_t capV, uint32_t* seg_start, DevCounters* dc) const {
        if (BIX || dc->ev_overflow) return;
        const uint32_t nchunks = (dcap + DS_CHUNK - 1u) / DS_CHUNK;
        uint32_t ch = 0, cc = 0;
        for (uint32_t b0 = 0; b0 < nchunks; b0 += 256u) {
            const uint32_t b = b0 + threadIdx.x;
            const uint32_t h = b < nchunks ? part[2u * b] : 0u, c = b < nchunks ? part[2u * b + 1u] : 0u;
            uint32_t eh, ec, th, tc;
            block_excl_scan2(h, c, &eh, &ec, &th, &tc);
            if (b < nchunks) { part[2u * b] = ch + eh; part[2u * b + 1u] = cc + ec; }
            ch += th; cc += tc;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            dc->n_voxels = ch; dc->n_valid = cc;
            if (ch <= capV) seg_start[ch] = cc; else { dc->error = F3DS_ERR_UNSUPPORTED; dc->ev_overflow = F3DS_OVF_TILE_VOXELS; }
        }
    }
};
struct d_desc_apply {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* dkeys, const uint32_t* dvals, uint32_t dcap, uint32_t capV, int tile_bits, FrameArgs fa, const GridInfo* gp,
                               const uint32_t* part, uint2* bo_te, uint32_t* seg_start, uint32_t* vkey, const DevCounters* dc) const {
        if (dc->ev_overflow) return;
        const uint32_t D = dc->seg_count < dcap ? dc->seg_count : dcap;
        const int depth = gp->depth;
        const uint32_t nchunks = (D + DS_CHUNK - 1u) / DS_CHUNK;
        for (uint32_t b = BIX; b < nchunks; b += gridDim.x) {
            const uint32_t db = b * DS_CHUNK + threadIdx.x * DS_IT;
            DescThread t;
            desc_load(dkeys, dvals, D, tile_bits, db, t, true);
            uint32_t eh, ec, th, tc;
            block_excl_scan2(t.nheads, t.npts, &eh, &ec, &th, &tc);
            uint32_t ord = part[2u * b] + eh;          // leaves before this thread's first descriptor
            uint32_t pos = part[2u * b + 1u] + ec;     // points before it
        #pragma unroll
            for (uint32_t k = 0; k < DS_IT; ++k) {
                if (db + k >= D) break;
                if (t.headmask & (1u << k)) {
                    if (ord < capV) {
                        seg_start[ord] = pos;
                        uint64_t c2 = t.code[k];
                        if (fa.leaf_order == 1) c2 = (~c2) & ((1ull << (3 * depth)) - 1ull);
                        unsigned k3[3];
                        n_demorton(c2, depth, k3);
                        vkey[ord * 3] = k3[0]; vkey[ord * 3 + 1] = k3[1]; vkey[ord * 3 + 2] = k3[2];
                    }
                    ord++;
                }
                bo_te[t.te[k]] = make_uint2(pos, ord - 1u);
                pos += t.cnt[k];
            }
            __syncthreads();
        }
    }
};
// second pass over the per-point words, a workgroup per tile: the tile's (list base, leaf ordinal) table comes into LDS in one coalesced read, then every point finds its
// list position and its voxel there (gathered from global memory per point the two tables -- 4 MB per frame -- did not stay in L2 beside 23 other frames')
struct d_tile_place {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint32_t* ploc, uint32_t n, const uint2* bo_te, uint32_t* list, int* pt_voxel, const DevCounters* dc) const {
        __shared__ uint2 tab[VT_TAB];
        if (dc->ev_overflow) return;      // (the host reruns the stage on the sort path, which writes pt_voxel itself)
        const uint32_t ntiles = (n + VT_TILE - 1u) / VT_TILE;
        for (uint32_t tile = BIX; tile < ntiles; tile += gridDim.x) {
            const uint32_t t0 = tile * VT_TILE, t1 = n - t0 < VT_TILE ? n : t0 + VT_TILE;
            constexpr uint32_t PF = 4;
            uint32_t pl[PF];
    #pragma unroll
            for (uint32_t j = 0; j < PF; ++j) { const uint32_t i = t0 + j * 256u + threadIdx.x; pl[j] = i < t1 ? ploc[i] : VOX_NONE; }      // (the first words are on their way while the table arrives)
            __syncthreads();              // (the previous tile's readers are done)
            for (uint32_t e = threadIdx.x; e < VT_TAB; e += 256u) tab[e] = bo_te[(size_t)tile * VT_TAB + e];
            __syncthreads();
            for (uint32_t i0 = t0; i0 < t1; i0 += 256u * PF) {
                uint32_t nx[PF];
    #pragma unroll
                for (uint32_t j = 0; j < PF; ++j) { const uint32_t i = i0 + (PF + j) * 256u + threadIdx.x; nx[j] = i < t1 ? ploc[i] : VOX_NONE; }      // next round's words
    #pragma unroll
                for (uint32_t j = 0; j < PF; ++j) {
                    const uint32_t i = i0 + j * 256u + threadIdx.x;
                    if (i >= t1) continue;
                    if (pl[j] == VOX_NONE) { pt_voxel[i] = -1; continue; }
                    const uint2 bo = tab[pl[j] >> 16];
                    list[bo.x + (pl[j] & 0xFFFFu)] = i;
                    pt_voxel[i] = (int)bo.y;
                }
    #pragma unroll
                for (uint32_t j = 0; j < PF; ++j) pl[j] = nx[j];
            }
        }
    }
};
// leaf keys -> voxel table of the neighbour search (vt_* / bt_* above), on both stage-0 paths: they leave vkey in leaf order.  Block layout: a lane per leaf; a leaf whose block key
// differs from its predecessor's is the HEAD of its block's run and gives the entry its base ordinal; the cell bits of the run are ORed along the lanes of a wave (a suffix scan cut at
// the heads, no LDS) and the first lane of every piece of a run -- the head, or lane 0 where a run continues across a wave border -- clears them in the entry's mask with one atomic AND.
// So a frame of 77 k leaves costs ~7 k compare-and-swaps where an entry per voxel cost 77 k.  On the tile path ONE workgroup builds a frame's table: its waves share a compute unit, so
// WORKGROUP-scope atomics -- resolved in the XCD's L2, not beyond it -- are all the coherence the build needs; the readers come in later kernels.  The sort path (a lone frame: nothing
// else to fill the chip with) spreads the leaves over several workgroups, and its atomics are agent-scope then.
struct d_vox_table {
    static constexpr bool LATENCY_KERNEL = true;
    static constexpr int BLOCK = 1024;
    __device__ void operator()(const uint32_t* vkey, uint32_t V, const GridInfo* gp, uint64_t* hkeys, uint32_t* hvals, uint32_t hmask) const {
        const bool blocks = vt_blocks(gp->depth);
        const bool agent = gridDim.x > 1u;
        BtEntry* const tab = reinterpret_cast<BtEntry*>(hkeys);
        const uint32_t lane = (uint32_t)lane_id();
        constexpr uint32_t PF = 4;      // keys per thread requested together
        for (uint32_t s0 = BIX * (BLOCK * PF); s0 < V; s0 += gridDim.x * (BLOCK * PF)) {      // (uniform: every lane takes part in the shuffles)
            unsigned k[PF][3]; uint32_t prev[PF];
    #pragma unroll
            for (uint32_t j = 0; j < PF; ++j) { const uint32_t v = s0 + j * BLOCK + threadIdx.x, vv = v < V ? v : 0u; k[j][0] = vkey[vv * 3]; k[j][1] = vkey[vv * 3 + 1]; k[j][2] = vkey[vv * 3 + 2]; }
            if (!blocks) {
    #pragma unroll
                for (uint32_t j = 0; j < PF; ++j) { const uint32_t v = s0 + j * BLOCK + threadIdx.x; if (v < V) vt_insert(hkeys, hvals, hmask, agent, k[j][0], k[j][1], k[j][2], v); }
                continue;
            }
    #pragma unroll
            for (uint32_t j = 0; j < PF; ++j) {      // lane 0 of a wave: the block of the leaf before the wave's first
                const uint32_t v = s0 + j * BLOCK + threadIdx.x;
                prev[j] = lane == 0u && v > 0u && v < V ? n_block_key(vkey[(v - 1u) * 3], vkey[(v - 1u) * 3 + 1], vkey[(v - 1u) * 3 + 2]) : BT_EMPTY;
            }
    #pragma unroll
            for (uint32_t j = 0; j < PF; ++j) {
                const uint32_t v = s0 + j * BLOCK + threadIdx.x;
                const bool in = v < V;
                const uint32_t bk = n_block_key(k[j][0], k[j][1], k[j][2]);
                const uint32_t up = __shfl_up(bk, 1, 64);
                const bool head = in && bk != (lane ? up : prev[j]);
                const uint64_t cuts = __ballot(head || !in);            // lanes that start a piece (lane 0 always does)
                const uint64_t ahead = (cuts >> 1) >> lane;             // bit d-1: lane + d starts a piece
                unsigned long long m = in ? 1ull << n_block_cell(k[j][0], k[j][1], k[j][2]) : 0ull;
    #pragma unroll
                for (uint32_t d = 1; d < 64u; d <<= 1) {                // m: OR over the lanes from this one to the end of its piece
                    const unsigned long long o = __shfl_down(m, d, 64);
                    if (lane + d < 64u && !(ahead & ((1ull << d) - 1ull))) m |= o;
                }
                if (in && (head || lane == 0u)) {
                    BtEntry* const e = bt_entry(tab, hmask, agent, bk);
                    if (agent) __hip_atomic_fetch_and(&e->vacant, ~m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else __hip_atomic_fetch_and(&e->vacant, ~m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (head) e->base = v;
                }
            }
        }
    }
};
struct d_voxel_list_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* pts, uint32_t* list, const uint32_t* seg_start, FrameArgs fa, float* vf, uint32_t* vcount, DevCounters* dc, uint32_t capV) const {
        __shared__ __attribute__((aligned(16))) uint4 buf[VG_CHUNK];
        if (dc->ev_overflow) return;
        const uint32_t V = dc->n_voxels < capV ? dc->n_voxels : capV;
        const bool disorder = dc->vox_disorder != 0u;      // (some list of the frame may not be ascending: every lane then passes an insertion sort over its list, in place)
        const uint32_t tid = threadIdx.x;
        for (uint32_t vb = BIX * 256u; vb < V; vb += gridDim.x * 256u) {
            const uint32_t v = vb + tid;
            const bool mine = v < V;
            const uint32_t s = mine ? seg_start[v] : 0u, e = mine ? seg_start[v + 1] : 0u;
            const uint32_t p0 = seg_start[vb], p1 = seg_start[vb + 256u < V ? vb + 256u : V];      // (uniform)
            if (__syncthreads_or(e - s > VL_MAX_RUN)) { if (tid == 0) { dc->error = F3DS_ERR_UNSUPPORTED; dc->ev_overflow = F3DS_OVF_DENSE_VOXEL; } return; }      // a dense voxel: sort path (host)
            if (disorder) {
                for (uint32_t a = s + 1u; a < e; ++a) {
                    const uint32_t x = list[a];
                    uint32_t b = a;
                    while (b > s && list[b - 1u] > x) { list[b] = list[b - 1u]; --b; }
                    if (b != a) list[b] = x;
                }
                __threadfence_block();
                __syncthreads();
            }
            // ---- the points pass through LDS in chunks all lanes gather together; every lane continues its leaf's ordered sums (as d_voxel_gather_accum)
            float sx = 0, sy = 0, sz = 0, sr = 0, sg = 0, sb = 0;
            for (uint32_t c0 = p0; c0 < p1; c0 += VG_CHUNK) {
                const uint32_t c1 = p1 - c0 < VG_CHUNK ? p1 : c0 + VG_CHUNK;
                uint32_t idx[VG_CHUNK / 256];
        #pragma unroll
                for (uint32_t j = 0; j < VG_CHUNK / 256; ++j) { const uint32_t i = c0 + j * 256u + tid; idx[j] = list[i < c1 ? i : c1 - 1u]; }
                uint4 q[VG_CHUNK / 256];
        #pragma unroll
                for (uint32_t j = 0; j < VG_CHUNK / 256; ++j) q[j] = reinterpret_cast<const uint4*>(pts)[idx[j]];
        #pragma unroll
                for (uint32_t j = 0; j < VG_CHUNK / 256; ++j) buf[j * 256u + tid] = q[j];
                __syncthreads();
                const uint32_t a = s > c0 ? s : c0, b = e < c1 ? e : c1;
                for (uint32_t i = a; i < b; ++i) {
                    const uint4 w = buf[i - c0];
                    float z = __uint_as_float(w.z); n_prelude(z, fa.fold_negative_z);
                    sx += __uint_as_float(w.x); sy += __uint_as_float(w.y); sz += z;
                    sr += (float)((w.w >> 16) & 255u); sg += (float)((w.w >> 8) & 255u); sb += (float)(w.w & 255u);
                }
                __syncthreads();
            }
            if (!mine) continue;
            const float c = (float)(e - s);
            vcount[v] = e - s;
            float4* row = reinterpret_cast<float4*>(vf + (size_t)v * 12);
            row[0] = make_float4(sx / c, sy / c, sz / c, sr / c);
            row[1] = make_float4(sg / c, sb / c, 0.0f, 0.0f);
            row[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
};
__device__ inline int hash_find(const uint64_t* hkeys, const uint32_t* hvals, uint32_t hmask, uint64_t pk) {
    uint32_t h = (uint32_t)hash64(pk) & hmask;
    for (;;) {
        uint64_t k = hkeys[h];
        if (k == pk) return (int)hvals[h];
        if (k == HASH_EMPTY) return -1;
        h = (h + 1u) & hmask;
    }
}

// ------------------------------------------------------------------------------------------------
// stage 1: neighbour table and voxel normals
// ------------------------------------------------------------------------------------------------
struct d_neighbors {
    static constexpr int BLOCK = 256;
    // What a gather or scatter costs a compute unit is the number of distinct lines it touches (tools/ubench/ta_cost.hip: ~2.4 cycles per line from L2, a full
    // 256-byte run 8): the kernel ran at exactly that rate, and a third of its lines were the slot-major stores (27 consecutive lanes = 27 rows of nbrT).  A
    // workgroup now takes 64 consecutive voxels, keeps their 27 x 64 results in LDS and writes the slot-major rows as 256-byte runs.
    // The lines left were the probes, one per lane: they now go to the 4x4x4 block table (bt_find), where the ~2.4 voxels of a wave ask for about ten entries between them.
    __device__ void operator()(const uint32_t* vkey, const DevCounters* dc, const GridInfo* gp, int leaf_order, const uint64_t* hkeys,
                                                  const uint32_t* hvals, uint32_t hmask, int* nbr, int* nbrT) const {
        __shared__ int tr[27][65];      // (65: consecutive slots of one voxel fall into different banks)
        const uint32_t V = dc->n_voxels;
        const unsigned max_key = gp->max_key;
        const bool blocks = vt_blocks(gp->depth);
        const BtEntry* const tab = reinterpret_cast<const BtEntry*>(hkeys);
        for (uint32_t vb = BIX * 64u; vb < V; vb += gridDim.x * 64u) {
            const uint32_t nv = V - vb < 64u ? V - vb : 64u, np = nv * 27u;
            for (uint32_t tl = threadIdx.x; tl < np; tl += 256u) {
                const uint32_t vl = tl / 27u, s = tl - vl * 27u, v = vb + vl;
                const int d[3] = {(int)(s / 9u) - 1, (int)((s / 3u) % 3u) - 1, (int)(s % 3u) - 1};
                bool ok = true; unsigned k[3];
                for (int a = 0; a < 3; ++a) {
                    long long q = (long long)vkey[v * 3 + a] + d[a];
                    if (q < 0 || q > (long long)max_key) ok = false;
                    k[a] = (unsigned)q;
                }
                const int u = !ok ? -1 : blocks ? bt_find(tab, hmask, leaf_order, k[0], k[1], k[2]) : vt_find(hkeys, hvals, hmask, k[0], k[1], k[2]);
                nbr[(size_t)vb * 27u + tl] = u;              // row-major: a voxel's 27 slots together (normals, adjacency)
                tr[s][vl] = u;
            }
            __syncthreads();
            for (uint32_t r = threadIdx.x; r < 27u * 64u; r += 256u) {
                const uint32_t s = r >> 6, vl = r & 63u;
                if (vl < nv) nbrT[(size_t)s * V + vb + vl] = tr[s][vl];      // slot-major: coalesced across consecutive voxels (sweeps)
            }
            __syncthreads();
        }
    }
};
// Voxel normals (computeVoxelData): every voxel accumulates, in list order and with duplicates, itself,
// each neighbour and each neighbour's neighbours -- up to 757 centroid reads and the same number of
// neighbour-table reads per voxel.  A workgroup takes 128 leaf-order-consecutive voxels (a compact
// patch of the surface), builds in LDS (1) a hash of every voxel in the patch's two-ring, (2) their
// centroids, (3) the neighbour rows of the one-ring as 16-bit LDS slot numbers, and then runs the
// 757-step ordered accumulation entirely out of LDS.  HBM/L2 sees each needed row once per workgroup
// instead of once per use.  Patches whose two-ring does not fit fall back to direct global gathers.
constexpr int NT_TILE = 128;        // voxels per workgroup
constexpr int NT_HCAP = 2048;       // hash entries
// Table sizes: a tile of 128 leaf-order-consecutive voxels of a surface has ~170-250 voxels in its one-ring and ~360-520 in its two-ring (profiles/r3_merge_prof.txt);
// 448 / 896 keep the workgroup at 55 KB of LDS (72 KB with the 512 / 1 536 of round 2), which is what lets it share a unit with a merge workgroup (d_normals_t below).
// A tile that needs more takes the global-memory path of the kernel (and of the sweeps): slower, same results.
#ifndef F3DS_NT_SLOTS
#define F3DS_NT_SLOTS 896
#endif
#ifndef F3DS_NT_RING1
#define F3DS_NT_RING1 448
#endif
constexpr int NT_SLOTS = F3DS_NT_SLOTS;      // distinct voxels in the two-ring union
constexpr int NT_RING1 = F3DS_NT_RING1;      // distinct voxels in the one-ring union
// whether slot sl (counted from 0) lies in a tile's table: a ring of exactly NT_RING1 / NT_SLOTS voxels fits, one more makes the tile overflow
__host__ __device__ constexpr bool nt_ring1_holds(uint32_t sl) { return sl < (uint32_t)NT_RING1; }
__host__ __device__ constexpr bool nt_slots_hold(uint32_t sl) { return sl < (uint32_t)NT_SLOTS; }
constexpr uint16_t NT_NONE = 0xFFFFu;
constexpr uint32_t NT_HNONE = 0x3FFu;              // slot field of a tile-hash entry that has not been numbered yet (NT_SLOTS < 1023)
constexpr uint32_t NT_ORD_LIMIT = (1u << 22) - 2u; // voxel ordinals + 1 must fit the 22 bits above the slot field
static_assert(NT_SLOTS < 1023, "slot numbers share a word with the ordinal");
constexpr uint16_t NT_ZERO = NT_SLOTS;     // slot that holds (0,0,0): an absent neighbour adds exact zeros
constexpr uint32_t SW_TILE_NONE = 0xFFFFFFFFu;     // tile_n1 of a tile whose one-ring did not fit: the sweeps gather from global memory there
constexpr int SW_SLOT_BITS = 9;                    // a list position (<= NT_RING1 = "no neighbour") per neighbour ...
constexpr int SW_SLOT_WORDS = (27 * SW_SLOT_BITS + 31) / 32;      // ... 27 of them bit-packed into 8 words per voxel (round 3: two per word, 14 words -- the sweeps' stencil kernels read them 3 x 16 times per frame)
static_assert(NT_RING1 < (1 << SW_SLOT_BITS), "a list position must fit its bit field");
__device__ __forceinline__ void sw_slots_pack(const uint32_t pos[27], uint32_t w[SW_SLOT_WORDS]) {
#pragma unroll
    for (int k = 0; k < SW_SLOT_WORDS; ++k) w[k] = 0u;
#pragma unroll
    for (int j = 0; j < 27; ++j) {
        const int bit = j * SW_SLOT_BITS, wi = bit >> 5, sh = bit & 31;
        w[wi] |= pos[j] << sh;
        if (sh + SW_SLOT_BITS > 32) w[wi + 1] |= pos[j] >> (32 - sh);
    }
}
__device__ __forceinline__ uint32_t sw_slot(const uint32_t w[SW_SLOT_WORDS], int j) {      // (j is a compile-time constant at every call: unrolled loops)
    const int bit = j * SW_SLOT_BITS, wi = bit >> 5, sh = bit & 31;
    uint32_t x = w[wi] >> sh;
    if (sh + SW_SLOT_BITS > 32) x |= w[wi + 1] << (32 - sh);
    return x & ((1u << SW_SLOT_BITS) - 1u);
}
__device__ inline void cov_add(float acc[9], const float4 q) {
    acc[0] += q.x * q.x; acc[1] += q.x * q.y; acc[2] += q.x * q.z;
    acc[3] += q.y * q.y; acc[4] += q.y * q.z; acc[5] += q.z * q.z;
    acc[6] += q.x; acc[7] += q.y; acc[8] += q.z;
}
__device__ __forceinline__ uint32_t lds_addr(const float* p);
// The same nine sums on register pairs (v_pk_mul_f32 / v_pk_add_f32: two IEEE single operations per instruction, each rounded as the
// scalar one -- results are bit-identical to cov_add): (xx, xy), (xz, yz), (zz, yy), (x, y) and z.  A centroid is kept in LDS as (x, y, z, y) and
// comes out as one 16-byte read, so (x, y) and (z, y) are aligned register pairs, the broadcasts are operand selects and no pair has to be built:
// 8 vector instructions per centroid where the compiler's own pairing of cov_add needs 12.6 (it forms (y, z) and (xx, x) pairs with register moves).
// One wave per SIMD saturates its vector issue in these sums (two accumulating waves on one SIMD take twice as long, DESIGN.md 4b): instructions are time.
typedef float f3ds_f2 __attribute__((ext_vector_type(2)));
typedef float f3ds_f4 __attribute__((ext_vector_type(4)));
struct CovPairs {
    f3ds_f2 a0, a1, a2, a3; float sz;
    __device__ void zero() { a0 = a1 = a2 = a3 = f3ds_f2{0.0f, 0.0f}; sz = 0.0f; }
    __device__ void add(const f3ds_f4 q) {      // q = (x, y, z, y)
        const f3ds_f2 xy = q.xy, zy = q.zw;
        a0 += xy * q.xx;
        a1 += xy * q.zz;
        a2 += zy * zy;
        a3 += xy;
        sz += q.z;
    }
    __device__ void store(float acc[9]) const { acc[0] = a0.x; acc[1] = a0.y; acc[2] = a1.x; acc[3] = a2.y; acc[4] = a1.y; acc[5] = a2.x; acc[6] = a3.x; acc[7] = a3.y; acc[8] = sz; }
};
// NTT threads build a tile's tables: 384 for a lone frame or a small call (the shortest kernel), 256 for the calls of a batch pipeline -- four waves of <= 256 VGPRs and
// 55 KB of LDS are what fits on a compute unit beside a 4-wave merge workgroup of another call (one wave and ~250 VGPRs per SIMD, ~103 KB), and the merge loops of
// the calls in flight sit on most units most of the time: +6 % on the bench, DESIGN.md 4i.  (Six waves never fit there: two of them share a SIMD.)
template <int NTT>
struct d_normals_t {
    static constexpr int BLOCK = NTT;
    static constexpr int PT = (NT_RING1 * 27 + NTT - 1) / NTT;          // two-ring table words per thread
    static constexpr int PR = PT % 9 == 0 ? 9 : (PT % 8 == 0 ? 8 : (PT % 6 == 0 ? 6 : (PT % 4 == 0 ? 4 : (PT % 3 == 0 ? 3 : (PT % 2 == 0 ? 2 : 1)))));      // hash probes of a thread that are read together
#ifndef F3DS_NORMALS_WPS
#define F3DS_NORMALS_WPS 3      // two six-wave workgroups per unit (LDS allows no more): 168 VGPRs
#endif
#ifndef F3DS_NORMALS_WPS256
#define F3DS_NORMALS_WPS256 3      // (<= 168 VGPRs, 40 of them spilled to scratch: three four-wave workgroups per unit since the tile hash is one word per entry; 11.1 -> 8.5 ms per 192-frame launch, +3.9 % on the bench over three alternating runs; =2: 231 VGPRs, two per unit)
#endif
    static constexpr int WAVES_PER_SIMD = NTT > 256 ? F3DS_NORMALS_WPS : F3DS_NORMALS_WPS256;
    __device__ static uint32_t hslot(uint32_t ord) { return (ord * 2654435761u) >> 21; }       // 11 bits
    __device__ void one_tile(const uint32_t bix, float* vf, const int* nbr, const DevCounters* dc, uint32_t* tile_n1, uint32_t* tile_ord, uint32_t* tile_slots, uint32_t holes) const {
        __shared__ uint32_t hw[NT_HCAP];               // (ordinal + 1) << 10 | slot (NT_HNONE = not numbered yet), 0 = empty.  One word per entry instead of a key word and a 16-bit
                                                       // value: 50.3 KB of LDS per workgroup instead of 54.3, i.e. THREE workgroups per compute unit instead of two (and two beside a 52 KB merge workgroup)
        __shared__ __attribute__((aligned(16))) float4 xyz[NT_SLOTS + 1];
        __shared__ uint32_t sord[NT_SLOTS];
        __shared__ uint16_t rows[NT_RING1 + 1][28];    // 27 slot numbers (NT_ZERO = absent) + how many are present; row NT_RING1: nobody (what an absent one-ring neighbour reads)
        __shared__ uint32_t n_slots, overflow;
        __shared__ uint16_t tme[NT_TILE];              // one-ring slot of every voxel of the tile
        // the rows hold slot numbers + KB, KB = LDS address of the centroid table / 16: shifted left by four such an entry IS the LDS address of the centroid (4, below)
        const uint32_t KB = lds_addr(reinterpret_cast<const float*>(xyz)) >> 4;
        const uint32_t V = dc->n_voxels;
        const uint32_t v0 = bix * NT_TILE;
        if (v0 >= V) return;
        const uint32_t nt = V - v0 < (uint32_t)NT_TILE ? V - v0 : (uint32_t)NT_TILE;      // voxels of this tile
#ifdef F3DS_MERGE_PROF
        unsigned long long tp[8], tq = __builtin_amdgcn_s_memtime(); int tpi = 0;
        unsigned long long tx_[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tq2 = tq;      // finer probes inside the table phases
#define NPH() do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); tp[tpi++] = n_ - tq; tq = n_; } while (0)
#define NPX(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); tx_[i] = n_ - tq2; tq2 = n_; } while (0)
#else
#define NPH() do { } while (0)
#define NPX(i) do { } while (0)
#endif
        for (int i = threadIdx.x; i < NT_HCAP; i += NTT) hw[i] = 0u;
        if (threadIdx.x == 0) { n_slots = 0; overflow = V >= NT_ORD_LIMIT ? 1u : 0u; xyz[NT_ZERO] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }      // (more than 4 M voxels: ordinals do not fit the packed word, every tile takes the global path)
        __syncthreads();
        // an insert whose first probe is already read (`old` = hkey[h], possibly stale: a slot only ever goes from empty to one key, so a stale "empty" is settled by the
        // compare-and-swap and everything else is final).  The callers read the first probes of a run of keys together: one trip to LDS instead of one per key.  Nine in ten
        // inserts find their key already there (a voxel is the neighbour of up to 27 others): a plain read answers those, and only an empty slot costs an LDS atomic.
        auto insert_key_from = [&](uint32_t ord, uint32_t h, uint32_t old) -> uint32_t {      // returns the entry the key sits in
            for (int probes = 0; probes < NT_HCAP; ++probes) {
                if (old == 0u) old = atomicCAS(&hw[h], 0u, ((ord + 1u) << 10) | NT_HNONE);
                if (old == 0u || (old >> 10) == ord + 1u) return h;
                h = (h + 1u) & (NT_HCAP - 1);
                old = hw[h];
            }
            overflow = 1;
            return 0u;
        };
        auto lookup = [&](uint32_t ord) -> uint16_t {
            uint32_t h = hslot(ord);
            for (;;) {
                const uint32_t k = hw[h];
                if ((k >> 10) == ord + 1u) return (k & NT_HNONE) == NT_HNONE ? NT_NONE : (uint16_t)(k & NT_HNONE);
                if (k == 0u) return NT_NONE;
                h = (h + 1u) & (NT_HCAP - 1);
            }
        };
        NPH();
        // (1) one-ring keys: all of a thread's table words are requested before the first insert (a load behind an LDS atomic
        // waits for it: nine dependent trips to L2 / HBM otherwise)
        {
            constexpr int R1 = (NT_TILE * 27 + NTT - 1) / NTT;      // 9
            int u1[R1];
#pragma unroll
            for (int j = 0; j < R1; ++j) {
                const uint32_t t = threadIdx.x + (uint32_t)j * NTT;
                const uint32_t tt = t < nt * 27u ? t : 0u;
                u1[j] = nbr[(size_t)v0 * 27 + tt];             // (v0 + i) * 27 + sl with i = t / 27, sl = t % 27
            }
            uint32_t h1[R1], o1[R1];
#pragma unroll
            for (int j = 0; j < R1; ++j) { h1[j] = hslot((uint32_t)u1[j]); o1[j] = hw[h1[j]]; }      // (u1 < 0: some slot, not used)
            NPX(0);      // init + ring-1 table words arrived + first probes read
#pragma unroll
            for (int j = 0; j < R1; ++j) {
                const uint32_t t = threadIdx.x + (uint32_t)j * NTT;
                if (t < nt * 27u && u1[j] >= 0 && (o1[j] >> 10) != (uint32_t)u1[j] + 1u) insert_key_from((uint32_t)u1[j], h1[j], o1[j]);
            }
        }
        NPX(1);          // ring-1 inserts
        __syncthreads();
        NPX(2);
        // slot numbers: one LDS atomic per wave and round (ballot + prefix count), not one per key -- a few hundred returning atomics on
        // one address are served one after the other and were a fifth of the kernel
        // (ONE atomic per wave for all its rounds: the entries of every round are read first, the wave's count is their sum -- a returning LDS atomic per round was
        // ~500 cycles, six or eight times in a row, twice per tile)
        constexpr int NI = (NT_HCAP + NTT - 1) / NTT;
        {
            uint32_t key[NI]; uint64_t mask[NI]; uint32_t total = 0;
#pragma unroll
            for (int r = 0; r < NI; ++r) {
                const int i = r * NTT + (int)threadIdx.x;
                key[r] = i < NT_HCAP ? hw[i] : 0u;
                mask[r] = __ballot(key[r] != 0u);
                total += (uint32_t)__popcll(mask[r]);
            }
            uint32_t first = 0;
            if (lane_id() == 0 && total) first = atomicAdd(&n_slots, total);
            first = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
#pragma unroll
            for (int r = 0; r < NI; ++r) {
                const int i = r * NTT + (int)threadIdx.x;
                if (key[r]) { const uint32_t sl = first + (uint32_t)__popcll(mask[r] & lanemask_lt()); if (nt_ring1_holds(sl)) { hw[i] = (key[r] & ~NT_HNONE) | sl; sord[sl] = (key[r] >> 10) - 1u; } else overflow = 1; }
                first += (uint32_t)__popcll(mask[r]);
            }
        }
        NPX(3);          // ring-1 numbering
        __syncthreads();
        NPH();
        NPX(4);
        const uint32_t n1 = n_slots < NT_RING1 ? n_slots : NT_RING1;
        if (threadIdx.x < nt && !overflow) tme[threadIdx.x] = lookup(v0 + threadIdx.x);      // (a tile voxel is its own neighbour: it has a one-ring slot since the first numbering)
        // (2) two-ring keys.  Where a key sits in the hash (11 bits) goes straight into its place in `rows` (free until (3)): (3) turns it into the slot number with two
        // LDS reads and no probing, and no per-thread array lives across the phases (the 48 ordinals a thread of the 4-wave variant used to keep were what spilled to
        // scratch under its 168-VGPR budget: 63 -> 21 MB of HBM traffic per frame)
        if (!overflow) {
            int u2c[PT];
            // as above: first every load (clamped index, no per-lane guard in front of it), then the inserts
            const uint32_t lim = n1 * 27u;
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                u2c[j] = -1;
                if ((uint32_t)j * NTT < lim) {          // (uniform)
                    const uint32_t t = threadIdx.x + (uint32_t)j * NTT;
                    const uint32_t tt = t < lim ? t : lim - 1u;
                    const uint32_t i = tt / 27u, sl = tt - i * 27u;
                    u2c[j] = nbr[(size_t)sord[i] * 27 + sl];
                }
            }
            constexpr int G = PR;       // first probes read together
            { int any_ = 0;
#pragma unroll
              for (int j = 0; j < PT; ++j) any_ |= u2c[j];
              asm volatile("" :: "v"(any_)); }
            NPX(5);      // ring-2 table words arrived
#pragma unroll
            for (int j0 = 0; j0 < PT; j0 += G) {
                uint32_t h2[G], o2[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint32_t t = threadIdx.x + (uint32_t)(j0 + g) * NTT;
                    if (t >= lim) u2c[j0 + g] = -1;
                    h2[g] = hslot((uint32_t)u2c[j0 + g]); o2[g] = hw[h2[g]];
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    uint32_t pos = 0xFFFFu;
                    if (u2c[j0 + g] >= 0) pos = (o2[g] >> 10) == (uint32_t)u2c[j0 + g] + 1u ? h2[g] : insert_key_from((uint32_t)u2c[j0 + g], h2[g], o2[g]);
                    const uint32_t t = threadIdx.x + (uint32_t)(j0 + g) * NTT;
                    if (t < lim) { const uint32_t i = t / 27u, sl = t - i * 27u; rows[i][sl] = (uint16_t)pos; }
                }
            }
        }
        NPX(6);          // ring-2 probes, inserts, positions into `rows`
        __syncthreads();
        NPX(7);
        if (!overflow) {
            uint32_t key[NI]; uint64_t mask[NI]; uint32_t total = 0;
#pragma unroll
            for (int r = 0; r < NI; ++r) {
                const int i = r * NTT + (int)threadIdx.x;
                const uint32_t kw = i < NT_HCAP ? hw[i] : 0u;
                key[r] = (kw & NT_HNONE) == NT_HNONE ? kw : 0u;      // (an entry that has a key and no number yet)
                mask[r] = __ballot(key[r] != 0u);
                total += (uint32_t)__popcll(mask[r]);
            }
            uint32_t first = 0;
            if (lane_id() == 0 && total) first = atomicAdd(&n_slots, total);
            first = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
#pragma unroll
            for (int r = 0; r < NI; ++r) {
                const int i = r * NTT + (int)threadIdx.x;
                if (key[r]) { const uint32_t sl = first + (uint32_t)__popcll(mask[r] & lanemask_lt()); if (nt_slots_hold(sl)) { hw[i] = (key[r] & ~NT_HNONE) | sl; sord[sl] = (key[r] >> 10) - 1u; } else overflow = 1; }
                first += (uint32_t)__popcll(mask[r]);
            }
        }
        NPX(8);          // ring-2 numbering
        __syncthreads();
        NPH();
        NPX(9);
        if (overflow) {
            // ---- fallback: the same accumulation straight from global memory (the sweeps take their global path on this tile too)
            if (threadIdx.x == 0) tile_n1[bix] = SW_TILE_NONE;
            const uint32_t v = v0 + threadIdx.x;
            if (threadIdx.x < nt) {
                float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
                unsigned cnt = 1;
                const float4 self = *reinterpret_cast<const float4*>(vf + (size_t)v * 12);
                cov_add(acc, self);
                for (int s = 0; s < 27; ++s) {
                    const int u = nbr[(size_t)v * 27 + s];
                    if (u < 0) continue;
                    cov_add(acc, *reinterpret_cast<const float4*>(vf + (size_t)u * 12)); cnt++;
                    for (int s2 = 0; s2 < 27; ++s2) {
                        const int u2 = nbr[(size_t)u * 27 + s2];
                        if (u2 >= 0) { cov_add(acc, *reinterpret_cast<const float4*>(vf + (size_t)u2 * 12)); cnt++; }
                    }
                }
                const float vp[3] = {self.x, self.y, self.z};
                float n4[4];
                n_plane_normal(acc, cnt, vp, n4);
                float* nout = vf + (size_t)v * 12 + 6;
                nout[0] = n4[0]; nout[1] = n4[1]; nout[2] = n4[2];
            }
            return;
        }
        // (3) centroids of every slot, neighbour rows of the one-ring as slot numbers
        const uint32_t ns = n_slots;
        for (uint32_t i = threadIdx.x; i < ns; i += NTT) { float4 q = *reinterpret_cast<const float4*>(vf + (size_t)sord[i] * 12); q.w = q.y; xyz[i] = q; }      // (x, y, z, y): CovPairs
        // (every table entry: hash position -> slot number + KB; an absent neighbour -> the zero slot)
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const uint32_t t = threadIdx.x + (uint32_t)j * NTT;
            if (t < n1 * 27u) {
                const uint32_t i = t / 27u, sl = t - i * 27u;
                const uint32_t pos = rows[i][sl];
                const uint32_t w = hw[pos != 0xFFFFu ? pos : 0u];
                rows[i][sl] = (uint16_t)((pos != 0xFFFFu ? (w & NT_HNONE) : (uint32_t)NT_ZERO) + KB);
            }
        }
        __syncthreads();
        // One thread per one-ring row.  (3b) If the row is a tile voxel's own, its 27 list positions (NT_RING1 = absent) go out for the sweep kernels, bit-packed into 8
        // words and staged in the hash table's memory (the hash is dead from here on) so that they leave as coalesced stores below.  Then the row is COMPACTED in
        // place (round 6): the present neighbours first, in their order, the zero slot behind them, their number in entry 27.  Adding +0 is the identity and the order of
        // the others is what it was, so the sums are the same bits -- but a voxel of a surface has 17 of its 27 neighbours on average, and the ordered accumulation below
        // now runs as many positions as the wave's fullest row has (22 on average), not 27.  (The positions matter to the sweeps -- bit k of a thief mask is neighbour
        // slot k --: that is why the rows' own copies for them are taken before the compaction.)
        {
            uint32_t* const stage_slots = hw;      // [SW_SLOT_WORDS][NT_TILE]
            static_assert(SW_SLOT_WORDS * NT_TILE <= NT_HCAP, "the staged slot words fit the hash table's memory");
            const uint16_t ZBv = (uint16_t)(NT_ZERO + KB);
            for (uint32_t i = threadIdx.x; i < n1; i += NTT) {
                uint2 rw[7];
                const uint2* rp = reinterpret_cast<const uint2*>(&rows[i][0]);
#pragma unroll
                for (int k = 0; k < 7; ++k) rw[k] = rp[k];
                uint32_t ent[27];
#pragma unroll
                for (int j = 0; j < 27; ++j) { const uint32_t w = ((j >> 1) & 1) ? rw[j >> 2].y : rw[j >> 2].x; ent[j] = (j & 1) ? (w >> 16) : (w & 0xFFFFu); }
                const uint32_t ti = sord[i] - v0;      // the tile voxel this row belongs to, if any
                if (ti < nt) {
                    uint32_t pos[27], pk[SW_SLOT_WORDS];
#pragma unroll
                    for (int j = 0; j < 27; ++j) { const uint32_t e = ent[j] - KB; pos[j] = e == NT_ZERO ? (uint32_t)NT_RING1 : e; }
                    sw_slots_pack(pos, pk);
#pragma unroll
                    for (int k = 0; k < SW_SLOT_WORDS; ++k) stage_slots[k * NT_TILE + ti] = pk[k];
                }
                uint16_t* const r = &rows[i][0];
                uint32_t w = 0;
#pragma unroll
                for (int j = 0; j < 27; ++j) if (ent[j] != (uint32_t)ZBv) { r[w] = (uint16_t)ent[j]; ++w; }
                for (uint32_t k = w; k < 27u; ++k) r[k] = ZBv;
                r[27] = (uint16_t)w;
            }
        }
        if (threadIdx.x < 28u) rows[NT_RING1][threadIdx.x] = threadIdx.x < 27u ? (uint16_t)(NT_ZERO + KB) : (uint16_t)0;
        __syncthreads();
        // (3b) the tile's one-ring for the sweep kernels (d_sweep_R_pre, d_sweep_claim): the ordinals of its n1 one-ring voxels and, per tile
        // voxel, 27 16-bit positions in that list (NT_RING1 = absent), two per word, slot-major.  Every neighbour of a tile voxel is in the
        // list by construction, so the sweeps stage one word per list entry in LDS and read neighbours from there: no per-lane escape.
        if (threadIdx.x == 0) tile_n1[bix] = (holes && bix % holes == 1u) ? SW_TILE_NONE : n1;      // (holes: tests of the sweeps' mixed tiled / global path)
        for (uint32_t i = threadIdx.x; i < n1; i += NTT) tile_ord[(size_t)bix * NT_RING1 + i] = sord[i];
        for (uint32_t e = threadIdx.x; e < (uint32_t)(SW_SLOT_WORDS * NT_TILE); e += NTT) if ((e & (uint32_t)(NT_TILE - 1)) < nt) tile_slots[(size_t)bix * SW_SLOT_WORDS * NT_TILE + e] = hw[e];
        NPH();
        // which lanes run the ordered sums (everything they read is in LDS: any wave can take any voxel)
        // waves 0 and 2 (each has a SIMD's vector issue to itself: on waves 0 and 4, which share one, the kernel takes 19.7 ms per 192-frame launch instead of 11.5;
        // waves 0 and 1: 11.8; odd tiles on waves 2 and 3, in case two workgroups of a unit met on SIMDs 0 and 1: 11.9 -- F3DS_NT_ACC_MODE=1 / 2 / 3 at build time)
#ifndef F3DS_NT_ACC_MODE
#define F3DS_NT_ACC_MODE 0
#endif
        const uint32_t wv = threadIdx.x >> 6;
        uint32_t ai = wv == 0u ? threadIdx.x : (wv == 2u ? threadIdx.x - 64u : 0xFFFFFFFFu);
        if (F3DS_NT_ACC_MODE == 1) ai = threadIdx.x - ((bix & 1u) ? 128u : 0u);
        if (F3DS_NT_ACC_MODE == 2) ai = wv == 0u ? threadIdx.x : (wv == 4u ? threadIdx.x - 192u : 0xFFFFFFFFu);
        if (F3DS_NT_ACC_MODE == 3) ai = threadIdx.x;
        if (F3DS_NT_ACC_MODE == 4) ai = (bix & 1u) ? (wv == 1u ? threadIdx.x - 64u : (wv == 3u ? threadIdx.x - 128u : 0xFFFFFFFFu)) : ai;      // odd tiles on waves 1 and 3: the other two SIMDs
        if (ai >= nt) return;
        // (4) the ordered accumulation, out of LDS.  Absent two-ring neighbours point at the zero slot: x + 0 is
        // x for every x an accumulator can hold (they start at +0 and never become -0), so no select is needed.
        const uint32_t v = v0 + ai;
        const uint16_t me = tme[ai];
        CovPairs cp; cp.zero();
        unsigned cnt = 1;
        const f3ds_f4* xyz4 = reinterpret_cast<const f3ds_f4*>(xyz);
        const float4 self = xyz[me];
        cp.add(xyz4[me]);
        // The 27 one-ring positions without a branch: an absent neighbour reads the zero slot and the row of nobody (27 zero slots, count 0) -- adding +0 leaves every
        // accumulator as it is, see above.  (A wave skipped a position only when all its 64 voxels lacked that neighbour: rare.)  That makes the loop a software
        // pipeline: a position is 28 centroids (the neighbour's own, then its 27) in four batches of seven; while one batch is summed the next is on its way out of
        // LDS, a position's row is requested a position ahead and its slot number two ahead -- the dependent reads slot number -> row -> centroids (800 cycles of a
        // position's 1 900) were exposed.  Positions go in pairs (A, B) so that no register that a read is still filling has to be moved; a 28th position (nobody)
        // completes the last pair.  The LDS reads are issued and awaited by hand (as in the fold loops of d_merge_cw_t): hipcc gathers a position's reads and waits
        // with lgkmcnt(0) whatever the source order.  LDS returns in order, so "lgkmcnt(n)" = everything but the n youngest reads has arrived; every LDS read between
        // the first and the last macro below is one of these macros ("memory" clobbers: the compiler's own accesses stay outside).
        typedef uint32_t nt_u4 __attribute__((ext_vector_type(4)));
        typedef uint32_t nt_u2 __attribute__((ext_vector_type(2)));
#define NT_ROW_ISSUE(R, addr) asm volatile("ds_read2_b64 %0, %4 offset1:1\n\tds_read2_b64 %1, %4 offset0:2 offset1:3\n\tds_read2_b64 %2, %4 offset0:4 offset1:5\n\tds_read_b64 %3, %4 offset:48" \
            : "=&v"(R##a), "=&v"(R##b), "=&v"(R##c), "=&v"(R##d) : "v"(addr) : "memory")                                   /* 4 reads: the 14 words of a row */
#define NT_ROW_WORD(R, i) ((i) < 4 ? R##a[(i) & 3] : (i) < 8 ? R##b[(i) & 3] : (i) < 12 ? R##c[(i) & 3] : R##d[(i) & 1])
#define NT_C_ISSUE(cen_, addr) asm volatile("ds_read_b128 %0, %1" : "=v"(cen_) : "v"(addr) : "memory")
#define NT_U16_ISSUE(x, addr) asm volatile("ds_read_u16 %0, %1" : "=v"(x) : "v"(addr) : "memory")
#define NT_ENTRY_ADDR(a_, w_, hi_) do { if (hi_) asm volatile("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(a_) : "v"(four), "v"(w_)); \
            else asm volatile("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(a_) : "v"(four), "v"(w_)); } while (0)      /* (16-bit half of w_) << 4 in one instruction */
        /* batch b_ (0..3) of the position whose row is R and whose own entry is e_: centroid 0 is the neighbour's own, centroid j its neighbour j - 1; entry << 4 = LDS address */
#define NT_Q_ISSUE(Q, R, e_, b_) do { _Pragma("unroll") for (int k_ = 0; k_ < 7; ++k_) { const int j_ = 7 * (b_) + k_; uint32_t a_; \
            if (j_ == 0) a_ = (e_) << 4; else { const uint32_t w_ = NT_ROW_WORD(R, (j_ - 1) >> 1); NT_ENTRY_ADDR(a_, w_, (j_ - 1) & 1); } \
            NT_C_ISSUE(Q[k_], a_); } } while (0)
#define NT_Q_WAIT(Q, n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(Q[0]), "+v"(Q[1]), "+v"(Q[2]), "+v"(Q[3]), "+v"(Q[4]), "+v"(Q[5]), "+v"(Q[6]) :: "memory")
#define NT_ROW_WAIT(R, ent_, n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(R##a), "+v"(R##b), "+v"(R##c), "+v"(R##d), "+v"(ent_) :: "memory")
#define NT_ADD7(Q) do { _Pragma("unroll") for (int k_ = 0; k_ < 7; ++k_) cp.add(Q[k_]); } while (0)
        /* one position: row RX (arrived), own entry eX, batch 0 in q0 on its way; meanwhile the row RY of the next position (entry eY) and the entry eZ of the one after */
#define NT_POSITION(RX, eX, RY, eY, eZ, zpos) do { \
            NT_Q_ISSUE(q1, RX, eX, 1); \
            NT_Q_WAIT(q0, 7); \
            cnt += ((eX) != ZB ? 1u : 0u) + (RX##d[1] >> 16); \
            NT_ADD7(q0); \
            NT_U16_ISSUE(eZ, myrow_a + 2u * (uint32_t)((zpos) < 27 ? (zpos) : 26)); \
            NT_ROW_ISSUE(RY, row_addr(eY)); \
            NT_Q_ISSUE(q0, RX, eX, 2); \
            NT_Q_WAIT(q1, 12); \
            NT_ADD7(q1); \
            NT_Q_ISSUE(q1, RX, eX, 3); \
            NT_Q_WAIT(q0, 7); \
            NT_ADD7(q0); \
            NT_ROW_WAIT(RY, eZ, 7); \
            NT_Q_ISSUE(q0, RY, eY, 0); \
            NT_Q_WAIT(q1, 7); \
            NT_ADD7(q1); } while (0)
        const uint32_t rows_a = lds_addr(reinterpret_cast<const float*>(&rows[0][0])), myrow_a = rows_a + (uint32_t)me * 56u;
        const uint32_t ZB = (uint32_t)NT_ZERO + KB;                      // the entry of an absent neighbour
        uint32_t four = 4u; asm volatile("" : "+v"(four));          // (SDWA takes its shift count from a register)
        auto row_addr = [&](uint32_t e) { return rows_a + (e != ZB ? e - KB : (uint32_t)NT_RING1) * 56u; };
        const uint16_t* myrow = &rows[me][0];
        uint32_t eA = myrow[0], eB = myrow[1], eA2 = 0u, eB2 = 0u;     // entries (slot + KB) of the positions of a pair, and of the next pair
        nt_u4 RAa, RAb, RAc, RBa, RBb, RBc; nt_u2 RAd, RBd;
        f3ds_f4 q0[7], q1[7];
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(eA), "+v"(eB) :: "memory");
        NT_ROW_ISSUE(RA, row_addr(eA));
        NT_ROW_WAIT(RA, eA, 0);
        NT_Q_ISSUE(q0, RA, eA, 0);
        // (the rows are compacted: positions behind a voxel's last present neighbour add zeros only -- the wave runs as many as its fullest row has)
        uint32_t pmax = 0u;
        { const uint32_t mine_ = rows[me][27];      // (the largest count among the wave's active lanes, bit by bit: five ballots)
#pragma unroll
          for (uint32_t bit = 16u; bit; bit >>= 1) if (__ballot(mine_ >= (pmax | bit))) pmax |= bit; }
        const int phalf = (int)((pmax + 1u) >> 1);
#pragma unroll 1
        for (int p = 0; p < phalf; ++p) {
            if (2 * p + 1 >= 27) eB = ZB;
            NT_POSITION(RA, eA, RB, eB, eA2, 2 * p + 2);
            if (2 * p + 2 >= 27) eA2 = ZB;
            NT_POSITION(RB, eB, RA, eA2, eB2, 2 * p + 3);
            eA = eA2; eB = eB2;
        }
        NT_Q_WAIT(q0, 0);        // (the first batch of a 29th position: nothing may still be writing registers when the code below reuses them)
#undef NT_ROW_ISSUE
#undef NT_ROW_WORD
#undef NT_ENTRY_ADDR
#undef NT_C_ISSUE
#undef NT_U16_ISSUE
#undef NT_Q_ISSUE
#undef NT_Q_WAIT
#undef NT_ROW_WAIT
#undef NT_ADD7
#undef NT_POSITION
        NPH();
        float acc[9];
        cp.store(acc);
        const float vp[3] = {self.x, self.y, self.z};
        float n4[4];
        n_plane_normal(acc, cnt, vp, n4);
        float* nout = vf + (size_t)v * 12 + 6;
        nout[0] = n4[0]; nout[1] = n4[1]; nout[2] = n4[2];
        NPH();
#ifdef F3DS_MERGE_PROF
        if (ai == 0u && f3ds_frame() == 0 && (bix == 10u || bix == 200u)) printf("d_normals tile %u, table phases: words+probes %llu | inserts %llu barrier %llu | numbering %llu barrier %llu | ring-2 words %llu | probes+inserts %llu barrier %llu | numbering %llu barrier %llu\n", bix, tx_[0], tx_[1], tx_[2], tx_[3], tx_[4], tx_[5], tx_[6], tx_[7], tx_[8], tx_[9]);
        if (ai == 0u && f3ds_frame() == 0 && (bix == 10u || bix == 200u)) printf("d_normals tile %u: init %llu ring1 %llu ring2 %llu rows+centroids %llu accumulate %llu normal %llu cycles (slots %u)\n", bix, tp[0], tp[1], tp[2], tp[3], tp[4], tp[5], ns);
#endif
#undef NPH
#undef NPX
    }
    // every gridDim.x-th tile (the host launches one workgroup per tile unless F3DS_NORMALS_WGS asks for long-lived workgroups: f3ds_hip.hip, seg_normals)
    __device__ void operator()(float* vf, const int* nbr, const DevCounters* dc, uint32_t* tile_n1, uint32_t* tile_ord, uint32_t* tile_slots, uint32_t holes) const {
        const uint32_t V = dc->n_voxels;
#ifdef F3DS_NORMALS_LOOP      // experiment (long-lived workgroups, F3DS_NORMALS_WGS): the loop costs the kernel 100 VGPRs and scratch (152 -> 256), so it is not in the default build
        for (uint32_t b = BIX; b * (uint32_t)NT_TILE < V; b += gridDim.x) {
            one_tile(b, vf, nbr, dc, tile_n1, tile_ord, tile_slots, holes);
            __syncthreads();
        }
#else
        if (BIX * (uint32_t)NT_TILE < V) one_tile(BIX, vf, nbr, dc, tile_n1, tile_ord, tile_slots, holes);
#endif
    }
};

// ------------------------------------------------------------------------------------------------
// stage 2: seeds
// ------------------------------------------------------------------------------------------------
constexpr int SEED_CHUNK = 256;
struct d_chunkbox {
    static constexpr int BLOCK = SEED_CHUNK;
    __device__ void operator()(const float* vf, const DevCounters* dc, float* boxes) const {
        const uint32_t V = dc->n_voxels;
        const uint32_t v = BIX * SEED_CHUNK + threadIdx.x;
        if (BIX * SEED_CHUNK >= V) return;
        float mn[3] = {F3DS_FLT_MAX, F3DS_FLT_MAX, F3DS_FLT_MAX}, mx[3] = {-F3DS_FLT_MAX, -F3DS_FLT_MAX, -F3DS_FLT_MAX};
        if (v < V) { const float* p = vf + (size_t)v * 12; for (int a = 0; a < 3; ++a) { mn[a] = p[a]; mx[a] = p[a]; } }
        __shared__ float smn[SEED_CHUNK / 64][3], smx[SEED_CHUNK / 64][3];
    #pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            for (int a = 0; a < 3; ++a) {
                float t = __shfl_xor(mn[a], d, 64); if (t < mn[a]) mn[a] = t;
                t = __shfl_xor(mx[a], d, 64); if (t > mx[a]) mx[a] = t;
            }
        if (lane_id() == 0) for (int a = 0; a < 3; ++a) { smn[threadIdx.x >> 6][a] = mn[a]; smx[threadIdx.x >> 6][a] = mx[a]; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < SEED_CHUNK / 64; ++w)
                for (int a = 0; a < 3; ++a) { if (smn[w][a] < mn[a]) mn[a] = smn[w][a]; if (smx[w][a] > mx[a]) mx[a] = smx[w][a]; }
            for (int a = 0; a < 3; ++a) { boxes[BIX * 6 + a] = mn[a]; boxes[BIX * 6 + 3 + a] = mx[a]; }
        }
    }
};
// replay of OctreePointCloud::adoptBoundingBoxToPoint over the voxel centroids in leaf order:
// the cube only changes when a point falls outside it, so look for the first such point (chunk
// boxes first, then the points of that chunk), grow, and continue behind it.
struct d_seed_grow {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 256;      // (1 024 threads until round 4: with other calls filling the chip a 16-wave workgroup of 96 VGPRs waited 5 ms for a compute unit with that much free, on every call's critical path)
    __device__ void operator()(const float* vf, const float* boxes, DevCounters* dc, float seed_res, SeedGrid* out) const {
        __shared__ SeedGrid g;
        __shared__ uint32_t cursor;
        __shared__ uint32_t found;
        const uint32_t V = dc->n_voxels;
        const uint32_t C = (V + SEED_CHUNK - 1) / SEED_CHUNK;
        if (threadIdx.x == 0) { a_seed_init(g, seed_res); cursor = 0; }
        __syncthreads();
        for (;;) {
            if (threadIdx.x == 0) found = 0xFFFFFFFFu;
            __syncthreads();
            const uint32_t c0 = cursor / SEED_CHUNK;
            if (cursor >= V || g.error) break;
            uint32_t mine = 0xFFFFFFFFu;
            for (uint32_t c = c0 + threadIdx.x; c < C; c += (uint32_t)BLOCK)
                if (a_seed_box_violates(g, boxes + c * 6, boxes + c * 6 + 3)) { mine = c; break; }
            if (mine != 0xFFFFFFFFu) atomicMin(&found, mine);
            __syncthreads();
            const uint32_t cstar = found;
            __syncthreads();
            if (cstar == 0xFFFFFFFFu) break;
            if (threadIdx.x == 0) found = 0xFFFFFFFFu;
            __syncthreads();
            {
                const uint32_t v = cstar * SEED_CHUNK + threadIdx.x;
                if (threadIdx.x < SEED_CHUNK && v < V && v >= cursor && a_seed_violates(g, vf + (size_t)v * 12)) atomicMin(&found, v);
            }
            __syncthreads();
            const uint32_t istar = found;
            __syncthreads();
            if (threadIdx.x == 0) {
                if (istar == 0xFFFFFFFFu) cursor = (cstar + 1u) * SEED_CHUNK;
                else { a_seed_grow(g, (int)istar, vf + (size_t)istar * 12); cursor = istar + 1u; }
            }
            __syncthreads();
        }
        __syncthreads();
        if (threadIdx.x == 0) { *out = g; dc->sdepth = g.depth; if (g.error) dc->error = g.error; }
    }
};
struct d_seed_keys {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const float* vf, const DevCounters* dc, const SeedGrid* gp, uint32_t* ckey, uint64_t* keys, uint32_t* vals) const {
        __shared__ SeedGrid g;
        if (threadIdx.x == 0) g = *gp;
        __syncthreads();
        const uint32_t V = dc->n_voxels;
        for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
            unsigned k[3];
            a_seed_key(g, (int)v, vf + (size_t)v * 12, k);
            ckey[v * 3] = k[0]; ckey[v * 3 + 1] = k[1]; ckey[v * 3 + 2] = k[2];
            keys[v] = n_morton(k[0], k[1], k[2], g.depth);
            vals[v] = v;
        }
    }
};
struct d_cell_hash {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint32_t* ckey, const uint32_t* sorted_vox, const uint32_t* cell_start, const DevCounters* dc,
                                                  uint64_t* hkeys, uint32_t* hvals, uint32_t hmask) const {
        const uint32_t C = dc->n_cells;
        for (uint32_t c = BIX * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
            const uint32_t v = sorted_vox[cell_start[c]];
            const uint64_t pk = n_pack_key(ckey[v * 3], ckey[v * 3 + 1], ckey[v * 3 + 2]);
            uint32_t h = (uint32_t)hash64(pk) & hmask;
            for (;;) {
                unsigned long long old = atomicCAS((unsigned long long*)&hkeys[h], (unsigned long long)HASH_EMPTY, (unsigned long long)pk);
                if (old == HASH_EMPTY || old == pk) { hvals[h] = c; break; }
                h = (h + 1u) & hmask;
            }
        }
    }
};
constexpr uint32_t SEED_CELLS_PER_WG = 4;      // seed cells per workgroup of d_seed_nn / d_seed_filter, a wave each (their launches: seed_cell_grid)
constexpr uint32_t SEED_CAND_STRIDE = 256;     // list entries a wave takes per round of their candidate loops (four per lane)
constexpr double SEED_NN_MARGIN = 1e-3;        // d_seed_nn: the own-cell shortcut holds below (half cell)^2 * (1 - this) ...
constexpr double SEED_NN_ULP = 0x1p-23;        // ... the half cell less this much of the centre's largest coordinate
constexpr double SEED_PRUNE_MARGIN = 1.001;    // d_seed_filter: a cell is looked up when its box is within r2 * this of the seed voxel
static_assert(SEED_CELLS_PER_WG * 64u == 256u && SEED_CAND_STRIDE == 4u * 64u, "a wave per cell in a 256-thread workgroup, four entries per lane and round");
// one wave per occupied seed cell: exact nearest voxel to the cell centre (3x3x3 cell block)
// (four seed cells per workgroup, a wave each: one-wave workgroups -- ~1 500 per frame, 290 k per batched launch -- were bound by the rate at which workgroups are dispatched)
struct d_seed_nn {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const float* vf, const uint32_t* ckey, const uint32_t* sorted_vox, const uint32_t* cell_start,
                                               const DevCounters* dc, const SeedGrid* gp, const uint64_t* hkeys, const uint32_t* hvals, uint32_t hmask,
                                               int* seed_orig) const {
        const uint32_t c = BIX * SEED_CELLS_PER_WG + (threadIdx.x >> 6);
        if (c >= dc->n_cells) return;
        const uint32_t v0 = sorted_vox[cell_start[c]];
        const unsigned key[3] = {ckey[v0 * 3], ckey[v0 * 3 + 1], ckey[v0 * 3 + 2]};
        float centre[3];
        for (int a = 0; a < 3; ++a) centre[a] = (float)(((double)key[a] + 0.5f) * gp->res + gp->min[a]);
        float bd = F3DS_FLT_MAX; int best = 0x7fffffff;
        const int lane = lane_id();
        // The cell's own voxels first: a voxel of any other cell is at least half a cell away from this cell's centre (up to rounding: 1e-3 of margin below), so a
        // voxel nearer than that is the answer -- 27 cells are only searched when the surface cuts a corner of the cell.  Same (distance, ordinal) minimum.
        {
            const uint32_t b0 = cell_start[c], e0 = cell_start[c + 1];
            for (uint32_t i0 = b0; i0 < e0; i0 += SEED_CAND_STRIDE) {
                int j[4]; bool ok[4];
    #pragma unroll
                for (int u = 0; u < 4; ++u) { const uint32_t i = i0 + 64u * (uint32_t)u + (uint32_t)lane; ok[u] = i < e0; j[u] = (int)sorted_vox[ok[u] ? i : b0]; }
                float4 p[4];
    #pragma unroll
                for (int u = 0; u < 4; ++u) p[u] = *reinterpret_cast<const float4*>(vf + (size_t)j[u] * 12);
    #pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!ok[u]) continue;
                    const float pp[3] = {p[u].x, p[u].y, p[u].z};
                    const float d = a_sqdist(centre, pp);
                    if (best == 0x7fffffff || d < bd || (d == bd && j[u] < best)) { bd = d; best = j[u]; }
                }
            }
    #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float od = __shfl_xor(bd, d, 64); const int ob = __shfl_xor(best, d, 64);
                if (ob != 0x7fffffff && (best == 0x7fffffff || od < bd || (od == bd && ob < best))) { bd = od; best = ob; }
            }
            // The centre is a float: it lies up to half an ulp -- 2^-24 of its largest coordinate -- off the cell's true centre, so a voxel of another cell may come that much
            // nearer than half a cell.  The half cell gives up twice that before it is squared (the 1e-3 is for the roundings of a_sqdist alone, 2.4e-7 relative), and where
            // that takes more than half of it away (coordinates beyond 2^21 cells) no shortcut is taken: DESIGN.md 7.
            const float cmax = fmaxf(fabsf(centre[0]), fmaxf(fabsf(centre[1]), fabsf(centre[2])));
            const double half = 0.5 * gp->res - (double)cmax * SEED_NN_ULP;
            const float near = half > 0.25 * gp->res ? (float)(half * half * (1.0 - SEED_NN_MARGIN)) : 0.0f;
            if (best != 0x7fffffff && bd < near) { if (lane == 0) seed_orig[c] = best; return; }      // (uniform: every lane holds the wave's minimum)
            bd = F3DS_FLT_MAX; best = 0x7fffffff;
        }
        // lanes 0..26 look up the 27 cells at the same time; their voxels are then visited as one flat list
        // (the nearest voxel under the (distance, ordinal) order does not depend on the visiting order)
        __shared__ uint32_t s_beg4[SEED_CELLS_PER_WG][28], s_pre4[SEED_CELLS_PER_WG][28];
        uint32_t* s_beg = s_beg4[threadIdx.x >> 6]; uint32_t* s_pre = s_pre4[threadIdx.x >> 6];
        uint32_t beg = 0, cnt = 0;
        if (lane < 27) {
            const long long x = (long long)key[0] + lane / 9 - 1, y = (long long)key[1] + (lane / 3) % 3 - 1, z = (long long)key[2] + lane % 3 - 1;
            if (x >= 0 && y >= 0 && z >= 0) {
                const int cc = hash_find(hkeys, hvals, hmask, n_pack_key((unsigned)x, (unsigned)y, (unsigned)z));
                if (cc >= 0) { beg = cell_start[cc]; cnt = cell_start[cc + 1] - beg; }
            }
        }
        uint32_t pre = cnt;
    #pragma unroll
        for (int d = 1; d < 32; d <<= 1) { const uint32_t t = __shfl_up(pre, d, 64); if (lane >= d) pre += t; }
        if (lane < 27) { s_beg[lane] = beg; s_pre[lane] = pre - cnt; }
        const uint32_t total = __shfl(pre, 26, 64);
        wave_lds_sync();
        // (four rounds of 64 list entries at a time: their ordinals, then their centroids, are requested together -- entry by entry the ~1 300 voxels of the 27 cells
        // were ~20 rounds of two dependent trips to L2 per wave)
        for (uint32_t i0 = 0; i0 < total; i0 += SEED_CAND_STRIDE) {
            int j[4]; bool ok[4];
    #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = i0 + 64u * (uint32_t)u + (uint32_t)lane;
                ok[u] = i < total;
                const uint32_t ii = ok[u] ? i : 0u;
                int cell = 0;
    #pragma unroll
                for (int k = 1; k < 27; ++k) cell += s_pre[k] <= ii;
                j[u] = (int)sorted_vox[s_beg[cell] + (ii - s_pre[cell])];
            }
            float4 p[4];
    #pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = *reinterpret_cast<const float4*>(vf + (size_t)j[u] * 12);
    #pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
                const float pp[3] = {p[u].x, p[u].y, p[u].z};
                const float d = a_sqdist(centre, pp);
                if (best == 0x7fffffff || d < bd || (d == bd && j[u] < best)) { bd = d; best = j[u]; }
            }
        }
    #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float od = __shfl_xor(bd, d, 64); const int ob = __shfl_xor(best, d, 64);
            if (ob != 0x7fffffff && (best == 0x7fffffff || od < bd || (od == bd && ob < best))) { bd = od; best = ob; }
        }
        if (lane_id() == 0) seed_orig[c] = best;
    }
};
// one wave per candidate seed: voxels closer than seed_res/2 to the seed voxel.  Lanes 0..26 look up the 27 seed
// cells around it at the same time; the voxels of all of them are then counted as one flat list.
struct d_seed_filter {
    static constexpr int BLOCK = 256;      // (four candidates per workgroup, a wave each: d_seed_nn)
    __device__ void operator()(const float* vf, const uint32_t* ckey, const uint32_t* sorted_vox, const uint32_t* cell_start,
                                                   const DevCounters* dc, const SeedGrid* gp, const uint64_t* hkeys, const uint32_t* hvals, uint32_t hmask,
                                                   const int* seed_orig, float r2, float min_points, uint32_t* keep) const {
        __shared__ uint32_t s_beg4[SEED_CELLS_PER_WG][28], s_pre4[SEED_CELLS_PER_WG][28];
        uint32_t* s_beg = s_beg4[threadIdx.x >> 6]; uint32_t* s_pre = s_pre4[threadIdx.x >> 6];
        const uint32_t c = BIX * SEED_CELLS_PER_WG + (threadIdx.x >> 6);
        if (c >= dc->n_cells) return;
        const int lane = lane_id();
        const int s0 = seed_orig[c];
        const unsigned key[3] = {ckey[s0 * 3], ckey[s0 * 3 + 1], ckey[s0 * 3 + 2]};
        const float4 q = *reinterpret_cast<const float4*>(vf + (size_t)s0 * 12);
        const float sp[3] = {q.x, q.y, q.z};
        uint32_t beg = 0, cnt = 0;
        if (lane < 27) {
            const long long x = (long long)key[0] + lane / 9 - 1, y = (long long)key[1] + (lane / 3) % 3 - 1, z = (long long)key[2] + lane % 3 - 1;
            // a cell the sphere around the seed voxel cannot reach (distance to the cell's box, 1e-3 of margin for the roundings of keys and distances) holds nothing to
            // count: the radius is half a cell, so at most 8 of the 27 cells are looked up and walked
            const int dxyz[3] = {lane / 9 - 1, (lane / 3) % 3 - 1, lane % 3 - 1};
            double far2 = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double lo = gp->min[a] + (double)key[a] * gp->res;
                double t = dxyz[a] < 0 ? (double)sp[a] - lo : (dxyz[a] > 0 ? (lo + gp->res) - (double)sp[a] : 0.0);
                if (t < 0.0) t = 0.0;
                far2 += t * t;
            }
            if (x >= 0 && y >= 0 && z >= 0 && far2 <= (double)r2 * SEED_PRUNE_MARGIN) {
                const int cc = hash_find(hkeys, hvals, hmask, n_pack_key((unsigned)x, (unsigned)y, (unsigned)z));
                if (cc >= 0) { beg = cell_start[cc]; cnt = cell_start[cc + 1] - beg; }
            }
        }
        uint32_t pre = cnt;                      // inclusive prefix over lanes 0..26
    #pragma unroll
        for (int d = 1; d < 32; d <<= 1) { const uint32_t t = __shfl_up(pre, d, 64); if (lane >= d) pre += t; }
        if (lane < 27) { s_beg[lane] = beg; s_pre[lane] = pre - cnt; }
        const uint32_t total = __shfl(pre, 26, 64);
        if (lane == 27) s_pre[27] = total;
        wave_lds_sync();
        uint32_t num = 0;
        for (uint32_t i0 = 0; i0 < total; i0 += SEED_CAND_STRIDE) {       // (four rounds at a time: d_seed_nn)
            uint32_t vv[4]; bool ok[4];
    #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = i0 + 64u * (uint32_t)u + (uint32_t)lane;
                ok[u] = i < total;
                const uint32_t ii = ok[u] ? i : 0u;
                int cell = 0;
    #pragma unroll
                for (int k = 1; k < 27; ++k) cell += s_pre[k] <= ii;          // last cell whose exclusive prefix is <= i
                vv[u] = sorted_vox[s_beg[cell] + (ii - s_pre[cell])];
            }
            float4 p[4];
    #pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = *reinterpret_cast<const float4*>(vf + (size_t)vv[u] * 12);
    #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float pp[3] = {p[u].x, p[u].y, p[u].z};
                if (ok[u] && a_sqdist(sp, pp) < r2) num++;
            }
        }
    #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) num += __shfl_xor(num, d, 64);
        if (lane == 0) keep[c] = ((float)num > min_points) ? 1u : 0u;
    }
};
struct d_seed_compact {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const int* seed_orig, const uint32_t* keep, const uint32_t* incl, DevCounters* dc, int* seed_kept) const {
        const uint32_t C = dc->n_cells;
        for (uint32_t c = BIX * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
            if (keep[c]) seed_kept[incl[c] - 1u] = seed_orig[c];
            if (c + 1 == C) dc->n_seeds = incl[c];
        }
    }
};

// ------------------------------------------------------------------------------------------------
// stage 3: helpers and label-propagation sweeps
// ------------------------------------------------------------------------------------------------
// createSupervoxelHelpers: the LAST helper seeded on a voxel owns it (addLeaf overwrites owner_)
// Where a helper's leaves are.  Supervoxels are compact in space but not in leaf ordinal (a 22-leaf
// supervoxel spans 1900 ordinals on average and 50 000 when it straddles a high Morton boundary), so each
// helper keeps the list of 64-voxel tiles it has leaves in: d_sweep_claim appends, d_centroid rewrites it
// exactly.  The list holds HT_CAP raw entries (d_sweep_claim appends one per voxel gained: tiles repeat -- with 150-voxel supervoxels,
// BASELINE config 4, a helper gains more than 64 voxels in one sweep, and with a 64-entry list it fell back to scanning its whole
// ordinal window: d_centroid was 12 ms of that frame's 18 ms of sweeps); up to 64 DISTINCT tiles are visited through the list,
// more than that, or more than HT_CAP raw entries: the ordinal window [lo, hi].
constexpr uint32_t HT_CAP = 256;
// the row path of d_centroid / d_sv_fill (four helpers per wave, 16 lanes each) takes a helper of at most HT_ROW tile-list entries and QL leaves; a frame of more
// than BY_WAVE_RATIO voxels per seed goes straight to the wave-wide path
constexpr uint32_t HT_ROW = 16;
constexpr uint32_t QL = 64;
constexpr uint32_t BY_WAVE_RATIO = 48;
struct d_helper_own {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const int* seed_kept, uint32_t S0, uint32_t* owner) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < S0; i += gridDim.x * blockDim.x) atomicMax(&owner[seed_kept[i]], i + 1u);
    }
};
struct d_helper_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const int* seed_kept, uint32_t S0, const uint32_t* owner, int* ghost_vox, unsigned char* ghost_active,
                                                    unsigned char* ghost_done, uint32_t* hlo, uint32_t* hhi, uint32_t* hcount, float* hc, uint32_t* tl,
                                                    uint32_t* tcnt) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i <= S0; i += gridDim.x * blockDim.x) {
            for (int k = 0; k < 12; ++k) hc[(size_t)i * 12 + k] = 0.0f;
            ghost_done[i] = 0;
            if (i == 0) { ghost_vox[0] = -1; ghost_active[0] = 0; hlo[0] = 0; hhi[0] = 0; hcount[0] = 0; tcnt[0] = 0; continue; }
            const int v = seed_kept[i - 1];
            const bool ghost = owner[v] != i;
            ghost_vox[i] = ghost ? v : -1;
            ghost_active[i] = ghost ? 1 : 0;
            hlo[i] = (uint32_t)v; hhi[i] = (uint32_t)v; hcount[i] = 1;
            tl[(size_t)i * HT_CAP] = (uint32_t)v >> 6; tcnt[i] = ghost ? 0u : 1u;
        }
    }
};
// ---- refineSupervoxels (row N3; viewer-only in the reference, src/supervoxel_clustering.cpp:369-375) ----
// The helper whose refineNormals() writes voxel v last: its owner, or a higher helper that holds v as a ghost leaf.
struct d_refine_ghost_L {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t S0, const int* ghost_vox, const unsigned char* ghost_active, uint32_t* L) const {
        for (uint32_t h = 1u + BIX * blockDim.x + threadIdx.x; h <= S0; h += gridDim.x * blockDim.x)
            if (ghost_active[h] && ghost_vox[h] >= 0) atomicMax(&L[ghost_vox[h]], h);
    }
};
// SupervoxelHelper::refineNormals: computeVoxelData's duplicate-keeping two-ring list restricted to the voxels helper
// L[v] owns (the voxel itself is pushed unconditionally).  Lane per voxel, global gathers: not a hot kernel.
struct d_refine_normals {
    static constexpr int BLOCK = 256;
    __device__ void operator()(float* vf, const int* nbr, const uint32_t* owner, const uint32_t* L, uint32_t V) const {
        for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
            const uint32_t me = L[v];
            if (me == 0u) continue;
            float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            unsigned cnt = 1;
            const float4 self = *reinterpret_cast<const float4*>(vf + (size_t)v * 12);
            cov_add(acc, self);
            for (int s = 0; s < 27; ++s) {
                const int u = nbr[(size_t)v * 27 + s];
                if (u < 0 || owner[u] != me) continue;
                cov_add(acc, *reinterpret_cast<const float4*>(vf + (size_t)u * 12)); cnt++;
                for (int s2 = 0; s2 < 27; ++s2) {
                    const int u2 = nbr[(size_t)u * 27 + s2];
                    if (u2 >= 0 && owner[u2] == me) { cov_add(acc, *reinterpret_cast<const float4*>(vf + (size_t)u2 * 12)); cnt++; }
                }
            }
            const float vp[3] = {self.x, self.y, self.z};
            float n4[4];
            n_plane_normal(acc, cnt, vp, n4);
            float* nout = vf + (size_t)v * 12 + 6;
            nout[0] = n4[0]; nout[1] = n4[1]; nout[2] = n4[2];
        }
    }
};
// reseedSupervoxels: the voxel nearest to each live helper's centroid (voxel_kdtree_->nearestKSearch(centroid, 1);
// exact ties go to the lowest ordinal, fence F2) -- one workgroup per helper over all voxels.
struct d_reseed {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const float* vf, uint32_t V, uint32_t S0, const uint32_t* hcount, const float* hc, int* seed) const {
        __shared__ float sd[BLOCK];
        __shared__ int sv[BLOCK];
        const uint32_t h = BIX + 1u;
        if (h > S0) return;
        if (hcount[h] == 0u) { if (threadIdx.x == 0) seed[h - 1u] = -1; return; }
        const float centre[3] = {hc[(size_t)h * 12], hc[(size_t)h * 12 + 1], hc[(size_t)h * 12 + 2]};
        float bd = 0.0f; int best = -1;
        for (uint32_t v = threadIdx.x; v < V; v += blockDim.x) {
            const float4 q = *reinterpret_cast<const float4*>(vf + (size_t)v * 12);
            const float pp[3] = {q.x, q.y, q.z};
            const float d = a_sqdist(centre, pp);
            if (best < 0 || d < bd) { bd = d; best = (int)v; }       // ascending v per thread: the first minimum stays
        }
        sd[threadIdx.x] = bd; sv[threadIdx.x] = best;
        __syncthreads();
        for (int w = BLOCK / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                const int ob = sv[threadIdx.x + w]; const float od = sd[threadIdx.x + w];
                const int mb = sv[threadIdx.x]; const float md = sd[threadIdx.x];
                if (ob >= 0 && (mb < 0 || od < md || (od == md && ob < mb))) { sv[threadIdx.x] = ob; sd[threadIdx.x] = od; }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) seed[h - 1u] = sv[0];
    }
};
// addLeaf(seed) of reseedSupervoxels: like d_helper_own / d_helper_init, but helpers erased earlier have no seed and
// the centroids are the ones the last updateCentroid left
struct d_reseed_own {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const int* seed, uint32_t S0, uint32_t* owner) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < S0; i += gridDim.x * blockDim.x) if (seed[i] >= 0) atomicMax(&owner[seed[i]], i + 1u);
    }
};
struct d_reseed_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const int* seed, uint32_t S0, const uint32_t* owner, int* ghost_vox, unsigned char* ghost_active, unsigned char* ghost_done, uint32_t* hlo,
                               uint32_t* hhi, uint32_t* hcount, uint32_t* tl, uint32_t* tcnt) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i <= S0; i += gridDim.x * blockDim.x) {
            ghost_done[i] = 0;
            const int v = i == 0u ? -1 : seed[i - 1];
            if (v < 0) { ghost_vox[i] = -1; ghost_active[i] = 0; hlo[i] = 0; hhi[i] = 0; hcount[i] = 0; tcnt[i] = 0; continue; }
            const bool ghost = owner[v] != i;
            ghost_vox[i] = ghost ? v : -1;
            ghost_active[i] = ghost ? 1 : 0;
            hlo[i] = (uint32_t)v; hhi[i] = (uint32_t)v; hcount[i] = 1;
            tl[(size_t)i * HT_CAP] = (uint32_t)v >> 6; tcnt[i] = ghost ? 0u : 1u;
        }
    }
};
// per-frame arguments of the sweep kernels
//
// Dirty tiles.  A sweep changes fewer and fewer voxels (1M-point frame: 38k, 30k, 21k, 15k, 6k, 2.9k,
// 1.4k, 700, 330, 140, 50, ... of 75k), and a voxel whose inputs are the same as in the previous sweep
// ends the sweep unchanged again.  So from the moment a sweep changes at most V >> inc_shift voxels, the
// next one only re-evaluates 64-voxel tiles that were told their inputs changed ("marked").  Inputs of
// R(w) / claim(v): own owner and distance, the neighbours' owners, the neighbours' R, the centroids of the
// neighbours' owners.  Who marks (all push, 27 stores per event, stamp = sweep + 1, no clearing):
//   E1  d_sweep_claim changes (owner, dist) of v          -> R and claim of N(v), next sweep; both helpers dirty (marked by the claiming thread itself)
//   E2  d_centroid recomputes helper h                    -> R and claim of N(leaf) for every leaf of h, next sweep (marked by the helper's wave itself)
//   E3  d_sweep_R_round changes ownR[w] (owner or R bit)  -> claim of N(w) this sweep, R of N(w) next round
// The R rounds iterate a_eval_R_step to its fixed point (unique: R depends on lower owners only); if
// F3DS_R_ROUNDS rounds are not enough, or ghost leaves are active, or the previous sweep changed too much,
// the sweep is "full": the chain-walking d_sweep_R and an all-tiles claim run instead.  Either way the
// state after the sweep is the same bits.
struct SweepFrame {
    SweepView sv;                   // sv.owner / sv.dist: the state, updated in place by d_sweep_claim
    unsigned char* R; uint32_t* ownR;
    uint32_t* owner_out; float* dist_out;     // the same arrays as sv.owner / sv.dist, writable
    unsigned char *ghost_done, *ghost_active; int* ghost_vox; uint32_t *ghost_head, *ghost_next;
    uint32_t *hlo, *hhi, *hcount; float* hc; DevCounters* dc; uint32_t S0;
    uint32_t *tR0, *tR1, *tC0, *tC1;  // tile stamps for the R / claim pass of even and odd sweeps (no arrays: a runtime index would
                                    // push the whole by-value struct into scratch memory)
    uint32_t* tRr;                  // (F3DS_R_ROUNDS - 1) x T stamps for R rounds 1..
    uint32_t* hD;                   // helper stamps: membership changed in this sweep
    uint32_t *tl, *tcnt;            // helper tile lists (HT_CAP entries each) and their lengths
    uint32_t *wl, *wl2;             // V each: voxels whose R needs the chain walker in this (full) sweep, and the retry list
    uint32_t* tmask;                // V: per listed voxel the neighbour slots that carry a thief (a_thief_mask_words), written by the pre-pass of a full sweep
    uint32_t T, thr;                // tiles; a sweep that changes more than thr voxels makes the next one full
    const uint32_t *tile_n1, *tile_ord, *tile_slots;      // one-ring tables of the 128-voxel tiles (written by d_normals): list length, list of ordinals, 27 list positions per voxel
    // the stamp arrays sweep t reads (R round 0 / claim pass) and the ones it marks for sweep t + 1 (ternaries, not an index: see tR0 above)
    __device__ uint32_t* tR_this(uint32_t t) const { return (t & 1u) ? tR1 : tR0; }
    __device__ uint32_t* tC_this(uint32_t t) const { return (t & 1u) ? tC1 : tC0; }
    __device__ uint32_t* tR_next(uint32_t t) const { return (t & 1u) ? tR0 : tR1; }
    __device__ uint32_t* tC_next(uint32_t t) const { return (t & 1u) ? tC0 : tC1; }
};
template <bool ROWS = false>      // ROWS: the lanes hold scattered voxels (a helper's leaves): neighbours from the row-major table
__device__ inline void mark_tiles(const SweepView& s, int v, uint32_t* a, uint32_t* b, uint32_t stamp) {
#pragma unroll
    for (int k0 = 0; k0 < 27; k0 += 9) {            // nine loads in flight, then their stores (27 at once costs too many registers)
        int nu[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) nu[k] = ROWS ? a_nbr_w(s, v, k0 + k) : a_nbr(s, v, k0 + k);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int u = nu[k] >= 0 ? nu[k] : v;           // an absent neighbour marks v's own tile again
            a[u >> 6] = stamp; b[u >> 6] = stamp;
        }
    }
}
// start of sweep t: ghost chains, and whether this sweep may skip clean tiles
struct d_sweep_begin {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 256;
    __device__ void operator()(SweepFrame f, uint32_t t) const {
        __shared__ uint32_t s_n;
        if (threadIdx.x == 0) s_n = 0;
        for (uint32_t h = 1 + threadIdx.x; h <= f.S0; h += blockDim.x) if (f.ghost_vox[h] >= 0) f.ghost_head[f.ghost_vox[h]] = 0u;
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t h = 1 + threadIdx.x; h <= f.S0; h += blockDim.x)
            if (f.ghost_active[h]) { f.ghost_next[h] = atomicExch(&f.ghost_head[f.ghost_vox[h]], h); mine++; }
        if (mine) atomicAdd(&s_n, mine);
        __syncthreads();
        if (threadIdx.x == 0) {
            f.dc->n_ghosts = s_n;
            if (t == 0u) f.dc->sweep_stats[0] = f.dc->sweep_stats[1] = f.dc->sweep_stats[2] = f.dc->sweep_stats[3] = 0u;          // a run of sweeps starts (again: refineSupervoxels)
            if (!a_sweep_begin(sweep_ctl(f.dc), t, s_n, f.thr)) { f.dc->sweep_stats[F3DS_SWEEP_IDLE]++; return; }
            for (int p = 0; p <= F3DS_R_PASSES; ++p) f.dc->rq[p] = 0u;
        }
    }
};
// R pass of a full sweep, part 1: the voxels no lower helper can reach keep their owner for sure (R = true,
// also entered in the memo); the others go on the work list of part 2.  While ghost leaves are active every
// owned voxel goes on the list.
// LDS-staged neighbour tiles.  A workgroup of 256 threads takes two 128-voxel tiles at a time (threads 0..127 / 128..255); per tile the
// one word per one-ring voxel the kernel needs (sweep-start owner for the R pre-pass, ownR for the claim pass) is gathered ONCE into
// LDS through the tile's ordinal list, and every voxel then reads its 27 neighbours from LDS through 16-bit list positions (14 coalesced
// words per voxel instead of 27, and 27 LDS reads instead of 27 gathers from L2).  Position NT_RING1 holds 0 = "no neighbour".
// Tiles whose one-ring overflowed d_normals' tables, and sweeps with ghost leaves, keep the global path (a_has_thief / a_claim).
struct SweepTile {
    uint32_t (*lds)[NT_RING1 + 1];
    uint32_t (*lds2)[NT_RING1 + 1];      // second staged word per one-ring voxel: ghost_head, only while ghost leaves are active
    int half, li;
    // stage src[ord[i]] (and src2[ord[i]] when given) for the one-ring of tile `tl`; returns whether the tile is staged.  Contains two workgroup
    // barriers: every thread of the workgroup calls it the same number of times.
    // (The list entries of a thread, then the words they point at, are requested TOGETHER -- unconditional loads, an entry past the list reads entry 0 -- and
    // before the first barrier: written as a loop over the list the compiler emitted load, wait, load, wait, LDS store per entry, i.e. up to eight dependent
    // trips to L2 per tile where two do.)
    static constexpr int SR = (NT_RING1 + NT_TILE - 1) / NT_TILE;      // list entries per thread
    __device__ bool stage(const SweepFrame& f, uint32_t tl, const uint32_t* src, const uint32_t* src2) {
        uint32_t n1 = SW_TILE_NONE;
        if (f.tile_n1 && tl * (uint32_t)NT_TILE < (uint32_t)f.sv.V) n1 = f.tile_n1[tl];
        const bool tiled = n1 != SW_TILE_NONE;
        uint32_t a[SR], b[SR];
        if (tiled) {
            const uint32_t* ord = f.tile_ord + (size_t)tl * NT_RING1;
            uint32_t u[SR];
#pragma unroll
            for (int k = 0; k < SR; ++k) { const uint32_t i = (uint32_t)(li + k * NT_TILE); u[k] = ord[i < n1 ? i : 0u]; }
#pragma unroll
            for (int k = 0; k < SR; ++k) a[k] = src[u[k]];
            if (src2) {
#pragma unroll
                for (int k = 0; k < SR; ++k) b[k] = src2[u[k]];
            }
        }
        __syncthreads();                                  // the previous tile's readers are done
        if (tiled) {
#pragma unroll
            for (int k = 0; k < SR; ++k) { const uint32_t i = (uint32_t)(li + k * NT_TILE); if (i < n1) { lds[half][i] = a[k]; if (src2) lds2[half][i] = b[k]; } }
            if (li == 0) { lds[half][NT_RING1] = 0u; lds2[half][NT_RING1] = 0u; }
        }
        __syncthreads();
        return tiled;
    }
    // the same for the incremental R rounds: one word per one-ring voxel -- its sweep-start owner if, as far as ownR knows, that owner still holds it at its
    // turn, else 0 -- so that the rounds gather 27 words, not 54, and filter nothing
    __device__ bool stage_held(const SweepFrame& f, uint32_t tl) {
        uint32_t n1 = SW_TILE_NONE;
        if (f.tile_n1 && tl * (uint32_t)NT_TILE < (uint32_t)f.sv.V) n1 = f.tile_n1[tl];
        const bool tiled = n1 != SW_TILE_NONE;
        uint32_t g[SR], r[SR];
        if (tiled) {
            const uint32_t* ord = f.tile_ord + (size_t)tl * NT_RING1;
            uint32_t u[SR];
#pragma unroll
            for (int k = 0; k < SR; ++k) { const uint32_t i = (uint32_t)(li + k * NT_TILE); u[k] = ord[i < n1 ? i : 0u]; }
#pragma unroll
            for (int k = 0; k < SR; ++k) { g[k] = f.sv.owner[u[k]]; r[k] = f.ownR[u[k]]; }
        }
        __syncthreads();
        if (tiled) {
#pragma unroll
            for (int k = 0; k < SR; ++k) { const uint32_t i = (uint32_t)(li + k * NT_TILE); if (i < n1) lds[half][i] = (r[k] & F3DS_OWNR_RTRUE) ? g[k] : 0u; }
            if (li == 0) lds[half][NT_RING1] = 0u;
        }
        __syncthreads();
        return tiled;
    }
    // the staged words of voxel `li`'s 27 neighbours (0 for an absent one); *near2 = some neighbour (or the voxel itself) has a non-zero second word
    __device__ void gather(const SweepFrame& f, uint32_t tl, uint32_t out[27], bool* near2) const {
        uint32_t w[SW_SLOT_WORDS];
        const uint32_t* sp = f.tile_slots + (size_t)tl * SW_SLOT_WORDS * NT_TILE + li;
#pragma unroll
        for (int k = 0; k < SW_SLOT_WORDS; ++k) w[k] = sp[k * NT_TILE];
#pragma unroll
        for (int k = 0; k < 27; ++k) out[k] = lds[half][sw_slot(w, k)];
        if (near2) {
            uint32_t any = 0u;
#pragma unroll
            for (int k = 0; k < 27; ++k) any |= lds2[half][sw_slot(w, k)];
            *near2 = any != 0u;
        }
    }
};
// Ghost leaves (two seeds on one voxel: a handful per frame, alive for the first sweep or two) used to send the WHOLE frame down the general
// paths -- every owned voxel to the chain walker, every voxel through a_claim's ghost-chain loops (27 more dependent gathers each): sweep 0's
// claim pass cost five times a later full sweep's.  A ghost leaf on u only concerns the voxels of N(u): with ghost_head staged beside the
// owners, a voxel with no ghost leaf in its neighbourhood takes the plain path (for R: the ghost clause of its defining equation is empty,
// so "no lower helper reaches it at all" still settles it), the others the general one.  Same results, bit for bit.
// Which of a workgroup's next 64 tile pairs (tp0, tp0 + step, ...: 256 voxels = four stamps each) hold a stamped tile: all 256 stamps are requested at once, one per
// thread, and come back as a 64-bit mask (uniform).  Asked pair by pair -- a load and a __syncthreads_or each -- the "no"s of a late sweep cost a workgroup of a batched
// launch ~20 dependent trips to L2 in a row, which was most of what the late sweeps' claim pass and R rounds took.  Two workgroup barriers: call uniformly.
__device__ inline uint64_t marked_pairs(const uint32_t* stamps, uint32_t stamp, uint32_t tp0, uint32_t step, uint32_t V, uint32_t* s_marked) {
    const uint32_t k = threadIdx.x >> 2, q = threadIdx.x & 3u;      // pair k of the 64, stamp q of its four
    const uint32_t v0 = (tp0 + k * step) * 256u + q * 64u;
    const bool on = v0 < V && stamps[v0 >> 6] == stamp;
    const uint64_t b = __ballot(on);                                // (a wave holds 16 pairs: four lanes each)
    uint32_t m16 = 0;
    for (int i = 0; i < 16; ++i) m16 |= ((uint32_t)(b >> (4 * i)) & 0xFu) ? 1u << i : 0u;
    __syncthreads();                                                // (the previous chunk's mask has been read)
    if (threadIdx.x < 2) s_marked[threadIdx.x] = 0u;
    __syncthreads();
    if (lane_id() == 0) atomicOr(&s_marked[threadIdx.x >> 7], m16 << (16u * ((threadIdx.x >> 6) & 1u)));
    __syncthreads();
    return (uint64_t)s_marked[0] | ((uint64_t)s_marked[1] << 32);
}
struct d_sweep_R_pre {
    static constexpr int BLOCK = 256;
    __device__ void operator()(SweepFrame f, unsigned char tag, uint32_t t) const {
        if (!a_sweep_is_full(sweep_ctl(f.dc), t)) return;
        __shared__ uint32_t nown[2][NT_RING1 + 1], ngh[2][NT_RING1 + 1];
        const SweepView s = f.sv;
        const bool ghosts = *s.n_ghosts != 0u;
        const int lane = lane_id();
        SweepTile st{nown, ngh, (int)(threadIdx.x >> 7), (int)(threadIdx.x & 127u)};
        for (uint32_t tp = BIX; tp * 256u < (uint32_t)s.V; tp += gridDim.x) {
            const uint32_t tl = tp * 2u + (uint32_t)st.half;
            const int v = (int)(tl * (uint32_t)NT_TILE) + st.li;
            const bool tiled = st.stage(f, tl, s.owner, ghosts ? s.ghost_head : nullptr);
            bool later = false;
            if (v < s.V) {
                const uint32_t o = s.owner[v];
                if (o == 0u) f.ownR[v] = 0u;
                else {
                    // the slots that carry a thief (round 6: the chain walker works on these masks, a_eval_R_mask); a ghost leaf on v or around it (known exactly on
                    // staged tiles) is a flag in the mask: the walker looks at it
                    uint32_t mask;
                    if (tiled) {
                        uint32_t og[27];
                        bool near = false;
                        st.gather(f, tl, og, ghosts ? &near : nullptr);
                        mask = a_thief_mask_words(s, v, o, og) | (near ? F3DS_TMASK_GHOST : 0u);      // (the owners of the one-ring, v's own among them: only labels below o count)
                    } else mask = a_thief_mask(s, v) | (ghosts ? F3DS_TMASK_GHOST : 0u);
                    if (mask == 0u) { f.ownR[v] = o | F3DS_OWNR_RTRUE; f.R[v] = (unsigned char)((tag << 2) | F3DS_R_TRUE); }
                    else { f.tmask[v] = mask; later = true; }
                }
            }
            const uint64_t m = __ballot(later);
            if (m) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&f.dc->rq[0], (uint32_t)__popcll(m));
                base = __builtin_amdgcn_readfirstlane(base);
                if (later) f.wl[base + (uint32_t)__popcll(m & lanemask_lt())] = (uint32_t)v;
            }
        }
    }
};
// part 2: the chain walker on the work list.  A voxel whose dependency chain is deeper than the walker's stack
// (F3DS_R_STACK) is put on the list of the next pass: by then the lower part of its chain has been settled and
// memoised by the voxels down there, so every pass reaches F3DS_R_STACK levels further up.
struct d_sweep_R {
    static constexpr int BLOCK = 256;
    __device__ void operator()(SweepFrame f, unsigned char tag, uint32_t t, uint32_t pass) const {
        if (!a_sweep_is_full(sweep_ctl(f.dc), t)) return;
        const SweepView s = f.sv;
        const uint32_t* src = (pass & 1u) ? f.wl2 : f.wl;
        uint32_t* dst = (pass & 1u) ? f.wl : f.wl2;
        if (!a_sweep_full_from_start(sweep_ctl(f.dc), t)) {
            // The sweep started incremental and its last R round still changed ownR (d_sweep_R_round): no pre-pass has run, the work list is empty and ownR is
            // somewhere between the sweep-start state and the fixed point.  Pass 0 then derives R for EVERY voxel with the memoised walker (nothing carries this
            // sweep's tag yet, so every entry reads "unknown"; no ghost leaf is active in an incremental sweep); chains deeper than its stack go to the next pass
            // as usual.  Rare (two rounds settle every frame seen so far) and slow, but the sweep ends in the bits a full sweep gives.
            if (pass != 0u) return;      // (F3DS_R_PASSES > 1: the later passes find their list through rq[pass] below)
            for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < (uint32_t)s.V; v += gridDim.x * blockDim.x) {
                const uint32_t o = s.owner[v];
                if (o == 0u) { f.ownR[v] = 0u; continue; }
                int overflow = 0;
                const bool r = a_eval_R(s, (int)v, f.R, tag, &overflow, false);
                if (!overflow) f.ownR[v] = o | (r ? F3DS_OWNR_RTRUE : 0u);
                else dst[atomicAdd(&f.dc->rq[pass + 1u], 1u)] = v;
            }
            return;
        }
        const uint32_t n = f.dc->rq[pass];
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const uint32_t e = src[i];
            const int v = (int)(e & 0x7fffffffu);
            int overflow = 0;
            const uint32_t o = s.owner[v];
            const bool r = a_eval_R_mask(s, v, f.R, tag, f.tmask, &overflow);
            if (!overflow) f.ownR[v] = o | (r ? F3DS_OWNR_RTRUE : 0u);
            else dst[atomicAdd(&f.dc->rq[pass + 1u], 1u)] = e;
        }
    }
};
// part 3, normally idle: what is still unsettled after F3DS_R_PASSES passes (dependency chains of hundreds of levels:
// tiny supervoxels, seed / voxel ratios of 2-3, whose labels fall monotonically along a path) is finished by ONE
// workgroup that keeps passing over its list until it is empty; every pass settles at least F3DS_R_STACK more levels.
struct d_sweep_R_tail {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 256;       // not 1024: with ~128 VGPRs that would need an empty CU, and while other batches fill the
                                            // chip this (normally idle) launch then waits ~1 ms for one, 16 times per batch
    __device__ void operator()(SweepFrame f, unsigned char tag, uint32_t t) const {
        // (the one place that sees how the sweep's R phase went, once per sweep and frame: by now the rounds have either converged or turned the sweep full)
        const SweepCtl ctl = sweep_ctl(f.dc);
        if (a_sweep_is_idle(ctl, t)) return;
        if (threadIdx.x == 0) f.dc->sweep_stats[a_sweep_kind(ctl, t)]++;
        if (!a_sweep_is_full(ctl, t)) return;
        __shared__ uint32_t s_n, s_next;
        const SweepView s = f.sv;
        const bool masks = a_sweep_full_from_start(ctl, t);      // (the list comes from the pre-pass: every entry has its thief mask; else from the fallback pass of d_sweep_R)
        uint32_t q = F3DS_R_PASSES;
        if (threadIdx.x == 0) { s_n = f.dc->rq[F3DS_R_PASSES]; s_next = 0; }
        __syncthreads();
        for (uint32_t round = 0; round < 1000000u; ++round, ++q) {
            const uint32_t n = s_n;
            if (n == 0u) break;
            const uint32_t* src = (q & 1u) ? f.wl2 : f.wl;
            uint32_t* dst = (q & 1u) ? f.wl : f.wl2;
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
                const uint32_t e = src[i];
                const int v = (int)(e & 0x7fffffffu);
                int overflow = 0;
                const uint32_t o = s.owner[v];
                const bool r = masks ? a_eval_R_mask(s, v, f.R, tag, f.tmask, &overflow) : a_eval_R(s, v, f.R, tag, &overflow, false);
                if (!overflow) f.ownR[v] = o | (r ? F3DS_OWNR_RTRUE : 0u);
                else dst[atomicAdd(&s_next, 1u)] = e;
            }
            __threadfence();
            __syncthreads();
            if (threadIdx.x == 0) { if (s_next == n) f.dc->r_overflow = 1; s_n = s_next == n ? 0u : s_next; s_next = 0; }     // no progress cannot happen; do not spin if it does
            __syncthreads();
        }
    }
};
// round r of the incremental R pass of sweep t: one wave per marked tile
struct d_sweep_R_round {
    static constexpr int BLOCK = 256;
    static constexpr int WAVES_PER_SIMD = 6;      // (80 VGPRs, 8 bytes of scratch; occupancy 7: slower, 5 -- the compiler's own choice -- too: profiles/r4_ab_bench.txt 24)
    __device__ void operator()(SweepFrame f, uint32_t t, uint32_t r, uint32_t nrounds) const {      // nrounds: rounds recorded for this sweep (F3DS_R_ROUNDS; fewer under F3DS_R_ROUNDS_RUN, a test switch)
        const SweepCtl ctl = sweep_ctl(f.dc);
        if (a_sweep_is_full(ctl, t) || a_sweep_is_idle(ctl, t)) return;
        __shared__ uint32_t nown[2][NT_RING1 + 1];
        const SweepView s = f.sv;
        const uint32_t stamp = t + 1u;
        const uint32_t* cur = r == 0u ? f.tR_this(t) : f.tRr + (size_t)(r - 1u) * f.T;
        const bool last = r + 1u == nrounds;
        uint32_t* tc = f.tC_this(t);
        uint32_t* nxt = last ? tc : f.tRr + (size_t)r * f.T;
        SweepTile st{nown, nown, (int)(threadIdx.x >> 7), (int)(threadIdx.x & 127u)};
        __shared__ uint32_t s_marked[2];
        const uint32_t bix = BIX, step = gridDim.x;
        for (uint32_t tp0 = bix; tp0 * 256u < (uint32_t)s.V; tp0 += 64u * step)
          for (uint64_t marked = marked_pairs(cur, stamp, tp0, step, (uint32_t)s.V, s_marked); marked; marked &= marked - 1ull) {
            const uint32_t tp = tp0 + (uint32_t)__builtin_ctzll(marked) * step;
            const uint32_t tl = tp * 2u + (uint32_t)st.half;
            const int v = (int)(tl * (uint32_t)NT_TILE) + st.li;
            const bool active = v < s.V && cur[v >> 6] == stamp;      // (uniform per wave)
            // (the staged words may be older than what another workgroup writes in this very round: whoever changes ownR[u] marks N(u) for the next
            // round, and a change in the last round sends the sweep to the chain walker -- reading early is as good as reading late)
            const bool tiled = st.stage_held(f, tl);
            if (!active) continue;
            const uint32_t o = s.owner[v];
            bool keeps;
            if (tiled) {
                uint32_t og[27];
                st.gather(f, tl, og, nullptr);
                keeps = o != 0u && !a_has_thief_words(s, v, o, og);
            } else keeps = a_eval_R_step(s, f.ownR, v);
            const uint32_t nw = o | (keeps ? F3DS_OWNR_RTRUE : 0u);
            if (nw != f.ownR[v]) {
                f.ownR[v] = nw;
                mark_tiles(s, v, nxt, tc, stamp);
                if (last) a_sweep_turn_full(ctl, t);      // not converged: the chain walker redoes this sweep's R
            }
        }
    }
};
// The first kernel of a sweep's R phase: the pre-pass of a full sweep or round 0 of an incremental one -- each body returns at once when the sweep is of the other
// kind (device-side decision, d_sweep_begin), so one dispatch serves both (two until round 4: ~100 us of latency per dispatch and call with other calls on the chip).
#ifndef F3DS_RFIRST_WPS
#define F3DS_RFIRST_WPS 6
#endif
struct d_sweep_R_first {
    static constexpr int BLOCK = 256;
    static constexpr int WAVES_PER_SIMD = F3DS_RFIRST_WPS;      // (80 VGPRs, 8 bytes of scratch; occupancy 7: slower, 5 -- the compiler's own choice -- too: profiles/r4_ab_bench.txt 24)
    __device__ void operator()(SweepFrame f, unsigned char tag, uint32_t t, uint32_t rounds) const {
        d_sweep_R_pre{}(f, tag, t);
        if (rounds) d_sweep_R_round{}(f, t, 0u, rounds);
    }
};
struct d_sweep_claim {
    static constexpr int BLOCK = 256;
    // (no register bound here: at 80 VGPRs / occupancy 6 the kernel alone is 5 % faster, but its 40 bytes of scratch per lane are 11 MB of HBM traffic per frame, and
    // with other calls in flight the bench does not move: profiles/r4_ab_bench.txt 24)
    __device__ void operator()(SweepFrame f, uint32_t t) const {
        __shared__ uint32_t nr[2][NT_RING1 + 1], ngh[2][NT_RING1 + 1];
        const SweepCtl ctl = sweep_ctl(f.dc);
        if (a_sweep_is_idle(ctl, t)) return;
        const SweepView s = f.sv;
        const bool full = a_sweep_is_full(ctl, t);
        const bool marks = a_sweep_marks(ctl, t);
        const bool ghosts = *s.n_ghosts != 0u;
        const uint32_t* cur = f.tC_this(t);
        uint32_t changed = 0;
        SweepTile st{nr, ngh, (int)(threadIdx.x >> 7), (int)(threadIdx.x & 127u)};
        __shared__ uint32_t s_marked[2];
        const uint32_t bix = BIX, step = gridDim.x;
        for (uint32_t tp0 = bix; tp0 * 256u < (uint32_t)s.V; tp0 += 64u * step) {
          uint64_t marked = ~0ull;
          if (!full) marked = marked_pairs(cur, t + 1u, tp0, step, (uint32_t)s.V, s_marked);
          for (; marked; marked &= marked - 1ull) {
            const uint32_t tp = tp0 + (uint32_t)__builtin_ctzll(marked) * step;
            if (tp * 256u >= (uint32_t)s.V) break;
            const uint32_t tl = tp * 2u + (uint32_t)st.half;
            const int v = (int)(tl * (uint32_t)NT_TILE) + st.li;
            const bool active = v < s.V && (full || cur[v >> 6] == t + 1u);      // (uniform per wave: a stamp covers 64 voxels)
            const bool tiled = st.stage(f, tl, f.ownR, ghosts ? s.ghost_head : nullptr);
            if (!active) continue;
            uint32_t o; float d;
            bool plain = false;
            if (tiled) {
                uint32_t cand[27];
                bool near = false;
                st.gather(f, tl, cand, ghosts ? &near : nullptr);
                if (!near) {        // (no ghost leaf on v or around it: the ghost-chain loops of a_claim have nothing to add)
                    a_claim_words(s, v, cand, &o, &d);      // (raw ownR words: the search itself keeps the R-true ones)
                    plain = true;
                }
            }
            if (!plain) a_claim(s, f.ownR, v, &o, &d, f.ghost_done);
            const uint32_t o0 = s.owner[v];
            bool gained = false;
            if (o != o0 || __float_as_uint(d) != __float_as_uint(s.dist[v])) {
                f.owner_out[v] = o; f.dist_out[v] = d;
                if (o != o0) {
                    gained = o != 0u;
                    if (o0 != 0u) f.hD[o0] = t + 1u;
                }
                // E1 of the dirty-tile scheme on the spot (a kernel of its own, d_claim_mark, until round 4: a dispatch costs a call ~100 us of latency with other
                // calls' kernels on the chip, 15 times per call): the tiles around a voxel that changed look again in the next sweep
                if (marks) mark_tiles(s, v, f.tR_next(t), f.tC_next(t), t + 2u);
                changed++;
            }
            // A helper's books (ordinal window, dirty stamp, tile list) once per helper and WAVE, not once per voxel: the 64 voxels of a wave are one tile of the
            // tile lists, and the lanes that go to one helper are found with a ballot.  Per voxel this was three L2 atomics on a handful of addresses per helper --
            // 38-65 k voxels change hands per frame in the first sweeps, and sweep 0's claim pass took twice a late full sweep's time.
            for (uint64_t todo = __ballot(gained); todo;) {       // (the active lanes of the wave are here together: `active` is uniform per wave)
                const int first = __builtin_ctzll(todo);
                const uint32_t og = (uint32_t)__builtin_amdgcn_readlane((int)o, first);
                const uint64_t peers = __ballot(gained && o == og);
                if (lane_id() == first) {
                    const uint32_t vmax = (uint32_t)v + (uint32_t)(63 - __builtin_clzll(peers)) - (uint32_t)first;
                    atomicMin(&f.hlo[og], (uint32_t)v); atomicMax(&f.hhi[og], vmax); f.hD[og] = t + 1u;
                    const uint32_t pos = atomicAdd(&f.tcnt[og], 1u);
                    if (pos < HT_CAP) f.tl[(size_t)og * HT_CAP + pos] = (uint32_t)v >> 6;
                }
                todo &= ~peers;
            }
          }
        }
    #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) changed += __shfl_xor(changed, d, 64);
        if (lane_id() == 0 && changed) atomicAdd(ctl.n_changed, changed);
    }
};
// Sorted distinct tiles that can hold leaves of a helper (its list plus the tile of its ghost leaf), into
// srt[] (LDS of this wave).  Returns how many, or -1 when the list overflowed.
__device__ inline int helper_tile_list(const uint32_t* tl, uint32_t cnt, int gv, uint32_t* srt) {
    const uint32_t n = cnt + (gv >= 0 ? 1u : 0u);
    if (cnt > HT_CAP) return -1;
    const uint32_t lane = (uint32_t)lane_id();
    if (n <= 64u) {      // the usual case: one entry per lane
        uint32_t tid = 0xFFFFFFFFu;
        if (lane < cnt) tid = tl[lane];
        else if (lane == cnt && gv >= 0) tid = (uint32_t)gv >> 6;
        bool dup = lane >= n;
        for (uint32_t j = 0; j + 1u < n; ++j) { const uint32_t tj = __builtin_amdgcn_readlane(tid, j); if (j < lane && tj == tid) dup = true; }
        const uint64_t keep = __ballot(!dup);
        uint32_t rank = 0;
        for (uint64_t m = keep; m; m &= m - 1ull) { const uint32_t tj = __builtin_amdgcn_readlane(tid, (uint32_t)__builtin_ctzll(m)); rank += tj < tid; }
        if (!dup) srt[rank] = tid;
        wave_lds_sync();
        return __popcll(keep);
    }
    // more raw entries than lanes: the distinct ones are collected 64 entries a round (srt[0..nd) unsorted), then sorted
    uint32_t nd = 0;
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t idx = base + lane;
        uint32_t tid = 0xFFFFFFFFu;
        if (idx < cnt) tid = tl[idx];
        else if (idx == cnt && gv >= 0) tid = (uint32_t)gv >> 6;
        bool dup = idx >= n;
        for (uint32_t j = 0; j < 64u; ++j) { const uint32_t tj = __builtin_amdgcn_readlane(tid, j); if (j < lane && tj == tid) dup = true; }
        for (uint32_t j = 0; j < nd; ++j) if (srt[j] == tid) dup = true;
        const uint64_t keep = __ballot(!dup);
        const uint32_t k = (uint32_t)__popcll(keep);
        if (nd + k > 64u) return -1;          // (uniform)
        wave_lds_sync();
        if (!dup) srt[nd + (uint32_t)__popcll(keep & lanemask_lt())] = tid;
        nd += k;
        wave_lds_sync();
    }
    const uint32_t mine = lane < nd ? srt[lane] : 0xFFFFFFFFu;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < nd; ++j) { const uint32_t tj = __builtin_amdgcn_readlane(mine, j); rank += tj < mine; }
    wave_lds_sync();
    if (lane < nd) srt[rank] = mine;
    wave_lds_sync();
    return (int)nd;
}
// Ascending sort of the 16 values a DPP row holds (one per lane; every lane of the wave active): the flip variant of the bitonic network -- partner = mirror image inside
// a block of 2, 4, 8, 16 lanes, then partners at distance 4, 2, 1 -- so that every exchange is one DPP lane pattern (quad permutes, half-row and row mirrors, row rotations).
template <int CTRL> __device__ __forceinline__ uint32_t row_dpp_u32(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xF, 0xF, false); }
__device__ inline uint32_t row_sort16(uint32_t x, const uint32_t l16) {
#define F3DS_CX(CTRL, bit) { const uint32_t p_ = row_dpp_u32<CTRL>(x); const uint32_t lo_ = x < p_ ? x : p_, hi_ = x < p_ ? p_ : x; x = (l16 & (bit)) ? hi_ : lo_; }
    F3DS_CX(0xB1, 1u)                                                   // blocks of 2
    F3DS_CX(0x1B, 2u) F3DS_CX(0xB1, 1u)                                 // blocks of 4: quad mirror, then distance 1
    F3DS_CX(0x141, 4u) F3DS_CX(0x4E, 2u) F3DS_CX(0xB1, 1u)              // blocks of 8: half-row mirror, distances 2, 1
    F3DS_CX(0x140, 8u)                                                  // the row: row mirror ...
    { const uint32_t a_ = row_dpp_u32<0x12C>(x), b_ = row_dpp_u32<0x124>(x);      // ... distance 4: lane + 4 (rotate by 12) for the lower lane of a pair, lane - 4 for the upper
      const uint32_t p_ = (l16 & 4u) ? b_ : a_; const uint32_t lo_ = x < p_ ? x : p_, hi_ = x < p_ ? p_ : x; x = (l16 & 4u) ? hi_ : lo_; }
    F3DS_CX(0x4E, 2u) F3DS_CX(0xB1, 1u)
#undef F3DS_CX
    return x;
}
// The leaves of the helper a 16-lane row holds (h; `tid` = lane l16's entry of its raw tile list, 0xFFFFFFFF for none; gv = its ghost leaf or -1), in ascending ordinal
// into qleaf[0 ..] (at most cap entries are written; `spare` = the index writes of non-leaves go to).  Returns the number of leaves; *nd_out = distinct tiles (left in
// qt[row][0 .. nd), ascending), *kept_out = bit i set iff tile i holds a leaf the helper OWNS.  Every lane of the wave must call it (DPP sort, ballots).
__device__ inline uint32_t row_leaves(const uint32_t* owner, const uint32_t V, const uint32_t h, const uint32_t tid, const int gv, uint32_t (*qt)[16], uint32_t* qleaf,
                                  const uint32_t cap, const uint32_t spare, uint32_t* nd_out, uint32_t* kept_out) {
    const uint32_t lane = (uint32_t)lane_id(), row = lane >> 4, l16 = lane & 15u;
    // distinct tiles, ascending
    const uint32_t srt = row_sort16(tid, l16);
    const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp((int)~srt, (int)srt, 0x111, 0xF, 0xF, false);      // row_shr:1 (lane 0 of a row keeps ~srt: never equal)
    const bool keep = srt != 0xFFFFFFFFu && srt != prev;
    const uint32_t kbits = (uint32_t)(__ballot(keep) >> (row * 16u)) & 0xFFFFu;
    const uint32_t nd = (uint32_t)__popc(kbits);
    if (keep) qt[row][__popc(kbits & ((1u << l16) - 1u))] = srt;
    wave_lds_sync();
    const uint32_t ndmax = a_umax(a_umax((uint32_t)__builtin_amdgcn_readlane((int)nd, 0), (uint32_t)__builtin_amdgcn_readlane((int)nd, 16)),
                                  a_umax((uint32_t)__builtin_amdgcn_readlane((int)nd, 32), (uint32_t)__builtin_amdgcn_readlane((int)nd, 48)));
    // per tile: the owner words of its 64 voxels as four loads of 16 consecutive words (lane l16 holds voxels l16, 16 + l16, ...), the four ballots give every lane of
    // the row the tile's leaf mask in voxel order; a leaf's place in the list = leaves before it (population counts)
    const uint32_t below = (1u << l16) - 1u, below_hi = (below << 16) | 0xFFFFu;
    uint32_t count = 0u, keptbits = 0u;
    for (uint32_t i0 = 0; i0 < ndmax; i0 += 4u) {      // (wave-uniform trip count: the ballots below want every lane; four tiles' owner words in flight)
        const uint4 t4 = *reinterpret_cast<const uint4*>(&qt[row][i0]);
        const uint32_t tile4[4] = {t4.x, t4.y, t4.z, t4.w};
        uint32_t own[4][4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint32_t v0 = (i0 + k < nd ? tile4[k] : 0u) * 64u + l16;
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) { const uint32_t v = v0 + 16u * c; own[k][c] = owner[v < V ? v : V - 1u]; }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (i0 + k >= ndmax) break;      // (uniform)
            const uint32_t i = i0 + k;
            const bool on = i < nd;
            const uint32_t tile = on ? tile4[k] : 0u;
            const uint32_t v0 = tile * 64u + l16;
            uint32_t r[4];
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) r[c] = (uint32_t)(__ballot(on && v0 + 16u * c < V && own[k][c] == h) >> (row * 16u)) & 0xFFFFu;
            uint32_t lo = r[0] | (r[1] << 16), hi = r[2] | (r[3] << 16);
            if (on && (lo | hi)) keptbits |= 1u << i;      // (the tile stays on the helper's list iff it holds a leaf the helper OWNS)
            const uint32_t g = (uint32_t)gv - tile * 64u;      // the ghost leaf, if it sits in this tile
            if (on && gv >= 0 && g < 64u) { if (g < 32u) lo |= 1u << g; else hi |= 1u << (g - 32u); }
            const uint32_t nlo = (uint32_t)__popc(lo);
            const uint32_t p[4] = {(uint32_t)__popc(lo & below), (uint32_t)__popc(lo & below_hi), nlo + (uint32_t)__popc(hi & below), nlo + (uint32_t)__popc(hi & below_hi)};
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) {
                const uint32_t bit = ((c < 2u ? lo : hi) >> (16u * (c & 1u) + l16)) & 1u;
                const uint32_t at = count + p[c];
                qleaf[bit && at < cap ? at : spare] = v0 + 16u * c;      // (no leaf here: the write goes to the spare entry at the end)
            }
            count += nlo + (uint32_t)__popc(hi);
        }
    }
    *nd_out = nd; *kept_out = keptbits;
    return count;
}
// SupervoxelHelper::updateCentroid.  The helper's leaves are the voxels it owns (plus its ghost leaf); they are visited in ascending
// ordinal, i.e. std::set<leaf, compareLeaves> order, tile by tile.  A helper whose leaf set did not change keeps its centroid (same
// leaves, same order, same bits).
//
// FOUR helpers per wave, one per 16-lane row (round 6; one helper per wave until then).  A supervoxel of the bench frame holds 27 voxels in 4-8 tiles: a whole wave
// per helper left three lanes in four idle in every step and the kernel was bound by the instructions it issued (~700 per helper; 28 us per frame).  A row now does for
// its helper what the wave did: its tile list (<= 16 raw entries) sorted and deduplicated with a DPP sorting network; per tile 64 owner words as four coalesced loads of
// 16, the leaves' places in the ordered list from population counts of the tile's 64-bit leaf mask; the nine ordered sums on lanes 0..8 of the row straight from the
// leaves' feature rows, eight in flight.  A helper that does not fit a row (more than 16 list entries or more than QL leaves: supervoxels of > 64 voxels, BASELINE config 4)
// takes the wave-wide path `one` as before.  Same leaves in the same order: same bits.
struct d_centroid {
    static constexpr int BLOCK = 256;
#ifndef F3DS_CENTROID_WPS
#define F3DS_CENTROID_WPS 5
#endif
    static constexpr int WAVES_PER_SIMD = F3DS_CENTROID_WPS;
    __device__ void operator()(SweepFrame f, uint32_t t) const {
        __shared__ __attribute__((aligned(16))) float tiles[4][64][12];              // (wave-wide path: feature rows of up to 64 leaves)
        __shared__ uint32_t srts[4][64], leafs[4][64];
        // the row path's tables live in the wave-wide path's row buffer (a wave is in one path or the other): per wave and row the helper's distinct tiles, ascending
        // (16 words); its leaves, ascending (QL + 32: the sums read F3DS_CEN_ROUND entries at a time); the nine sums (12 words)
        static_assert(4u * (16u + QL + 32u + 12u) <= 64u * 12u, "the row path's tables fit the wave-wide path's row buffer");
        uint32_t (*const q_tile)[16] = reinterpret_cast<uint32_t (*)[16]>(&tiles[threadIdx.x >> 6][0][0]);
        uint32_t (*const q_leaf)[QL + 32] = reinterpret_cast<uint32_t (*)[QL + 32]>(&tiles[threadIdx.x >> 6][0][0] + 4 * 16);
        float (*const q_fin)[12] = reinterpret_cast<float (*)[12]>(&tiles[threadIdx.x >> 6][0][0] + 4 * 16 + 4 * (QL + 32));
        const int wv = (int)(threadIdx.x >> 6);
        if (a_sweep_is_idle(sweep_ctl(f.dc), t)) return;
        // Which helpers have anything to do is asked for 64 of them at once, one per lane (late sweeps: a handful of ~1 500 do; asked helper by
        // helper, every "no" cost the wave a trip to L2); those that do are taken four at a time.  The 64 are the 16 groups of four consecutive helpers
        // the wave would own if the groups were dealt round-robin over all waves of the frame's launch: a full sweep (every helper has work) is spread
        // evenly, whatever the number of waves.
        const uint32_t W = gridDim.x * 4u, w = BIX * 4u + (uint32_t)wv;
        // A sweep that marks tiles for the next one (few helpers change any more: a tenth of them from the eighth sweep on) keeps a wave per helper: what such a launch
        // takes is the chain of dependent loads behind one helper -- the 27 + 54 accesses of mark_tiles per leaf on top of the sums --, and a row walks it four
        // times slower than a wave (measured per launch of 192 frames, sweeps 9..15: 70-210 us a wave per helper, 160-280 us four per wave).
        // (and so do frames of big supervoxels -- 48 voxels and more on average, BASELINE config 4 has 190: most helpers would overflow a row's 64 leaves)
        const bool by_wave = a_sweep_marks_after_claim(sweep_ctl(f.dc), t, f.thr) || (uint32_t)f.sv.V > BY_WAVE_RATIO * f.S0;
        if (by_wave) {
            // (neighbouring labels are neighbours in space and change together: the four helpers of a group go to the four waves of a workgroup, side by side)
            const uint32_t bix = BIX, stp = gridDim.x;
            for (uint32_t hb0 = bix; hb0 * 4u < f.S0; hb0 += 64u * stp) {
                const uint32_t h = (hb0 + (uint32_t)lane_id() * stp) * 4u + (uint32_t)wv + 1u;
                bool todo = false;
                if (h <= f.S0) todo = t == 0u || f.hD[h] == t + 1u || f.ghost_active[h] != 0;
                for (uint64_t m = __ballot(todo); m; m &= m - 1ull) one(f, t, (hb0 + (uint32_t)__builtin_ctzll(m) * stp) * 4u + (uint32_t)wv + 1u, tiles[wv], srts[wv], leafs[wv]);
            }
            return;
        }
        const uint32_t lq = (uint32_t)lane_id() >> 2, lm = (uint32_t)lane_id() & 3u;
        for (uint32_t q0 = w; q0 * 4u < f.S0; q0 += 16u * W) {
            const uint32_t hc_ = (q0 + lq * W) * 4u + lm + 1u;
            bool todo = false;
            if (hc_ <= f.S0) todo = t == 0u || f.hD[hc_] == t + 1u || f.ghost_active[hc_] != 0;
            for (uint64_t m = __ballot(todo); m;) {
                uint32_t hs[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t bit = (uint32_t)__builtin_ctzll(m | (1ull << 63));
                    hs[r] = m ? (q0 + (bit >> 2) * W) * 4u + (bit & 3u) + 1u : 0u;
                    m &= m - 1ull;
                }
                const uint32_t big = quad(f, t, hs, q_tile, q_leaf, q_fin);
                if (big) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (big & (1u << r)) one(f, t, hs[r], tiles[wv], srts[wv], leafs[wv]);
                }
            }
        }
    }
    // four helpers (hs[row]; 0 = none), one per row of the wave.  Returns a bit per row whose helper has to take the wave-wide path instead (nothing was written for it).
    __device__ uint32_t quad(const SweepFrame& f, uint32_t t, const uint32_t hs[4], uint32_t (*qt)[16], uint32_t (*ql)[QL + 32], float (*qf)[12]) const {
        const uint32_t lane = (uint32_t)lane_id(), row = lane >> 4, l16 = lane & 15u;
        const uint32_t h = row == 0u ? hs[0] : (row == 1u ? hs[1] : (row == 2u ? hs[2] : hs[3]));
        const bool live = h != 0u;
        const uint32_t V = (uint32_t)f.sv.V;
        const uint32_t* owner = f.owner_out;
        // the helper's books (every lane of the row reads the same words)
        // (one round of loads, none behind a test of another: h = 0 is a valid row of every array)
        const unsigned char ga_ = f.ghost_active[h], gd_ = f.ghost_done[h];
        const int gvx_ = f.ghost_vox[h];
        const uint32_t cnt = f.tcnt[h];
        uint32_t* tl = f.tl + (size_t)h * HT_CAP;
        const uint32_t tl_ = tl[l16];
        const bool gact = live && ga_ != 0 && !gd_;
        const int gv = gact ? gvx_ : -1;
        const bool fits = live && cnt + (gv >= 0 ? 1u : 0u) <= HT_ROW;      // (row-uniform; a list that overflowed reads HT_CAP + 1)
        uint32_t tid = 0xFFFFFFFFu;
        if (fits) { if (l16 < cnt) tid = tl_; else if (l16 == cnt && gv >= 0) tid = (uint32_t)gv >> 6; }
        uint32_t nd, keptbits;
        const uint32_t count = row_leaves(owner, V, h, tid, gv, qt, ql[row], QL, QL + 31u, &nd, &keptbits);
        const uint32_t below = (1u << l16) - 1u;
        const bool big_row = live && (!fits || count > QL);
        const bool run = live && !big_row;
        wave_lds_sync();
        if (run) { ql[row][count + l16] = ql[row][0]; ql[row][count + 16u + l16] = ql[row][0]; }      // (the sums read 16 or 32 entries at a time: the tail points at a real voxel, its value is not added)
        wave_lds_sync();
        // (no tile marks here: a sweep that marks takes the wave-per-helper path, operator())
        // the nine ordered sums: lane k < 9 of the row adds component k of the leaves' feature rows in list order, eight loads in flight
        float acc = 0.0f;
        if (run && l16 < 9u) {
            const float* vf = f.sv.vf + l16;
#ifndef F3DS_CEN_ROUND
#define F3DS_CEN_ROUND 16
#endif
            constexpr int RN = F3DS_CEN_ROUND;
            for (uint32_t j0 = 0; j0 < count; j0 += (uint32_t)RN) {
                uint32_t lf[RN];
#pragma unroll
                for (int k = 0; k < RN; k += 4) { const uint4 l4 = *reinterpret_cast<const uint4*>(&ql[row][j0 + (uint32_t)k]); lf[k] = l4.x; lf[k + 1] = l4.y; lf[k + 2] = l4.z; lf[k + 3] = l4.w; }
                float x[RN];
#pragma unroll
                for (int k = 0; k < RN; ++k) x[k] = vf[(size_t)lf[k] * 12];
#pragma unroll
                for (int k = 0; k < RN; ++k) if (j0 + (uint32_t)k < count) acc += x[k];
            }
            qf[row][l16] = acc;
        }
        wave_lds_sync();
        if (run) {
            if (l16 == 0u) { f.ghost_active[h] = gact ? 1 : 0; f.ghost_done[h] = 0; f.hcount[h] = count; f.tcnt[h] = (uint32_t)__popc(keptbits); }
            // the list is rewritten exactly: the tiles that hold a leaf the helper owns, ascending (lane i of the row holds tile i)
            if (l16 < nd && ((keptbits >> l16) & 1u)) tl[__popc(keptbits & below)] = qt[row][l16];
            if (count != 0u && l16 < 12u) {
                // a_centroid_finish (f3ds_algo.h) with its nine divisions side by side: lane k < 6 divides sum k by the count, lanes 6..8 the normal's components by its length
                const float nx = qf[row][6], ny = qf[row][7], nz = qf[row][8];
                const float z = (nx * nx + ny * ny) + (nz * nz + 0.0f);
                float den = (float)count;
                bool divide = true;
                if (l16 >= 6u) { divide = z > 0.0f; den = divide ? n_sqrtf(z) : 1.0f; }
                const float res = divide ? acc / den : acc;
                f.hc[(size_t)h * 12 + l16] = l16 < 9u ? res : 0.0f;
            }
        }
        wave_lds_sync();      // (the row tables are reused by the wave's next four helpers)
#ifdef F3DS_CEN_STATS
        {
            const uint32_t cmax = a_umax(a_umax((uint32_t)__builtin_amdgcn_readlane((int)count, 0), (uint32_t)__builtin_amdgcn_readlane((int)count, 16)),
                                         a_umax((uint32_t)__builtin_amdgcn_readlane((int)count, 32), (uint32_t)__builtin_amdgcn_readlane((int)count, 48)));
            if (lane == 0u) { atomicAdd(&f.dc->cen_stats[0], 1u); atomicAdd(&f.dc->cen_stats[4], ndmax); atomicAdd(&f.dc->cen_stats[7], cmax); }
            if (l16 == 0u && live) { atomicAdd(&f.dc->cen_stats[1], 1u); if (!fits) atomicAdd(&f.dc->cen_stats[2], 1u); else if (count > QL) atomicAdd(&f.dc->cen_stats[3], 1u);
                                     atomicAdd(&f.dc->cen_stats[5], nd); atomicAdd(&f.dc->cen_stats[6], count); }
        }
#endif
        uint32_t big = 0u;
        const uint64_t bb = __ballot(big_row);
#pragma unroll
        for (int r = 0; r < 4; ++r) if ((bb >> (16 * r)) & 1ull) big |= 1u << r;
        return big;
    }
    // Two memory round trips per helper, not one per tile: first the owner words of its tiles (eight tiles in flight) give the ordered list of its
    // leaves (ascending ordinal: tiles ascending, lanes ascending), then the feature rows of up to 64 listed leaves are fetched together, one lane
    // each, and lanes 0..8 add them up in list order.  (Round 2 fetched the rows tile by tile: ~10 dependent round trips for a 22-leaf helper.)
    __device__ void one(const SweepFrame& f, uint32_t t, uint32_t h, float (*tile)[12], uint32_t* srt, uint32_t* leaf) const {
        if (h > f.S0) return;
        const bool gact0 = f.ghost_active[h] != 0;
        if (t != 0u && f.hD[h] != t + 1u && !gact0) return;
        const float* vf = f.sv.vf; const uint32_t* owner = f.owner_out;
        const uint32_t V = (uint32_t)f.sv.V;
        const int lane = lane_id();
        bool gact = gact0 && !f.ghost_done[h];
        const int gv = gact ? f.ghost_vox[h] : -1;
        const uint32_t lo = f.hlo[h], hi = f.hhi[h];
        uint32_t* tl = f.tl + (size_t)h * HT_CAP;
        const int nl = helper_tile_list(tl, f.tcnt[h], gv, srt);
        const uint32_t base_w = lo & ~63u;
        const uint32_t nchunks = nl >= 0 ? (uint32_t)nl : ((hi - base_w) >> 6) + 1u;
        float acc = 0.0f;
        uint32_t count = 0, kept = 0, nbuf = 0;
        // E2 of the dirty-tile scheme on the spot (d_centroid_mark until round 4): the leaves of a helper whose centroid is recomputed tell the tiles around them
        // to look again in the next sweep -- only when that sweep is allowed to skip tiles
        const bool do_mark = a_sweep_marks_after_claim(sweep_ctl(f.dc), t, f.thr);
        uint32_t* const mR = f.tR_next(t); uint32_t* const mC = f.tC_next(t);
        auto flush = [&]() {      // the listed leaves' rows, all requested at once, then added in list order
            if (nbuf == 0u) return;
            wave_lds_sync();
            if (do_mark && (uint32_t)lane < nbuf) mark_tiles(f.sv, (int)leaf[lane], mR, mC, t + 2u);
            if ((uint32_t)lane < nbuf) {
                const float4* row = reinterpret_cast<const float4*>(vf + (size_t)leaf[lane] * 12);
                const float4 r0 = row[0], r1 = row[1], r2 = row[2];
                float4* t4 = reinterpret_cast<float4*>(&tile[lane][0]);
                t4[0] = r0; t4[1] = r1; t4[2] = r2;
            }
            wave_lds_sync();
            // (eight rows requested together, then added in order: row by row the loop was one LDS round trip per leaf -- read, wait, add)
            if (lane < 9) for (uint32_t j = 0; j < nbuf; j += 8u) {
                float r[8];
        #pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = tile[(j + (uint32_t)k) & 63u][lane];
        #pragma unroll
                for (int k = 0; k < 8; ++k) if (j + (uint32_t)k < nbuf) acc += r[k];
            }
            count += nbuf; nbuf = 0u;
            wave_lds_sync();
        };
        for (uint32_t i0 = 0; i0 < nchunks; i0 += 8u) {
            uint32_t own[8], cb[8];
        #pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t i = i0 + c < nchunks ? i0 + c : nchunks - 1u;
                cb[c] = nl >= 0 ? srt[i] * 64u : base_w + 64u * i;
                const uint32_t v = cb[c] + lane;
                own[c] = owner[v < V ? v : V - 1u];
            }
        #pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (i0 + c >= nchunks) break;
                const uint32_t v = cb[c] + lane;
                const bool mine = v < V && own[c] == h;
                const bool m = mine || (int)v == gv;
                const uint64_t mask = __ballot(m);
                if (__ballot(mine)) { if (lane == 0 && kept < HT_CAP) tl[kept] = cb[c] >> 6; kept++; }
                if (!mask) continue;
                const uint32_t cnt = (uint32_t)__popcll(mask);
                if (nbuf + cnt > 64u) flush();
                if (m) leaf[nbuf + (uint32_t)__popcll(mask & lanemask_lt())] = v;
                nbuf += cnt;
            }
        }
        flush();
        if (lane == 0) { f.ghost_active[h] = gact ? 1 : 0; f.ghost_done[h] = 0; f.hcount[h] = count; f.tcnt[h] = kept <= HT_CAP ? kept : HT_CAP + 1u; }
        if (count == 0) return;
        // a_centroid_finish (f3ds_algo.h) with its nine divisions side by side: lane k < 6 divides sum k by the count, lanes 6..8 the normal's components by its length (the
        // same quotients, one division sequence instead of nine on one lane -- the kernel is bound by the instructions it issues: ~700 per helper)
        const float nx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 6)), ny = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 7)),
                    nz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 8));
        const float z = (nx * nx + ny * ny) + (nz * nz + 0.0f);
        float den = (float)count;
        bool divide = true;
        if (lane >= 6) { divide = z > 0.0f; den = divide ? n_sqrtf(z) : 1.0f; }
        const float res = divide ? acc / den : acc;
        if (lane < 12) f.hc[(size_t)h * 12 + lane] = lane < 9 ? res : 0.0f;
    }
};
#include "f3ds_quad.h"      // n_ciede00_quad, edge_weight_quad, lab_three_lanes

// ------------------------------------------------------------------------------------------------
// stage 4: supervoxel payload, adjacency, initial weights
// ------------------------------------------------------------------------------------------------
// makeSupervoxels: payload rows of every helper's leaves in leaf order, the ordered sums of the leaf (what computeCentroid / computePointNormal / mean_color
// would accumulate over voxels_), and the initial region record.
// FOUR helpers per wave, one per 16-lane row (round 6, as d_centroid; a wave per helper until then): the leaves through row_leaves, a lane per leaf computes and
// writes its payload row (three 16-byte stores), lanes 0..11 of the row continue the twelve ordered sums out of LDS, and the rgb -> Lab of the four mean colours
// (three gamma curves and three cube roots in f64 each: half of the old kernel's instructions) runs side by side on lanes 0..2 of the four rows.  A helper that
// does not fit a row (more than 16 list entries, more than 64 leaves) takes the wave-wide path `one_helper`.
struct d_sv_fill {
    static constexpr int BLOCK = 64;
    __device__ void operator()(const float* vf, const uint32_t* owner, uint32_t S0, const uint32_t* hlo, const uint32_t* hhi,
                                               const int* ghost_vox, const unsigned char* ghost_active, const uint32_t* hcount, const uint32_t* loff,
                                               const float* hc, float* rows, int* row_voxel, float* racc0, uint32_t* rcnt0, float* rrec0,
                                               unsigned char* ralive0, DevCounters* dc, const uint32_t* tl, const uint32_t* tcnt, uint32_t V) const {
        __shared__ __attribute__((aligned(16))) float pay[4][QL][12];      // payload rows of the four helpers (the wave-wide path: its feature rows and payload rows)
        __shared__ __attribute__((aligned(16))) uint32_t qt[4][16];
        __shared__ __attribute__((aligned(16))) uint32_t ql[4][QL + 32];
        __shared__ int tile_v[64];
        __shared__ uint32_t srt[64];
        const uint32_t lane = (uint32_t)lane_id(), row = lane >> 4, l16 = lane & 15u;
        const uint32_t h0 = BIX * 4u + row + 1u;
        const bool live = h0 <= S0;
        const uint32_t h = live ? h0 : 0u;      // (row 0 of every array exists)
        const uint32_t len = hcount[h], cnt = tcnt[h], off = loff[h];
        const int gv = ghost_active[h] ? ghost_vox[h] : -1;
        const uint32_t tl_ = tl[(size_t)h * HT_CAP + l16];
        if (live && len == 0u) {
            if (l16 == 0u) { ralive0[h] = 0; rcnt0[h] = 0; }
            if (l16 < 12u) racc0[(size_t)h * 12 + l16] = 0.0f;
            rrec0[(size_t)h * 16 + l16] = 0.0f;
        }
        const bool active = live && len != 0u;
        const bool fits = active && cnt + (gv >= 0 ? 1u : 0u) <= HT_ROW && V <= BY_WAVE_RATIO * S0;      // (frames of big supervoxels -- 48 voxels and more on average -- go straight to the wave-wide path)
        uint32_t tid = 0xFFFFFFFFu;
        if (fits) { if (l16 < cnt) tid = tl_; else if (l16 == cnt && gv >= 0) tid = (uint32_t)gv >> 6; }
        uint32_t nd, keptbits;
        const uint32_t count = row_leaves(owner, V, h, tid, fits ? gv : -1, qt, ql[row], QL, QL + 31u, &nd, &keptbits);
        const bool run = fits && count <= QL;
        const bool big_row = active && !run;
        wave_lds_sync();
        // a lane per leaf: feature row in, payload row out (global memory and LDS)
        if (run) for (uint32_t j = l16; j < count; j += 16u) {
            const uint32_t v = ql[row][j];
            const float4* fr = reinterpret_cast<const float4*>(vf + (size_t)v * 12);
            const float4 r0 = fr[0], r1 = fr[1];
            row_voxel[off + j] = (int)v;
            const float x = r0.x, y = r0.y, z = r0.z;
            const float4 p0 = make_float4(x * x, x * y, x * z, y * y), p1 = make_float4(y * z, z * z, x, y),
                         p2 = make_float4(z, (float)((uint32_t)r0.w & 255u), (float)((uint32_t)r1.x & 255u), (float)((uint32_t)r1.y & 255u));      // a_payload_row
            float4* dst = reinterpret_cast<float4*>(rows + (size_t)(off + j) * 12);
            dst[0] = p0; dst[1] = p1; dst[2] = p2;
            float4* pl = reinterpret_cast<float4*>(&pay[row][j][0]);
            pl[0] = p0; pl[1] = p1; pl[2] = p2;
        }
        wave_lds_sync();
        // the twelve ordered sums (nine sums, the running colour mean) on lanes 0..11 of the row, eight rows per LDS round trip
        float acc = 0.0f;
        if (run && l16 < 12u) {
            for (uint32_t j0 = 0; j0 < count; j0 += 8u) {
                float r[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = pay[row][(j0 + (uint32_t)k) & (QL - 1u)][l16];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t j = j0 + (uint32_t)k;
                    if (j >= count) break;
                    if (l16 < 9u) acc += r[k];
                    else { const float cf = (float)(j + 1u); const float inv = 1 / cf; acc = acc + inv * (r[k] - acc); }
                }
            }
            racc0[(size_t)h * 12 + l16] = acc;
        }
        // the region record: centroid and normal as the last updateCentroid left them, the mean colour and its Lab (lanes 0..2 of every row side by side)
        const int rb = (int)(lane & 48u);
        const float mr = __shfl(acc, rb + 9, 64), mg = __shfl(acc, rb + 10, 64), mb = __shfl(acc, rb + 11, 64);
        float lab[3];
        lab_three_lanes(l16 == 0u ? mr : (l16 == 1u ? mg : mb), (int)l16, lab, m_lit(), rb);
        if (run) {
            const float* c = hc + (size_t)h * 12;
            float val = 0.0f;
            if (l16 < 3u) val = c[l16];
            else if (l16 < 6u) val = c[l16 + 3u];
            else if (l16 < 9u) val = l16 == 6u ? mr : (l16 == 7u ? mg : mb);
            else if (l16 < 12u) val = l16 == 9u ? lab[0] : (l16 == 10u ? lab[1] : lab[2]);
            rrec0[(size_t)h * 16 + l16] = val;
            if (l16 == 0u) { rcnt0[h] = len; ralive0[h] = 1; }
        }
        const uint32_t nrun = (uint32_t)__popcll(__ballot(run && l16 == 0u));
        if (lane == 0u && nrun) atomicAdd(&dc->n_alive, nrun);
        const uint64_t bb = __ballot(big_row);
        if (bb) {
            wave_lds_sync();
#pragma unroll
            for (uint32_t r = 0; r < 4u; ++r) if ((bb >> (16u * r)) & 1ull)
                one_helper(BIX * 4u + r + 1u, vf, owner, S0, hlo, hhi, ghost_vox, ghost_active, hcount, loff, hc, rows, row_voxel, racc0, rcnt0, rrec0, ralive0, dc, tl, tcnt, V,
                           pay[0], pay[1], tile_v, srt);
        }
    }
    // the wave-wide path: one helper on all 64 lanes (any number of list entries and leaves)
    __device__ void one_helper(const uint32_t h, const float* vf, const uint32_t* owner, uint32_t S0, const uint32_t* hlo, const uint32_t* hhi,
                               const int* ghost_vox, const unsigned char* ghost_active, const uint32_t* hcount, const uint32_t* loff,
                               const float* hc, float* rows, int* row_voxel, float* racc0, uint32_t* rcnt0, float* rrec0,
                               unsigned char* ralive0, DevCounters* dc, const uint32_t* tl, const uint32_t* tcnt, uint32_t V,
                               float (*tile)[12], float (*pay)[12], int* tile_v, uint32_t* srt) const {
        if (h > S0) return;
        const int lane = lane_id();
        const uint32_t len = hcount[h];
        if (len == 0) {
            if (lane == 0) { ralive0[h] = 0; rcnt0[h] = 0; }
            if (lane < 12) racc0[(size_t)h * 12 + lane] = 0.0f;
            if (lane < 16) rrec0[(size_t)h * 16 + lane] = 0.0f;
            return;
        }
        const uint32_t off = loff[h];
        const int gv = ghost_active[h] ? ghost_vox[h] : -1;
        const uint32_t lo = hlo[h], hi = hhi[h];
        float acc = 0.0f;
        uint32_t done = 0;
        const int nl = helper_tile_list(tl + (size_t)h * HT_CAP, tcnt[h], gv, srt);
        const uint32_t base_w = lo & ~63u;
        const uint32_t nchunks = nl >= 0 ? (uint32_t)nl : ((hi - base_w) >> 6) + 1u;
        // As in d_centroid: the owner words of eight tiles in flight give the helper's leaves in order; up to 64 of them are listed, then their feature rows are fetched
        // together (one lane each), the payload rows are computed and written by all 64 lanes (consecutive lanes = consecutive words of `rows`), and lanes 0..11 continue
        // the ordered sums over the listed rows, eight per LDS round trip.  (Until round 4 every tile was a round of its own: fetch, barrier, a store per row from 12 lanes.)
        uint32_t nbuf = 0;
        auto flush = [&]() {
            if (nbuf == 0u) return;
            wave_lds_sync();
            if ((uint32_t)lane < nbuf) {
                const float4* row = reinterpret_cast<const float4*>(vf + (size_t)tile_v[lane] * 12);
                const float4 r0 = row[0], r1 = row[1], r2 = row[2];
                float4* t = reinterpret_cast<float4*>(&tile[lane][0]);
                t[0] = r0; t[1] = r1; t[2] = r2;
                row_voxel[off + done + (uint32_t)lane] = tile_v[lane];
            }
            wave_lds_sync();
            for (uint32_t e = (uint32_t)lane; e < nbuf * 12u; e += 64u) {      // payload element e = row j, column c
                const uint32_t j = e / 12u, c = e - j * 12u;
                const int ca = c < 6u ? (c < 3u ? 0 : (c < 5u ? 1 : 2)) : (int)c - 6;
                const int cb2 = c < 6u ? (c < 3u ? (int)c : (c < 5u ? (int)c - 2 : 2)) : 0;
                const float ta = tile[j][ca], tb = tile[j][cb2];
                const float val = c < 6u ? ta * tb : (c < 9u ? ta : (float)((uint32_t)ta & 255u));
                rows[(size_t)(off + done) * 12 + e] = val;
                pay[j][c] = val;
            }
            wave_lds_sync();
            if (lane < 12) for (uint32_t j0 = 0; j0 < nbuf; j0 += 8u) {
                float r[8];
        #pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = pay[(j0 + (uint32_t)k) & 63u][lane];
        #pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint32_t j = j0 + (uint32_t)k;
                    if (j >= nbuf) break;
                    if (lane < 9) acc += r[k];
                    else { const float count = (float)(done + j + 1u); const float inv = 1 / count; acc = acc + inv * (r[k] - acc); }
                }
            }
            done += nbuf; nbuf = 0u;
            wave_lds_sync();
        };
        for (uint32_t i0 = 0; i0 < nchunks; i0 += 8u) {
          uint32_t own[8], cb[8];
        #pragma unroll
          for (int c = 0; c < 8; ++c) {
              const uint32_t i = i0 + c < nchunks ? i0 + c : nchunks - 1u;
              cb[c] = nl >= 0 ? srt[i] * 64u : base_w + 64u * i;
              const uint32_t vv = cb[c] + lane;
              own[c] = owner[vv < V ? vv : V - 1u];
          }
        #pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (i0 + c >= nchunks) break;
            const uint32_t v = cb[c] + lane;
            const bool m = (v < V && own[c] == h) || (int)v == gv;
            const uint64_t mask = __ballot(m);
            if (!mask) continue;
            const uint32_t cnt = (uint32_t)__popcll(mask);
            if (nbuf + cnt > 64u) flush();
            if (m) tile_v[nbuf + (uint32_t)__popcll(mask & lanemask_lt())] = (int)v;
            nbuf += cnt;
          }
        }
        flush();
        if (lane < 12) racc0[(size_t)h * 12 + lane] = acc;
        const float mr = __shfl(acc, 9, 64), mg = __shfl(acc, 10, 64), mb = __shfl(acc, 11, 64);
        float lab[3];
        lab_three_lanes(lane == 0 ? mr : (lane == 1 ? mg : mb), lane, lab);      // n_rgb2lab with the three gamma curves and the three cube roots in lanes 0..2 (as the merge loop's record has it)
        if (lane == 0) {
            rcnt0[h] = len; ralive0[h] = 1;
            atomicAdd(&dc->n_alive, 1u);
            float rec[16];
            const float* c = hc + (size_t)h * 12;
            rec[0] = c[0]; rec[1] = c[1]; rec[2] = c[2]; rec[3] = c[6]; rec[4] = c[7]; rec[5] = c[8];
            rec[6] = mr; rec[7] = mg; rec[8] = mb;
            rec[9] = lab[0]; rec[10] = lab[1]; rec[11] = lab[2];
            rec[12] = rec[13] = rec[14] = rec[15] = 0.0f;
            for (int k = 0; k < 16; ++k) rrec0[(size_t)h * 16 + k] = rec[k];
        }
    }
};
// The same summaries for supervoxels the CALLER supplies (f3ds_cluster_supervoxels = Clustering::set_initialstate(segm, adj),
// /root/reference/src/clustering.cpp:605-612): one wave per map entry in ascending key (h = rank + 1, src[h] = the caller's row).
// voxels_ stays where the caller put it -- payload row v belongs to input voxel v, loff[h] = the caller's offset --, centroid_ and
// normal_ are taken as given (delta_c_g reads them, :126-129), the mean colour is mean_color's running mean over voxels_
// (src/color_utilities.cpp:117-142).  owner[v] = h and row_voxel[v] = v make stage 6 write one region id per input voxel.
struct d_sv_user_fill {
    static constexpr int BLOCK = 64;
    __device__ void operator()(uint32_t S0, const uint32_t* src, const uint32_t* voff, const float* vxyz, const uint32_t* vrgba, const float* cxyz,
                               const float* cnrm, float* rows, int* row_voxel, uint32_t* owner, float* racc0, uint32_t* rcnt0, float* rrec0,
                               unsigned char* ralive0, float* hc, DevCounters* dc) const {
        __shared__ __attribute__((aligned(16))) float pay[64][12];
        const uint32_t h = BIX + 1u;
        if (h > S0) return;
        const int lane = lane_id();
        const uint32_t i = src[h], off = voff[i], len = voff[i + 1u] - off;
        float acc = 0.0f;
        for (uint32_t done = 0; done < len; done += 64u) {
            const uint32_t nbuf = len - done < 64u ? len - done : 64u;
            wave_lds_sync();
            if ((uint32_t)lane < nbuf) {
                const uint32_t v = off + done + (uint32_t)lane;
                const float x = vxyz[(size_t)v * 3], y = vxyz[(size_t)v * 3 + 1], z = vxyz[(size_t)v * 3 + 2];
                const uint32_t c = vrgba[v];
                const float row[12] = {x * x, x * y, x * z, y * y, y * z, z * z, x, y, z, (float)((c >> 16) & 255u), (float)((c >> 8) & 255u), (float)(c & 255u)};
        #pragma unroll
                for (int k = 0; k < 12; ++k) { pay[lane][k] = row[k]; rows[(size_t)v * 12 + k] = row[k]; }
                row_voxel[v] = (int)v; owner[v] = h;
            }
            wave_lds_sync();
            if (lane < 12) for (uint32_t j = 0; j < nbuf; ++j) {
                const float r = pay[j][lane];
                if (lane < 9) acc += r;
                else { const float count = (float)(done + j + 1u); const float inv = 1 / count; acc = acc + inv * (r - acc); }
            }
        }
        if (lane < 12) racc0[(size_t)h * 12 + lane] = acc;
        const float mr = __shfl(acc, 9, 64), mg = __shfl(acc, 10, 64), mb = __shfl(acc, 11, 64);
        float lab[3];
        lab_three_lanes(lane == 0 ? mr : (lane == 1 ? mg : mb), lane, lab);
        if (lane == 0) {
            rcnt0[h] = len; ralive0[h] = 1;
            atomicAdd(&dc->n_alive, 1u);
            float rec[16];
            rec[0] = cxyz[(size_t)i * 3]; rec[1] = cxyz[(size_t)i * 3 + 1]; rec[2] = cxyz[(size_t)i * 3 + 2];
            rec[3] = cnrm[(size_t)i * 3]; rec[4] = cnrm[(size_t)i * 3 + 1]; rec[5] = cnrm[(size_t)i * 3 + 2];
            rec[6] = mr; rec[7] = mg; rec[8] = mb;
            rec[9] = lab[0]; rec[10] = lab[1]; rec[11] = lab[2];
            rec[12] = rec[13] = rec[14] = rec[15] = 0.0f;
            for (int k = 0; k < 16; ++k) rrec0[(size_t)h * 16 + k] = rec[k];
            float* c12 = hc + (size_t)h * 12;      // the layout f3ds_get_supervoxels reads: centroid, mean colour, normal
            c12[0] = rec[0]; c12[1] = rec[1]; c12[2] = rec[2]; c12[3] = mr; c12[4] = mg; c12[5] = mb; c12[6] = rec[3]; c12[7] = rec[4]; c12[8] = rec[5]; c12[9] = c12[10] = c12[11] = 0.0f;
        }
    }
};
__device__ inline void edge_insert(uint64_t key, uint64_t* hkeys, uint32_t hmask, uint64_t* ekeys, uint32_t ecap, DevCounters* dc) {
    uint32_t hh = (uint32_t)hash64(key) & hmask;
    for (uint32_t probes = 0; probes <= hmask; ++probes) {
        unsigned long long old = atomicCAS((unsigned long long*)&hkeys[hh], (unsigned long long)HASH_EMPTY, (unsigned long long)key);
        if (old == key) return;
        if (old == HASH_EMPTY) {
            uint32_t pos = atomicAdd(&dc->n_edges, 1u);
            if (pos < ecap) ekeys[pos] = key; else { dc->error = F3DS_ERR_UNSUPPORTED; dc->ev_overflow = F3DS_OVF_EDGE_LIST; }      // adjacency list full: the host reruns the stage with more room
            return;
        }
        hh = (hh + 1u) & hmask;
    }
    dc->error = F3DS_ERR_UNSUPPORTED;
}
// getSupervoxelAdjacency + clear_adjacency: pairs (h, o), h < o, seen from a leaf of h
// (nbrT is the slot-major table: lanes of consecutive voxels read consecutive words)
__device__ inline void leaf_edges(uint32_t h, uint32_t v, uint32_t V, uint32_t S0, const int* nbrT, const uint32_t* owner, uint64_t* hkeys, uint32_t hmask,
                                  uint64_t* ekeys, uint32_t ecap, DevCounters* dc) {
    int nu[27]; uint32_t og[27];
#pragma unroll
    for (int s = 0; s < 27; ++s) nu[s] = nbrT[(size_t)s * V + v];
#pragma unroll
    for (int s = 0; s < 27; ++s) {
        const uint32_t o = owner[nu[s] >= 0 ? (uint32_t)nu[s] : v];       // unconditional: all 27 gathers in flight together
        og[s] = (nu[s] >= 0 && o && o != h && h < o) ? o : 0u;
    }
    uint32_t last = 0;
#pragma unroll
    for (int s = 0; s < 27; ++s) {
        const uint32_t o = og[s];
        if (o && o != last) { last = o; edge_insert((uint64_t)h * (S0 + 1ull) + o, hkeys, hmask, ekeys, ecap, dc); }
    }
}
struct d_edges {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t V, uint32_t S0, const int* nbrT, const uint32_t* owner, uint64_t* hkeys, uint32_t hmask,
                                              uint64_t* ekeys, uint32_t ecap, DevCounters* dc) const {
        for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
            const uint32_t h = owner[v];
            if (h) leaf_edges(h, v, V, S0, nbrT, owner, hkeys, hmask, ekeys, ecap, dc);
        }
    }
};
struct d_edges_ghost {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t V, uint32_t S0, const int* ghost_vox, const unsigned char* ghost_active, const int* nbrT,
                                                    const uint32_t* owner, uint64_t* hkeys, uint32_t hmask, uint64_t* ekeys, uint32_t ecap, DevCounters* dc) const {
        for (uint32_t h = 1 + BIX * blockDim.x + threadIdx.x; h <= S0; h += gridDim.x * blockDim.x)
            if (ghost_active[h]) leaf_edges(h, (uint32_t)ghost_vox[h], V, S0, nbrT, owner, hkeys, hmask, ekeys, ecap, dc);
    }
};
struct d_iota {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* v, uint32_t n) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = i;
    }
};
struct d_fill_f32 {
    static constexpr int BLOCK = 256;
    __device__ void operator()(float* v, uint32_t n, float x) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) v[i] = x;
    }
};
struct d_edge_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* ekeys, uint32_t E, uint32_t S0, uint32_t* ea0, uint32_t* eb0) const {
        for (uint32_t e = BIX * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
            ea0[e] = (uint32_t)(ekeys[e] / (S0 + 1ull)); eb0[e] = (uint32_t)(ekeys[e] % (S0 + 1ull));
        }
    }
};
struct d_edge_deltas {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t E, const uint32_t* ea, const uint32_t* eb, const float* rrec, int color_metric, int geom_metric,
                                                    float* deltas, uint64_t* skeys, uint32_t* svals) const {
        for (uint32_t e = BIX * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
            float dc_, dg_;
            n_delta_c_g(rrec + (size_t)ea[e] * 16, rrec + (size_t)eb[e] * 16, color_metric, geom_metric, &dc_, &dg_);
            deltas[e * 2] = dc_; deltas[e * 2 + 1] = dg_;
            if (skeys) {   // one sort orders both multisets: (which << 32 | key)
                skeys[e] = (uint64_t)n_weight_key(dc_); svals[e] = e * 2u;
                skeys[E + e] = (1ull << 32) | (uint64_t)n_weight_key(dg_); svals[E + e] = e * 2u + 1u;
            }
        }
    }
};
// Clustering::deltas_mean over the ascending multisets, then lambda (src/clustering.cpp:267-273).
// The running mean is a serial chain; the 64 lanes fetch the next 64 sorted values of both
// multisets together and lanes 0 (colour) / 1 (geometry) consume them through readlane.
struct d_lambda {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 64;
    __device__ void operator()(uint32_t E, const float* deltas, const uint32_t* svals, DevCounters* dc) const {
        const int lane = lane_id();
        float count = 0, mean_d = 0;
        for (uint32_t base = 0; base < E; base += 64u) {
            const uint32_t i = base + lane;
            const float vc = i < E ? deltas[svals[i]] : 0.0f;
            const float vg = i < E ? deltas[svals[(size_t)E + i]] : 0.0f;
            const int nb = E - base < 64u ? (int)(E - base) : 64;
            // 1 / count of the next 64 steps, one division per lane, off the serial chain (count = base + j + 1 exactly:
            // the float counter of the reference is exact below 2^24)
            const float inv = 1 / (count + (float)(lane + 1));
    #pragma unroll
            for (int j = 0; j < 64; ++j) {
                if (j < nb) {
                    const float dcj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vc), j));
                    const float dgj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vg), j));
                    const float ij = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, inv), j));
                    const float d = lane == 0 ? dcj : dgj;
                    mean_d = mean_d + ij * (d - mean_d);
                }
            }
            count += (float)nb;
        }
        const float mean_c = __shfl(mean_d, 0, 64), mean_g = __shfl(mean_d, 1, 64);
        if (lane == 0) dc->lambda = mean_g / (mean_c + mean_g);
    }
};
// Clustering::compute_cdf (src/clustering.cpp:289-314) for delta_c (w=0) and delta_g (w=1)
struct d_cdf_hist {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t E, const float* deltas, int bins, uint32_t* hist, DevCounters* dc) const {
        for (uint32_t t = BIX * blockDim.x + threadIdx.x; t < 2u * E; t += gridDim.x * blockDim.x) {
            const uint32_t w = t / E, e = t - w * E;
            const float d = deltas[e * 2 + w];
            short bin = (short)__builtin_floorf(d * (float)(short)bins);
            if (bin == (short)bins) bin--;
            if (bin < 0 || bin >= (short)bins) { dc->error = F3DS_ERR_EQ_BIN; continue; }
            atomicAdd(&hist[w * (uint32_t)bins + (uint32_t)bin], 1u);
        }
    }
};
struct d_cdf_scan {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 64;
    __device__ void operator()(uint32_t E, int bins, const uint32_t* hist, float* cdf) const {
        const int w = threadIdx.x;
        if (w >= 2) return;
        float v = 0;
        for (int i = 0; i < bins; ++i) { v += (float)hist[w * bins + i]; cdf[w * bins + i] = v / (float)(int)E; }
    }
};
struct MergeDev {
    uint32_t E, S0;
    uint32_t *ea, *eb; float* ew; uint32_t* eku; int* ehist; unsigned char* ealive;
    uint32_t *ev_epoch, *ev_key; int* ev_prev; uint32_t ev_cap;
    float *racc, *rrec; uint32_t* rcnt; unsigned char* ralive;
    uint32_t *rhead, *rtail, *lnext, *parent;
    const uint32_t *loff, *llen; const float* rows;
    uint32_t *markA, *markB, *tl;
    uint32_t* merges;
    float threshold;
    MergeParams mp;
    DevCounters* dc;
};
struct d_edge_weights {
    static constexpr int BLOCK = 256;
    __device__ void operator()(MergeDev m, const float* deltas) const {
        MergeParams mp = m.mp;
        if (mp.merging == 1) mp.lambda = m.dc->lambda;
        for (uint32_t e = BIX * blockDim.x + threadIdx.x; e < m.E; e += gridDim.x * blockDim.x) {
            int err = 0;
            const float w = a_tc(mp, deltas[e * 2], &err) + a_tg(mp, deltas[e * 2 + 1], &err);
            if (err) m.dc->error = err;
            m.ew[e] = w; m.eku[e] = n_weight_key(w); m.ehist[e] = (int)e; m.ealive[e] = 1;
            m.ev_epoch[e] = 0u; m.ev_key[e] = m.eku[e]; m.ev_prev[e] = -1;
        }
    }
};
struct d_region_reset {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t S0, const uint32_t* hcount, uint32_t* rhead, uint32_t* rtail, uint32_t* lnext, uint32_t* parent,
                                                     uint32_t* markA, uint32_t* markB, uint2* pool, uint32_t* rstart, uint32_t* rnleaf, uint32_t* rcap,
                                                     const uint32_t* loff) const {
        for (uint32_t h = BIX * blockDim.x + threadIdx.x; h <= S0; h += gridDim.x * blockDim.x) {
            const bool alive = h > 0 && hcount[h] > 0;
            rhead[h] = alive ? h : 0u; rtail[h] = alive ? h : 0u; lnext[h] = 0u; parent[h] = h; markA[h] = 0u; markB[h] = 0u;
            pool[h] = make_uint2(loff[h], hcount[h]); rstart[h] = h; rnleaf[h] = alive ? 1u : 0u; rcap[h] = 1u;     // a leaf = (first payload row, rows)
        }
    }
};

// ------------------------------------------------------------------------------------------------
// stage 5: the merge loop (Clustering::cluster / merge), one persistent workgroup.
// Per merge: block-wide argmin in weight_map order, then wave 0 folds region b's voxels into
// region a's ordered sums and rebuilds a's record while the other waves collect the incident
// edges; duplicates (x adjacent to both a and b) keep the earlier map entry; kept edges get a
// new weight and a history event.
// ------------------------------------------------------------------------------------------------
constexpr int MG_THREADS = 1024;
__device__ inline bool edge_before(const MergeDev& m, uint32_t e, uint32_t f) {
    EdgeHist H{m.ev_epoch, m.ev_key, m.ev_prev};
    return a_edge_before(H, e, m.eku[e], m.ehist[e], f, m.eku[f], m.ehist[f]);
}
struct d_merge {
    static constexpr int BLOCK = MG_THREADS;
    __device__ void operator()(MergeDev m) const {
        __shared__ int s_wbest[MG_THREADS / 64];
        __shared__ uint32_t s_a, s_b, s_ntouched, s_nmerges, s_nevents;
        __shared__ int s_stop;
        const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
        MergeParams mp = m.mp;
        if (mp.merging == 1) mp.lambda = m.dc->lambda;
        if (tid == 0) { s_ntouched = 0; s_nmerges = 0; s_nevents = m.E; s_stop = 0; }
        __syncthreads();
        for (uint32_t epoch = 1;; ++epoch) {
            // ---- next = *weight_map.begin()
            int best = -1;
            for (uint32_t e = tid; e < m.E; e += MG_THREADS)
                if (m.ealive[e] && (best < 0 || edge_before(m, e, (uint32_t)best))) best = (int)e;
    #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const int ob = __shfl_xor(best, d, 64);
                if (ob >= 0 && (best < 0 || edge_before(m, (uint32_t)ob, (uint32_t)best))) best = ob;
            }
            if (lane == 0) s_wbest[wave] = best;
            __syncthreads();
            if (tid == 0) {
                int b = -1;
                for (int w = 0; w < MG_THREADS / 64; ++w) { const int ob = s_wbest[w]; if (ob >= 0 && (b < 0 || edge_before(m, (uint32_t)ob, (uint32_t)b))) b = ob; }
                if (b < 0 || !(m.ew[b] < m.threshold)) s_stop = 1;
                else {
                    s_a = m.ea[b]; s_b = m.eb[b];
                    const uint32_t k = s_nmerges++;
                    m.merges[k * 3] = s_a; m.merges[k * 3 + 1] = s_b; m.merges[k * 3 + 2] = __float_as_uint(m.ew[b]);
                    m.ealive[b] = 0;
                }
            }
            __syncthreads();
            if (s_stop) break;
            const uint32_t a = s_a, b = s_b;
            if (wave == 0) {
                // ---- voxels_new = voxels_a ++ voxels_b: continue a's ordered sums over b's rows
                float acc = lane < 12 ? m.racc[(size_t)a * 12 + lane] : 0.0f;
                uint32_t cnt = m.rcnt[a];
                for (uint32_t leaf = m.rhead[b]; leaf; leaf = m.lnext[leaf]) {
                    const uint32_t off = m.loff[leaf], len = m.llen[leaf];
                    for (uint32_t j0 = 0; j0 < len; j0 += 16u) {
                        float val[16];
    #pragma unroll
                        for (int t = 0; t < 16; ++t) val[t] = (lane < 12 && j0 + t < len) ? m.rows[(size_t)(off + j0 + t) * 12 + lane] : 0.0f;
    #pragma unroll
                        for (int t = 0; t < 16; ++t)
                            if (j0 + t < len) {
                                cnt++;
                                if (lane < 9) acc += val[t];
                                else { const float count = (float)cnt; const float inv = 1 / count; acc = acc + inv * (val[t] - acc); }
                            }
                    }
                }
                if (lane < 12) m.racc[(size_t)a * 12 + lane] = acc;
                float all[12];
    #pragma unroll
                for (int k = 0; k < 12; ++k) all[k] = __shfl(acc, k, 64);
                float rec[16];
                a_region_from_acc(all, cnt, rec);
                if (lane == 0) {
                    for (int k = 0; k < 16; ++k) m.rrec[(size_t)a * 16 + k] = rec[k];
                    m.rcnt[a] = cnt;
                    m.lnext[m.rtail[a]] = m.rhead[b]; m.rtail[a] = m.rtail[b];
                    m.ralive[b] = 0; m.parent[b] = a;
                }
            } else {
                // ---- edges that touch a or b
                for (uint32_t e = tid - 64; e < m.E; e += MG_THREADS - 64) {
                    if (!m.ealive[e]) continue;
                    const uint32_t p = m.ea[e], q = m.eb[e];
                    const bool on_a = p == a || q == a, on_b = p == b || q == b;
                    if (!on_a && !on_b) continue;
                    const uint32_t x = (p == a || p == b) ? q : p;
                    m.tl[atomicAdd(&s_ntouched, 1u)] = e;
                    if (on_a) m.markA[x] = e + 1u; else m.markB[x] = e + 1u;
                }
            }
            __syncthreads();
            const uint32_t nt = s_ntouched;
            // ---- contains(): of (a,x) and (b,x) the entry that comes first in the old map survives
            for (uint32_t i = tid; i < nt; i += MG_THREADS) {
                const uint32_t e = m.tl[i];
                const uint32_t p = m.ea[e], q = m.eb[e];
                const bool on_a = p == a || q == a;
                const uint32_t x = (p == a || p == b) ? q : p;
                const uint32_t partner = on_a ? m.markB[x] : m.markA[x];
                if (partner && edge_before(m, partner - 1u, e)) m.ealive[e] = 0;
            }
            __syncthreads();
            // ---- re-weight the survivors (delta(), src/clustering.cpp:438-463)
            for (uint32_t i = tid; i < nt; i += MG_THREADS) {
                const uint32_t e = m.tl[i];
                const uint32_t p = m.ea[e], q = m.eb[e];
                const uint32_t x = (p == a || p == b) ? q : p;
                m.markA[x] = 0u; m.markB[x] = 0u;
                if (!m.ealive[e]) continue;
                const uint32_t lo = a < x ? a : x, hi = a < x ? x : a;
                int err = 0;
                const float w = a_edge_weight(mp, m.rrec + (size_t)lo * 16, m.rrec + (size_t)hi * 16, &err);
                if (err) m.dc->error = err;
                const uint32_t ev = atomicAdd(&s_nevents, 1u);
                if (ev >= m.ev_cap) { m.dc->error = F3DS_ERR_UNSUPPORTED; m.dc->ev_overflow = F3DS_OVF_EVENTS; continue; }
                const uint32_t ku = n_weight_key(w);
                m.ev_epoch[ev] = epoch; m.ev_key[ev] = ku; m.ev_prev[ev] = m.ehist[e];
                m.ea[e] = lo; m.eb[e] = hi; m.ew[e] = w; m.eku[e] = ku; m.ehist[e] = (int)ev;
            }
            if (tid == 0) s_ntouched = 0;
            __syncthreads();
            if (m.dc->error) break;
        }
        __syncthreads();
        if (tid == 0) { m.dc->n_merges = s_nmerges; m.dc->n_events = s_nevents; }
    }
};


constexpr uint32_t KEY_DEAD = 0xFFFFFFFFu;
constexpr uint32_t MC_TL_CAP = 1024;      // edges incident to the two regions of one merge (more: the host reruns the stage with d_merge)
// voxel rows the speculative second merge of an epoch may fold: 128, staged one per lane by waves 2 and 3, in the 4-wave layout (the other two carry the first merge's
// folds); in the 8-wave layout as many of 1024 / 512 / 256 / 128 as the frame's LDS layout has room for, staged one per lane by the whole workgroup, 512 rows a round (BASELINE
// config 4: supervoxels of ~190 voxels -- at 128 rows one runner-up in seven was small enough and the speculation rested; at 512 five in six are)
constexpr uint32_t MC_LDS_STATIC = 2560;      // bytes of the 160 KB kept back for the kernel's static LDS
constexpr uint32_t MC_LDS_LIMIT = 160u * 1024u - MC_LDS_STATIC;      // dynamic LDS a workgroup may ask for
constexpr uint32_t MC_CH_ROWS4 = 128, MC_CH_ROWS8 = 256;      // rows per staging buffer of the 4-wave / 8-wave layout
constexpr uint32_t MC_SP_ROWS_MIN = 128;      // rows the speculative second merge may fold at the least (the 4-wave layout: always)
constexpr uint32_t MC_SP_REST_TRIES = 64, MC_SP_REST_EPOCHS = 256;      // the speculation's rest rule: judged every 64 attempts, a rest lasts 256 epochs (F3DS_SP_REST_DIV)
constexpr uint32_t MC_SP_TL = 256;        // and adjacencies it may touch (its own touched list)
#ifndef F3DS_SP_REST_DIV
#define F3DS_SP_REST_DIV 4u      // the speculation rests for 256 epochs when fewer than one in F3DS_SP_REST_DIV of the last 64 attempts were committed
#endif
#ifndef F3DS_SP_ROWS8
#define F3DS_SP_ROWS8 1024u      // (a power of two >= 128)
#endif
#ifndef F3DS_SP_LEAVES
#define F3DS_SP_LEAVES 8
#endif
constexpr uint32_t MC_SP_LEAVES = F3DS_SP_LEAVES;      // and supervoxels the region it absorbs may consist of (1: a single supervoxel only, as in round 3)
constexpr uint32_t MC_GROUP = 16;         // edge slots per order-key group (one DPP row): G1 holds every group's smallest key
struct MergeLds {
    uint2* pool; uint32_t pool_cap; uint32_t* rstart; uint32_t* rnleaf; uint32_t* rcap;      // leaf arrays of the regions: (row offset, rows) per leaf
    uint32_t* ilist; uint32_t ilist_cap; uint32_t* istart; uint32_t* ilen; uint32_t* icap;   // incident-edge lists of the regions: slots of the adjacencies that touch a region (dead ones linger until the region's next merge)
    uint32_t Ecap, NGcap, lds_bytes, stop_key;      // LDS layout of d_merge_il_t (merge_il_layout below, shared by host and device)
    int keys_in_lds;
    int spec;                                       // whether to attempt a speculative second merge per epoch at all
};
// LDS carve-up of d_merge_il_t<NW, RES> for a frame with E adjacencies; the host sizes the launch with it, the kernel finds its arrays with it
struct MergeIlLayout {
    uint32_t Ecap, NGcap, CH, sp_rows;
    uint32_t off_eab, off_akey, off_g1, off_dlist, off_dmask, off_tl, off_tx, off_hsh, off_lstart, off_lsrc, off_stage, off_stage2, total;
};
__host__ __device__ inline MergeIlLayout merge_il_offsets(uint32_t E, int nw, int res) {
    MergeIlLayout L;
    const uint32_t T = (uint32_t)nw * 64u;
    L.CH = nw == 4 ? MC_CH_ROWS4 : MC_CH_ROWS8;                                           // rows per staging buffer
    L.Ecap = (E + 63u) & ~63u; if (!L.Ecap) L.Ecap = 64u;                    // whole waves of slots
    const uint32_t NG = L.Ecap / MC_GROUP;
    L.NGcap = (NG + T - 1u) / T * T;                                        // every thread reads whole rounds of group minima: no bounds tests
    uint32_t o = 0u;
    L.off_eab = o; if (res == 2) o += L.Ecap * 4u;
    L.off_akey = o; if (res == 2) o += L.Ecap * 4u;
    L.off_g1 = o; o += L.NGcap * 4u;
    L.off_dlist = o; o += L.NGcap * 4u;
    L.off_dmask = o; o += ((L.NGcap + 31u) / 32u) * 4u;
    L.off_tl = o; o += MC_TL_CAP * 4u;
    L.off_tx = o; o += MC_TL_CAP * 4u;
    L.off_hsh = o; o += 2u * MC_TL_CAP * 4u;
    L.off_lstart = o; o += (T + 1u) * 4u;
    L.off_lsrc = o; o += T * 4u;
    o = (o + 15u) & ~15u;
    L.off_stage = o; o += 2u * L.CH * 52u + 64u;                            // two row buffers + 1 / count per row (+ 64: the fold loops read up to 16 rows ahead)
    L.sp_rows = MC_SP_ROWS_MIN;
    if (nw == 8) for (uint32_t r = F3DS_SP_ROWS8; r > MC_SP_ROWS_MIN; r >>= 1) if (o + r * 52u + MC_SP_TL * 8u + 64u <= MC_LDS_LIMIT) { L.sp_rows = r; break; }
    L.off_stage2 = o; o += L.sp_rows * 52u + MC_SP_TL * 8u + 64u;               // the speculative second merge: rows, 1 / count, its touched list
    L.total = o;
    return L;
}
// Incident-edge lists, built once per cluster stage by one workgroup: every region's list = the slots of the adjacencies it is an endpoint
// of (degree counted with atomics, exclusive scan over the regions, filled in arbitrary order: nothing depends on the order inside a list).
// The merge loop walks the lists of a and b instead of scanning all E endpoints (Clustering::merge, src/clustering.cpp:403-469, visits
// exactly these entries of weight_map), and leaves the merged region's list behind.
struct d_inc_build {
    static constexpr bool LATENCY_KERNEL = true;      // one workgroup per frame on the call's critical path: its waves go first on their SIMD (k_batched)
    static constexpr int BLOCK = 256;       // (a wider workgroup waits for a compute unit with that many free wave slots when other calls fill the chip)
    __device__ void operator()(uint32_t E, uint32_t S0, const uint32_t* ea, const uint32_t* eb, uint32_t* istart, uint32_t* ilen, uint32_t* icap, uint32_t* ilist) const {
        if (BIX) return;
        const uint32_t tid = threadIdx.x;
        for (uint32_t r = tid; r <= S0; r += BLOCK) icap[r] = 0u;           // (icap doubles as the fill cursor first)
        __syncthreads();
        for (uint32_t e = tid; e < E; e += BLOCK) { atomicAdd(&icap[ea[e]], 1u); atomicAdd(&icap[eb[e]], 1u); }
        __syncthreads();
        uint32_t carry = 0u;
        for (uint32_t r0 = 0; r0 <= S0; r0 += BLOCK) {
            const uint32_t r = r0 + tid;
            const uint32_t d = r <= S0 ? __hip_atomic_load(&icap[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;      // (the counts were made by atomics in L2)
            uint32_t tot;
            const uint32_t inc = block_incl_scan<BLOCK>(d, &tot);
            if (r <= S0) { istart[r] = carry + inc - d; ilen[r] = d; }
            carry += tot;
            __syncthreads();
        }
        for (uint32_t r = tid; r <= S0; r += BLOCK) icap[r] = 0u;
        __syncthreads();
        for (uint32_t e = tid; e < E; e += BLOCK) {
            const uint32_t a = ea[e], b = eb[e];
            ilist[istart[a] + atomicAdd(&icap[a], 1u)] = e;
            ilist[istart[b] + atomicAdd(&icap[b], 1u)] = e;
        }
        __syncthreads();
        for (uint32_t r = tid; r <= S0; r += BLOCK) icap[r] = ilen[r];      // capacity of a fresh list = its length
    }
};
// wave-wide unsigned minimum with DPP lane swizzles (quad, half-row, row, row broadcasts): six VALU
// steps instead of six ds_bpermute round trips; every lane returns the result.
__device__ inline uint32_t wave_min_u32(uint32_t v) {
#define F3DS_DPP_MIN(ctrl, rmask)                                                                          \
    { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rmask, 0xF, false); v = t_ < v ? t_ : v; }
    F3DS_DPP_MIN(0xB1, 0xF)     // quad_perm [1,0,3,2]
    F3DS_DPP_MIN(0x4E, 0xF)     // quad_perm [2,3,0,1]
    F3DS_DPP_MIN(0x141, 0xF)    // row_half_mirror
    F3DS_DPP_MIN(0x140, 0xF)    // row_mirror: every lane of a row holds the row minimum
    F3DS_DPP_MIN(0x142, 0xA)    // row_bcast15 into rows 1 and 3
    F3DS_DPP_MIN(0x143, 0xC)    // row_bcast31 into rows 2 and 3
#undef F3DS_DPP_MIN
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ inline bool edge_before_k(const MergeDev& m, uint32_t e, uint32_t ke, uint32_t f, uint32_t kf) {
    EdgeHist H{m.ev_epoch, m.ev_key, m.ev_prev};
    return a_edge_before(H, e, ke, m.ehist[e], f, kf, m.ehist[f]);
}

// ------------------------------------------------------------------------------------------------
// stage 5, one workgroup per frame: the same merge loop (Clustering::cluster / merge, src/clustering.cpp:384-469) for a workgroup of
// NW = 8 waves (a lone call: the shortest loop) or 4 (calls that share the device: one wave slot per SIMD), with the per-edge arrays --
// endpoints (a << 16 | b) and order keys, 4 bytes each -- in LDS (RES = 2) or in global memory / L2 (RES = 0: any E, ~52 KB of LDS).
// Nothing in an epoch is O(E):
//   * next edge = argmin over the minima of 16-slot groups (G1; E / 16 values, a few per thread), after the groups whose keys the last
//     merge changed (dlist: ~50 of them) had their two smallest keys worked out again, one DPP row per group.  The group's second key
//     (G2) and the second group minimum give the runner-up for the speculative second merge.  Equal minimum keys (rare) take a slow
//     path through the weight-history comparator;
//   * touched edges = walk of the two regions' incident-edge lists (d_inc_build; the merged region's list is the touched list), not a
//     scan of all endpoints.  Slots never move: the history index of an edge is its slot;
//   * every wave works out the winner from the NW partial results itself (one barrier, not two);
//   * b's voxel rows are staged through two LDS buffers of one row per thread: the loads of chunk c+1 are in flight
//     while waves 0 / 1 fold chunk c (nine ordered sums / the running colour mean);
//   * contains() compares keys before it touches the history arrays (no global load on the common path).
// Results are bit-identical to d_merge (MERGES, region records, leaf order).
// ------------------------------------------------------------------------------------------------
__device__ inline bool edge_before_fast(const MergeDev& m, uint32_t e, uint32_t ke, uint32_t f, uint32_t kf) {
    if (ke != kf) return ke < kf;
    EdgeHist H{m.ev_epoch, m.ev_key, m.ev_prev};
    return a_edge_before(H, e, ke, m.ehist[e], f, kf, m.ehist[f]);
}
// minimum over each 16-lane DPP row (quad swaps, half-row mirror, row mirror): every lane of a row returns its row's minimum
__device__ inline uint32_t row_min_u32(uint32_t v) {
#define F3DS_DPP_MIN(ctrl)                                                                          \
    { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, 0xF, 0xF, false); v = t_ < v ? t_ : v; }
    F3DS_DPP_MIN(0xB1) F3DS_DPP_MIN(0x4E) F3DS_DPP_MIN(0x141) F3DS_DPP_MIN(0x140)
#undef F3DS_DPP_MIN
    return v;
}
// wave-wide inclusive sum: Hillis-Steele inside the four rows of 16 lanes with DPP row shifts (lanes shifted in from
// outside a row read 0), then the totals of the earlier rows are added (three readlanes): no LDS round trip
__device__ inline uint32_t wave_incl_scan_dpp(uint32_t v) {
#define F3DS_DPP_SHR_ADD(n) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + (n), 0xF, 0xF, true);
    F3DS_DPP_SHR_ADD(1) F3DS_DPP_SHR_ADD(2) F3DS_DPP_SHR_ADD(4) F3DS_DPP_SHR_ADD(8)
#undef F3DS_DPP_SHR_ADD
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 15), t1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 31), t2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 47);
    const int row = lane_id() >> 4;
    return v + (row >= 1 ? t0 : 0u) + (row >= 2 ? t1 : 0u) + (row >= 3 ? t2 : 0u);
}
// (plane_normal_wave and wave_pick: f3ds_quad.h)
// LDS reads of the ordered folds, issued and awaited by hand (see the fold loops of d_merge_cw_t)
typedef float f2v __attribute__((ext_vector_type(2)));
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t lds_addr(const float* p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const float*)p; }
#define FOLD_ISSUE_SUM(S, arow) asm volatile("ds_read2_b32 %0, %4 offset1:12\n\tds_read2_b32 %1, %4 offset0:24 offset1:36\n\tds_read2_b32 %2, %4 offset0:48 offset1:60\n\tds_read2_b32 %3, %4 offset0:72 offset1:84" \
    : "=&v"(S##_0), "=&v"(S##_1), "=&v"(S##_2), "=&v"(S##_3) : "v"(arow))
#define FOLD_WAIT_SUM(S, n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(S##_0), "+v"(S##_1), "+v"(S##_2), "+v"(S##_3))
#define FOLD_ISSUE_COL(S, arow, ainv) asm volatile("ds_read2_b32 %0, %6 offset1:12\n\tds_read2_b32 %1, %6 offset0:24 offset1:36\n\tds_read2_b32 %2, %6 offset0:48 offset1:60\n\tds_read2_b32 %3, %6 offset0:72 offset1:84\n\tds_read_b128 %4, %7\n\tds_read_b128 %5, %7 offset:16" \
    : "=&v"(S##_0), "=&v"(S##_1), "=&v"(S##_2), "=&v"(S##_3), "=&v"(S##i0), "=&v"(S##i1) : "v"(arow), "v"(ainv))
#define FOLD_WAIT_COL(S, n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(S##_0), "+v"(S##_1), "+v"(S##_2), "+v"(S##_3), "+v"(S##i0), "+v"(S##i1))
#ifndef F3DS_MERGE_WPS4
#define F3DS_MERGE_WPS4 2
#endif
template <int NW, int RES>      // NW waves per frame: 8 (a lone call: the shortest loop) or 4 (calls that share the device); RES = 2: endpoints and order keys in LDS, 0: both in global memory (L2)
struct d_merge_il_t {
    static constexpr bool IN_LDS = RES == 2;
    static constexpr int BLOCK = NW * 64;
#ifdef F3DS_MERGE_WPS
    static constexpr int WAVES_PER_SIMD = NW == 8 ? F3DS_MERGE_WPS : 2;
#else
    static constexpr int WAVES_PER_SIMD = NW == 4 ? F3DS_MERGE_WPS4 : 1;      // (four waves: two workgroups per unit)
#endif
    __device__ void operator()(MergeDev m, MergeLds x) const {
        static_assert(NW == 4 || NW == 8, "four or eight waves");
        constexpr uint32_t T = (uint32_t)BLOCK;
        constexpr uint32_t CH = NW == 4 ? 128u : 256u;          // rows per staging buffer (merge_il_offsets)
        extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
        const MergeIlLayout L = merge_il_offsets(m.E, NW, RES);
        uint32_t* eab = IN_LDS ? reinterpret_cast<uint32_t*>(smem + L.off_eab) : reinterpret_cast<uint32_t*>(m.ew);      // Ecap: endpoints a << 16 | b, 0xFFFFFFFF = edge gone
        uint32_t* akey = IN_LDS ? reinterpret_cast<uint32_t*>(smem + L.off_akey) : m.eku;                                // Ecap: order key of the weight, KEY_DEAD = edge gone
        uint32_t* G1 = reinterpret_cast<uint32_t*>(smem + L.off_g1);           // NGcap: smallest key of every group of MC_GROUP slots (exact at every argmin)
        uint32_t* dlist = reinterpret_cast<uint32_t*>(smem + L.off_dlist);     // NGcap: groups one of whose keys changed in this epoch
        uint32_t* dmask = reinterpret_cast<uint32_t*>(smem + L.off_dmask);     // one bit per group: already on dlist
        uint32_t* tl = reinterpret_cast<uint32_t*>(smem + L.off_tl);           // MC_TL_CAP: edges that touch a or b
        uint32_t* tx = reinterpret_cast<uint32_t*>(smem + L.off_tx);           // MC_TL_CAP: region on their other end, bit 31 = the edge hangs on b
        uint32_t* hsh = reinterpret_cast<uint32_t*>(smem + L.off_hsh);         // 2 * MC_TL_CAP: (region, side) -> index into tl
        uint32_t* lstart = reinterpret_cast<uint32_t*>(smem + L.off_lstart);   // T + 1
        uint32_t* lsrc = reinterpret_cast<uint32_t*>(smem + L.off_lsrc);       // T
        float* stage = reinterpret_cast<float*>(smem + L.off_stage);           // 2 buffers x CH rows x 12 floats
        float* sinv = stage + 2u * CH * 12u;                                   // 2 x CH: 1 / count of every staged row (running colour mean)
        const uint32_t SPR = L.sp_rows;                                        // rows a speculative second merge may fold (uniform)
        float* stage2 = reinterpret_cast<float*>(smem + L.off_stage2);         // SPR rows x 12 floats of the speculative second merge
        float* sinv2 = stage2 + SPR * 12u;                                     // SPR
        uint32_t* tl2 = reinterpret_cast<uint32_t*>(sinv2 + SPR);              // MC_SP_TL: the second merge's touched edges
        uint32_t* tx2 = tl2 + MC_SP_TL;                                        // MC_SP_TL
        __shared__ __attribute__((aligned(16))) uint32_t s_arg[8];              // wave 0's argmin for the other waves: key, slot, tie, speculate?, runner-up slot, its key, endpoints of both
        __shared__ uint32_t s_nt2, s_cross, s_min1;                            // length of the second touched list, an edge between the two merges, smallest new key of the first
        __shared__ float s_rec2[16];
        __shared__ uint32_t s_nt, s_nevents, s_pool_end, s_ipool_end, s_best, s_ndirty;
        __shared__ int s_err;
        __shared__ float s_rec[16];
        __shared__ __attribute__((aligned(16))) double s_mtab[MC_COUNT];      // the f64 constants of the record and weight arithmetic (f3ds_math.h: two per ds_read_b128 instead of two s_mov_b32 each)
        // pointers used once per merge, per published edge or on error paths: parked in LDS so that they do not hold 16 of the 106 SGPRs through the loop (the loop state
        // and constants of the arithmetic phases spill to VGPR lanes otherwise: 192 -> 154 spilled SGPRs, merge stage of a lone frame 33.0 -> 31.8 ms); every access through them
        // is a FLAT one with its address in VGPRs anyway.  The region bookkeeping (rstart, rnleaf, rcap, rcnt) stays in SGPRs: its scalar loads head every merge (parked: 32.2 ms)
        struct Cold { uint32_t* merges; unsigned char* ralive; uint32_t* parent; uint32_t* ev_epoch; uint32_t* ev_key; int* ev_prev; int* ehist; DevCounters* dc; };
        __shared__ Cold s_cold;
        const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
        MergeParams mp = m.mp;
        if (mp.merging == 1) mp.lambda = m.dc->lambda;
        for (uint32_t e = tid; e < L.Ecap; e += T) {
            if (IN_LDS) akey[e] = e < m.E ? m.eku[e] : KEY_DEAD;
            else if (e >= m.E) akey[e] = KEY_DEAD;
            eab[e] = e < m.E ? ((m.ea[e] << 16) | m.eb[e]) : 0xFFFFFFFFu;
        }
        for (uint32_t i = tid; i < 2u * MC_TL_CAP; i += T) hsh[i] = 0u;
        for (uint32_t i = tid; i < L.NGcap; i += T) G1[i] = KEY_DEAD;
        for (uint32_t i = tid; i < (L.NGcap + 31u) / 32u; i += T) dmask[i] = 0u;
        m_table_fill(s_mtab, tid, (int)T);
        if (wave < 2) __builtin_amdgcn_s_setprio(3);       // the waves that carry the sequential parts go first on their SIMD (raised priority for ALL waves of the 4-wave loop: no difference in flight, 2 774 vs 2 800 Mpoints/s over three alternating runs)
        if (tid == 0) { s_nt = 0; s_nevents = m.E; s_err = 0; s_pool_end = m.S0 + 1u; s_ipool_end = 2u * m.E; s_ndirty = 0u; s_nt2 = 0u; s_cross = 0u; s_min1 = KEY_DEAD; }
        if (tid == 0) { s_cold.merges = m.merges; s_cold.ralive = m.ralive; s_cold.parent = m.parent; s_cold.ev_epoch = m.ev_epoch; s_cold.ev_key = m.ev_key; s_cold.ev_prev = m.ev_prev; s_cold.ehist = m.ehist; s_cold.dc = m.dc; }
        const uint32_t ev_cap = m.ev_cap;
        uint32_t nmerges = 0;
        __syncthreads();
        // ---- the smallest key of every group of MC_GROUP = 16 slots (G1), one 16-lane DPP row per group: four v_min with lane swizzles.  For all groups once, here;
        // afterwards a changed key below its group's minimum lowers G1 with an LDS atomicMin, and only the groups whose minimum itself went away (the merged edge, a
        // re-weighted or dropped edge that WAS the minimum: a tenth of the touched edges) are looked at again (dlist) before the next argmin.
        auto rescan = [&](const uint32_t count, const bool from_list) {
            const uint32_t row = (uint32_t)lane >> 4, l16 = (uint32_t)lane & 15u;
            for (uint32_t base = (uint32_t)wave * 4u; base < count; base += (uint32_t)NW * 4u) {      // (wave-uniform: four groups per wave and round)
                const uint32_t i = base + row;
                const bool valid = i < count;
                const uint32_t g = valid ? (from_list ? dlist[i] : i) : 0u;
                const uint32_t k = valid ? akey[g * MC_GROUP + l16] : KEY_DEAD;
                const uint32_t m1 = row_min_u32(k);
                if (valid && l16 == 0u) {
                    G1[g] = m1;
                    if (from_list) atomicAnd(&dmask[g >> 5], ~(1u << (g & 31u)));
                }
            }
        };
        auto mark_dirty = [&](const uint32_t e) {      // the group of slot e has its smallest key worked out again before the next argmin
            const uint32_t g = e / MC_GROUP, bit = 1u << (g & 31u);
            if (!(atomicOr(&dmask[g >> 5], bit) & bit)) dlist[atomicAdd(&s_ndirty, 1u)] = g;
        };
        // slot e's key goes from kold to knew (KEY_DEAD: the edge is gone).  A smaller key than the group's minimum becomes the minimum on the spot; a key that WAS the
        // minimum and moves up sends the group to the rescan list; any other change leaves G1 as it is.  (G1 may already have been lowered by another lane of this epoch
        // when it is read here: then that lower key is the group's minimum whatever became of the old one, and nothing is lost by not rescanning.)
        auto key_changed = [&](const uint32_t e, const uint32_t kold, const uint32_t knew) {
            uint32_t* gp = &G1[e / MC_GROUP];
            const uint32_t g1 = *gp;
            if (knew < g1) atomicMin(gp, knew);
            else if (kold == g1) mark_dirty(e);
        };
        rescan(L.Ecap / MC_GROUP, false);
        __syncthreads();
    #ifdef F3DS_MERGE_PROF   // per-phase shader-clock totals, printed by thread 0 (make PROF=1)
        unsigned long long tph[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tlast = __builtin_amdgcn_s_memtime(), tph_nt = 0, tph_rows = 0, tph_slow = 0, tph_geo = 0, tph_lab = 0, tph_nd = 0;
        unsigned long long sp_cand = 0, sp_disjoint = 0, sp_small = 0, sp_scan = 0, sp_ok = 0, sp_epochs = 0;
        unsigned long long cls_n[4] = {0, 0, 0, 0}, cls_rows[4] = {0, 0, 0, 0}, cls_fold[4] = {0, 0, 0, 0}, cls_all[4] = {0, 0, 0, 0}, cls_prev_rows = 0, cls_prev_fold = 0, cls_prev_all = 0, cls_prev_w = 0, cls_prev_scan = 0;
        unsigned long long cle_n[4] = {0, 0, 0, 0}, cle_nt[4] = {0, 0, 0, 0}, cle_w[4] = {0, 0, 0, 0}, cle_scan[4] = {0, 0, 0, 0}, cle_all[4] = {0, 0, 0, 0};
        const unsigned long long loop_u0 = __builtin_amdgcn_s_memtime(), loop_w0 = __builtin_amdgcn_s_memrealtime();
    #define TPH(i) do { if (tid == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); tph[i] += now_ - tlast; tlast = now_; } } while (0)
    #else
    #define TPH(i) do { } while (0)
    #endif
        // Speculative second merge of an epoch (8 waves).  57 % of the merges of a 1M-point frame have nothing to do with the one before them: neither
        // region of the runner-up edge e2 is a, b or a neighbour of theirs.  Then e2 is the next merge PROVIDED no edge re-weighted by the first merge ends
        // up below it -- which is known once those weights are.  So while waves 0, 1, 4-7 carry the first merge, waves 2 and 3 (idle in the fold and record
        // phases otherwise) run the second one -- rows of b2 staged and folded, record built, its adjacencies re-weighted next to the first merge's --
        // into private state, and it is committed (epoch + 1) only if k2 < every new key of the first merge; otherwise it is dropped and e2 meets the next
        // epoch's scan again.  Kept simple: b2 at most MC_SP_LEAVES supervoxels of at most L.sp_rows voxels together, no ties at k2, all
        // touched edges of both merges re-weighted in one pass.  Same merges in the same order, same bits (MERGES, weights, histories).
        constexpr bool SPEC = true;
        const bool spec_on = SPEC && x.spec != 0;
        // (the attempt costs every epoch a wider scan and a second touched list: where few attempts end in a commit -- big supervoxels, BASELINE config 4:
        // b2 is rarely one small leaf -- it is a loss (merge stage 170 vs 158 ms there), so the speculation rests for 256 epochs whenever fewer than a
        // quarter of the last 64 attempts were committed)
        uint32_t sp_try = 0u, sp_hit = 0u, sp_rest = 0u;
        for (uint32_t epoch = 1;; ++epoch) {
            // ---- the groups whose keys the last merge changed get their two smallest keys again (four groups per wave and round)
#ifdef F3DS_EXP_DUP_A      // timing experiment: the whole argmin (rescan of the dirty groups, wave 0's argmin, hand-over) twice
            for (int dup_ = 0; dup_ < 2; ++dup_) {
#endif
            {
                const uint32_t nd = s_ndirty;
    #ifdef F3DS_MERGE_PROF
                if (tid == 0) { tph_nd += nd; TPH(15); }
    #endif
                rescan(nd, true);
            }
            TPH(11);
            __syncthreads();
            TPH(12);
#ifndef F3DS_EXP_DUP_A
            if (tid == 0) s_ndirty = 0u;
#endif
            // ---- next = *weight_map.begin(): argmin over the group minima, by wave 0 alone (E / 16 values: a handful per lane; eight waves doing it side by side would
            // share SIMDs, a split over the waves costs a second reduction level).  A lane keeps its minimum and the group it belongs to (and, for the speculation, its
            // second smallest with its group and the value of the third); DPP wave minima give the winner, the runner-up group minimum q2 and the third q3.
            if constexpr (SPEC) { if (sp_rest) sp_rest--; }
            if (wave == 0) {
                uint32_t kloc = KEY_DEAD, gloc = 0u, tieloc = 0u;
                uint32_t k2loc = KEY_DEAD, g2loc = 0u, k3loc = KEY_DEAD;
                // (four group minima per lane and LDS round trip: read one by one -- read, wait, compare -- the loop was an LDS latency per value, 8 per epoch on a
                // 1M-point frame and 25 on the 20M scene.  NGcap is a multiple of 64: a round is all lanes or none.)
                for (uint32_t g0 = (uint32_t)lane; g0 < L.NGcap; g0 += 256u) {
                    uint32_t mm[4];
            #pragma unroll
                    for (int u = 0; u < 4; ++u) { const uint32_t g = g0 + 64u * (uint32_t)u; mm[u] = G1[g < L.NGcap ? g : g0]; }
            #pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t g = g0 + 64u * (uint32_t)u;
                        if (g >= L.NGcap) break;
                        const uint32_t m4 = mm[u];
                        if constexpr (SPEC) {
                            const bool lt1 = m4 < kloc, lt2 = m4 < k2loc, lt3 = m4 < k3loc;
                            k3loc = lt2 ? k2loc : (lt3 ? m4 : k3loc);
                            g2loc = lt1 ? gloc : (lt2 ? g : g2loc); k2loc = lt1 ? kloc : (lt2 ? m4 : k2loc);
                        }
                        if (m4 == kloc) tieloc = 1u;
                        if (m4 < kloc) { kloc = m4; gloc = g; tieloc = 0u; }
                    }
                }
                const uint32_t kmin_ = wave_min_u32(kloc);
                const uint64_t hit = __ballot(kloc == kmin_);
                const int src = __builtin_ctzll(hit);
                const uint32_t gbest = (uint32_t)__builtin_amdgcn_readlane((int)gloc, src);
                uint32_t tie_ = ((hit & (hit - 1ull)) != 0ull || (__ballot(tieloc != 0u) & hit) != 0ull) ? 1u : 0u;
                // the wave's second and third smallest group minima (speculation): the winner lane offers its second value, then whoever won offers its next one
                const bool want2 = SPEC && spec_on && !tie_ && sp_rest == 0u && kmin_ < x.stop_key;      // (uniform)
                uint32_t q2 = KEY_DEAD, g2 = 0u, q3 = KEY_DEAD;
                if (want2) {
                    const uint32_t o2 = lane == src ? k2loc : kloc, og2 = lane == src ? g2loc : gloc;
                    q2 = wave_min_u32(o2);
                    const int src2 = __builtin_ctzll(__ballot(o2 == q2));
                    g2 = (uint32_t)__builtin_amdgcn_readlane((int)og2, src2);
                    const uint32_t o3 = lane == src ? (lane == src2 ? k3loc : k2loc) : (lane == src2 ? k2loc : kloc);
                    q3 = wave_min_u32(o3);
                }
                // the 16 keys of the winner's group (DPP row 0) and of the runner-up group (row 1): position of the smallest, the second smallest with its position,
                // and whether that second value occurs more than once
                const uint32_t row = (uint32_t)lane >> 4, l16 = (uint32_t)lane & 15u;
                // (the endpoints of the 16 + 16 slots travel WITH their keys: asked for once the position of the smallest key is known they were a second dependent trip --
                // to L2 when the per-edge arrays live in global memory, the layout of the calls that share the device)
                const bool rowon = row == 0u || (row == 1u && want2);
                const uint32_t slot0 = (row == 0u ? gbest : g2) * MC_GROUP + l16;
                const uint32_t kk0 = rowon ? akey[slot0] : KEY_DEAD;
                const uint32_t abrow = rowon ? eab[slot0] : 0u;
                const uint32_t m1 = row_min_u32(kk0);
                const uint32_t bits1 = (uint32_t)(__ballot(kk0 == m1) >> (row * 16u)) & 0xFFFFu;
                const uint32_t pos1 = (uint32_t)__builtin_ctz(bits1 | 0x10000u);
                const uint32_t kk1 = l16 == pos1 ? KEY_DEAD : kk0;
                const uint32_t m2 = row_min_u32(kk1);
                const uint32_t bits2 = (uint32_t)(__ballot(kk1 == m2) >> (row * 16u)) & 0xFFFFu;
                const uint32_t pos2 = (uint32_t)__builtin_ctz(bits2 | 0x10000u) & 15u;
                const uint32_t dup2 = (m2 != KEY_DEAD && __popc(bits2) >= 2) ? 1u : 0u;
                const uint32_t c2 = (uint32_t)__builtin_amdgcn_readlane((int)m2, 0), p1 = (uint32_t)__builtin_amdgcn_readlane((int)pos1, 0), p2 = (uint32_t)__builtin_amdgcn_readlane((int)pos2, 0);
                const uint32_t d2 = (uint32_t)__builtin_amdgcn_readlane((int)dup2, 0);
                if (c2 == kmin_) tie_ = 1u;
                const uint32_t best_ = gbest * MC_GROUP + p1;
                uint32_t best2_ = 0u, kmin2_ = KEY_DEAD, spec_ = 0u, lane2_ = 0u;
                if (want2 && !tie_) {
                    // the runner-up KEY: the smaller of the winner group's second key and the second group minimum.  It has to be the only key of its value
                    // (an equal key anywhere means the map order decides -> no speculation): inside the winner's group dup2 says whether its second value
                    // repeats; across groups an equal key shows as an equal group minimum (q3) or as the runner-up group's own second key
                    const uint32_t r_c2 = (uint32_t)__builtin_amdgcn_readlane((int)m2, 16), r_p1 = (uint32_t)__builtin_amdgcn_readlane((int)pos1, 16);
                    bool unique = false;
                    if (c2 < q2) { kmin2_ = c2; best2_ = gbest * MC_GROUP + p2; lane2_ = p2; unique = d2 == 0u; }
                    else if (q2 < c2) { kmin2_ = q2; best2_ = g2 * MC_GROUP + r_p1; lane2_ = 16u + r_p1; unique = r_c2 != q2 && q3 != q2; }
                    spec_ = (unique && kmin2_ > kmin_ && kmin2_ < x.stop_key) ? 1u : 0u;
                }
                const uint32_t ab_ = (uint32_t)__builtin_amdgcn_readlane((int)abrow, (int)p1), ab2_ = spec_ ? (uint32_t)__builtin_amdgcn_readlane((int)abrow, (int)lane2_) : 0u;
                if (lane == 0) { s_arg[0] = kmin_; s_arg[1] = best_; s_arg[2] = tie_; s_arg[3] = spec_; s_arg[4] = best2_; s_arg[5] = kmin2_; s_arg[6] = ab_; s_arg[7] = ab2_; }
            }
            TPH(13);
            __syncthreads();
            TPH(14);
#ifdef F3DS_EXP_DUP_A
            }
            if (tid == 0) s_ndirty = 0u;
#endif
            const uint4 arg0 = *reinterpret_cast<const uint4*>(&s_arg[0]), arg1 = *reinterpret_cast<const uint4*>(&s_arg[4]);
            const uint32_t kmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)arg0.x);
            if (!(kmin < x.stop_key)) break;              // (uniform) nothing left below the threshold
            uint32_t best = (uint32_t)__builtin_amdgcn_readfirstlane((int)arg0.y);
            const uint32_t tie = (uint32_t)__builtin_amdgcn_readfirstlane((int)arg0.z);
            bool spec = __builtin_amdgcn_readfirstlane((int)arg0.w) != 0;
            const uint32_t best2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)arg1.x), kmin2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)arg1.y);      // runner-up edge and its key
    #ifdef F3DS_MERGE_PROF
            if (spec) sp_cand++;
    #endif
            if (tie) {
                // equal minimum keys: the weight_map order (history comparator) decides among all of them
                for (uint32_t e = tid; e < L.Ecap; e += T)
                    if (akey[e] == kmin) { const uint32_t i = atomicAdd(&s_nt, 1u); if (i < MC_TL_CAP) tl[i] = e; }
                __syncthreads();
                const uint32_t nc = s_nt;
                if (nc > MC_TL_CAP) { if (tid == 0) s_cold.dc->error = F3DS_ERR_UNSUPPORTED; break; }      // (uniform) the host falls back to d_merge
                if (tid == 0) {
                    uint32_t bb = tl[0];
                    for (uint32_t i = 1; i < nc; ++i) { const uint32_t f = tl[i]; if (a_edge_before(EdgeHist{s_cold.ev_epoch, s_cold.ev_key, s_cold.ev_prev}, f, kmin, s_cold.ehist[f], bb, kmin, s_cold.ehist[bb])) bb = f; }
                    s_best = bb; s_nt = 0u;
                }
                __syncthreads();
                best = s_best;
    #ifdef F3DS_MERGE_PROF
                tph_slow++;
    #endif
            }
            TPH(0);
            const uint32_t ab_best = tie ? eab[best] : (uint32_t)__builtin_amdgcn_readfirstlane((int)arg1.z);
            const uint32_t a = ab_best >> 16, b = ab_best & 0xFFFFu;
            uint32_t a2 = 0u, b2 = 0u;
            if constexpr (SPEC) {
                if (spec) {
                    const uint32_t ab2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)arg1.w);
                    a2 = ab2 >> 16; b2 = ab2 & 0xFFFFu;
                    if (a2 == a || a2 == b || b2 == a || b2 == b) spec = false;      // (uniform) the runner-up hangs on the first merge's regions: it is re-weighted, not merged
                    if (spec) sp_try++;
    #ifdef F3DS_MERGE_PROF
                    if (spec) sp_disjoint++;
    #endif
                }
            }
            if (tid == 0) {
                const uint32_t wb = (kmin & 0x80000000u) ? (kmin & 0x7fffffffu) : ~kmin;      // weight bits from the order key (never -0 or NaN here)
                uint32_t* mg = s_cold.merges; mg[nmerges * 3u] = a; mg[nmerges * 3u + 1u] = b; mg[nmerges * 3u + 2u] = wb;
            }
            nmerges++;
            // the leaf arrays of a and b: their loads are in flight while the endpoints are scanned
            const uint32_t a_start = x.rstart[a], na = x.rnleaf[a], cap_a = x.rcap[a], b_start = x.rstart[b], nb = x.rnleaf[b];
            const uint32_t cnt_a = m.rcnt[a];
            // the incident-edge lists of a and b (and of a2, b2), walked below instead of a scan of all endpoints
            const uint32_t il_a = x.istart[a], il_na = x.ilen[a], il_ca = x.icap[a], il_b = x.istart[b], il_nb = x.ilen[b];
            // b's own voxel rows: while b is a single supervoxel (most merges) they are its only leaf -- known from this first round of loads, without the trip through its leaf array
            const uint32_t b_off0 = m.loff[b], b_len0 = m.llen[b];
            // (speculative second merge: the same of a2 and b2, requested now and looked at after the scan -- b2 has to be a few leaves of at most L.sp_rows rows together.
            // Requested as VECTOR loads, through an index the compiler cannot see is zero: as scalar loads -- the addresses are uniform -- the dependent pair
            // rstart[b2] -> pool[...] would sit on the LDS wait counter, and the endpoint scan's first LDS read would wait for both round trips.)
            uint32_t v_a2s = 0u, v_na2 = 0u, v_cnt2 = 0u, v_cap2 = 0u, v_nb2 = 0u, v_b2s = 0u, v_rows2 = 0u;
            uint32_t v_il_a2 = 0u, v_il_na2 = 0u, v_il_ca2 = 0u, v_il_b2 = 0u, v_il_nb2 = 0u;
            uint2 v_leaf2 = make_uint2(0u, 0u);
            if constexpr (SPEC) {
                if (spec) {
                    uint32_t vz;
                    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
                    v_a2s = x.rstart[a2 + vz]; v_na2 = x.rnleaf[a2 + vz]; v_cnt2 = m.rcnt[a2 + vz]; v_cap2 = x.rcap[a2 + vz]; v_nb2 = x.rnleaf[b2 + vz];
                    v_leaf2 = make_uint2(m.loff[b2 + vz], m.llen[b2 + vz]);      // (while b2 is a single supervoxel its own rows are its only leaf; else its leaf array is fetched by the staging waves)
                    v_b2s = x.rstart[b2 + vz]; v_rows2 = m.rcnt[b2 + vz];
                    v_il_a2 = x.istart[a2 + vz]; v_il_na2 = x.ilen[a2 + vz]; v_il_ca2 = x.icap[a2 + vz]; v_il_b2 = x.istart[b2 + vz]; v_il_nb2 = x.ilen[b2 + vz];
                }
            }
            float acc = 0.0f;
            if (wave == 0 && lane < 9) acc = m.racc[(size_t)a * 12 + lane];
            if (wave == 1 && lane < 3) acc = m.racc[(size_t)a * 12 + 9 + lane];
            if constexpr (SPEC) {
                if (spec && wave == 2 && lane < 9) acc = m.racc[(size_t)a2 * 12 + lane];
                if (spec && wave == 3 && lane < 3) acc = m.racc[(size_t)a2 * 12 + 9 + lane];
            }
            const uint2 leaf0 = (uint32_t)tid < nb ? x.pool[b_start + tid] : make_uint2(0u, 0u);      // first T leaves of b, kept for the gather
            TPH(5);
            // ---- edges that touch a or b: the two regions' incident lists are walked (Clustering::merge visits exactly these weight_map entries); an entry whose edge
            // is gone, or is the merged edge itself, is skipped.  One ballot + one LDS atomic per wave and round give the hits their slots in the touched list,
            // the lanes enter them in the partner hash.  With a speculative second merge the upper half of the workgroup walks the lists of a2 and b2 into a
            // second touched list (tl2 / tx2; hash keys carry the list) at the same time; an edge from a or b to a2 or b2 joins the two merges: no speculation then.
            auto walk = [&](const uint32_t i0, const uint32_t stride, const uint32_t sA, const uint32_t lA, const uint32_t sB, const uint32_t lB, const uint32_t pa, const uint32_t pb,
                            const uint32_t skip, const uint32_t second, const uint32_t oa, const uint32_t ob) {
                const uint32_t n = lA + lB;
                for (uint32_t base = 0; base < n; base += stride) {       // (uniform per wave)
                    const uint32_t i = base + i0;
                    uint32_t e = 0u, ab = 0xFFFFFFFFu;
                    if (i < n) { e = x.ilist[i < lA ? sA + i : sB + (i - lA)]; ab = eab[e]; }
                    const bool hit = ab != 0xFFFFFFFFu && e != skip;
                    const uint32_t p = ab >> 16, q = ab & 0xFFFFu;
                    const bool on_a = p == pa || q == pa;
                    const uint32_t xx = (p == pa || p == pb) ? q : p;
                    if (hit && (xx == oa || xx == ob)) s_cross = 1u;
                    const uint64_t hm = __ballot(hit);
                    if (hm == 0ull) continue;
                    uint32_t wbase = 0u;
                    if (lane == 0) wbase = atomicAdd(second ? &s_nt2 : &s_nt, (uint32_t)__popcll(hm));
                    wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
                    const uint32_t idx = wbase + (uint32_t)__popcll(hm & lanemask_lt());
                    if (hit && idx < (second ? MC_SP_TL : MC_TL_CAP)) {
                        (second ? tl2 : tl)[idx] = e; (second ? tx2 : tx)[idx] = xx | (on_a ? 0u : 0x80000000u);
                        const uint32_t hk = ((xx << 2) | (second << 1) | (on_a ? 0u : 1u)) + 1u;      // (region on the far end, which merge, which side)
                        for (uint32_t sl = (hk * 2654435761u) >> 21;; sl = (sl + 1u) & (2u * MC_TL_CAP - 1u))
                            if (atomicCAS(&hsh[sl], 0u, (hk << 10) | idx) == 0u) break;
                    }
                }
            };
            if (SPEC && spec) {
                if ((uint32_t)tid < T / 2u) walk((uint32_t)tid, T / 2u, il_a, il_na, il_b, il_nb, a, b, best, 0u, a2, b2);
                else walk((uint32_t)tid - T / 2u, T / 2u, v_il_a2, v_il_na2, v_il_b2, v_il_nb2, a2, b2, best2, 1u, 0xFFFFFFFFu, 0xFFFFFFFFu);
            } else walk((uint32_t)tid, T, il_a, il_na, il_b, il_nb, a, b, best, 0u, 0xFFFFFFFFu, 0xFFFFFFFFu);
            TPH(6);
            // leaf array of a ++ b: append in place while a's segment has room, else move to a segment twice the size
            const bool in_place = na + nb <= cap_a;
            const uint32_t new_start = in_place ? a_start : s_pool_end;
            const uint32_t new_cap = in_place ? cap_a : 2u * (na + nb);
            if (!in_place && new_start + new_cap > x.pool_cap) { if (tid == 0) { DevCounters* dcp = s_cold.dc; dcp->error = F3DS_ERR_UNSUPPORTED; dcp->ev_overflow = F3DS_OVF_LEAF_POOL; } break; }      // (uniform) leaf pool full: rerun with a larger one
            if (in_place) { for (uint32_t i = tid; i < nb; i += T) x.pool[a_start + na + i] = i < T ? leaf0 : x.pool[b_start + i]; }
            else { for (uint32_t i = tid; i < na + nb; i += T) x.pool[new_start + i] = i < na ? x.pool[a_start + i] : x.pool[b_start + (i - na)]; }
            TPH(7);
            __syncthreads();
            TPH(1);
            const uint32_t nt = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_nt);
            uint32_t nt2 = 0u;
            uint32_t a2_start = 0u, na2 = 0u, cnt_a2 = 0u, cap_a2 = 0u, nb2 = 0u, il_a2 = 0u, il_ca2 = 0u, b2_start = 0u, rows2 = 0u;
            uint2 leaf2 = make_uint2(0u, 0u);
            if constexpr (SPEC) {
                if (spec) {
                    nt2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_nt2);
                    // an edge between the two merges, lists that do not fit side by side, or more touched edges than one re-weighting pass has lanes: the first merge alone
                    if (s_cross != 0u || nt2 > MC_SP_TL || nt + nt2 > T) spec = false;      // (uniform)
    #ifdef F3DS_MERGE_PROF
                    if (spec) sp_scan++;
    #endif
                }
                if (spec) {
                    a2_start = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_a2s); na2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_na2); cnt_a2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_cnt2);
                    cap_a2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_cap2); nb2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_nb2);
                    leaf2.x = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_leaf2.x); leaf2.y = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_leaf2.y);
                    il_a2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_il_a2); il_ca2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_il_ca2);
                    b2_start = (uint32_t)__builtin_amdgcn_readfirstlane((int)v_b2s);
                    // the absorbed region: at most MC_SP_LEAVES supervoxels of at most SPR voxels together (staged by the two spare waves)
                    rows2 = nb2 == 1u ? leaf2.y : (uint32_t)__builtin_amdgcn_readfirstlane((int)v_rows2);
                    if (nb2 == 0u || nb2 > MC_SP_LEAVES || rows2 > SPR || rows2 == 0u) spec = false;            // (uniform)
    #ifdef F3DS_MERGE_PROF
                    if (spec) sp_small++;
    #endif
                }
            }
            // leaf array of a2 ++ b2, prepared by waves 2 and 3: in place behind a2's leaves, else in a fresh segment behind the first merge's (the pool end only
            // moves when the second merge is committed; what is written here is beyond every region's reach until then)
            bool in_place2 = true; uint32_t new_start2 = 0u, new_cap2 = 0u;
            if constexpr (SPEC) {
                if (spec) {
                    in_place2 = na2 + nb2 <= cap_a2;
                    new_start2 = in_place2 ? a2_start : s_pool_end + (in_place ? 0u : new_cap);
                    new_cap2 = in_place2 ? cap_a2 : 2u * (na2 + nb2);
                    if (!in_place2 && new_start2 + new_cap2 > x.pool_cap) spec = false;              // (uniform) no room to prepare it: the first merge alone
                }
            }
    #ifdef F3DS_MERGE_PROF
            if (tid == 0) tph_nt += nt;
    #endif
            if (nt > MC_TL_CAP) { if (tid == 0) s_cold.dc->error = F3DS_ERR_UNSUPPORTED; break; }      // (uniform) the host falls back to d_merge
            // the merged region's incident list = the touched list (the duplicates contains() drops below stay in it as dead entries until a's next merge):
            // over a's old list when it fits, else in a fresh segment at the end of the list pool
            const bool il_in_place = nt <= il_ca;
            const uint32_t il_pool_end = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_ipool_end);
            const uint32_t il_new = il_in_place ? il_a : il_pool_end;
            const uint32_t il_newcap = il_in_place ? il_ca : nt + (nt >> 1) + 4u;
            if (!il_in_place && il_new + il_newcap > x.ilist_cap) { if (tid == 0) { DevCounters* dcp = s_cold.dc; dcp->error = F3DS_ERR_UNSUPPORTED; dcp->ev_overflow = F3DS_OVF_ILIST_POOL; } break; }      // (uniform) list pool full: rerun with a larger one (its own multiplier: f3ds_ctx::ilist_mult)
            for (uint32_t i = tid; i < nt; i += T) x.ilist[il_new + i] = tl[i];
            bool il_in_place2 = true; uint32_t il_new2 = 0u, il_newcap2 = 0u;
            if constexpr (SPEC) {
                if (spec) {       // (written only if the second merge is committed)
                    il_in_place2 = nt2 <= il_ca2;
                    il_new2 = il_in_place2 ? il_a2 : il_pool_end + (il_in_place ? 0u : il_newcap);
                    il_newcap2 = il_in_place2 ? il_ca2 : nt2 + (nt2 >> 1) + 4u;
                    if (!il_in_place2 && il_new2 + il_newcap2 > x.ilist_cap) spec = false;      // (uniform) no room to prepare it: the first merge alone
                }
            }
            // ---- voxels_new = voxels_a ++ voxels_b: b's rows through LDS (two buffers), a's ordered sums continue over them
            uint32_t rows_done = 0;
            bool dedupe_done = false;
            for (uint32_t lc = 0; lc < nb; lc += T) {
                const uint32_t nl = nb - lc < T ? nb - lc : T;
                uint32_t Tl;
                const bool one_leaf = nb == 1u;           // b is a single supervoxel (most merges): its rows are one run, nothing to scan
                uint32_t only_x = 0u;
                if (one_leaf) { Tl = b_len0; only_x = b_off0; }      // (uniform values from the scalar loads at the head of the merge: no hand-over, no barrier)
                else {
                    uint32_t len = 0, off = 0;
                    if ((uint32_t)tid < nl) { const uint2 lf = lc == 0u ? leaf0 : x.pool[b_start + lc + tid]; off = lf.x; len = lf.y; }
                    const uint32_t inc = block_incl_scan<BLOCK>(len, &Tl);
                    lstart[tid] = inc - len; lsrc[tid] = off;
                    if (tid == 0) lstart[T] = Tl;
                    __syncthreads();
                }
                TPH(8);
                Tl = (uint32_t)__builtin_amdgcn_readfirstlane((int)Tl);
                const uint32_t nchunks = (Tl + CH - 1u) / CH;
                float4 q0 = make_float4(0, 0, 0, 0), q1 = q0, q2 = q0;
                auto load_row = [&](uint32_t rr) {          // row rr of this leaf chunk -> registers
                    uint32_t lo = 0, hi = nl;              // last leaf with lstart <= rr
                    if (!one_leaf) while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (lstart[mid] <= rr) lo = mid; else hi = mid; }
                    const float4* src = reinterpret_cast<const float4*>(m.rows + (size_t)(one_leaf ? only_x + rr : lsrc[lo] + (rr - lstart[lo])) * 12);
                    q0 = src[0]; q1 = src[1]; q2 = src[2];
                };
                auto store_row = [&](uint32_t buf, uint32_t r, uint32_t index_plus_1) {
                    float4* dst = reinterpret_cast<float4*>(stage + ((size_t)buf * CH + r) * 12);
                    dst[0] = q0; dst[1] = q1; dst[2] = q2;
                    const float count = (float)index_plus_1;
                    sinv[buf * CH + r] = 1 / count;
                };
                // the threads that stage rows (one row each per chunk): with 8 waves the last four, so that the two waves that carry the
                // ordered folds do nothing else inside the chunk loop (leaf search, row loads and stores are the others' work)
                const uint32_t ld = (uint32_t)tid - (T - CH);
                const bool loader = (uint32_t)tid >= T - CH;
                if (loader && ld < Tl) load_row(ld);
                // (speculative second merge: b2's rows -- at most SPR -- are staged beside the loaders' first chunk, one per lane: rows 0..127 by waves 2 and 3, with eight waves
                // the next 256 by waves 4..7 and the last 128 by waves 0 and 1, which have nothing else to do before their folds)
                const bool sp_wave = SPEC && spec && lc == 0u && (wave == 2 || wave == 3);
                const uint32_t sp_r = ((uint32_t)tid - 128u) & (T - 1u);      // the row of b2 this lane stages
                const bool sp_loader = SPEC && spec && lc == 0u && sp_r < rows2;      // (rows2 <= SPR)
                float4 p0 = make_float4(0, 0, 0, 0), p1 = p0, p2 = p0;
                uint2 my_leaf2 = leaf2;          // the leaf of b2 this lane appends to a2's leaf array (lane t2 < nb2)
                uint32_t src_row2 = 0u;          // (8 waves) where this lane's row of a second round (sp_r + T) comes from
                if (SPEC && spec && lc == 0u && (NW == 8 || wave >= 2)) {  // (uniform per wave)
                    uint32_t src_row = leaf2.x + sp_r;
                    src_row2 = src_row + T;
                    if (nb2 > 1u) {              // b2 is a few supervoxels: its leaf array, then every lane finds the leaf its row sits in
                        uint2 lf[MC_SP_LEAVES];
        #pragma unroll
                        for (uint32_t j = 0; j < MC_SP_LEAVES; ++j) lf[j] = j < nb2 ? x.pool[b2_start + j] : make_uint2(0u, 0u);
                        if (sp_wave && sp_r < nb2) my_leaf2 = x.pool[b2_start + sp_r];
                        uint32_t first = 0u; src_row = 0u; src_row2 = 0u;
        #pragma unroll
                        for (uint32_t j = 0; j < MC_SP_LEAVES; ++j) {
                            if (sp_r >= first && sp_r - first < lf[j].y) src_row = lf[j].x + (sp_r - first);
                            if (NW == 8 && sp_r + T >= first && sp_r + T - first < lf[j].y) src_row2 = lf[j].x + (sp_r + T - first);
                            first += lf[j].y;
                        }
                    }
                    if (sp_loader) { const float4* src = reinterpret_cast<const float4*>(m.rows + (size_t)src_row * 12); p0 = src[0]; p1 = src[1]; p2 = src[2]; }
                }
                // (and prepare a2's leaf array: its first 128 leaves travel with the rows, a longer array behind them)
                uint2 pl = make_uint2(0u, 0u);
                if (sp_wave && !in_place2 && (uint32_t)(tid - 128) < na2) pl = x.pool[a2_start + (uint32_t)(tid - 128)];
                if (!dedupe_done) {
                    // contains(): of (a,x) and (b,x) the entry that comes first in the old map survives (while the first rows are in flight)
                    auto dedupe = [&](uint32_t* dl, uint32_t* dx, uint32_t n, uint32_t second) {
                        for (uint32_t i = tid; i < n; i += T) {
                            const uint32_t t = dx[i], want = (((t & 0xFFFFu) << 2) | (second << 1) | ((t >> 31) ^ 1u)) + 1u;     // the edge from the other of a, b to the same region
                            uint32_t pj = 0xFFFFFFFFu;
                            for (uint32_t sl = (want * 2654435761u) >> 21;; sl = (sl + 1u) & (2u * MC_TL_CAP - 1u)) {
                                const uint32_t h = hsh[sl];
                                if (h == 0u) break;
                                if ((h >> 10) == want) { pj = h & 1023u; break; }
                            }
                            if (pj != 0xFFFFFFFFu) {
                                const uint32_t e = dl[i] & 0x7fffffffu, partner = dl[pj] & 0x7fffffffu;
                                if (akey[partner] != akey[e] ? akey[partner] < akey[e] : a_edge_before(EdgeHist{s_cold.ev_epoch, s_cold.ev_key, s_cold.ev_prev}, partner, akey[partner], s_cold.ehist[partner], e, akey[e], s_cold.ehist[e])) dx[i] = t | 0x40000000u;      // dropped (flag in tx: tl is read by the partner)
                            }
                        }
                    };
                    dedupe(tl, tx, nt, 0u);
                    if (SPEC && spec) dedupe(tl2, tx2, nt2, 1u);
                    dedupe_done = true;
                }
                if (loader && ld < Tl) store_row(0u, ld, cnt_a + rows_done + ld + 1u);
                if (sp_loader) {
                    float4* dst = reinterpret_cast<float4*>(stage2 + (size_t)sp_r * 12);
                    dst[0] = p0; dst[1] = p1; dst[2] = p2;
                    const float count = (float)(cnt_a2 + sp_r + 1u);
                    sinv2[sp_r] = 1 / count;
                    if (NW == 8 && sp_r + T < rows2) {      // a second round (more than 512 rows: rare outside scenes of big supervoxels), after the first: no registers held across the dedupe above
                        const uint32_t r = sp_r + T;
                        const float4* src = reinterpret_cast<const float4*>(m.rows + (size_t)src_row2 * 12);
                        const float4 s0 = src[0], s1 = src[1], s2 = src[2];
                        float4* d2 = reinterpret_cast<float4*>(stage2 + (size_t)r * 12);
                        d2[0] = s0; d2[1] = s1; d2[2] = s2;
                        const float c2 = (float)(cnt_a2 + r + 1u);
                        sinv2[r] = 1 / c2;
                    }
                }
                if (sp_wave) {
                    const uint32_t t2 = (uint32_t)(tid - 128);
                    if (in_place2) { if (t2 < nb2) x.pool[a2_start + na2 + t2] = my_leaf2; }
                    else {
                        if (t2 < na2) x.pool[new_start2 + t2] = pl;
                        for (uint32_t i = t2 + 128u; i < na2; i += 128u) x.pool[new_start2 + i] = x.pool[a2_start + i];
                        if (t2 < nb2) x.pool[new_start2 + na2 + t2] = my_leaf2;
                    }
                }
                TPH(9);
                __syncthreads();
                TPH(10);
                for (uint32_t c = 0; c < nchunks; ++c) {
                    // (the row count is the same in every lane, but it comes out of LDS: telling the compiler spares the loops below their exec-mask bookkeeping)
                    const uint32_t nr = (uint32_t)__builtin_amdgcn_readfirstlane((int)(Tl - c * CH < CH ? Tl - c * CH : CH));
                    const bool more = c + 1u < nchunks;
                    const uint32_t rn = (c + 1u) * CH + ld;
                    // (four waves: waves 2 and 3 are the loaders AND run the speculative second merge's folds in chunk 0.  Their row loads are FLAT loads, which count on the
                    // same wait counter as the folds' hand-counted LDS reads and may return out of order with them: "lgkmcnt(4)" would then no longer mean "set A has
                    // arrived".  Those waves request the next chunk's rows after their fold instead -- a merge that has both more than one chunk and a second merge is rare.)
                    const bool fold2_here = SPEC && spec && lc == 0u && c == 0u && (wave == 2 || wave == 3);
                    const bool load_later = fold2_here && loader;
                    if (more && loader && rn < Tl && !load_later) load_row(rn);
                    const float* buf = stage + (size_t)(c & 1u) * CH * 12;
                    const float* bi = sinv + (c & 1u) * CH;
                    // Both folds are one dependent chain per lane (one add per row; subtract, multiply, add per row): what can be saved is the wait for
                    // LDS.  Eight rows (set A) are consumed while the next eight (set B) are in flight.  The compiler does not keep such a pipeline (it
                    // regroups the reads and waits for all of them before the first add, also behind sched_barrier), so the reads and the waits are
                    // spelled out: FOLD_ISSUE_* requests a set, FOLD_WAIT_* waits until at most the younger set is outstanding (LDS answers in order) and
                    // ties the set's registers to that point.  The reads run up to 8 rows past nr: inside the staging area and its 64-byte tail, never used.
                    auto fold_sums = [&](const float* buf, const uint32_t nr) {          // lanes 0..8: nine ordered sums continue over nr staged rows
                        if (lane < 9) {
                            uint32_t arow = lds_addr(buf + lane);
                            f2v A_0, A_1, A_2, A_3, B_0, B_1, B_2, B_3;
                            FOLD_ISSUE_SUM(A, arow); arow += 8u * 48u;
                            uint32_t j = 0;
                            for (; j + 16u <= nr; j += 16u) {
                                FOLD_ISSUE_SUM(B, arow); arow += 8u * 48u;
                                FOLD_WAIT_SUM(A, 4);
                                acc += A_0.x; acc += A_0.y; acc += A_1.x; acc += A_1.y; acc += A_2.x; acc += A_2.y; acc += A_3.x; acc += A_3.y;
                                FOLD_ISSUE_SUM(A, arow); arow += 8u * 48u;
                                FOLD_WAIT_SUM(B, 4);
                                acc += B_0.x; acc += B_0.y; acc += B_1.x; acc += B_1.y; acc += B_2.x; acc += B_2.y; acc += B_3.x; acc += B_3.y;
                            }
                            // the last 0..15 rows: one more set requested at once, then as many adds as there are rows (uniform conditions: selects) -- a row-by-row
                            // tail paid an LDS round trip per row, and half of all merges fold fewer than 32 rows
    #define FOLD_TAIL_SUM(S, r) do { if ((r) > 0u) acc += S##_0.x; if ((r) > 1u) acc += S##_0.y; if ((r) > 2u) acc += S##_1.x; if ((r) > 3u) acc += S##_1.y; \
                                     if ((r) > 4u) acc += S##_2.x; if ((r) > 5u) acc += S##_2.y; if ((r) > 6u) acc += S##_3.x; if ((r) > 7u) acc += S##_3.y; } while (0)
                            // STRAIGHT-LINE on purpose: with the two sets consumed in the arms of an if / else the compiler unifies the arms' registers with copies that it
                            // places BEFORE the hand-written wait of one arm -- copying registers whose reads are still in flight (it cannot know they are asynchronous).
                            // So set B is always requested (reading past the rows is harmless: inside the staging area and what follows it), both sets are consumed with
                            // per-row conditions.
                            const uint32_t left = nr - j, la = left < 8u ? left : 8u;
                            FOLD_ISSUE_SUM(B, arow);
                            FOLD_WAIT_SUM(A, 4);
                            FOLD_TAIL_SUM(A, la);
                            FOLD_WAIT_SUM(B, 0);
                            FOLD_TAIL_SUM(B, left - la);
    #undef FOLD_TAIL_SUM
                        }
                    };
                    auto fold_colour = [&](const float* buf, const float* bi, const uint32_t nr) {      // lanes 0..2: the running colour mean continues over nr staged rows
                        if (lane < 3) {
                            uint32_t arow = lds_addr(buf + 9 + lane), ainv = lds_addr(bi);
                            f2v A_0, A_1, A_2, A_3, B_0, B_1, B_2, B_3;
                            f4v Ai0, Ai1, Bi0, Bi1;
    #define FOLD_STEP(c, i) acc = acc + (i) * ((c) - acc)
    #define FOLD_EIGHT(S) do { FOLD_STEP(S##_0.x, S##i0.x); FOLD_STEP(S##_0.y, S##i0.y); FOLD_STEP(S##_1.x, S##i0.z); FOLD_STEP(S##_1.y, S##i0.w); \
                               FOLD_STEP(S##_2.x, S##i1.x); FOLD_STEP(S##_2.y, S##i1.y); FOLD_STEP(S##_3.x, S##i1.z); FOLD_STEP(S##_3.y, S##i1.w); } while (0)
                            FOLD_ISSUE_COL(A, arow, ainv); arow += 8u * 48u; ainv += 32u;
                            uint32_t j = 0;
                            for (; j + 16u <= nr; j += 16u) {
                                FOLD_ISSUE_COL(B, arow, ainv); arow += 8u * 48u; ainv += 32u;
                                FOLD_WAIT_COL(A, 6);
                                FOLD_EIGHT(A);
                                FOLD_ISSUE_COL(A, arow, ainv); arow += 8u * 48u; ainv += 32u;
                                FOLD_WAIT_COL(B, 6);
                                FOLD_EIGHT(B);
                            }
    #define FOLD_TAIL_COL(S, r) do { if ((r) > 0u) FOLD_STEP(S##_0.x, S##i0.x); if ((r) > 1u) FOLD_STEP(S##_0.y, S##i0.y); if ((r) > 2u) FOLD_STEP(S##_1.x, S##i0.z); if ((r) > 3u) FOLD_STEP(S##_1.y, S##i0.w); \
                                     if ((r) > 4u) FOLD_STEP(S##_2.x, S##i1.x); if ((r) > 5u) FOLD_STEP(S##_2.y, S##i1.y); if ((r) > 6u) FOLD_STEP(S##_3.x, S##i1.z); if ((r) > 7u) FOLD_STEP(S##_3.y, S##i1.w); } while (0)
                            const uint32_t left = nr - j, la = left < 8u ? left : 8u;      // (straight-line: see fold_sums)
                            FOLD_ISSUE_COL(B, arow, ainv);
                            FOLD_WAIT_COL(A, 6);
                            FOLD_TAIL_COL(A, la);
                            FOLD_WAIT_COL(B, 0);
                            FOLD_TAIL_COL(B, left - la);
    #undef FOLD_TAIL_COL
    #undef FOLD_EIGHT
    #undef FOLD_STEP
                        }
                    };
#ifdef F3DS_EXP_DUP_F      // timing experiment: both ordered folds twice over every chunk (the first pass's result is thrown away behind an opaque move)
                    { const float acc0 = acc;
                      if (wave == 0) fold_sums(buf, nr); else if (wave == 1) fold_colour(buf, bi, nr);
                      float t_ = acc; asm volatile("" : "+v"(t_)); acc = acc0 + (t_ - t_); }
#endif
                    if (wave == 0) fold_sums(buf, nr);
                    else if (wave == 1) fold_colour(buf, bi, nr);
                    else if (fold2_here) {
                        const uint32_t nr2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rows2);
                        if (wave == 2) fold_sums(stage2, nr2); else fold_colour(stage2, sinv2, nr2);
                        if (more && load_later && rn < Tl) load_row(rn);
                    }
                    rows_done += nr;
                    if (more && loader && rn < Tl) store_row((c + 1u) & 1u, ld, cnt_a + rows_done + ld + 1u);
                    __syncthreads();
                }
    #ifdef F3DS_MERGE_PROF
                if (tid == 0) tph_rows += Tl;
    #endif
            }
            TPH(2);
            if (wave == 0 && lane < 9) m.racc[(size_t)a * 12 + lane] = acc;
            if (wave == 1 && lane < 3) m.racc[(size_t)a * 12 + 9 + lane] = acc;
            // ---- the merged region's record: wave 0 centroid + PCA normal, wave 1 mean colour -> Lab, each straight from
            // the sums it has just folded (no hand-over, no barrier: the last staging barrier is behind all waves).  Waves 2 and 3 do the same for the
            // speculative second merge, into s_rec2 only: nothing of it reaches global memory before it is committed.
            const uint32_t npre = (NW > 2 && !(SPEC && spec && T <= 256u)) ? (nt < 2u * CH ? nt : 2u * CH) : 0u;      // far-end records prefetched into the (free) staging area (four waves with a second merge: nobody is free to)
            auto record_geometry = [&](const uint32_t cnt, float* srec, const bool commit) {      // wave 0 (wave 2: second merge)
    #ifdef F3DS_MERGE_PROF
                const unsigned long long tg0 = __builtin_amdgcn_s_memtime();
    #endif
                float cen[3], n4[4];
                const m_lds mc = m_lds_here(s_mtab);
                if (cnt >= 3u) plane_normal_wave(acc, cnt, lane, cen, n4, mc);      // (uniform)
                else {
                    float all[9];
    #pragma unroll
                    for (int k = 0; k < 9; ++k) all[k] = wave_pick(acc, k);
                    const float c = (float)cnt;
                    cen[0] = all[6] / c; cen[1] = all[7] / c; cen[2] = all[8] / c;
                    n_plane_normal(all, cnt, cen, n4);
                }
    #ifdef F3DS_MERGE_PROF
                if (tid == 0) tph_geo += __builtin_amdgcn_s_memtime() - tg0;
    #endif
                if (lane == 0) {
                    for (int k = 0; k < 3; ++k) { srec[k] = cen[k]; srec[3 + k] = n4[k]; }
                    if (commit) {
                        for (int k = 0; k < 3; ++k) { m.rrec[(size_t)a * 16 + k] = cen[k]; m.rrec[(size_t)a * 16 + 3 + k] = n4[k]; }
                        m.rcnt[a] = cnt;
                        x.rstart[a] = new_start; x.rnleaf[a] = na + nb; x.rcap[a] = new_cap; if (!in_place) s_pool_end = new_start + new_cap;
                        x.istart[a] = il_new; x.ilen[a] = nt; x.icap[a] = il_newcap; if (!il_in_place) s_ipool_end = il_new + il_newcap;
                        s_cold.ralive[b] = 0; s_cold.parent[b] = a;
                    }
                }
            };
            auto record_colour = [&](float* srec, const bool commit) {        // wave 1 (wave 3: second merge)
                // n_rgb2lab with the three gamma curves and the three cube roots evaluated in lanes 0..2
    #ifdef F3DS_MERGE_PROF
                const unsigned long long tc0 = __builtin_amdgcn_s_memtime();
    #endif
                const float mr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 0)), mg = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 1)),
                            mb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), 2));
                float lab[3];
                const m_lds mc = m_lds_here(s_mtab);
                lab_three_lanes(lane == 0 ? mr : (lane == 1 ? mg : mb), lane, lab, mc);
                if (lane == 0) {
                    const float rec[6] = {mr, mg, mb, lab[0], lab[1], lab[2]};
                    for (int k = 0; k < 6; ++k) { srec[6 + k] = rec[k]; if (commit) m.rrec[(size_t)a * 16 + 6 + k] = rec[k]; }
    #ifdef F3DS_MERGE_PROF
                    if (commit) s_rec[12] = (float)(__builtin_amdgcn_s_memtime() - tc0);
    #endif
                }
            };
            auto prefetch_far_ends = [&](uint32_t first, uint32_t step) {
                for (uint32_t i = first; i < npre; i += step) {
                    if (tx[i] & 0x40000000u) continue;
                    const float4* gx = reinterpret_cast<const float4*>(m.rrec + (size_t)(tx[i] & 0xFFFFu) * 16);
                    const float4 x0 = gx[0], x1 = gx[1], x2 = gx[2];
                    float4* dst = reinterpret_cast<float4*>(stage + (size_t)i * 12);
                    dst[0] = x0; dst[1] = x1; dst[2] = x2;
                }
            };
            auto publish_edge = [&](uint32_t e, uint32_t lo, uint32_t hi, int hprev, uint32_t ku, uint32_t ep, uint32_t kold) {      // the new weight enters the edge's history and the order keys
                const uint32_t ev = atomicAdd(&s_nevents, 1u);
                if (ev >= ev_cap) { DevCounters* dcp = s_cold.dc; dcp->error = F3DS_ERR_UNSUPPORTED; dcp->ev_overflow = F3DS_OVF_EVENTS; s_err = 1; return; }
                s_cold.ev_epoch[ev] = ep; s_cold.ev_key[ev] = ku; s_cold.ev_prev[ev] = hprev;
                s_cold.ehist[e] = (int)ev;
                akey[e] = ku; eab[e] = (lo << 16) | hi;
                key_changed(e, kold, ku);
            };
            if (!(SPEC && spec)) rows2 = 0u;
#ifdef F3DS_EXP_DUP_R      // timing experiment: the record of the merged region twice
            if (wave == 0) record_geometry(cnt_a + rows_done, s_rec, true);
            else if (wave == 1) record_colour(s_rec, true);
#endif
            if (wave == 0) record_geometry(cnt_a + rows_done, s_rec, true);
            else if (wave == 1) record_colour(s_rec, true);
            else if (SPEC && spec && wave == 2) record_geometry(cnt_a2 + rows2, s_rec2, false);
            else if (SPEC && spec && wave == 3) record_colour(s_rec2, false);
            else if constexpr (NW > 2) {      // meanwhile the other waves bring the records on the far end of the kept edges into LDS
                if (SPEC && spec) { if (T > 256u && wave >= 4) prefetch_far_ends((uint32_t)tid - 256u, T - 256u); }
                else prefetch_far_ends((uint32_t)tid - 128u, T - 128u);
            }
            __syncthreads();
            TPH(3);
    #ifdef F3DS_MERGE_PROF
            if (tid == 0) tph_lab += (unsigned long long)s_rec[12];
    #endif
            // ---- re-weight the surviving incident edges (delta(), src/clustering.cpp:438-463).  With few edges a quad of
            // lanes shares one edge's CIEDE2000 (n_ciede00_quad); otherwise one lane per edge.
            // (a wave issues one f64 instruction per ~4.8 cycles whatever its active lanes, and two waves of one SIMD take turns:
            // the quad form pays only while its waves have a SIMD each); the two-wave layout is used for batches, where the
            // instructions issued count, not the latency: one lane per edge there.
            // (Measured and not kept: the colour distances on waves 1..7 as soon as wave 1 has the merged region's Lab, while wave 0 still
            // solves the normal's eigenproblem, geometry term and sum after the barrier -- Lab takes as long as the normal, so the chain
            // Lab -> CIEDE2000 -> geometry is no shorter than max(normal, Lab) -> weight: 32.4 vs 32.5 ms.)
            // With a speculative second merge its touched edges are re-weighted in the same pass (entries nt .. nt + nt2 - 1 of the pass), every edge on one
            // lane or quad at most once (nt + nt2 <= T), and nothing is published before the first merge's smallest new key is known.
            const uint32_t ntw = nt + (SPEC && spec ? nt2 : 0u);
            const bool quad = NW > 2 && mp.color_metric == 0 && ntw * 4u <= (T < 256u ? T : 256u);
            const int qsh = quad ? 2 : 0;
            bool valid2 = false;
            if (SPEC && spec) {
                const uint32_t i = (uint32_t)tid >> qsh;
                const bool mine = i < ntw, second = mine && i >= nt;
                const bool lead = !quad || (lane & 3) == 0;
                uint32_t e = 0u, txi = 0x40000000u, ku = KEY_DEAD, lo = 0u, hi = 0u, kold = KEY_DEAD; int hprev = 0, err = 0;
                if (mine) {
                    const uint32_t j = second ? i - nt : i;
                    e = second ? tl2[j] : tl[j]; txi = second ? tx2[j] : tx[j];
                    kold = akey[e];
                }
                if (mine && !(txi & 0x40000000u)) {
                    const uint32_t xx = txi & 0xFFFFu, ra = second ? a2 : a;
                    lo = ra < xx ? ra : xx; hi = ra < xx ? xx : ra;
                    float r1[12], r2[12];
                    hprev = s_cold.ehist[e];
                    {
                        const float4* gx = (!second && i < npre) ? reinterpret_cast<const float4*>(stage + (size_t)i * 12) : reinterpret_cast<const float4*>(m.rrec + (size_t)xx * 16);
                        const float4 x0 = gx[0], x1 = gx[1], x2 = gx[2];
                        const float rx[12] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w};
                        const bool a_first = ra < xx;
                        const float* sr = second ? s_rec2 : s_rec;
    #pragma unroll
                        for (int k = 0; k < 12; ++k) { const float rr = sr[k]; r1[k] = a_first ? rr : rx[k]; r2[k] = a_first ? rx[k] : rr; }
                    }
                    const m_lds mc = m_lds_here(s_mtab);
#ifdef F3DS_EXP_DUP_W      // timing experiment: the weight function twice (the second evaluation depends on the first: w0 - w0)
                    { const float w0 = quad ? edge_weight_quad(mp, r1, r2, lane & 3, &err, mc) : a_edge_weight(mp, r1, r2, &err, mc); r1[9] += (w0 - w0); }
#endif
                    const float w = quad ? edge_weight_quad(mp, r1, r2, lane & 3, &err, mc) : a_edge_weight(mp, r1, r2, &err, mc);
                    ku = n_weight_key(w);
                    if (lead && !second) atomicMin(&s_min1, ku);
                }
                __syncthreads();
                // the runner-up is the next merge iff every adjacency the first merge re-weighted now lies strictly above it (an equal key would have
                // to go through the map-order comparator) -- and it did not raise an error of its own
                valid2 = s_min1 > kmin2;
                if (mine && lead && (!second || valid2)) {
                    if (txi & 0x40000000u) { akey[e] = KEY_DEAD; eab[e] = 0xFFFFFFFFu; key_changed(e, kold, KEY_DEAD); }
                    else {
                        if (err) { s_cold.dc->error = err; s_err = 1; }
                        publish_edge(e, lo, hi, hprev, ku, second ? epoch + 1u : epoch, kold);
                    }
                }
            } else {
                for (uint32_t i = (uint32_t)tid >> qsh; i < nt; i += T >> qsh) {
                    const uint32_t e = tl[i], txi = tx[i];
                    const uint32_t xx = txi & 0xFFFFu;
                    const uint32_t kold = akey[e];
                    const bool lead = !quad || (lane & 3) == 0;           // the lane that keeps the edge's books
                    if (txi & 0x40000000u) { if (lead) { akey[e] = KEY_DEAD; eab[e] = 0xFFFFFFFFu; key_changed(e, kold, KEY_DEAD); } continue; }
                    const uint32_t lo = a < xx ? a : xx, hi = a < xx ? xx : a;
                    float r1[12], r2[12];          // record of the lower label first, like delta(segments.at(first), segments.at(second))
                    const int hprev = s_cold.ehist[e];          // (in flight while the weight is computed)
                    {
                        const float4* gx = i < npre ? reinterpret_cast<const float4*>(stage + (size_t)i * 12) : reinterpret_cast<const float4*>(m.rrec + (size_t)xx * 16);
                        const float4 x0 = gx[0], x1 = gx[1], x2 = gx[2];
                        const float rx[12] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w};
                        const bool a_first = a < xx;
    #pragma unroll
                        for (int k = 0; k < 12; ++k) { const float ra = s_rec[k]; r1[k] = a_first ? ra : rx[k]; r2[k] = a_first ? rx[k] : ra; }
                    }
                    int err = 0;
                    const m_lds mc = m_lds_here(s_mtab);
#ifdef F3DS_EXP_DUP_W      // timing experiment: the weight function twice (the second evaluation depends on the first: w0 - w0)
                    { const float w0 = quad ? edge_weight_quad(mp, r1, r2, lane & 3, &err, mc) : a_edge_weight(mp, r1, r2, &err, mc); r1[9] += (w0 - w0); }
#endif
                    const float w = quad ? edge_weight_quad(mp, r1, r2, lane & 3, &err, mc) : a_edge_weight(mp, r1, r2, &err, mc);
                    if (lead) {
                        if (err) { s_cold.dc->error = err; s_err = 1; }
                        publish_edge(e, lo, hi, hprev, n_weight_key(w), epoch, kold);
                    }
                }
            }
            if (tid == 0) { s_nt = 0; akey[best] = KEY_DEAD; eab[best] = 0xFFFFFFFFu; mark_dirty(best); }      // the merged edge leaves the map
            if constexpr (SPEC) {
                if (spec) {
                    if (valid2) {
                        // ---- the second merge is the next one: its books (epoch + 1), from the registers and LDS it was prepared in
                        if (wave == 2 && lane < 9) m.racc[(size_t)a2 * 12 + lane] = acc;
                        if (wave == 3 && lane < 3) m.racc[(size_t)a2 * 12 + 9 + lane] = acc;
                        if (tid == 128) {
                            for (int k = 0; k < 12; ++k) m.rrec[(size_t)a2 * 16 + k] = s_rec2[k];
                            m.rcnt[a2] = cnt_a2 + rows2;
                            x.rstart[a2] = new_start2; x.rnleaf[a2] = na2 + nb2; x.rcap[a2] = new_cap2; if (!in_place2) s_pool_end = new_start2 + new_cap2;
                            s_cold.ralive[b2] = 0; s_cold.parent[b2] = a2;
                            const uint32_t wb2 = (kmin2 & 0x80000000u) ? (kmin2 & 0x7fffffffu) : ~kmin2;
                            uint32_t* mg = s_cold.merges; mg[nmerges * 3u] = a2; mg[nmerges * 3u + 1u] = b2; mg[nmerges * 3u + 2u] = wb2;
                            akey[best2] = KEY_DEAD; eab[best2] = 0xFFFFFFFFu; mark_dirty(best2);
                            x.istart[a2] = il_new2; x.ilen[a2] = nt2; x.icap[a2] = il_newcap2; if (!il_in_place2) s_ipool_end = il_new2 + il_newcap2;
                        }
                        for (uint32_t i = tid; i < nt2; i += T) x.ilist[il_new2 + i] = tl2[i];
                        nmerges++; epoch++; sp_hit++;
    #ifdef F3DS_MERGE_PROF
                        sp_ok++;
    #endif
                    }
                    if (tid == 0) { s_nt2 = 0u; s_cross = 0u; s_min1 = KEY_DEAD; }
                } else if (tid == 0 && (s_nt2 | s_cross)) { s_nt2 = 0u; s_cross = 0u; }      // (a speculation given up after the scan)
            }
            if (SPEC && sp_try >= MC_SP_REST_TRIES) { if (sp_hit * F3DS_SP_REST_DIV < sp_try) sp_rest = MC_SP_REST_EPOCHS; sp_try = 0u; sp_hit = 0u; }
            for (uint32_t i = tid; i < 2u * MC_TL_CAP; i += T) hsh[i] = 0u;
            __syncthreads();
            TPH(4);
    #ifdef F3DS_MERGE_PROF
            sp_epochs++;
            if (tid == 0) {      // per size class: how a merge's cycles depend on the rows it folds and the edges it re-weights
                unsigned long long all_ = 0; for (int k = 0; k < 16; ++k) all_ += tph[k];
                const uint32_t rc = tph_rows - cls_prev_rows < 32 ? 0 : (tph_rows - cls_prev_rows < 256 ? 1 : (tph_rows - cls_prev_rows < 1024 ? 2 : 3));
                const uint32_t ec = nt <= 16 ? 0 : (nt <= 64 ? 1 : (nt <= 256 ? 2 : 3));
                cls_n[rc] += 1; cls_rows[rc] += tph_rows - cls_prev_rows; cls_fold[rc] += (tph[2] + tph[10] + tph[9] + tph[8]) - cls_prev_fold; cls_all[rc] += all_ - cls_prev_all;
                cle_n[ec] += 1; cle_nt[ec] += nt; cle_w[ec] += tph[4] - cls_prev_w; cle_scan[ec] += (tph[6] + tph[0]) - cls_prev_scan; cle_all[ec] += all_ - cls_prev_all;
                cls_prev_rows = tph_rows; cls_prev_fold = tph[2] + tph[10] + tph[9] + tph[8]; cls_prev_all = all_; cls_prev_w = tph[4]; cls_prev_scan = tph[6] + tph[0];
                tlast = __builtin_amdgcn_s_memtime();      // (this bookkeeping is not part of the next merge's first phase)
            }
    #endif
            if (s_err) break;        // (an LDS flag: a global read here would sit on every merge's critical path)
        }
        __syncthreads();
        if (tid == 0) { DevCounters* dcp = s_cold.dc; dcp->n_merges = nmerges; dcp->n_events = s_nevents; }
    #ifdef F3DS_MERGE_PROF
        if (tid == 0 && f3ds_frame() == 0) {
            const double nm = nmerges ? (double)nmerges : 1.0;
            { const unsigned long long loop_u1 = __builtin_amdgcn_s_memtime(), loop_w1 = __builtin_amdgcn_s_memrealtime();
              printf("  whole loop: %.0f shader clocks, %.1f per tick of the 100 MHz clock (%.2f ms)\n", (double)(loop_u1 - loop_u0), (double)(loop_u1 - loop_u0) / (double)(loop_w1 - loop_w0), (double)(loop_w1 - loop_w0) * 1e-5); }
            printf("d_merge_il<%d,%d> cycles/merge: argmin (dirty groups + group minima) %.0f [log+meta %.0f list walk %.0f pool %.0f barrier %.0f] [leaves %.0f load+dedupe+store %.0f barrier %.0f fold %.0f] record %.0f weights %.0f  (merges %u, touched/merge %.1f, rows/merge %.1f, tie slow paths %llu)\n",
                   NW, RES, (double)(tph[0] + tph[11] + tph[12] + tph[13] + tph[14] + tph[15]) / nm, (double)tph[5] / nm, (double)tph[6] / nm, (double)tph[7] / nm, (double)tph[1] / nm, (double)tph[8] / nm, (double)tph[9] / nm, (double)tph[10] / nm, (double)tph[2] / nm, (double)tph[3] / nm, (double)tph[4] / nm, nmerges, (double)tph_nt / nm, (double)tph_rows / nm, tph_slow);
            printf("  argmin phase: epoch head %.0f, dirty-group rescan %.0f (%.1f groups per epoch), barrier %.0f, wave 0: group-minima argmin + runner-up %.0f, barrier %.0f, rest %.0f\n", (double)tph[15] / nm, (double)tph[11] / nm, (double)tph_nd / (double)sp_epochs, (double)tph[12] / nm, (double)tph[13] / nm, (double)tph[14] / nm, (double)tph[0] / nm);
            printf("  record: wave 0 (centroid, normal) %.0f cycles/merge, wave 1 (Lab) %.0f\n", (double)tph_geo / nm, (double)tph_lab / nm);
            printf("  speculation: %llu epochs for %u merges; runner-up unique and below the threshold %llu, regions disjoint %llu, second merge small enough %llu, no joining edge %llu, committed %llu\n", sp_epochs, nmerges, sp_cand, sp_disjoint, sp_small, sp_scan, sp_ok);
            for (int k = 0; k < 4; ++k) printf("  rows class %d (<32, <256, <1024, more): %llu merges, %llu rows, leaves+load+fold %.0f cycles/merge = %.1f per row, whole merge %.0f\n", k, cls_n[k], cls_rows[k], cls_n[k] ? (double)cls_fold[k] / cls_n[k] : 0.0, cls_rows[k] ? (double)cls_fold[k] / cls_rows[k] : 0.0, cls_n[k] ? (double)cls_all[k] / cls_n[k] : 0.0);
            for (int k = 0; k < 4; ++k) printf("  touched class %d (<=16, <=64, <=256, more): %llu merges, %llu edges, weights %.0f cycles/merge = %.1f per edge, argmin+scan %.0f, whole merge %.0f\n", k, cle_n[k], cle_nt[k], cle_n[k] ? (double)cle_w[k] / cle_n[k] : 0.0, cle_nt[k] ? (double)cle_w[k] / cle_nt[k] : 0.0, cle_n[k] ? (double)cle_scan[k] / cle_n[k] : 0.0, cle_n[k] ? (double)cle_all[k] / cle_n[k] : 0.0);
        }
    #endif
    #undef TPH
    }
};

#ifdef F3DS_WHATIF      // (make WHATIF=1: not in the default library)
// EXPERIMENT (F3DS_FAKE_MERGE=us,waves: timing only, wrong results): a stand-in for the merge loop that holds a workgroup with the
// real kernel's LDS for `us` microseconds with `waves` of its eight waves awake and does nothing -- what a merge dispatch costs the
// OTHER calls in flight by its footprint alone, as opposed to by its work (DESIGN.md 4i).
struct d_fake_merge {
    static constexpr int BLOCK = 512;
    __device__ void operator()(MergeDev m, uint32_t us, uint32_t waves) const {
        extern __shared__ uint32_t fm_lds[];
        if (threadIdx.x == 0) { fm_lds[0] = 0u; m.dc->n_merges = 0u; m.dc->n_events = 0u; }
        if ((threadIdx.x >> 6) < waves) {
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();      // 100 MHz
            while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)us * 100ull) __builtin_amdgcn_s_sleep(64);
        }
        __syncthreads();
    }
};
#endif

// ------------------------------------------------------------------------------------------------
// stage 6: region ids and per-point labels
// ------------------------------------------------------------------------------------------------
// Clustering::get_labeled_cloud (/root/reference/src/clustering.cpp:640-663) numbers the surviving segments 0..K-1 in ascending
// key; a point's label is the number of the segment that holds the supervoxel of its voxel.  The union-find relabel of one
// frame, by ONE workgroup (every workgroup of d_relabel repeats it into its own LDS: S0 is a few thousand, the frame a million):
//   pass 1  surviving roots (ralive) in ascending label -> ids: __ballot + mbcnt inside a wave, the four wave totals through LDS,
//           a running carry across the 256-label chunks;
//   pass 2  every supervoxel walks parent[] to its root and takes the root's id.
// rank[h] = id of the region of supervoxel h (F3DS_NO_LABEL for h = 0 and never-alive helpers); `writer` also leaves root[] and
// the inclusive count incl[] (id of root r = incl[r] - 1) in global memory for the accessors and the evaluation.
__device__ inline void relabel_tables(uint32_t S0, const uint32_t* parent, const unsigned char* ralive, uint32_t* rank, bool writer,
                                      uint32_t* root_out, uint32_t* incl_out, DevCounters* dc) {
    __shared__ uint32_t rl_wtot[4];
    const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base <= S0; base += 256u) {
        const uint32_t h = base + threadIdx.x;
        const bool alive = h > 0u && h <= S0 && ralive[h] != 0;
        const uint64_t mask = __ballot(alive);
        const uint32_t within = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));      // alive lanes below this one
        if (lane == 0u) rl_wtot[w] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) { const uint32_t t = rl_wtot[k]; total += t; if (k < w) before += t; }
        const uint32_t incl = carry + before + within + (alive ? 1u : 0u);
        if (h <= S0) {
            rank[h] = alive ? incl - 1u : F3DS_NO_LABEL;
            if (writer) incl_out[h] = incl;
        }
        carry += total;
        __syncthreads();
    }
    if (writer && threadIdx.x == 0) dc->n_regions = carry;
    // (a root's entry is only read below, a non-root's only written, each by the one thread that owns it)
    for (uint32_t h = threadIdx.x; h <= S0; h += 256u) {
        uint32_t r = h;
        while (parent[r] != r) r = parent[r];
        if (writer) root_out[h] = r;
        if (r != h) rank[h] = rank[r];
    }
    __syncthreads();
}
__device__ inline void relabel_points(uint32_t n, const int* pt_voxel, const uint32_t* owner, const uint32_t* rank, uint32_t* labels) {
    for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int v = pt_voxel[i];
        const uint32_t o = owner[v >= 0 ? v : 0];          // (unconditional: the two gathers are in flight together with the next point's)
        labels[i] = (v >= 0 && o) ? rank[o] : F3DS_NO_LABEL;
    }
}
// stage 6 as one kernel: the rank table in LDS ((S0 + 1) words of dynamic LDS), then the grid-stride label write
constexpr uint32_t RL_LDS_CAP = 12288;       // labels 0..S0 that fit the LDS table (48 KB); larger frames take d_region_ids + d_point_labels
struct d_relabel {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, const int* pt_voxel, const uint32_t* owner, uint32_t S0, const uint32_t* parent, const unsigned char* ralive,
                               uint32_t* root_out, uint32_t* incl_out, uint32_t* labels, DevCounters* dc) const {
        extern __shared__ uint32_t rl_rank[];
        if (BIX > 0 && BIX * blockDim.x >= n) return;
        relabel_tables(S0, parent, ralive, rl_rank, BIX == 0, root_out, incl_out, dc);
        relabel_points(n, pt_voxel, owner, rl_rank, labels);
    }
};
// the same as two kernels for frames with more supervoxels than the LDS table holds: the rank table in global memory
struct d_region_ids {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t S0, const uint32_t* parent, const unsigned char* ralive, uint32_t* rank, uint32_t* root_out, uint32_t* incl_out, DevCounters* dc) const {
        if (BIX) return;
        relabel_tables(S0, parent, ralive, rank, true, root_out, incl_out, dc);
    }
};
struct d_point_labels {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, const int* pt_voxel, const uint32_t* owner, const uint32_t* rank, uint32_t* labels) const {
        relabel_points(n, pt_voxel, owner, rank, labels);
    }
};

// ---- ground-truth evaluation (reference main():387-400 and Testing, src/testing.cpp) ----------
// voxel colour sums of the label-coloured truth cloud; the sums are integers < 2^24, so the
// float accumulation of the reference's leaf is order-free and exact
struct d_truth_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, const int* pt_voxel, const uint32_t* truth, const uint32_t* lut, uint32_t* tsum) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const int v = pt_voxel[i];
            if (v < 0) continue;
            const uint32_t c = lut[truth[i] & 255u];
            atomicAdd(&tsum[(size_t)v * 3], (c >> 16) & 255u); atomicAdd(&tsum[(size_t)v * 3 + 1], (c >> 8) & 255u); atomicAdd(&tsum[(size_t)v * 3 + 2], c & 255u);
        }
    }
};
struct d_truth_color {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t V, const uint32_t* tsum, const uint32_t* vcount, uint32_t* tcol) const {
        for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
            const float c = (float)vcount[v];
            tcol[v] = (uint32_t)((float)tsum[(size_t)v * 3] / c) << 16 | (uint32_t)((float)tsum[(size_t)v * 3 + 1] / c) << 8 | (uint32_t)((float)tsum[(size_t)v * 3 + 2] / c);
        }
    }
};
// contingency table of (segment, truth label) over the voxels each segment holds
struct d_contingency {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t V, uint32_t M, const uint32_t* owner, const uint32_t* root, const uint32_t* incl, const uint32_t* tlab,
                               uint32_t* table, uint32_t* ssize) const {
        for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
            const uint32_t o = owner[v];
            if (!o) continue;
            const uint32_t i = incl[root[o]] - 1u;
            atomicAdd(&table[(size_t)i * M + tlab[v]], 1u);
            atomicAdd(&ssize[i], 1u);
        }
    }
};
// a ghost leaf puts its voxel into a second segment's cloud; it adds to the intersection only the
// first time that voxel shows up in that segment (set_intersection pairs equal points one to one)
struct d_contingency_ghost {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t S0, uint32_t M, const int* ghost_vox, const unsigned char* ghost_active, const uint32_t* owner,
                               const uint32_t* root, const uint32_t* incl, const uint32_t* tlab, uint32_t* table, uint32_t* ssize) const {
        for (uint32_t h = 1 + BIX * blockDim.x + threadIdx.x; h <= S0; h += gridDim.x * blockDim.x) {
            if (!ghost_active[h]) continue;
            const uint32_t v = (uint32_t)ghost_vox[h], r = root[h], i = incl[r] - 1u;
            atomicAdd(&ssize[i], 1u);
            bool seen = owner[v] && root[owner[v]] == r;
            for (uint32_t g = 1; g < h && !seen; ++g) seen = ghost_active[g] && (uint32_t)ghost_vox[g] == v && root[g] == r;
            if (!seen) atomicAdd(&table[(size_t)i * M + tlab[v]], 1u);
        }
    }
};
struct d_fill_u32 {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* p, uint32_t value, uint32_t count) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) p[i] = value;
    }
};
struct d_copy_u32 {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* dst, const uint32_t* src, uint32_t count) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) dst[i] = src[i];
    }
};
// Up to eight fills / copies of one frame as ONE dispatch: the host merges the rec_fill / rec_copy calls that follow each other (a stage starts with a run of them:
// the sweeps with eight, the cluster stage with six copies).  With other calls on the chip every dispatch of a call costs ~80 us of queue latency whatever it does.
// (The loop over the entries is unrolled: a by-value argument struct indexed with a runtime index would live in scratch memory.)
constexpr int MULTI_OPS = 8;
struct MultiOp { uint32_t* dst[MULTI_OPS]; const uint32_t* src[MULTI_OPS]; uint32_t val[MULTI_OPS]; uint32_t words[MULTI_OPS]; uint32_t n; uint32_t pad_; };
struct d_multi_op {
    static constexpr int BLOCK = 256;
    __device__ void operator()(MultiOp m) const {
        const uint32_t i0 = BIX * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
#pragma unroll
        for (int k = 0; k < MULTI_OPS; ++k) {
            if ((uint32_t)k >= m.n) break;
            uint32_t* d = m.dst[k]; const uint32_t* sp = m.src[k]; const uint32_t v = m.val[k], w = m.words[k];
            if (sp) { for (uint32_t i = i0; i < w; i += step) d[i] = sp[i]; }
            else { for (uint32_t i = i0; i < w; i += step) d[i] = v; }
        }
    }
};
// one frame's counters into the batch's contiguous block (a single device-to-host copy then serves the whole batch)
struct d_dc_gather {
    static constexpr int BLOCK = 64;
    __device__ void operator()(const DevCounters* dc, DevCounters* slot) const {
        if (BIX) return;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(dc);
        uint32_t* dst = reinterpret_cast<uint32_t*>(slot);
        for (uint32_t i = threadIdx.x; i < sizeof(DevCounters) / 4u; i += 64u) dst[i] = src[i];
    }
};
struct d_init_counters {
    static constexpr int BLOCK = 64;
    __device__ void operator()(DevCounters* dc) const {
        if (threadIdx.x || BIX) return;
        DevCounters z;
        memset(&z, 0, sizeof z);
        z.bbox[0] = z.bbox[1] = z.bbox[2] = 0xFFFFFFFFu;
        *dc = z;
    }
};

}  // namespace
