// f3ds_regions.inc -- the device path of the region table (f3ds_region_table, include/f3ds.h; the rules are in f3ds_regions.h; DESIGN.md section 18).
// Included by f3ds_hip.hip after f3ds_track.inc.
//
//   d_region_init     the n_regions accumulators (RgAcc, 24 words) get their empty values, the head its zeros
//   d_region_accum    ONE read of the images.  A workgroup takes a CONTIGUOUS span of pixels (a label image is spatially coherent: a span meets a handful of
//                     regions, an interleaved grid-stride assignment would meet all of them) and adds its pixels into an LDS table keyed by label; at the end of
//                     the span the occupied slots go to the global accumulators, one integer atomic per field and (workgroup, label).  No global atomic per
//                     pixel: a million atomic adds onto forty words took 8 ms in the tracker (DESIGN.md section 17).
//   d_region_finish   the sets of accumulators merged (rgt_copies), rg_finish per region into the caller's rows (or the staging of a host caller), n_nonempty into the head; nothing but the head when a
//                     label was out of range
// Every field is a count, a minimum, a maximum or an integer sum (f3ds_regions.h): arrival order does not matter, so integer atomics in LDS and in global
// memory give the bits of the host function.  No float atomics.

struct RegionArgs {
    uint32_t width, n;                 // n = width * height
    uint32_t depth_pitch, color_pitch; // bytes per row (never 0 here)
    int depth_f32, color_format;       // F3DS_COLOR_*, or -1: no colour image
    uint32_t K;                        // regions
    uint32_t copies;                   // accumulator sets (rgt_copies): workgroup b adds into set b % copies
    float depth_scale, fx, fy, cx, cy;
};
constexpr uint32_t RGT_HEAD = 8;       // words of the head: [0] non-empty regions, [1] 1 if a label was >= K, [2..3] labelled pixels (u64), [4..5] clamped pixels (u64), [6] [7] spare
constexpr int RGT_SLOT_BITS = 7, RGT_SLOTS = 1 << RGT_SLOT_BITS;      // LDS table: 128 slots of a label + an RgAcc (100 B), 12.5 KiB
constexpr int RGT_PROBES = 8;          // a label that finds neither its slot nor a free one in this many steps goes straight to the global accumulator
constexpr uint32_t RGT_TRIPS = 4;      // trips of a workgroup the grid is sized for: fewer, longer spans mean fewer flushes onto the same global words
// Atomics onto one cache line go through one at a time, some 20 ns each (a million onto forty words: 8 ms, DESIGN.md section 17; d_bbox measured 13 ns), and with
// a few regions every workgroup's flush meets the same two lines: a thousand workgroups x 18 fields onto the largest region of a 1M-pixel frame took 230 us.  So
// a frame with few regions gets several sets of accumulators -- workgroup b adds into set b % copies, d_region_finish merges the sets (rg_merge: exact) -- up to 32
// sets and 2048 accumulators in all; a frame with thousands of regions spreads its flushes by itself and keeps one set.
constexpr uint32_t RGT_MAX_COPIES = 32, RGT_COPY_BUDGET = 2048;
inline uint32_t rgt_copies(uint32_t K) { const uint32_t c = RGT_COPY_BUDGET / (K ? K : 1u); return c < 1u ? 1u : (c > RGT_MAX_COPIES ? RGT_MAX_COPIES : c); }

typedef unsigned long long rg_u64;

struct d_region_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* acc_words, uint32_t n_acc, uint32_t* head) const {      // n_acc = regions x copies
        const size_t words = (size_t)n_acc * RG_WORDS;
        for (size_t w = (size_t)BIX * blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) acc_words[w] = rg_empty_word((uint32_t)(w % RG_WORDS));
        if (BIX == 0u && threadIdx.x < RGT_HEAD) head[threadIdx.x] = 0u;
    }
};

// wave-wide reductions with DPP lane swizzles, as wave_min_u32 (f3ds_kernels.inc): lane 63 holds the result after the two row broadcasts (other lanes may not)
template <class Op> __device__ __forceinline__ uint32_t rg_wave_u32(uint32_t v, Op op) {
#define F3DS_RG_DPP(ctrl, rmask) { const uint32_t t_ = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rmask, 0xF, false); v = op(t_, v); }
    F3DS_RG_DPP(0xB1, 0xF) F3DS_RG_DPP(0x4E, 0xF) F3DS_RG_DPP(0x141, 0xF) F3DS_RG_DPP(0x140, 0xF) F3DS_RG_DPP(0x142, 0xA) F3DS_RG_DPP(0x143, 0xC)
#undef F3DS_RG_DPP
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint64_t rg_wave_add_u64(uint64_t v) {
#define F3DS_RG_DPP(ctrl, rmask) { const uint32_t lo_ = (uint32_t)v, hi_ = (uint32_t)(v >> 32); \
      const uint32_t tl_ = (uint32_t)__builtin_amdgcn_update_dpp((int)lo_, (int)lo_, ctrl, rmask, 0xF, false), th_ = (uint32_t)__builtin_amdgcn_update_dpp((int)hi_, (int)hi_, ctrl, rmask, 0xF, false); \
      v += ((uint64_t)th_ << 32) | tl_; }
    F3DS_RG_DPP(0xB1, 0xF) F3DS_RG_DPP(0x4E, 0xF) F3DS_RG_DPP(0x141, 0xF) F3DS_RG_DPP(0x140, 0xF) F3DS_RG_DPP(0x142, 0xA) F3DS_RG_DPP(0x143, 0xC)
#undef F3DS_RG_DPP
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((uint64_t)hi << 32) | lo;
}
struct RgMin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
struct RgMax { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct RgAdd { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };

// the LDS table of a workgroup: field-major, so the lanes of a wave that update different slots touch different banks
struct RgTable { uint32_t key[RGT_SLOTS]; uint32_t w[RG_W][RGT_SLOTS]; rg_u64 s[RG_S][RGT_SLOTS]; };

// the slot of label l, claimed on the way if it is new; -1: none within RGT_PROBES steps.  Slots are never given back within a span, so every lane that asks
// for l walks the same occupied slots and ends at the same one.
__device__ __forceinline__ int rg_slot(RgTable& t, uint32_t l) {
    uint32_t h = (l * 0x9E3779B1u) >> (32 - RGT_SLOT_BITS);
    for (int k = 0; k < RGT_PROBES; ++k) {
        const uint32_t old = atomicCAS(&t.key[h], RG_NONE, l);
        if (old == RG_NONE || old == l) return (int)h;
        h = (h + 1u) & (uint32_t)(RGT_SLOTS - 1);
    }
    return -1;
}
__device__ __forceinline__ void rg_lds_add(RgTable& t, int slot, const RgAcc& a) {
    atomicAdd(&t.w[0][slot], a.w[0]);
#pragma unroll
    for (int k = 1; k < 4; ++k) atomicMin(&t.w[k][slot], a.w[k]);
    atomicMax(&t.w[4][slot], a.w[4]); atomicMax(&t.w[5][slot], a.w[5]);
#pragma unroll
    for (int k = 6; k < 9; ++k) atomicMin(&t.w[k][slot], a.w[k]);
#pragma unroll
    for (int k = 9; k < 12; ++k) atomicMax(&t.w[k][slot], a.w[k]);
#pragma unroll
    for (int k = 0; k < RG_S; ++k) atomicAdd(&t.s[k][slot], (rg_u64)a.s[k]);
}
// a into the global accumulator of its region.  A minimum or maximum that the word already meets is not sent: the word only ever moves one way, so a value
// that does not improve on what a plain load sees (stale or not) cannot improve on what is there now.
__device__ __forceinline__ void rg_global_add(RgAcc* dst, const RgAcc& a) {
    atomicAdd(&dst->w[0], a.w[0]);
#pragma unroll
    for (int k = 1; k < 4; ++k) if (a.w[k] < __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMin(&dst->w[k], a.w[k]);
#pragma unroll
    for (int k = 4; k < 6; ++k) if (a.w[k] > __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMax(&dst->w[k], a.w[k]);
#pragma unroll
    for (int k = 6; k < 9; ++k) if (a.w[k] < __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMin(&dst->w[k], a.w[k]);
#pragma unroll
    for (int k = 9; k < 12; ++k) if (a.w[k] > __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMax(&dst->w[k], a.w[k]);
#pragma unroll
    for (int k = 0; k < RG_S; ++k) if (a.s[k]) atomicAdd(reinterpret_cast<rg_u64*>(&dst->s[k]), (rg_u64)a.s[k]);
}

// COLOR: -1 none, else F3DS_COLOR_*.  Span of workgroup b: [b * span, min(n, (b + 1) * span)), span = ceil(n / gridDim.x) rounded up to a multiple of the block:
// every lane of the workgroup makes the same number of trips (the ballots and barriers below are uniform), a lane past the end contributes nothing.
template <bool DEPTH_F32, int COLOR>
__device__ __forceinline__ void region_accum_span(const unsigned char* depth, const unsigned char* color, const uint32_t* label, const RegionArgs& a, RgAcc* acc, uint32_t* head,
                                         RgTable& tab, rg_u64* s_count) {
    acc += (size_t)(BIX % a.copies) * a.K;      // this workgroup's set of accumulators
    for (uint32_t k = threadIdx.x; k < (uint32_t)RGT_SLOTS; k += blockDim.x) {
        tab.key[k] = RG_NONE;
#pragma unroll
        for (int f = 0; f < RG_W; ++f) tab.w[f][k] = rg_empty_word((uint32_t)f);
#pragma unroll
        for (int f = 0; f < RG_S; ++f) tab.s[f][k] = 0ull;
    }
    if (threadIdx.x < 2u) s_count[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t per = ((uint64_t)a.n + gridDim.x - 1u) / gridDim.x;
    const uint64_t span = (per + blockDim.x - 1u) / blockDim.x * blockDim.x;
    const uint64_t begin64 = (uint64_t)BIX * span;
    const uint32_t begin = begin64 < a.n ? (uint32_t)begin64 : a.n, end = begin64 + span < a.n ? (uint32_t)(begin64 + span) : a.n;
    const uint32_t sv = blockDim.x / a.width, su = blockDim.x - sv * a.width;      // a trip moves every lane this many rows and columns on (as d_deproject)
    uint32_t i = begin + threadIdx.x;
    uint32_t v = i / a.width, u = i - v * a.width;
    uint32_t my_labelled = 0u, my_clamped = 0u;
    bool bad = false;
    for (uint32_t base = begin; base < end; base += blockDim.x, i += blockDim.x) {
        const bool active = i < end;
        uint32_t l = RG_NONE, rgba = 0u;
        float z = 0.0f;
        bool valid = false;
        if (active) {
            const unsigned char* drow = depth + (size_t)v * a.depth_pitch;
            if constexpr (DEPTH_F32) valid = n_depth_to_z(reinterpret_cast<const float*>(drow)[u], a.depth_scale, z);
            else valid = n_depth_to_z(reinterpret_cast<const uint16_t*>(drow)[u], a.depth_scale, z);
            l = label[i];
            if constexpr (COLOR == 0) { const unsigned char* p = color + (size_t)v * a.color_pitch + 3u * (size_t)u; rgba = n_color_word(p[0], p[1], p[2], 255u); }
            else if constexpr (COLOR > 0) {
                const uint32_t w = load_unaligned<uint32_t>(color + (size_t)v * a.color_pitch + 4u * (size_t)u);
                rgba = COLOR == 1 ? n_color_word(w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, 255u) : w;
            }
        }
        bad = bad || (l != RG_NONE && l >= a.K);
        const bool labelled = valid && l < a.K;      // (K <= RG_MAX_REGIONS: RG_NONE is never below it)
        RgAcc one;
        rg_empty(one);
        if (labelled) {
            float x, y, zo;
            n_deproject(u, v, true, z, a.fx, a.fy, a.cx, a.cy, x, y, zo);
            if (rg_pixel(i, u, v, x, y, zo, rgba, one)) ++my_clamped;
            ++my_labelled;
        }
        // one label in the wave (the usual case inside a region): reduce across the wave -- the lanes without a labelled pixel hold the empty values -- and lane 0
        // sends the sum; otherwise every labelled lane sends its own pixel
        const uint64_t m = __ballot(labelled);
        uint32_t target = l;
        bool send = labelled;
        if (m) {      // (wave-uniform, and so is the next one)
            const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)l, (int)__builtin_ctzll(m));
            if (__ballot(labelled && l != l0) == 0ull) {
                one.w[0] = rg_wave_u32(one.w[0], RgAdd{});
#pragma unroll
                for (int k = 1; k < 4; ++k) one.w[k] = rg_wave_u32(one.w[k], RgMin{});
                one.w[4] = rg_wave_u32(one.w[4], RgMax{}); one.w[5] = rg_wave_u32(one.w[5], RgMax{});
#pragma unroll
                for (int k = 6; k < 9; ++k) one.w[k] = rg_wave_u32(one.w[k], RgMin{});
#pragma unroll
                for (int k = 9; k < 12; ++k) one.w[k] = rg_wave_u32(one.w[k], RgMax{});
#pragma unroll
                for (int k = 0; k < 3; ++k) one.s[k] = rg_wave_add_u64(one.s[k]);
#pragma unroll
                for (int k = 3; k < 6; ++k) one.s[k] = COLOR < 0 ? 0ull : (uint64_t)rg_wave_u32((uint32_t)one.s[k], RgAdd{});      // (64 bytes add up inside 32 bits)
                target = l0; send = lane_id() == 0;
            }
        }
        if (send) {
            const int slot = rg_slot(tab, target);
            if (slot >= 0) rg_lds_add(tab, slot, one); else rg_global_add(acc + target, one);
        }
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
    const uint32_t wl = rg_wave_u32(my_labelled, RgAdd{}), wc = rg_wave_u32(my_clamped, RgAdd{});
    if (lane_id() == 0) { if (wl) atomicAdd(&s_count[0], (rg_u64)wl); if (wc) atomicAdd(&s_count[1], (rg_u64)wc); }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)RGT_SLOTS; k += blockDim.x) {
        const uint32_t l = tab.key[k];
        if (l == RG_NONE) continue;
        RgAcc t;
#pragma unroll
        for (int f = 0; f < RG_W; ++f) t.w[f] = tab.w[f][k];
#pragma unroll
        for (int f = 0; f < RG_S; ++f) t.s[f] = tab.s[f][k];
        rg_global_add(acc + l, t);      // (l < K: only checked labels get a slot)
    }
    if (threadIdx.x == 0u) {
        if (s_count[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 2), s_count[0]);
        if (s_count[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_count[1]);
    }
}
struct d_region_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const unsigned char* color, const uint32_t* label, RegionArgs a, RgAcc* acc, uint32_t* head) const {
        __shared__ RgTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ rg_u64 s_count[2];
        if (a.depth_f32) {
            if (a.color_format < 0) region_accum_span<true, -1>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 0) region_accum_span<true, 0>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 1) region_accum_span<true, 1>(depth, color, label, a, acc, head, tab, s_count);
            else region_accum_span<true, 2>(depth, color, label, a, acc, head, tab, s_count);
        } else {
            if (a.color_format < 0) region_accum_span<false, -1>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 0) region_accum_span<false, 0>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 1) region_accum_span<false, 1>(depth, color, label, a, acc, head, tab, s_count);
            else region_accum_span<false, 2>(depth, color, label, a, acc, head, tab, s_count);
        }
    }
};

struct d_region_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const RgAcc* acc, uint32_t K, uint32_t copies, uint32_t* head, f3ds_region_row* rows) const {
        if (head[1]) return;      // a label was out of range: the rows stay as they are
        uint32_t nonempty = 0u;
        for (uint32_t r = BIX * blockDim.x + threadIdx.x; r < K; r += gridDim.x * blockDim.x) {
            RgAcc a = acc[r];
            for (uint32_t c = 1; c < copies; ++c) rg_merge(a, acc[(size_t)c * K + r]);
            rg_finish(a, &rows[r]);
            nonempty += a.w[0] ? 1u : 0u;
        }
        const uint32_t wn = rg_wave_u32(nonempty, RgAdd{});
        if (lane_id() == 0 && wn) atomicAdd(&head[0], wn);
    }
};
