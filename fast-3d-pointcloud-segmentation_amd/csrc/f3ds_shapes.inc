// f3ds_shapes.inc -- the device path of the region shapes (f3ds_region_shapes, include/f3ds.h; the rules are in f3ds_shapes.h; DESIGN.md section 20).
// Included by f3ds_hip.hip after f3ds_contacts.inc.  The structure is d_region_accum's (f3ds_regions.inc), whose helpers it uses.
//
//   d_shape_init     the accumulators (ShAcc, 32 words) and the head get their zeros
//   d_shape_accum    ONE read of the depth image and the labels.  A workgroup takes a CONTIGUOUS span of pixels and adds its pixels into an LDS table keyed by
//                    label; at the end of the span the occupied slots go to the global accumulators, one 64-bit integer atomic per non-zero field and
//                    (workgroup, label).  No global atomic per pixel.
//   d_shape_finish   the sets of accumulators merged (rgt_copies), sh_finish per region into the caller's rows (or the staging of a host caller), n_nonempty
//                    into the head; nothing but the head when a label was out of range
// Every field is a count or a sum of 64-bit integers (f3ds_shapes.h: the 93-bit second moments as two half-sums each): arrival order does not matter, so
// integer atomics in LDS (ds_add_u64) and in global memory give the bits of the host function.  No float atomics.

struct ShapeArgs {
    uint32_t width, n;                 // n = width * height
    uint32_t depth_pitch;              // bytes per row (never 0 here)
    int depth_f32;
    uint32_t K;                        // regions
    uint32_t copies;                   // accumulator sets (rgt_copies): workgroup b adds into set b % copies
    float depth_scale, fx, fy, cx, cy;
};
constexpr uint32_t RGS_HEAD = 8;       // words of the head, as RGT_HEAD: [0] non-empty regions, [1] 1 if a label was >= K, [2..3] labelled pixels (u64), [4..5] clamped pixels (u64), [6] [7] spare
constexpr int RGS_SLOT_BITS = 7, RGS_SLOTS = 1 << RGS_SLOT_BITS;      // LDS table: 128 slots of a label, a count and fifteen sums (128 B), 16 KiB
constexpr int RGS_PROBES = 8;          // a label that finds neither its slot nor a free one in this many steps goes straight to the global accumulator
constexpr uint32_t RGS_TRIPS = 4;      // trips of a workgroup the grid is sized for, as RGT_TRIPS

struct d_shape_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* acc_words, uint32_t n_acc, uint32_t* head) const {      // n_acc = regions x copies
        const size_t words = (size_t)n_acc * SH_WORDS;
        for (size_t w = (size_t)BIX * blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) acc_words[w] = 0u;
        if (BIX == 0u && threadIdx.x < RGS_HEAD) head[threadIdx.x] = 0u;
    }
};

// the LDS table of a workgroup: field-major, so the lanes of a wave that update different slots touch different banks
struct ShTable { uint32_t key[RGS_SLOTS]; uint32_t n[RGS_SLOTS]; rg_u64 s[SH_S][RGS_SLOTS]; };

// the slot of label l, claimed on the way if it is new; -1: none within RGS_PROBES steps (as rg_slot)
__device__ __forceinline__ int sh_slot(ShTable& t, uint32_t l) {
    uint32_t h = (l * 0x9E3779B1u) >> (32 - RGS_SLOT_BITS);
    for (int k = 0; k < RGS_PROBES; ++k) {
        const uint32_t old = atomicCAS(&t.key[h], RG_NONE, l);
        if (old == RG_NONE || old == l) return (int)h;
        h = (h + 1u) & (uint32_t)(RGS_SLOTS - 1);
    }
    return -1;
}
__device__ __forceinline__ void sh_lds_add(ShTable& t, int slot, const ShAcc& a) {
    atomicAdd(&t.n[slot], a.n);
#pragma unroll
    for (int k = 0; k < SH_S; ++k) atomicAdd(&t.s[k][slot], (rg_u64)a.s[k]);
}
// a into the global accumulator of its region; a sum that is zero is not sent
__device__ __forceinline__ void sh_global_add(ShAcc* dst, const ShAcc& a) {
    atomicAdd(&dst->n, a.n);
#pragma unroll
    for (int k = 0; k < SH_S; ++k) if (a.s[k]) atomicAdd(reinterpret_cast<rg_u64*>(&dst->s[k]), (rg_u64)a.s[k]);
}

// Span of workgroup b: [b * span, min(n, (b + 1) * span)), span = ceil(n / gridDim.x) rounded up to a multiple of the block: every lane of the workgroup makes
// the same number of trips (the ballots and barriers below are uniform), a lane past the end contributes nothing.  (As region_accum_span.)
template <bool DEPTH_F32>
__device__ __forceinline__ void shape_accum_span(const unsigned char* depth, const uint32_t* label, const ShapeArgs& a, ShAcc* acc, uint32_t* head, ShTable& tab, rg_u64* s_count) {
    acc += (size_t)(BIX % a.copies) * a.K;      // this workgroup's set of accumulators
    for (uint32_t k = threadIdx.x; k < (uint32_t)RGS_SLOTS; k += blockDim.x) {
        tab.key[k] = RG_NONE; tab.n[k] = 0u;
#pragma unroll
        for (int f = 0; f < SH_S; ++f) tab.s[f][k] = 0ull;
    }
    if (threadIdx.x < 2u) s_count[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t per = ((uint64_t)a.n + gridDim.x - 1u) / gridDim.x;
    const uint64_t span = (per + blockDim.x - 1u) / blockDim.x * blockDim.x;
    const uint64_t begin64 = (uint64_t)BIX * span;
    const uint32_t begin = begin64 < a.n ? (uint32_t)begin64 : a.n, end = begin64 + span < a.n ? (uint32_t)(begin64 + span) : a.n;
    const uint32_t sv = blockDim.x / a.width, su = blockDim.x - sv * a.width;      // a trip moves every lane this many rows and columns on
    uint32_t i = begin + threadIdx.x;
    uint32_t v = i / a.width, u = i - v * a.width;
    uint32_t my_labelled = 0u, my_clamped = 0u;
    bool bad = false;
    for (uint32_t base = begin; base < end; base += blockDim.x, i += blockDim.x) {
        const bool active = i < end;
        uint32_t l = RG_NONE;
        float z = 0.0f;
        bool valid = false;
        if (active) {
            const unsigned char* drow = depth + (size_t)v * a.depth_pitch;
            if constexpr (DEPTH_F32) valid = n_depth_to_z(reinterpret_cast<const float*>(drow)[u], a.depth_scale, z);
            else valid = n_depth_to_z(reinterpret_cast<const uint16_t*>(drow)[u], a.depth_scale, z);
            l = label[i];
        }
        bad = bad || (l != RG_NONE && l >= a.K);
        const bool labelled = valid && l < a.K;      // (K <= RG_MAX_REGIONS: RG_NONE is never below it)
        ShAcc one;
        sh_empty(one);
        if (labelled) {
            float x, y, zo;
            n_deproject(u, v, true, z, a.fx, a.fy, a.cx, a.cy, x, y, zo);
            if (sh_pixel(x, y, zo, one)) ++my_clamped;
            ++my_labelled;
        }
        // one label in the wave (the usual case inside a region): reduce across the wave -- the lanes without a labelled pixel hold zeros -- and lane 0 sends the
        // sums; otherwise every labelled lane sends its own pixel
        const uint64_t m = __ballot(labelled);
        uint32_t target = l;
        bool send = labelled;
        if (m) {      // (wave-uniform, and so is the next one)
            const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)l, (int)__builtin_ctzll(m));
            if (__ballot(labelled && l != l0) == 0ull) {
                one.n = (uint32_t)__popcll(m);
#pragma unroll
                for (int k = 0; k < SH_S; ++k) one.s[k] = rg_wave_add_u64(one.s[k]);
                target = l0; send = lane_id() == 0;
            }
        }
        if (send) {
            const int slot = sh_slot(tab, target);
            if (slot >= 0) sh_lds_add(tab, slot, one); else sh_global_add(acc + target, one);
        }
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
    const uint32_t wl = rg_wave_u32(my_labelled, RgAdd{}), wc = rg_wave_u32(my_clamped, RgAdd{});
    if (lane_id() == 0) { if (wl) atomicAdd(&s_count[0], (rg_u64)wl); if (wc) atomicAdd(&s_count[1], (rg_u64)wc); }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)RGS_SLOTS; k += blockDim.x) {
        const uint32_t l = tab.key[k];
        if (l == RG_NONE) continue;
        ShAcc t;
        t.n = tab.n[k]; t.pad = 0u;
#pragma unroll
        for (int f = 0; f < SH_S; ++f) t.s[f] = tab.s[f][k];
        sh_global_add(acc + l, t);      // (l < K: only checked labels get a slot)
    }
    if (threadIdx.x == 0u) {
        if (s_count[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 2), s_count[0]);
        if (s_count[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_count[1]);
    }
}
struct d_shape_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, ShapeArgs a, ShAcc* acc, uint32_t* head) const {
        __shared__ ShTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ rg_u64 s_count[2];
        if (a.depth_f32) shape_accum_span<true>(depth, label, a, acc, head, tab, s_count);
        else shape_accum_span<false>(depth, label, a, acc, head, tab, s_count);
    }
};

struct d_shape_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const ShAcc* acc, uint32_t K, uint32_t copies, uint32_t* head, f3ds_region_shape* rows) const {
        if (head[1]) return;      // a label was out of range: the rows stay as they are
        uint32_t nonempty = 0u;
        for (uint32_t r = BIX * blockDim.x + threadIdx.x; r < K; r += gridDim.x * blockDim.x) {
            ShAcc a = acc[r];
            for (uint32_t c = 1; c < copies; ++c) sh_merge(a, acc[(size_t)c * K + r]);
            sh_finish(a, &rows[r]);
            nonempty += a.n ? 1u : 0u;
        }
        const uint32_t wn = rg_wave_u32(nonempty, RgAdd{});
        if (lane_id() == 0 && wn) atomicAdd(&head[0], wn);
    }
};
