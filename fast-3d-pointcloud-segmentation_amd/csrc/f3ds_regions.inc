// f3ds_regions.inc -- the device path of the region table (f3ds_region_table, include/f3ds.h; the rules are in f3ds_regions.h; DESIGN.md section 18), and in
// front of it the accumulate skeleton that the table and the region shapes (f3ds_shapes.inc) share (DESIGN.md "the label-image frame").
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

// ------------------------------------------------------------------------------------------------
// The skeleton: three kernel bodies over a RULE, a struct that says what an accumulator is (RegionRule below, ShapeRule in f3ds_shapes.inc):
//   Acc, Row, Args   the accumulator of a region, the row it becomes, the kernel's arguments (width, n, depth_pitch, K, copies, depth_scale, fx, fy, cx, cy)
//   Table            the LDS table of a workgroup: uint32_t key[LI_SLOTS] and the accumulators' fields, field-major, so the lanes of a wave that update
//                    different slots touch different banks
//   WORDS, empty_word(k), empty(acc), table_reset(tab, slot)      the size of an accumulator and its empty values, in global memory, in registers and in LDS
//   aux(u, v), pixel(i, u, v, x, y, z, aux, l, one_label, acc)    what a pixel needs besides its depth (loaded before the depth is known to be valid), and what a
//                                                                 labelled pixel adds to its region (returns: clamped?).  l: the pixel's label, for a rule that
//                                                                 keeps something per region to measure the pixel with (BoxRule: the region's frame); one_label
//                                                                 (wave-uniform): every labelled lane of the wave holds this l, and l is then passed as
//                                                                 one value for the whole wave.  The table and the shapes ignore both.
//   wave_reduce(acc, m)                                           the accumulators of a wave into one, m = the ballot of its labelled lanes
//   lds_add, table_get, global_add                                an accumulator into a slot, out of a slot, into the region's global accumulator
//   merge, finish(acc, r, row), nonempty                          the rules' own (rg_merge / rg_finish, sh_merge / sh_finish, bx_merge / bx_finish); r: the region
//   TALLY, tally(acc)                                             TALLY: the finish kernel adds the sum of tally(acc) over the regions into words 6 ... 7 of the head
// The head of the calls: [0] non-empty regions, [1] 1 if a label was >= K, [2..3] labelled pixels (u64), [4..5] clamped pixels (u64), [6..7] the rule's tally
// (u64; spare without one).
// ------------------------------------------------------------------------------------------------
constexpr int LI_SLOT_BITS = 7, LI_SLOTS = 1 << LI_SLOT_BITS;      // LDS table: 128 slots of a label + an accumulator (RgAcc: 100 B a slot, 12.5 KiB; ShAcc: 128 B, 16 KiB)
constexpr int LI_PROBES = 8;           // a label that finds neither its slot nor a free one in this many steps goes straight to the global accumulator
constexpr uint32_t LI_TRIPS = 4;       // trips of a workgroup the grid is sized for: fewer, longer spans mean fewer flushes onto the same global words
// Atomics onto one cache line go through one at a time, some 20 ns each (a million onto forty words: 8 ms, DESIGN.md section 17; d_bbox measured 13 ns), and with
// a few regions every workgroup's flush meets the same two lines: a thousand workgroups x 18 fields onto the largest region of a 1M-pixel frame took 230 us.  So
// a frame with few regions gets several sets of accumulators -- workgroup b adds into set b % copies, the finish kernel merges the sets (exact) -- up to 32
// sets and 2048 accumulators in all; a frame with thousands of regions spreads its flushes by itself and keeps one set.
constexpr uint32_t RGT_MAX_COPIES = 32, RGT_COPY_BUDGET = 2048;
inline uint32_t rgt_copies(uint32_t K) { const uint32_t c = RGT_COPY_BUDGET / (K ? K : 1u); return c < 1u ? 1u : (c > RGT_MAX_COPIES ? RGT_MAX_COPIES : c); }

typedef unsigned long long rg_u64;

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

// the slot of label l, claimed on the way if it is new; -1: none within LI_PROBES steps.  Slots are never given back within a span, so every lane that asks
// for l walks the same occupied slots and ends at the same one.
__device__ __forceinline__ int li_slot(uint32_t* key, uint32_t l) {
    uint32_t h = (l * 0x9E3779B1u) >> (32 - LI_SLOT_BITS);
    for (int k = 0; k < LI_PROBES; ++k) {
        const uint32_t old = atomicCAS(&key[h], LI_NONE, l);
        if (old == LI_NONE || old == l) return (int)h;
        h = (h + 1u) & (uint32_t)(LI_SLOTS - 1);
    }
    return -1;
}

template <class Rule>
__device__ __forceinline__ void label_init(uint32_t* acc_words, uint32_t n_acc, uint32_t* head) {      // n_acc = regions x copies
    const size_t words = (size_t)n_acc * Rule::WORDS;
    for (size_t w = (size_t)BIX * blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) acc_words[w] = Rule::empty_word((uint32_t)(w % Rule::WORDS));
    if (BIX == 0u && threadIdx.x < LI_HEAD_WORDS) head[threadIdx.x] = 0u;
}

// Span of workgroup b: [b * span, min(n, (b + 1) * span)), span = ceil(n / gridDim.x) rounded up to a multiple of the block: every lane of the workgroup makes
// the same number of trips (the ballots and barriers below are uniform), a lane past the end contributes nothing.
// This loop has a TWIN: cloud_accum_span (f3ds_cloud.inc) walks points instead of pixels with the same span arithmetic, one-label ballot, send logic, counts
// and final flush.  A fix to one of the two belongs in the other.
template <class Rule, bool DEPTH_F32>
__device__ __forceinline__ void label_accum_span(const Rule& rule, const unsigned char* depth, const uint32_t* label, const typename Rule::Args& a, typename Rule::Acc* acc,
                                                 uint32_t* head, typename Rule::Table& tab, rg_u64* s_count) {
    using Acc = typename Rule::Acc;
    acc += (size_t)(BIX % a.copies) * a.K;      // this workgroup's set of accumulators
    for (uint32_t k = threadIdx.x; k < (uint32_t)LI_SLOTS; k += blockDim.x) { tab.key[k] = LI_NONE; Rule::table_reset(tab, k); }
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
        uint32_t l = LI_NONE, aux = 0u;
        float z = 0.0f;
        bool valid = false;
        if (active) {
            valid = li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v, z);
            l = label[i];
            aux = rule.aux(u, v);
        }
        bad = bad || (l != LI_NONE && l >= a.K);
        const bool labelled = valid && l < a.K;      // (K <= LI_MAX_REGIONS: LI_NONE is never below it)
        // one label in the wave (the usual case inside a region)?  Known before the pixels are measured: a rule that looks something up by label then does so once a wave
        const uint64_t m = __ballot(labelled);
        uint32_t l0 = LI_NONE;
        bool one_label = false;
        if (m) {      // (wave-uniform, and so is one_label)
            l0 = (uint32_t)__builtin_amdgcn_readlane((int)l, (int)__builtin_ctzll(m));
            one_label = __ballot(labelled && l != l0) == 0ull;
        }
        Acc one;
        Rule::empty(one);
        if (labelled) {
            float x, y, zo;
            n_deproject(u, v, true, z, a.fx, a.fy, a.cx, a.cy, x, y, zo);
            if (rule.pixel(i, u, v, x, y, zo, aux, one_label ? l0 : l, one_label, one)) ++my_clamped;      // (the label is < K; l0: the same value in every lane)
            ++my_labelled;
        }
        // one label: reduce across the wave -- the lanes without a labelled pixel hold the empty values -- and lane 0 sends the sum; otherwise every labelled
        // lane sends its own pixel
        uint32_t target = l;
        bool send = labelled;
        if (one_label) {
            Rule::wave_reduce(one, m);
            target = l0; send = lane_id() == 0;
        }
        if (send) {
            const int slot = li_slot(tab.key, target);
            if (slot >= 0) Rule::lds_add(tab, slot, one); else Rule::global_add(acc + target, one);
        }
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
    const uint32_t wl = rg_wave_u32(my_labelled, RgAdd{}), wc = rg_wave_u32(my_clamped, RgAdd{});
    if (lane_id() == 0) { if (wl) atomicAdd(&s_count[0], (rg_u64)wl); if (wc) atomicAdd(&s_count[1], (rg_u64)wc); }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)LI_SLOTS; k += blockDim.x) {
        const uint32_t l = tab.key[k];
        if (l == LI_NONE) continue;
        Acc t;
        Rule::table_get(tab, k, t);
        Rule::global_add(acc + l, t);      // (l < K: only checked labels get a slot)
    }
    if (threadIdx.x == 0u) {
        if (s_count[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 2), s_count[0]);
        if (s_count[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_count[1]);
    }
}

template <class Rule>
__device__ __forceinline__ void label_finish(const Rule& rule, const typename Rule::Acc* acc, uint32_t K, uint32_t copies, uint32_t* head, typename Rule::Row* rows) {
    if (head[1]) return;      // a label was out of range: the rows stay as they are
    uint32_t nonempty = 0u;
    uint64_t tally = 0ull;
    for (uint32_t r = BIX * blockDim.x + threadIdx.x; r < K; r += gridDim.x * blockDim.x) {
        typename Rule::Acc a = acc[r];
        for (uint32_t c = 1; c < copies; ++c) Rule::merge(a, acc[(size_t)c * K + r]);
        rule.finish(a, r, &rows[r]);
        nonempty += Rule::nonempty(a) ? 1u : 0u;
        if constexpr (Rule::TALLY) tally += Rule::tally(a);
    }
    const uint32_t wn = rg_wave_u32(nonempty, RgAdd{});
    if (lane_id() == 0 && wn) atomicAdd(&head[0], wn);
    if constexpr (Rule::TALLY) {
        const uint64_t wt = rg_wave_add_u64(tally);
        if (lane_id() == 0 && wt) atomicAdd(reinterpret_cast<rg_u64*>(head + 6), (rg_u64)wt);
    }
}

// ------------------------------------------------------------------------------------------------
// the region table
// ------------------------------------------------------------------------------------------------
struct RegionArgs {
    uint32_t width, n;                 // n = width * height
    uint32_t depth_pitch, color_pitch; // bytes per row (never 0 here)
    int depth_f32, color_format;       // F3DS_COLOR_*, or -1: no colour image
    uint32_t K;                        // regions
    uint32_t copies;                   // accumulator sets (rgt_copies): workgroup b adds into set b % copies
    float depth_scale, fx, fy, cx, cy;
};
struct RgTable { uint32_t key[LI_SLOTS]; uint32_t w[RG_W][LI_SLOTS]; rg_u64 s[RG_S][LI_SLOTS]; };

template <int COLOR = -1>      // -1: no colour image, else F3DS_COLOR_* (only aux and wave_reduce look at it)
struct RegionRule {
    using Acc = RgAcc; using Row = f3ds_region_row; using Args = RegionArgs; using Table = RgTable;
    static constexpr int WORDS = RG_WORDS;
    static constexpr bool TALLY = false;
    const unsigned char* color; uint32_t color_pitch;

    static __device__ __forceinline__ uint32_t empty_word(uint32_t k) { return rg_empty_word(k); }
    static __device__ __forceinline__ void empty(RgAcc& a) { rg_empty(a); }
    static __device__ __forceinline__ void table_reset(RgTable& t, uint32_t k) {
#pragma unroll
        for (int f = 0; f < RG_W; ++f) t.w[f][k] = rg_empty_word((uint32_t)f);
#pragma unroll
        for (int f = 0; f < RG_S; ++f) t.s[f][k] = 0ull;
    }
    // the colour word of n_color_word (0 without a colour image)
    __device__ __forceinline__ uint32_t aux(uint32_t u, uint32_t v) const {
        if constexpr (COLOR == 0) { const unsigned char* p = color + (size_t)v * color_pitch + 3u * (size_t)u; return n_color_word(p[0], p[1], p[2], 255u); }
        else if constexpr (COLOR > 0) {
            const uint32_t w = load_unaligned<uint32_t>(color + (size_t)v * color_pitch + 4u * (size_t)u);
            return COLOR == 1 ? n_color_word(w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, 255u) : w;
        }
        else return 0u;
    }
    static __device__ __forceinline__ bool pixel(uint32_t p, uint32_t u, uint32_t v, float x, float y, float z, uint32_t rgba, uint32_t, bool, RgAcc& a) { return rg_pixel(p, u, v, x, y, z, rgba, a); }
    static __device__ __forceinline__ void wave_reduce(RgAcc& one, uint64_t) {
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
    }
    static __device__ __forceinline__ void lds_add(RgTable& t, int slot, const RgAcc& a) {
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
    static __device__ __forceinline__ void table_get(const RgTable& t, uint32_t k, RgAcc& a) {
#pragma unroll
        for (int f = 0; f < RG_W; ++f) a.w[f] = t.w[f][k];
#pragma unroll
        for (int f = 0; f < RG_S; ++f) a.s[f] = t.s[f][k];
    }
    // a into the global accumulator of its region.  A minimum or maximum that the word already meets is not sent: the word only ever moves one way, so a value
    // that does not improve on what a plain load sees (stale or not) cannot improve on what is there now.
    static __device__ __forceinline__ void global_add(RgAcc* dst, const RgAcc& a) {
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
    static __device__ __forceinline__ void merge(RgAcc& a, const RgAcc& b) { rg_merge(a, b); }
    static __device__ __forceinline__ void finish(const RgAcc& a, uint32_t, f3ds_region_row* row) { rg_finish(a, row); }
    static __device__ __forceinline__ bool nonempty(const RgAcc& a) { return a.w[0] != 0u; }
};

struct d_region_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* acc_words, uint32_t n_acc, uint32_t* head) const { label_init<RegionRule<>>(acc_words, n_acc, head); }
};
struct d_region_accum {
    static constexpr int BLOCK = 256;
    template <bool DEPTH_F32, int COLOR>
    static __device__ __forceinline__ void span(const unsigned char* depth, const unsigned char* color, const uint32_t* label, const RegionArgs& a, RgAcc* acc, uint32_t* head,
                                                RgTable& tab, rg_u64* s_count) {
        label_accum_span<RegionRule<COLOR>, DEPTH_F32>(RegionRule<COLOR>{color, a.color_pitch}, depth, label, a, acc, head, tab, s_count);
    }
    __device__ void operator()(const unsigned char* depth, const unsigned char* color, const uint32_t* label, RegionArgs a, RgAcc* acc, uint32_t* head) const {
        __shared__ RgTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ rg_u64 s_count[2];
        if (a.depth_f32) {
            if (a.color_format < 0) span<true, -1>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 0) span<true, 0>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 1) span<true, 1>(depth, color, label, a, acc, head, tab, s_count);
            else span<true, 2>(depth, color, label, a, acc, head, tab, s_count);
        } else {
            if (a.color_format < 0) span<false, -1>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 0) span<false, 0>(depth, color, label, a, acc, head, tab, s_count);
            else if (a.color_format == 1) span<false, 1>(depth, color, label, a, acc, head, tab, s_count);
            else span<false, 2>(depth, color, label, a, acc, head, tab, s_count);
        }
    }
};
struct d_region_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const RgAcc* acc, uint32_t K, uint32_t copies, uint32_t* head, f3ds_region_row* rows) const { label_finish<RegionRule<>>(RegionRule<>{nullptr, 0u}, acc, K, copies, head, rows); }
};
