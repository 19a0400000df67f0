// f3ds_shapes.inc -- the device path of the region shapes (f3ds_region_shapes, include/f3ds.h; the rules are in f3ds_shapes.h; DESIGN.md section 20).
// Included by f3ds_hip.hip after f3ds_contacts.inc.  The three kernels are the skeleton of f3ds_regions.inc (label_init, label_accum_span, label_finish) over
// ShapeRule; the head is the skeleton's.
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
struct ShTable { uint32_t key[LI_SLOTS]; uint32_t n[LI_SLOTS]; rg_u64 s[SH_S][LI_SLOTS]; };      // 128 slots of a label, a count and fifteen sums (128 B), 16 KiB

struct ShapeRule {
    using Acc = ShAcc; using Row = f3ds_region_shape; using Args = ShapeArgs; using Table = ShTable;
    static constexpr int WORDS = SH_WORDS;
    static constexpr bool TALLY = false;

    static __device__ __forceinline__ uint32_t empty_word(uint32_t) { return 0u; }
    static __device__ __forceinline__ void empty(ShAcc& a) { sh_empty(a); }
    static __device__ __forceinline__ void table_reset(ShTable& t, uint32_t k) {
        t.n[k] = 0u;
#pragma unroll
        for (int f = 0; f < SH_S; ++f) t.s[f][k] = 0ull;
    }
    static __device__ __forceinline__ uint32_t aux(uint32_t, uint32_t) { return 0u; }      // (nothing but the depth)
    static __device__ __forceinline__ bool pixel(uint32_t, uint32_t, uint32_t, float x, float y, float z, uint32_t, uint32_t, bool, ShAcc& a) { return sh_pixel(x, y, z, a); }
    static __device__ __forceinline__ void wave_reduce(ShAcc& one, uint64_t m) {
        one.n = (uint32_t)__popcll(m);
#pragma unroll
        for (int k = 0; k < SH_S; ++k) one.s[k] = rg_wave_add_u64(one.s[k]);
    }
    static __device__ __forceinline__ void lds_add(ShTable& t, int slot, const ShAcc& a) {
        atomicAdd(&t.n[slot], a.n);
#pragma unroll
        for (int k = 0; k < SH_S; ++k) atomicAdd(&t.s[k][slot], (rg_u64)a.s[k]);
    }
    static __device__ __forceinline__ void table_get(const ShTable& t, uint32_t k, ShAcc& a) {
        a.n = t.n[k]; a.pad = 0u;
#pragma unroll
        for (int f = 0; f < SH_S; ++f) a.s[f] = t.s[f][k];
    }
    // a into the global accumulator of its region; a sum that is zero is not sent
    static __device__ __forceinline__ void global_add(ShAcc* dst, const ShAcc& a) {
        atomicAdd(&dst->n, a.n);
#pragma unroll
        for (int k = 0; k < SH_S; ++k) if (a.s[k]) atomicAdd(reinterpret_cast<rg_u64*>(&dst->s[k]), (rg_u64)a.s[k]);
    }
    static __device__ __forceinline__ void merge(ShAcc& a, const ShAcc& b) { sh_merge(a, b); }
    static __device__ __forceinline__ void finish(const ShAcc& a, uint32_t, f3ds_region_shape* row) { sh_finish(a, row); }
    static __device__ __forceinline__ bool nonempty(const ShAcc& a) { return a.n != 0u; }
};

struct d_shape_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* acc_words, uint32_t n_acc, uint32_t* head) const { label_init<ShapeRule>(acc_words, n_acc, head); }
};
struct d_shape_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, ShapeArgs a, ShAcc* acc, uint32_t* head) const {
        __shared__ ShTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ rg_u64 s_count[2];
        if (a.depth_f32) label_accum_span<ShapeRule, true>(ShapeRule{}, depth, label, a, acc, head, tab, s_count);
        else label_accum_span<ShapeRule, false>(ShapeRule{}, depth, label, a, acc, head, tab, s_count);
    }
};
struct d_shape_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const ShAcc* acc, uint32_t K, uint32_t copies, uint32_t* head, f3ds_region_shape* rows) const { label_finish<ShapeRule>(ShapeRule{}, acc, K, copies, head, rows); }
};
