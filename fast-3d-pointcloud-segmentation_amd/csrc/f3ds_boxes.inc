// f3ds_boxes.inc -- the device path of the region boxes (f3ds_region_boxes, include/f3ds.h; the rules are in f3ds_boxes.h; DESIGN.md section 22).
// Included by f3ds_hip.hip after f3ds_shapes.inc.  The call records the three kernels of the shapes as they are, then
//
//   d_box_frame      one lane per region: the shape row becomes the region's frame (BxFrame, 64 bytes: c, n, m, l, plane_tol -- one cache line a region, so pass
//                    two loads aligned dwordx4s and does not derive m per pixel), the region's pass-two accumulators in every set get their empty values, the
//                    head of pass two its zeros.  Nothing but that head when pass one found a label out of range.
//   d_box_accum      the SECOND read of the depth image and the labels: the skeleton of f3ds_regions.inc (label_accum_span) over BoxRule, whose pixel() measures
//                    the pixel in the frame of its label.  Returns at once when pass one found a label out of range: no frame is indexed by an unchecked label.
//   d_box_finish     label_finish over BoxRule: the sets merged, bx_finish per region into the caller's rows (or the staging of a host caller), the sum of
//                    n_inliers into words 6 ... 7 of the head
// Pass two has a head of its own: the skeleton adds the labelled and clamped counts to the head it is given, and the caller's head holds them from pass one.
// Every field is a count, a minimum, a maximum or an integer sum (f3ds_boxes.h): integer atomics in LDS and in global memory give the bits of the host function.

typedef float bx_f4 __attribute__((ext_vector_type(4)));                          // a quarter of a frame: one aligned dwordx4
typedef __attribute__((address_space(4))) bx_f4 bx_f4_const;                      // ... read through the constant address space
struct BxTable { uint32_t key[LI_SLOTS]; uint32_t w[BX_W][LI_SLOTS]; rg_u64 s[LI_SLOTS]; };      // 128 slots of a label, eight words and a sum (40 B), 5.5 KiB

struct BoxRule {
    using Acc = BxAcc; using Row = f3ds_region_box; using Args = ShapeArgs; using Table = BxTable;
    static constexpr int WORDS = BX_WORDS;
    static constexpr bool TALLY = true;
    const BxFrame* frames;

    static __device__ __forceinline__ uint32_t empty_word(uint32_t k) { return bx_empty_word(k); }
    static __device__ __forceinline__ void empty(BxAcc& a) { bx_empty(a); }
    static __device__ __forceinline__ void table_reset(BxTable& t, uint32_t k) {
#pragma unroll
        for (int f = 0; f < BX_W; ++f) t.w[f][k] = bx_empty_word((uint32_t)f);
        t.s[k] = 0ull;
    }
    static __device__ __forceinline__ uint32_t aux(uint32_t, uint32_t) { return 0u; }      // (nothing but the depth)
    // The frame of label l (l < K: the skeleton checked it).  One label in the wave: the skeleton passes the one label of the wave, the address is the same
    // in every lane, and the compiler is shown so (readfirstlane), so the 64 bytes can come through the scalar cache; several labels: each lane gathers its
    // own line, four aligned dwordx4s, and a coherent image keeps those to a few lines.
    // The uniform load goes through the constant address space: the frames were written by the kernel before this one and nothing writes them while it runs,
    // which is what that address space promises, and a uniform address in it is a scalar load (s_load_dwordx16: one request a wave, no VGPR traffic).
    __device__ __forceinline__ bool pixel(uint32_t, uint32_t, uint32_t, float x, float y, float z, uint32_t, uint32_t l, bool one_label, BxAcc& a) const {
        bx_f4 q0, q1, q2, q3;
        if (one_label) {
            const bx_f4_const* p = (const bx_f4_const*)(frames + (uint32_t)__builtin_amdgcn_readfirstlane((int)l));
            q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3];
        } else {
            const bx_f4* p = reinterpret_cast<const bx_f4*>(frames + l);
            q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3];
        }
        BxFrame f;
        f.c[0] = q0.x; f.c[1] = q0.y; f.c[2] = q0.z; f.n[0] = q0.w; f.n[1] = q1.x; f.n[2] = q1.y; f.m[0] = q1.z; f.m[1] = q1.w; f.m[2] = q2.x;
        f.l[0] = q2.y; f.l[1] = q2.z; f.l[2] = q2.w; f.tol = q3.x; f.pad[0] = f.pad[1] = f.pad[2] = 0.0f;
        return bx_pixel(x, y, z, f, a);
    }
    static __device__ __forceinline__ void wave_reduce(BxAcc& one, uint64_t m) {
        one.w[0] = (uint32_t)__popcll(m);
        one.w[1] = rg_wave_u32(one.w[1], RgAdd{});
#pragma unroll
        for (int k = 2; k < 5; ++k) one.w[k] = rg_wave_u32(one.w[k], RgMin{});
#pragma unroll
        for (int k = 5; k < 8; ++k) one.w[k] = rg_wave_u32(one.w[k], RgMax{});
        one.s = rg_wave_add_u64(one.s);
    }
    static __device__ __forceinline__ void lds_add(BxTable& t, int slot, const BxAcc& a) {
        atomicAdd(&t.w[0][slot], a.w[0]);
        if (a.w[1]) atomicAdd(&t.w[1][slot], a.w[1]);
#pragma unroll
        for (int k = 2; k < 5; ++k) atomicMin(&t.w[k][slot], a.w[k]);
#pragma unroll
        for (int k = 5; k < 8; ++k) atomicMax(&t.w[k][slot], a.w[k]);
        atomicAdd(&t.s[slot], (rg_u64)a.s);
    }
    static __device__ __forceinline__ void table_get(const BxTable& t, uint32_t k, BxAcc& a) {
#pragma unroll
        for (int f = 0; f < BX_W; ++f) a.w[f] = t.w[f][k];
        a.s = t.s[k];
    }
    // a into the global accumulator of its region, as RegionRule: a minimum or maximum that a relaxed load shows the word to meet already is not sent (the
    // word only ever moves one way), nor is a sum that is zero
    static __device__ __forceinline__ void global_add(BxAcc* dst, const BxAcc& a) {
        atomicAdd(&dst->w[0], a.w[0]);
        if (a.w[1]) atomicAdd(&dst->w[1], a.w[1]);
#pragma unroll
        for (int k = 2; k < 5; ++k) if (a.w[k] < __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMin(&dst->w[k], a.w[k]);
#pragma unroll
        for (int k = 5; k < 8; ++k) if (a.w[k] > __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMax(&dst->w[k], a.w[k]);
        if (a.s) atomicAdd(reinterpret_cast<rg_u64*>(&dst->s), (rg_u64)a.s);
    }
    static __device__ __forceinline__ void merge(BxAcc& a, const BxAcc& b) { bx_merge(a, b); }
    __device__ __forceinline__ void finish(const BxAcc& a, uint32_t r, f3ds_region_box* row) const { bx_finish(a, frames[r], row); }
    static __device__ __forceinline__ bool nonempty(const BxAcc&) { return false; }      // (the shapes' finish counted the non-empty regions into this head already)
    static __device__ __forceinline__ uint64_t tally(const BxAcc& a) { return a.w[1]; }
};

struct d_box_frame {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const f3ds_region_shape* shapes, uint32_t K, uint32_t copies, float plane_tol, const uint32_t* head, BxFrame* frames, BxAcc* acc,
                               uint32_t* head2) const {
        if (BIX == 0u && threadIdx.x < LI_HEAD_WORDS) head2[threadIdx.x] = 0u;
        if (head[1]) return;      // a label was out of range: d_shape_finish wrote no row
        for (uint32_t r = BIX * blockDim.x + threadIdx.x; r < K; r += gridDim.x * blockDim.x) {
            BxFrame f;
            bx_frame(shapes[r], plane_tol, f);
            frames[r] = f;
            BxAcc e;
            bx_empty(e);
            for (uint32_t c = 0; c < copies; ++c) acc[(size_t)c * K + r] = e;
        }
    }
};
struct d_box_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, ShapeArgs a, const BxFrame* frames, BxAcc* acc, const uint32_t* head, uint32_t* head2) const {
        __shared__ BxTable tab;
        __shared__ rg_u64 s_count[2];
        if (head[1]) return;      // (every lane reads the same word: the workgroup leaves as one)
        if (a.depth_f32) label_accum_span<BoxRule, true>(BoxRule{frames}, depth, label, a, acc, head2, tab, s_count);
        else label_accum_span<BoxRule, false>(BoxRule{frames}, depth, label, a, acc, head2, tab, s_count);
    }
};
struct d_box_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const BxAcc* acc, const BxFrame* frames, uint32_t K, uint32_t copies, uint32_t* head, f3ds_region_box* rows) const {
        label_finish<BoxRule>(BoxRule{frames}, acc, K, copies, head, rows);
    }
};
