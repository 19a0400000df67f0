// f3ds_cloud.inc -- the device path of the region rows of a point cloud (f3ds_cloud_regions, include/f3ds.h; the rules are in f3ds_cloud.h; DESIGN.md section 25).
// Included by f3ds_hip.hip after f3ds_components.inc.
//
// The family's accumulate skeleton (label_accum_span, f3ds_regions.inc) reads an image and leans on its coherence: "a span meets a handful of regions".  The
// points of a cloud come in any order, so the walk over them is written beside it (cloud_accum_span) with the same parts -- the LDS table keyed by label, the
// wave that holds one label reduced across its lanes first, one flush per (workgroup, label) into rgt_copies sets of global accumulators -- and two orders:
//   DIRECT    contiguous spans in input order.  Chosen when K <= CD_DIRECT_MAX_K: every label then finds a slot within CD_PROBES steps whatever the order of
//             the points (cd_longest_run, f3ds_cloud.h), so nothing ever leaves LDS before the flush.
//   ORDERED   d_cloud_keys writes (label << idx_bits) | index per point (the label K for a point without one), the stage-0 radix sort orders them on the label
//             bits (stable: a label's points stay in index order), and the walk reads the sorted keys and GATHERS the 16-byte records through the index.  A span
//             then covers a stretch of consecutive labels.  When more than half the table has been claimed since the last flush, the workgroup flushes and
//             clears it at the end of the trip.  What that bounds is the fill at the START of a trip: at most CD_SLOTS / 2 labels.  Inside a trip nothing is
//             promised: a label whose LI_PROBES probe slots are all taken goes to its global accumulator, which can begin once the table holds some hundred
//             labels (cd_longest_run: the run of labels 0 ... 102 is 9) -- a trip of 256 points that adds the forty labels it takes to get there from 64
//             has six points a label on average.  The points of a label are contiguous in this order, so such atomics go to the label's own lines, a few
//             per label, and not to a line that other labels or many workgroups share: in neither order does the cost degrade to one global atomic per
//             point onto a shared line.
// The kernels of a call:
//   d_cloud_init        the K x copies accumulators (CdAcc, 44 words) get their empty values, the head its zeros
//   d_cloud_keys        (ordered) the keys, and word [1] of the head raised for a label >= K
//   d_cloud_accum       the read of the records and the labels (direct) or of the sorted keys and the gathered records (ordered)
//   d_cloud_finish      label_finish over CloudRule: the sets merged, cd_finish per region into the caller's rows and the shape rows the boxes are made of
//   d_box_frame, d_cloud_box_accum, d_box_finish      (boxes) the frames as the region boxes make them (f3ds_boxes.inc), the second walk in the SAME order with
//                       every point measured in the frame of its label, the boxes' finish as it is
// The head is the family's: [0] non-empty regions, [1] 1 if a label was >= K, [2..3] labelled points, [4..5] clamped points, [6..7] inliers.
// Every field is a count, a minimum, a maximum or an integer sum: integer atomics in LDS and in global memory give the bits of the host function.  No float atomics.

static_assert(CD_SLOT_BITS == LI_SLOT_BITS && CD_PROBES == LI_PROBES, "f3ds_cloud.h argues about the family's table");

struct CloudArgs {
    uint32_t n, K;                     // points, regions
    uint32_t copies;                   // accumulator sets (rgt_copies): workgroup b adds into set b % copies
    uint32_t idx_bits;                 // ordered: a key is (label << idx_bits) | index
    int fold_negative_z, ordered;
};
struct CdTable { uint32_t key[LI_SLOTS]; uint32_t w[CD_W][LI_SLOTS]; rg_u64 s[CD_S][LI_SLOTS]; };      // 128 slots of a label, eight words and eighteen sums (176 B): 22.5 KiB

// li_slot that also counts the slots it claims (the ordered walk clears a table that fills up)
__device__ __forceinline__ int cd_slot(uint32_t* key, uint32_t l, uint32_t* used) {
    uint32_t h = (l * 0x9E3779B1u) >> (32 - LI_SLOT_BITS);
    for (int k = 0; k < LI_PROBES; ++k) {
        const uint32_t old = atomicCAS(&key[h], LI_NONE, l);
        if (old == LI_NONE) { atomicAdd(used, 1u); return (int)h; }
        if (old == l) return (int)h;
        h = (h + 1u) & (uint32_t)(LI_SLOTS - 1);
    }
    return -1;
}

// A RULE says what a point adds (CloudRule: cd_point; CloudBoxRule: bx_pixel in the frame of the label): Acc, Table, empty, table_reset,
// point(i, x, y, z, rgba, l, one_label, acc) -> clamped?, wave_reduce, lds_add, table_get, global_add -- the members of the family's rules.
// Span of workgroup b: as label_accum_span, [b * span, min(n, (b + 1) * span)) with span a multiple of the block: every lane makes the same number of trips.
// The TWIN of label_accum_span (f3ds_regions.inc): span arithmetic, one-label ballot, send logic, counts and final flush are the same; a fix to one belongs in the other.
template <class Rule, bool ORDERED>
__device__ __forceinline__ void cloud_accum_span(const Rule& rule, const P16* pts, const uint32_t* label, const uint64_t* keys, const CloudArgs& a, typename Rule::Acc* acc,
                                                 uint32_t* head, typename Rule::Table& tab, rg_u64* s_count, uint32_t* s_used) {
    using Acc = typename Rule::Acc;
    acc += (size_t)(BIX % a.copies) * a.K;      // this workgroup's set of accumulators
    for (uint32_t k = threadIdx.x; k < (uint32_t)LI_SLOTS; k += blockDim.x) { tab.key[k] = LI_NONE; Rule::table_reset(tab, k); }
    if (threadIdx.x < 2u) s_count[threadIdx.x] = 0ull;
    if (threadIdx.x == 0u) *s_used = 0u;
    __syncthreads();
    const uint64_t per = ((uint64_t)a.n + gridDim.x - 1u) / gridDim.x;
    const uint64_t span = (per + blockDim.x - 1u) / blockDim.x * blockDim.x;
    const uint64_t begin64 = (uint64_t)BIX * span;
    const uint32_t begin = begin64 < a.n ? (uint32_t)begin64 : a.n, end = begin64 + span < a.n ? (uint32_t)(begin64 + span) : a.n;
    const uint64_t imask = (1ull << a.idx_bits) - 1ull;
    uint32_t j = begin + threadIdx.x;
    uint32_t my_labelled = 0u, my_clamped = 0u, flushed_at = 0u;
    bool bad = false;
    for (uint32_t base = begin; base < end; base += blockDim.x, j += blockDim.x) {
        uint32_t l = LI_NONE, i = j;
        if (j < end) {
            if constexpr (ORDERED) {
                const uint64_t k = keys[j];
                l = (uint32_t)(k >> a.idx_bits); i = (uint32_t)(k & imask);      // (i < n: d_cloud_keys wrote it; l == K: no label, or one out of range)
            } else {
                l = label[j];
                bad = bad || (l != LI_NONE && l >= a.K);
            }
        }
        float x = 0.0f, y = 0.0f, z = 0.0f; uint32_t rgba = 0u;
        bool labelled = false;
        if (l < a.K) {      // (K <= LI_MAX_REGIONS: LI_NONE is never below it)
            const P16 p = load_point(pts, i);
            x = p.x; y = p.y; z = p.z; rgba = p.rgba;
            labelled = cd_finite(x, y, z, a.fold_negative_z);
        }
        // one label in the wave (the rule inside a region of an organised cloud, and in the sorted order)?
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
            if (rule.point(i, x, y, z, rgba, one_label ? l0 : l, one_label, one)) ++my_clamped;
            ++my_labelled;
        }
        uint32_t target = l;
        bool send = labelled;
        if (one_label) {
            Rule::wave_reduce(one, m);
            target = l0; send = lane_id() == 0;
        }
        if (send) {
            const int slot = cd_slot(tab.key, target, s_used);
            if (slot >= 0) Rule::lds_add(tab, slot, one); else Rule::global_add(acc + target, one);
        }
        if constexpr (ORDERED) {
            // a table more than half taken goes to the global accumulators now: the labels of this trip are behind the walk for good (sorted order)
            __syncthreads();
            const uint32_t used = *s_used;      // (claims so far, never reset: every lane reads it between the two barriers and sees the same count)
            if (used - flushed_at > (uint32_t)LI_SLOTS / 2u) {
                for (uint32_t k = threadIdx.x; k < (uint32_t)LI_SLOTS; k += blockDim.x) {
                    const uint32_t lk = tab.key[k];
                    if (lk == LI_NONE) continue;
                    Acc t;
                    Rule::table_get(tab, k, t);
                    Rule::global_add(acc + lk, t);
                    tab.key[k] = LI_NONE; Rule::table_reset(tab, k);
                }
                flushed_at = used;
            }
            __syncthreads();
        }
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
    const uint32_t wl = rg_wave_u32(my_labelled, RgAdd{}), wc = rg_wave_u32(my_clamped, RgAdd{});
    if (lane_id() == 0) { if (wl) atomicAdd(&s_count[0], (rg_u64)wl); if (wc) atomicAdd(&s_count[1], (rg_u64)wc); }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < (uint32_t)LI_SLOTS; k += blockDim.x) {
        const uint32_t lk = tab.key[k];
        if (lk == LI_NONE) continue;
        Acc t;
        Rule::table_get(tab, k, t);
        Rule::global_add(acc + lk, t);      // (lk < K: only checked labels get a slot)
    }
    if (threadIdx.x == 0u) {
        if (s_count[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 2), s_count[0]);
        if (s_count[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_count[1]);
    }
}

// pass one: the table's and the shapes' fields of a point in one accumulator
struct CloudRule {
    using Acc = CdAcc; using Row = f3ds_cloud_region; using Table = CdTable;
    static constexpr int WORDS = CD_WORDS;
    static constexpr bool TALLY = false;
    f3ds_region_shape* shapes;      // finish: the shape row of every region (NULL: nobody wants them)

    static __device__ __forceinline__ uint32_t empty_word(uint32_t k) { return cd_empty_word(k); }
    static __device__ __forceinline__ void empty(CdAcc& a) { cd_empty(a); }
    static __device__ __forceinline__ void table_reset(CdTable& t, uint32_t k) {
#pragma unroll
        for (int f = 0; f < CD_W; ++f) t.w[f][k] = cd_empty_word((uint32_t)f);
#pragma unroll
        for (int f = 0; f < CD_S; ++f) t.s[f][k] = 0ull;
    }
    static __device__ __forceinline__ bool point(uint32_t i, float x, float y, float z, uint32_t rgba, uint32_t, bool, CdAcc& a) { return cd_point(i, x, y, z, rgba, a); }
    static __device__ __forceinline__ void wave_reduce(CdAcc& one, uint64_t m) {
        one.w[0] = (uint32_t)__popcll(m);
#pragma unroll
        for (int k = 1; k < 5; ++k) one.w[k] = rg_wave_u32(one.w[k], RgMin{});
#pragma unroll
        for (int k = 5; k < 8; ++k) one.w[k] = rg_wave_u32(one.w[k], RgMax{});
#pragma unroll
        for (int k = 0; k < SH_S; ++k) one.s[k] = rg_wave_add_u64(one.s[k]);
#pragma unroll
        for (int k = SH_S; k < CD_S; ++k) one.s[k] = (uint64_t)rg_wave_u32((uint32_t)one.s[k], RgAdd{});      // (64 bytes add up inside 32 bits)
    }
    static __device__ __forceinline__ void lds_add(CdTable& t, int slot, const CdAcc& a) {
        atomicAdd(&t.w[0][slot], a.w[0]);
#pragma unroll
        for (int k = 1; k < 5; ++k) atomicMin(&t.w[k][slot], a.w[k]);
#pragma unroll
        for (int k = 5; k < 8; ++k) atomicMax(&t.w[k][slot], a.w[k]);
#pragma unroll
        for (int k = 0; k < CD_S; ++k) atomicAdd(&t.s[k][slot], (rg_u64)a.s[k]);
    }
    static __device__ __forceinline__ void table_get(const CdTable& t, uint32_t k, CdAcc& a) {
#pragma unroll
        for (int f = 0; f < CD_W; ++f) a.w[f] = t.w[f][k];
#pragma unroll
        for (int f = 0; f < CD_S; ++f) a.s[f] = t.s[f][k];
    }
    // a into the global accumulator of its region, as RegionRule: a minimum or maximum that a relaxed load shows the word to meet already is not sent (the word
    // only ever moves one way), nor is a sum that is zero
    static __device__ __forceinline__ void global_add(CdAcc* dst, const CdAcc& a) {
        atomicAdd(&dst->w[0], a.w[0]);
#pragma unroll
        for (int k = 1; k < 5; ++k) if (a.w[k] < __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMin(&dst->w[k], a.w[k]);
#pragma unroll
        for (int k = 5; k < 8; ++k) if (a.w[k] > __atomic_load_n(&dst->w[k], __ATOMIC_RELAXED)) atomicMax(&dst->w[k], a.w[k]);
#pragma unroll
        for (int k = 0; k < CD_S; ++k) if (a.s[k]) atomicAdd(reinterpret_cast<rg_u64*>(&dst->s[k]), (rg_u64)a.s[k]);
    }
    static __device__ __forceinline__ void merge(CdAcc& a, const CdAcc& b) { cd_merge(a, b); }
    __device__ __forceinline__ void finish(const CdAcc& a, uint32_t r, f3ds_cloud_region* row) const {
        f3ds_region_shape s;
        cd_finish(a, row, &s);
        if (shapes) shapes[r] = s;
    }
    static __device__ __forceinline__ bool nonempty(const CdAcc& a) { return a.w[0] != 0u; }
};

// pass two: BoxRule (f3ds_boxes.inc) as it is, its pixel() given the point
struct CloudBoxRule : BoxRule {
    __device__ __forceinline__ bool point(uint32_t, float x, float y, float z, uint32_t, uint32_t l, bool one_label, BxAcc& a) const { return pixel(0u, 0u, 0u, x, y, z, 0u, l, one_label, a); }
};

struct d_cloud_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t* acc_words, uint32_t n_acc, uint32_t* head) const { label_init<CloudRule>(acc_words, n_acc, head); }
};
struct d_cloud_keys {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint32_t* label, CloudArgs a, uint64_t* keys, uint32_t* head) const {
        bool bad = false;
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
            const uint32_t l = label[i];
            bad = bad || (l != LI_NONE && l >= a.K);
            keys[i] = ((uint64_t)(l < a.K ? l : a.K) << a.idx_bits) | (uint64_t)i;
        }
        if (bad) head[1] = 1u;
    }
};
struct d_cloud_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* pts, const uint32_t* label, const uint64_t* keys, CloudArgs a, CdAcc* acc, uint32_t* head) const {
        __shared__ CdTable tab;
        __shared__ rg_u64 s_count[2];
        __shared__ uint32_t s_used;
        if (a.ordered) cloud_accum_span<CloudRule, true>(CloudRule{nullptr}, pts, label, keys, a, acc, head, tab, s_count, &s_used);
        else cloud_accum_span<CloudRule, false>(CloudRule{nullptr}, pts, label, keys, a, acc, head, tab, s_count, &s_used);
    }
};
struct d_cloud_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const CdAcc* acc, uint32_t K, uint32_t copies, uint32_t* head, f3ds_cloud_region* rows, f3ds_region_shape* shapes) const {
        label_finish<CloudRule>(CloudRule{shapes}, acc, K, copies, head, rows);
    }
};
struct d_cloud_box_accum {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const P16* pts, const uint32_t* label, const uint64_t* keys, CloudArgs a, const BxFrame* frames, BxAcc* acc, const uint32_t* head, uint32_t* head2) const {
        __shared__ BxTable tab;
        __shared__ rg_u64 s_count[2];
        __shared__ uint32_t s_used;
        if (head[1]) return;      // (every lane reads the same word: the workgroup leaves as one; no frame was written)
        CloudBoxRule rule;
        rule.frames = frames;
        if (a.ordered) cloud_accum_span<CloudBoxRule, true>(rule, pts, label, keys, a, acc, head2, tab, s_count, &s_used);
        else cloud_accum_span<CloudBoxRule, false>(rule, pts, label, keys, a, acc, head2, tab, s_count, &s_used);
    }
};
