// f3ds_joints.inc -- the device path of the region joints (f3ds_region_joints, include/f3ds.h; the rules are in f3ds_joints.h; DESIGN.md section 24).
// Included by f3ds_hip.hip after f3ds_boxes.inc.  In front of these kernels the call records the three kernels of the shapes as they are (f3ds_shapes.inc).
//
//   d_joint_init     the record keys become holes, the record indices 0, 1, 2, ..., the head its zeros
//   d_joint_accum    the structure of d_contact_accum: a workgroup takes a CONTIGUOUS span of pixels, a lane reads its pixel's label and the labels to the right
//                    and below, and a wave without a border pixel -- most waves -- goes on after ONE ballot; depths are read only behind it.  A border lane
//                    deprojects its own pixel and the neighbour's; a CLOSE pair adds two sh_pixel contributions (f3ds_shapes.h) to the LDS slot of its (a, b),
//                    next to the contacts' two counts.  At the end of the span the occupied slots are APPENDED as records (key, 34 words): one atomic per
//                    workgroup reserves the range.  A pair that finds no slot is a record of its own, one atomic per wave.  No global atomic per pixel or pair.
//   (the radix sort of the record keys with the record index as value, d_evl_heads and the scan of its flags, d_track_runs: run e = the e-th distinct key)
//   d_joint_finish   one wave per run: its records merged (jt_merge: exact) and wave-reduced, lane 0 runs jt_finish -- sh_finish on the samples and the join with
//                    shapes[a] and shapes[b] -- and writes the row in (a, b) order; the sums and counts into the head; nothing but the head when a label was
//                    out of range or the records did not fit (the host then runs the frame again with room for all)
// Every field that meets more than one pixel is a count or a sum of 64-bit integers: arrival order does not matter, so integer atomics in LDS (ds_add_u64)
// give the bits of the host function.  No float atomics.

struct JointArgs {
    uint32_t width, height, n;         // n = width * height
    uint32_t depth_pitch;              // bytes per row (never 0 here)
    int depth_f32;
    uint32_t K;                        // regions
    int kb;                            // ct_bits(K)
    uint32_t rec_cap;                  // records the buffers hold
    float depth_scale, depth_tol, fx, fy, cx, cy;
};
// the head (LI_HEAD_WORDS, f3ds_label_image.h): [0] rows, [1] 1 if a label was >= K, [2] records asked for (more than rec_cap: nothing else holds), [3] rows with a
// close pair (n_surface), [4..5] contact pairs (u64), [6..7] close ones (u64)
constexpr int RGJ_SLOT_BITS = 7, RGJ_SLOTS = 1 << RGJ_SLOT_BITS;      // LDS table: 128 slots of a key, two counts and fifteen sums (136 B), 17 KiB (DESIGN.md section 24: why not 256)
constexpr int RGJ_BLOCK = 256;
constexpr int RGJ_PROBES = 8;          // a pair that finds neither its slot nor a free one in this many steps becomes a record of its own
constexpr uint32_t RGJ_TRIPS = 8;      // trips of a workgroup the grid is sized for (the contacts' figure)
constexpr uint32_t RGJ_FIRST_CAP = 32768;      // records the first run has room for (4.3 MiB); F3DS_RGJ_FIRST_CAP (development) replaces it
constexpr uint32_t RGJ_FIRST_ROWS = 2048;      // rows of a host caller that ride with the head; a frame with more gets a second download
static_assert(RGJ_SLOTS <= RGJ_BLOCK, "slot k is thread k's at the flush");

struct d_joint_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint64_t* keys, uint32_t* vals, uint32_t rec_cap, uint32_t* head) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < rec_cap; i += gridDim.x * blockDim.x) { keys[i] = CT_NO_KEY; vals[i] = i; }
        if (BIX == 0u && threadIdx.x < LI_HEAD_WORDS) head[threadIdx.x] = 0u;
    }
};

// the LDS table of a workgroup: field-major, as CtTable and ShTable
struct JtTable { rg_u64 key[RGJ_SLOTS]; uint32_t w[2][RGJ_SLOTS]; rg_u64 s[SH_S][RGJ_SLOTS]; };

// the slot of a key, claimed on the way if it is new; -1: none within RGJ_PROBES steps (slots are never given back within a span: as ct_slot)
__device__ __forceinline__ int jt_slot(JtTable& t, uint64_t key) {
    uint32_t h = ((uint32_t)(key ^ (key >> 29)) * 0x9E3779B1u) >> (32 - RGJ_SLOT_BITS);
    for (int k = 0; k < RGJ_PROBES; ++k) {
        const rg_u64 old = atomicCAS(&t.key[h], (rg_u64)CT_NO_KEY, (rg_u64)key);
        if (old == (rg_u64)CT_NO_KEY || old == (rg_u64)key) return (int)h;
        h = (h + 1u) & (uint32_t)(RGJ_SLOTS - 1);
    }
    return -1;
}
// a into its slot; a pair that is not close has no sample: one atomic
__device__ __forceinline__ void jt_lds_add(JtTable& t, int slot, const JtAcc& a) {
    atomicAdd(&t.w[0][slot], a.n_pairs);
    if (a.n_close == 0u) return;
    atomicAdd(&t.w[1][slot], a.n_close);
#pragma unroll
    for (int k = 0; k < SH_S; ++k) atomicAdd(&t.s[k][slot], (rg_u64)a.sh.s[k]);
}
__device__ __forceinline__ void jt_record(uint64_t* keys, uint32_t* rec, uint32_t pos, uint64_t key, const JtAcc& a) {
    keys[pos] = key;
    uint2* r = reinterpret_cast<uint2*>(rec + (size_t)pos * JT_WORDS);      // (JT_WORDS * 4 is a multiple of 8)
    r[0] = make_uint2(a.n_pairs, a.n_close); r[1] = make_uint2(a.sh.n, 0u);
#pragma unroll
    for (int k = 0; k < SH_S; ++k) r[2 + k] = make_uint2((uint32_t)a.sh.s[k], (uint32_t)(a.sh.s[k] >> 32));
}

// What a wave does with the pairs of one direction (horizontal: a lane's pixel and its right neighbour; else its lower one); has: this lane has a contact pair.
// Called behind a wave-uniform branch: every lane of the wave is here.
__device__ __forceinline__ void joint_pairs(bool has, bool horizontal, uint32_t i, uint32_t u, uint32_t v, uint32_t l, float z, const float (&P)[3], uint32_t lq, float zq,
                                            const JointArgs& a, uint64_t* keys, uint32_t* rec, uint32_t* head, JtTable& tab) {
    const uint64_t m = __ballot(has);
    if (m == 0ull) return;
    JtAcc one;
    jt_empty(one);
    uint64_t key = CT_NO_KEY;
    if (has) {
        float Q[3];
        n_deproject(horizontal ? u + 1u : u, horizontal ? v : v + 1u, true, zq, a.fx, a.fy, a.cx, a.cy, Q[0], Q[1], Q[2]);
        uint32_t pa, pb;
        jt_pair(i, horizontal, l, z, lq, zq, a.depth_tol, P, Q, pa, pb, one);
        key = ct_key(pa, pb, a.kb);
    }
    bool send = has;
    // one pair of regions in the wave (the usual case along a border): reduce across the wave -- the lanes without a contact hold the empty values -- and
    // lane 0 sends the sum; otherwise every lane with a contact sends its own.  The fifteen 64-bit reductions are paid only where some pair is close.
    const int first = (int)__builtin_ctzll(m);
    const uint64_t key0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), first) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, first);
    if ((m & (m - 1ull)) != 0ull && __ballot(has && key != key0) == 0ull) {
        one.n_pairs = (uint32_t)__popcll(m);
        const uint64_t cm = __ballot(one.n_close != 0u);
        one.n_close = (uint32_t)__popcll(cm);
        one.sh.n = 2u * one.n_close;
        if (cm != 0ull) {
#pragma unroll
            for (int f = 0; f < SH_S; ++f) one.sh.s[f] = rg_wave_add_u64(one.sh.s[f]);
        }
        key = key0; send = lane_id() == 0;
    }
    int slot = -1;
    if (send) { slot = jt_slot(tab, key); if (slot >= 0) jt_lds_add(tab, slot, one); }
    const uint64_t over = __ballot(send && slot < 0);
    if (over != 0ull) {      // the table is full around these keys: records of their own, one reservation per wave
        const int lead = (int)__builtin_ctzll(over);
        uint32_t at = 0u;
        if (lane_id() == lead) at = atomicAdd(&head[2], (uint32_t)__popcll(over));
        at = (uint32_t)__builtin_amdgcn_readlane((int)at, lead);
        if (send && slot < 0) {
            const uint64_t pos = (uint64_t)at + (uint32_t)__popcll(over & lanemask_lt());
            if (pos < a.rec_cap) jt_record(keys, rec, (uint32_t)pos, key, one);
        }
    }
}

// Span of workgroup b: as contact_accum_span.  A pixel's right and lower neighbours are read wherever they lie -- the pair belongs to its first pixel.
template <bool DEPTH_F32>
__device__ __forceinline__ void joint_accum_span(const unsigned char* depth, const uint32_t* label, const JointArgs& a, uint64_t* keys, uint32_t* rec, uint32_t* head,
                                                 JtTable& tab, uint32_t* s_base) {
    for (uint32_t k = threadIdx.x; k < (uint32_t)RGJ_SLOTS; k += blockDim.x) {
        tab.key[k] = (rg_u64)CT_NO_KEY;
        tab.w[0][k] = tab.w[1][k] = 0u;
#pragma unroll
        for (int f = 0; f < SH_S; ++f) tab.s[f][k] = 0ull;
    }
    __syncthreads();
    const uint64_t per = ((uint64_t)a.n + gridDim.x - 1u) / gridDim.x;
    const uint64_t span = (per + blockDim.x - 1u) / blockDim.x * blockDim.x;
    const uint64_t begin64 = (uint64_t)BIX * span;
    const uint32_t begin = begin64 < a.n ? (uint32_t)begin64 : a.n, end = begin64 + span < a.n ? (uint32_t)(begin64 + span) : a.n;
    const uint32_t sv = blockDim.x / a.width, su = blockDim.x - sv * a.width;      // a trip moves every lane this many rows and columns on (as d_deproject)
    uint32_t i = begin + threadIdx.x;
    uint32_t v = i / a.width, u = i - v * a.width;
    bool bad = false;
    for (uint32_t base = begin; base < end; base += blockDim.x, i += blockDim.x) {
        uint32_t l = CT_NONE, lr = CT_NONE, ld = CT_NONE;      // this pixel's label, its right and its lower neighbour's
        if (i < end) {
            l = label[i];
            if (u + 1u < a.width) lr = label[i + 1u];
            if (v + 1u < a.height) ld = label[i + a.width];      // (i + width < n: v + 1 < height)
        }
        bad = bad || (l != CT_NONE && l >= a.K);
        bool hr = l < a.K && lr < a.K && lr != l;      // (K <= CT_MAX_REGIONS: CT_NONE is never below it)
        bool hd = l < a.K && ld < a.K && ld != l;
        if (__ballot(hr || hd) != 0ull) {      // (wave-uniform, and so are the branches on ballots in joint_pairs)  Inside a region no depth is read.
            float z = 0.0f, zr = 0.0f, zd = 0.0f;
            const bool valid = (hr || hd) && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v, z);
            hr = hr && valid && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u + 1u, v, zr);
            hd = hd && valid && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v + 1u, zd);
            float P[3] = {0.0f, 0.0f, 0.0f};
            if (hr || hd) n_deproject(u, v, true, z, a.fx, a.fy, a.cx, a.cy, P[0], P[1], P[2]);
            joint_pairs(hr, true, i, u, v, l, z, P, lr, zr, a, keys, rec, head, tab);
            joint_pairs(hd, false, i, u, v, l, z, P, ld, zd, a, keys, rec, head, tab);
        }
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
    __syncthreads();
    // the occupied slots become records: slot k is thread k's, the positions from a scan of the occupancy
    const bool mine = threadIdx.x < (uint32_t)RGJ_SLOTS;
    const uint64_t key = mine ? (uint64_t)tab.key[threadIdx.x] : CT_NO_KEY;
    const uint32_t occ = key != CT_NO_KEY ? 1u : 0u;
    uint32_t total;
    const uint32_t incl = block_incl_scan<RGJ_BLOCK>(occ, &total);
    if (threadIdx.x == 0u) *s_base = total ? atomicAdd(&head[2], total) : 0u;
    __syncthreads();
    if (occ) {
        const uint64_t pos = (uint64_t)*s_base + incl - 1u;
        if (pos < a.rec_cap) {
            JtAcc t;
            t.n_pairs = tab.w[0][threadIdx.x]; t.n_close = tab.w[1][threadIdx.x]; t.sh.n = 2u * t.n_close; t.sh.pad = 0u;
#pragma unroll
            for (int f = 0; f < SH_S; ++f) t.sh.s[f] = tab.s[f][threadIdx.x];
            jt_record(keys, rec, (uint32_t)pos, key, t);
        }
    }
}
struct d_joint_accum {
    static constexpr int BLOCK = RGJ_BLOCK;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, JointArgs a, uint64_t* keys, uint32_t* rec, uint32_t* head) const {
        __shared__ JtTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ uint32_t s_base;
        if (a.depth_f32) joint_accum_span<true>(depth, label, a, keys, rec, head, tab, &s_base);
        else joint_accum_span<false>(depth, label, a, keys, rec, head, tab, &s_base);
    }
};

// One wave per run of equal keys in the sorted records (ukey, ustart, uend, *total: d_track_runs); vals: the record indices in sorted order; shapes: the K shape
// rows d_shape_finish wrote earlier in the same flush.  rows may be null (a count-only call); more rows than row_cap: none is written.
struct d_joint_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* ukey, const uint32_t* ustart, const uint32_t* uend, const uint32_t* total, const uint32_t* vals, const uint32_t* rec,
                               const f3ds_region_shape* shapes, f3ds_joint_params prm, int kb, uint32_t rec_cap, uint32_t* head, f3ds_region_joint* rows, uint64_t row_cap) const {
        if (head[1] || head[2] > rec_cap) return;      // a label out of range, or records that did not fit: the rows stay as they are
        __shared__ rg_u64 s_sum[2];
        __shared__ uint32_t s_surface;
        if (threadIdx.x < 2u) s_sum[threadIdx.x] = 0ull;
        if (threadIdx.x == 2u) s_surface = 0u;
        __syncthreads();
        const uint32_t n = *total, waves = gridDim.x * (blockDim.x >> 6);
        const bool write = rows != nullptr && (uint64_t)n <= row_cap;
        const uint64_t bmask = (1ull << kb) - 1ull;
        uint64_t pairs = 0ull, close = 0ull;      // (lane 0's count)
        uint32_t surface = 0u;
        for (uint32_t e = BIX * (blockDim.x >> 6) + (threadIdx.x >> 6); e < n; e += waves) {      // (wave-uniform)
            JtAcc acc;
            jt_empty(acc);
            for (uint32_t r = ustart[e] + (uint32_t)lane_id(), r1 = uend[e]; r < r1; r += 64u) {
                const uint2* w = reinterpret_cast<const uint2*>(rec + (size_t)vals[r] * JT_WORDS);
                const uint2 c = w[0];
                acc.n_pairs += c.x; acc.n_close += c.y;
#pragma unroll
                for (int f = 0; f < SH_S; ++f) { const uint2 t = w[2 + f]; acc.sh.s[f] += ((uint64_t)t.y << 32) | t.x; }
            }
            acc.n_pairs = rg_wave_u32(acc.n_pairs, RgAdd{});
            acc.n_close = rg_wave_u32(acc.n_close, RgAdd{});
            acc.sh.n = 2u * acc.n_close;      // (two samples a close pair: what every record's word [2] adds up to)
            if (acc.n_close != 0u) {      // (wave-uniform)
#pragma unroll
                for (int f = 0; f < SH_S; ++f) acc.sh.s[f] = rg_wave_add_u64(acc.sh.s[f]);
            }
            if (lane_id() == 0) {
                const uint64_t k = ukey[e];
                const uint32_t ra = (uint32_t)(k >> kb), rb = (uint32_t)(k & bmask);
                if (write) jt_finish(ra, rb, acc, shapes[ra], shapes[rb], prm, &rows[e]);
                pairs += acc.n_pairs; close += acc.n_close; surface += acc.n_close != 0u ? 1u : 0u;
            }
        }
        if (lane_id() == 0) {
            if (pairs) atomicAdd(&s_sum[0], (rg_u64)pairs);
            if (close) atomicAdd(&s_sum[1], (rg_u64)close);
            if (surface) atomicAdd(&s_surface, surface);
        }
        __syncthreads();
        if (threadIdx.x == 0u) {
            if (s_sum[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_sum[0]);
            if (s_sum[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 6), s_sum[1]);
            if (s_surface) atomicAdd(&head[3], s_surface);
            if (BIX == 0u) head[0] = n;
        }
    }
};
