// f3ds_contacts.inc -- the device path of the region contacts (f3ds_region_contacts, include/f3ds.h; the rules are in f3ds_contacts.h; DESIGN.md section 19).
// Included by f3ds_hip.hip after f3ds_regions.inc.
//
//   d_contact_init    the record keys become holes, the record indices 0, 1, 2, ..., the head its zeros
//   d_contact_accum   a workgroup takes a CONTIGUOUS span of pixels (as d_region_accum: a span of a coherent label image meets few distinct pairs).  A lane
//                     reads its pixel's label and the labels to the right and below; only where labels differ are depths read at all, and a wave without such a
//                     pixel -- most waves -- goes on after ONE ballot.  Contacts go into an LDS table keyed by (a, b); at the end of the span the occupied slots
//                     are APPENDED as records (key, seven words) to the record buffer: one atomic per workgroup reserves the range.  A pair that finds no slot
//                     is appended as a record of its own, one atomic per wave.  No global atomic per pixel or per pair onto a few words (DESIGN.md sections 17, 18).
//   (the radix sort of the record keys with the record index as value, d_evl_heads and the scan of its flags, d_track_runs: run e = the e-th distinct key)
//   d_contact_finish  one wave per run: its records merged (ct_merge: exact), the row written in (a, b) order (ct_finish), the sums and the row count into the head;
//                     nothing but the head when a label was out of range or the records did not fit (the host then runs the frame again with room for all)
// Every field is a count, a minimum or an integer sum (f3ds_contacts.h): arrival order does not matter, so integer atomics in LDS give the bits of the host
// function.  No float atomics.

struct ContactArgs {
    uint32_t width, height, n;         // n = width * height
    uint32_t depth_pitch;              // bytes per row (never 0 here)
    int depth_f32;
    uint32_t K;                        // regions
    int kb;                            // ct_bits(K)
    uint32_t rec_cap;                  // records the buffers hold
    float depth_scale, depth_tol;
};
// the head (LI_HEAD_WORDS, f3ds_label_image.h): [0] rows, [1] 1 if a label was >= K, [2] records asked for (more than rec_cap: nothing else holds), [3] spare, [4..5] contact pairs (u64), [6..7] close ones (u64)
constexpr int RGC_SLOT_BITS = 8, RGC_SLOTS = 1 << RGC_SLOT_BITS;      // LDS table: 256 slots of a key + a CtAcc (36 B), 9 KiB; slot k is thread k's at the flush
constexpr int RGC_PROBES = 8;          // a pair that finds neither its slot nor a free one in this many steps becomes a record of its own
constexpr uint32_t RGC_TRIPS = 8;      // trips of a workgroup the grid is sized for: longer spans, fewer records of the same pair
constexpr uint32_t RGC_FIRST_CAP = 32768;      // records the first run has room for (a coherent 1M-pixel frame has a few thousand); F3DS_RGC_FIRST_CAP (development) replaces it
constexpr uint32_t RGC_FIRST_ROWS = 2048;      // rows of a host caller that ride with the head; a frame with more gets a second download

struct d_contact_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint64_t* keys, uint32_t* vals, uint32_t rec_cap, uint32_t* head) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < rec_cap; i += gridDim.x * blockDim.x) { keys[i] = CT_NO_KEY; vals[i] = i; }
        if (BIX == 0u && threadIdx.x < LI_HEAD_WORDS) head[threadIdx.x] = 0u;
    }
};

// the LDS table of a workgroup: field-major, as RgTable
struct CtTable { rg_u64 key[RGC_SLOTS]; uint32_t w[CT_W][RGC_SLOTS]; rg_u64 s[RGC_SLOTS]; };

// the slot of a key, claimed on the way if it is new; -1: none within RGC_PROBES steps (slots are never given back within a span: as li_slot)
__device__ __forceinline__ int ct_slot(CtTable& t, uint64_t key) {
    uint32_t h = ((uint32_t)(key ^ (key >> 29)) * 0x9E3779B1u) >> (32 - RGC_SLOT_BITS);
    for (int k = 0; k < RGC_PROBES; ++k) {
        const rg_u64 old = atomicCAS(&t.key[h], (rg_u64)CT_NO_KEY, (rg_u64)key);
        if (old == (rg_u64)CT_NO_KEY || old == (rg_u64)key) return (int)h;
        h = (h + 1u) & (uint32_t)(RGC_SLOTS - 1);
    }
    return -1;
}
__device__ __forceinline__ void ct_lds_add(CtTable& t, int slot, const CtAcc& a) {
#pragma unroll
    for (int k = 0; k < 4; ++k) if (a.w[k]) atomicAdd(&t.w[k][slot], a.w[k]);
    atomicMin(&t.w[4][slot], a.w[4]);
    atomicAdd(&t.s[slot], (rg_u64)a.s);
}
__device__ __forceinline__ void ct_record(uint64_t* keys, uint32_t* rec, uint32_t pos, uint64_t key, const CtAcc& a) {
    keys[pos] = key;
    uint32_t* r = rec + (size_t)pos * CT_WORDS;
#pragma unroll
    for (int k = 0; k < CT_W; ++k) r[k] = a.w[k];
    r[CT_W] = (uint32_t)a.s; r[CT_W + 1] = (uint32_t)(a.s >> 32);
}

// Span of workgroup b: [b * span, min(n, (b + 1) * span)), span = ceil(n / gridDim.x) rounded up to a multiple of the block (as label_accum_span): every lane of
// the workgroup makes the same number of trips, so the ballots and barriers below are uniform.  A pixel's right and lower neighbours are read wherever they
// lie: in the next lane's pixel, in another trip or in another workgroup's span -- the pair belongs to its first pixel.
template <bool DEPTH_F32>
__device__ __forceinline__ void contact_accum_span(const unsigned char* depth, const uint32_t* label, const ContactArgs& a, uint64_t* keys, uint32_t* rec, uint32_t* head,
                                                   CtTable& tab, uint32_t* s_base) {
    for (uint32_t k = threadIdx.x; k < (uint32_t)RGC_SLOTS; k += blockDim.x) {
        tab.key[k] = (rg_u64)CT_NO_KEY;
#pragma unroll
        for (int f = 0; f < 4; ++f) tab.w[f][k] = 0u;
        tab.w[4][k] = CT_NONE;
        tab.s[k] = 0ull;
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
        uint32_t l = CT_NONE, lq[2] = {CT_NONE, CT_NONE};      // this pixel's label, its right and its lower neighbour's
        if (i < end) {
            l = label[i];
            if (u + 1u < a.width) lq[0] = label[i + 1u];
            if (v + 1u < a.height) lq[1] = label[i + a.width];      // (i + width < n: v + 1 < height)
        }
        bad = bad || (l != CT_NONE && l >= a.K);
        bool has[2];      // (K <= CT_MAX_REGIONS: CT_NONE is never below it)
        has[0] = l < a.K && lq[0] < a.K && lq[0] != l;
        has[1] = l < a.K && lq[1] < a.K && lq[1] != l;
        if (__ballot(has[0] || has[1]) != 0ull) {      // (wave-uniform, and so are the branches on ballots below)  Inside a region no depth is read.
            float z = 0.0f, zq[2] = {0.0f, 0.0f};
            const bool valid = (has[0] || has[1]) && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v, z);
            has[0] = has[0] && valid && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u + 1u, v, zq[0]);
            has[1] = has[1] && valid && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v + 1u, zq[1]);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint64_t m = __ballot(has[k]);
                if (m == 0ull) continue;
                CtAcc one;
                ct_empty(one);
                uint64_t key = CT_NO_KEY;
                if (has[k]) { uint32_t pa, pb; ct_pair(i, k == 0, l, z, lq[k], zq[k], a.depth_tol, pa, pb, one); key = ct_key(pa, pb, a.kb); }
                bool send = has[k];
                // one pair of regions in the wave (the usual case along a border): reduce across the wave -- the lanes without a contact hold the empty
                // values -- and lane 0 sends the sum; otherwise every lane with a contact sends its own
                const int first = (int)__builtin_ctzll(m);
                const uint64_t key0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), first) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, first);
                if ((m & (m - 1ull)) != 0ull && __ballot(has[k] && key != key0) == 0ull) {
#pragma unroll
                    for (int f = 0; f < 4; ++f) one.w[f] = rg_wave_u32(one.w[f], RgAdd{});
                    one.w[4] = rg_wave_u32(one.w[4], RgMin{});
                    one.s = rg_wave_add_u64(one.s);
                    key = key0; send = lane_id() == 0;
                }
                int slot = -1;
                if (send) { slot = ct_slot(tab, key); if (slot >= 0) ct_lds_add(tab, slot, one); }
                const uint64_t over = __ballot(send && slot < 0);
                if (over != 0ull) {      // the table is full around these keys: records of their own, one reservation per wave
                    const int lead = (int)__builtin_ctzll(over);
                    uint32_t at = 0u;
                    if (lane_id() == lead) at = atomicAdd(&head[2], (uint32_t)__popcll(over));
                    at = (uint32_t)__builtin_amdgcn_readlane((int)at, lead);
                    if (send && slot < 0) {
                        const uint64_t pos = (uint64_t)at + (uint32_t)__popcll(over & lanemask_lt());
                        if (pos < a.rec_cap) ct_record(keys, rec, (uint32_t)pos, key, one);
                    }
                }
            }
        }
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
    __syncthreads();
    // the occupied slots become records: slot k is thread k's (RGC_SLOTS == BLOCK), the positions from a scan of the occupancy
    const uint64_t key = tab.key[threadIdx.x];
    const uint32_t occ = key != CT_NO_KEY ? 1u : 0u;
    uint32_t total;
    const uint32_t incl = block_incl_scan<RGC_SLOTS>(occ, &total);
    if (threadIdx.x == 0u) *s_base = total ? atomicAdd(&head[2], total) : 0u;
    __syncthreads();
    if (occ) {
        const uint64_t pos = (uint64_t)*s_base + incl - 1u;
        if (pos < a.rec_cap) {
            CtAcc t;
#pragma unroll
            for (int f = 0; f < CT_W; ++f) t.w[f] = tab.w[f][threadIdx.x];
            t.s = tab.s[threadIdx.x];
            ct_record(keys, rec, (uint32_t)pos, key, t);
        }
    }
}
struct d_contact_accum {
    static constexpr int BLOCK = RGC_SLOTS;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, ContactArgs a, uint64_t* keys, uint32_t* rec, uint32_t* head) const {
        __shared__ CtTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ uint32_t s_base;
        if (a.depth_f32) contact_accum_span<true>(depth, label, a, keys, rec, head, tab, &s_base);
        else contact_accum_span<false>(depth, label, a, keys, rec, head, tab, &s_base);
    }
};

// One wave per run of equal keys in the sorted records (ukey, ustart, uend, *total: d_track_runs); vals: the record indices in sorted order.  rows may be null
// (a count-only call); more rows than row_cap: none is written.
struct d_contact_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* ukey, const uint32_t* ustart, const uint32_t* uend, const uint32_t* total, const uint32_t* vals, const uint32_t* rec,
                               int kb, uint32_t rec_cap, uint32_t* head, f3ds_region_contact* rows, uint64_t row_cap) const {
        if (head[1] || head[2] > rec_cap) return;      // a label out of range, or records that did not fit: the rows stay as they are
        __shared__ rg_u64 s_sum[2];
        if (threadIdx.x < 2u) s_sum[threadIdx.x] = 0ull;
        __syncthreads();
        const uint32_t n = *total, waves = gridDim.x * (blockDim.x >> 6);
        const bool write = rows != nullptr && (uint64_t)n <= row_cap;
        const uint64_t bmask = (1ull << kb) - 1ull;
        uint64_t pairs = 0ull, close = 0ull;      // (lane 0's count)
        for (uint32_t e = BIX * (blockDim.x >> 6) + (threadIdx.x >> 6); e < n; e += waves) {      // (wave-uniform)
            CtAcc acc;
            ct_empty(acc);
            for (uint32_t r = ustart[e] + (uint32_t)lane_id(), r1 = uend[e]; r < r1; r += 64u) {
                const uint32_t* w = rec + (size_t)vals[r] * CT_WORDS;
                CtAcc t;
#pragma unroll
                for (int f = 0; f < CT_W; ++f) t.w[f] = w[f];
                t.s = ((uint64_t)w[CT_W + 1] << 32) | w[CT_W];
                ct_merge(acc, t);
            }
#pragma unroll
            for (int f = 0; f < 4; ++f) acc.w[f] = rg_wave_u32(acc.w[f], RgAdd{});
            acc.w[4] = rg_wave_u32(acc.w[4], RgMin{});
            acc.s = rg_wave_add_u64(acc.s);
            if (lane_id() == 0) {
                const uint64_t k = ukey[e];
                if (write) ct_finish((uint32_t)(k >> kb), (uint32_t)(k & bmask), acc, &rows[e]);
                pairs += acc.w[0]; close += acc.w[1];
            }
        }
        if (lane_id() == 0) { if (pairs) atomicAdd(&s_sum[0], (rg_u64)pairs); if (close) atomicAdd(&s_sum[1], (rg_u64)close); }
        __syncthreads();
        if (threadIdx.x == 0u) {
            if (s_sum[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_sum[0]);
            if (s_sum[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 6), s_sum[1]);
            if (BIX == 0u) head[0] = n;
        }
    }
};
