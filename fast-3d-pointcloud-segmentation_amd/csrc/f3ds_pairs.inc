// f3ds_pairs.inc -- the skeleton of the per-PAIR region calls: the region contacts (f3ds_contacts.inc, DESIGN.md section 19) and the region joints
// (f3ds_joints.inc, section 24) are two rules over it, as the table, the shapes and the boxes are rules over label_accum_span / label_finish (f3ds_regions.inc).
// Included by f3ds_hip.hip after f3ds_regions.inc, before f3ds_contacts.inc.
//
//   d_pair_init       the record keys become holes, the record indices 0, 1, 2, ..., the head its zeros
//   pair_accum_span   a workgroup takes a CONTIGUOUS span of pixels (as d_region_accum: a span of a coherent label image meets few distinct pairs).  A lane
//                     reads its pixel's label and the labels to the right and below; only where labels differ are depths read at all, and a wave without such a
//                     pixel -- most waves -- goes on after ONE ballot.  What a pair adds goes into an LDS table keyed by (a, b); at the end of the span the
//                     occupied slots are APPENDED as records (key, Rule::WORDS words) to the record buffer: one atomic per workgroup reserves the range.  A pair
//                     that finds no slot is appended as a record of its own, one atomic per wave.  No global atomic per pixel or per pair onto a few words
//                     (DESIGN.md sections 17, 18).
//   (the radix sort of the record keys with the record index as value, d_evl_heads and the scan of its flags, d_track_runs: run e = the e-th distinct key)
//   pair_finish       one wave per run: its records merged (exact) and wave-reduced, lane 0 writes the row in (a, b) order, the sums and the row count into the
//                     head; nothing but the head when a label was out of range or the records did not fit (the host then runs the frame again with room for all)
// A RULE says what the accumulator of a pair of regions is (ContactRule, JointRule), all of it at compile time:
//   Acc, Table, Row, Point                       the accumulator, the LDS table of a workgroup (rg_u64 key[SLOTS] and the accumulator's fields, field-major), the row
//                                                a run becomes, what a border lane knows of its own pixel besides the depth (the joints: its point in space)
//   SLOT_BITS, SLOTS, BLOCK, WORDS               the table's size, the accumulate kernel's block (slot k is thread k's at the flush), the words of a record
//   empty(acc), table_reset(tab, slot)           the empty values, in registers and in LDS
//   point(a, u, v, z, P)                         P of a lane with a contact pair, once for both directions
//   pair(a, p, horizontal, u, v, lp, zp, P, lq, zq, ra, rb, acc)    what one contact pair adds to its (ra, rb); the neighbour is (u + 1, v) or (u, v + 1)
//   wave_sum(acc, m)                             the accumulators of a wave with one key into one, m = the ballot of its lanes with a pair; the others hold empty()
//   lds_add, table_get, put, get                 an accumulator into a slot, out of a slot, into the words of a record, out of them
//   merge, wave_merge(acc)                       a += b; the accumulators of a wave's lanes into one in the finish
//   pairs(acc), close(acc), SURFACE              the counts that go into head words 4 ... 7; SURFACE: the rows with a close pair are counted into head[3]
//   finish(ra, rb, acc, row)                     the rule's own (ct_finish, jt_finish); not static: the joints' rule carries the shape rows and the parameters
// The head (LI_HEAD_WORDS, f3ds_label_image.h): [0] rows, [1] 1 if a label was >= K, [2] records asked for (more than rec_cap: nothing else holds), [3] rows with a
// close pair (SURFACE; else spare), [4..5] contact pairs (u64), [6..7] close ones (u64).
// Every field that meets more than one pixel is a count, a minimum or an integer sum: arrival order does not matter, so integer atomics in LDS give the bits of
// the host functions.  No float atomics.

struct PairArgs {
    uint32_t width, height, n;         // n = width * height
    uint32_t depth_pitch;              // bytes per row (never 0 here)
    int depth_f32;
    uint32_t K;                        // regions
    int kb;                            // ct_bits(K)
    uint32_t rec_cap;                  // records the buffers hold
    float depth_scale, depth_tol, fx, fy, cx, cy;
};
constexpr int PAIR_PROBES = 8;         // a pair that finds neither its slot nor a free one in this many steps becomes a record of its own

struct d_pair_init {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint64_t* keys, uint32_t* vals, uint32_t rec_cap, uint32_t* head) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < rec_cap; i += gridDim.x * blockDim.x) { keys[i] = CT_NO_KEY; vals[i] = i; }
        if (BIX == 0u && threadIdx.x < LI_HEAD_WORDS) head[threadIdx.x] = 0u;
    }
};

// the slot of a key, claimed on the way if it is new; -1: none within PAIR_PROBES steps (slots are never given back within a span: as li_slot)
template <int SLOT_BITS>
__device__ __forceinline__ int pair_slot(rg_u64* keys, uint64_t key) {
    uint32_t h = ((uint32_t)(key ^ (key >> 29)) * 0x9E3779B1u) >> (32 - SLOT_BITS);
    for (int k = 0; k < PAIR_PROBES; ++k) {
        const rg_u64 old = atomicCAS(&keys[h], (rg_u64)CT_NO_KEY, (rg_u64)key);
        if (old == (rg_u64)CT_NO_KEY || old == (rg_u64)key) return (int)h;
        h = (h + 1u) & (uint32_t)((1 << SLOT_BITS) - 1);
    }
    return -1;
}
template <class Rule>
__device__ __forceinline__ void pair_record(uint64_t* keys, uint32_t* rec, uint32_t pos, uint64_t key, const typename Rule::Acc& acc) {
    keys[pos] = key;
    Rule::put(rec + (size_t)pos * Rule::WORDS, acc);
}

// What a wave does with the pairs of one direction (horizontal: a lane's pixel and its right neighbour; else its lower one); has: this lane has a contact pair.
// Called behind a wave-uniform branch: every lane of the wave is here.
template <class Rule>
__device__ __forceinline__ void pair_direction(bool has, bool horizontal, uint32_t i, uint32_t u, uint32_t v, uint32_t l, float z, const typename Rule::Point& P, uint32_t lq, float zq,
                                               const PairArgs& a, uint64_t* keys, uint32_t* rec, uint32_t* head, typename Rule::Table& tab) {
    const uint64_t m = __ballot(has);
    if (m == 0ull) return;
    typename Rule::Acc one;
    Rule::empty(one);
    uint64_t key = CT_NO_KEY;
    if (has) { uint32_t ra, rb; Rule::pair(a, i, horizontal, u, v, l, z, P, lq, zq, ra, rb, one); key = ct_key(ra, rb, a.kb); }
    bool send = has;
    // one pair of regions in the wave (the usual case along a border): reduce across the wave -- the lanes without a contact hold the empty values -- and
    // lane 0 sends the sum; otherwise every lane with a contact sends its own
    const int first = (int)__builtin_ctzll(m);
    const uint64_t key0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), first) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, first);
    if ((m & (m - 1ull)) != 0ull && __ballot(has && key != key0) == 0ull) {
        Rule::wave_sum(one, m);
        key = key0; send = lane_id() == 0;
    }
    int slot = -1;
    if (send) { slot = pair_slot<Rule::SLOT_BITS>(tab.key, key); if (slot >= 0) Rule::lds_add(tab, slot, one); }
    const uint64_t over = __ballot(send && slot < 0);
    if (over != 0ull) {      // the table is full around these keys: records of their own, one reservation per wave
        const int lead = (int)__builtin_ctzll(over);
        uint32_t at = 0u;
        if (lane_id() == lead) at = atomicAdd(&head[2], (uint32_t)__popcll(over));
        at = (uint32_t)__builtin_amdgcn_readlane((int)at, lead);
        if (send && slot < 0) {
            const uint64_t pos = (uint64_t)at + (uint32_t)__popcll(over & lanemask_lt());
            if (pos < a.rec_cap) pair_record<Rule>(keys, rec, (uint32_t)pos, key, one);
        }
    }
}

// Span of workgroup b: [b * span, min(n, (b + 1) * span)), span = ceil(n / gridDim.x) rounded up to a multiple of the block (as label_accum_span): every lane of
// the workgroup makes the same number of trips, so the ballots and barriers below are uniform.  A pixel's right and lower neighbours are read wherever they
// lie: in the next lane's pixel, in another trip or in another workgroup's span -- the pair belongs to its first pixel.
template <class Rule, bool DEPTH_F32>
__device__ __forceinline__ void pair_accum_span(const unsigned char* depth, const uint32_t* label, const PairArgs& a, uint64_t* keys, uint32_t* rec, uint32_t* head,
                                                typename Rule::Table& tab, uint32_t* s_base) {
    static_assert(Rule::SLOTS <= Rule::BLOCK, "slot k is thread k's at the flush");
    for (uint32_t k = threadIdx.x; k < (uint32_t)Rule::SLOTS; k += blockDim.x) { tab.key[k] = (rg_u64)CT_NO_KEY; Rule::table_reset(tab, k); }
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
        if (__ballot(hr || hd) != 0ull) {      // (wave-uniform, and so are the branches on ballots in pair_direction)  Inside a region no depth is read.
            float z = 0.0f, zr = 0.0f, zd = 0.0f;
            const bool valid = (hr || hd) && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v, z);
            hr = hr && valid && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u + 1u, v, zr);
            hd = hd && valid && li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v + 1u, zd);
            typename Rule::Point P = {};
            if (hr || hd) Rule::point(a, u, v, z, P);
            pair_direction<Rule>(hr, true, i, u, v, l, z, P, lr, zr, a, keys, rec, head, tab);
            pair_direction<Rule>(hd, false, i, u, v, l, z, P, ld, zd, a, keys, rec, head, tab);
        }
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
    if (bad) head[1] = 1u;      // (every writer stores the same word)
    __syncthreads();
    // the occupied slots become records: slot k is thread k's, the positions from a scan of the occupancy
    const bool mine = Rule::SLOTS == Rule::BLOCK || threadIdx.x < (uint32_t)Rule::SLOTS;
    const uint64_t key = mine ? (uint64_t)tab.key[threadIdx.x] : CT_NO_KEY;
    const uint32_t occ = key != CT_NO_KEY ? 1u : 0u;
    uint32_t total;
    const uint32_t incl = block_incl_scan<Rule::BLOCK>(occ, &total);
    if (threadIdx.x == 0u) *s_base = total ? atomicAdd(&head[2], total) : 0u;
    __syncthreads();
    if (occ) {
        const uint64_t pos = (uint64_t)*s_base + incl - 1u;
        if (pos < a.rec_cap) {
            typename Rule::Acc t;
            Rule::table_get(tab, (int)threadIdx.x, t);
            pair_record<Rule>(keys, rec, (uint32_t)pos, key, t);
        }
    }
}

// One wave per run of equal keys in the sorted records (ukey, ustart, uend, *total: d_track_runs); vals: the record indices in sorted order.  rows may be null
// (a count-only call); more rows than row_cap: none is written.
template <class Rule>
__device__ __forceinline__ void pair_finish(const Rule& rule, const uint64_t* ukey, const uint32_t* ustart, const uint32_t* uend, const uint32_t* total, const uint32_t* vals,
                                            const uint32_t* rec, int kb, uint32_t rec_cap, uint32_t* head, typename Rule::Row* rows, uint64_t row_cap) {
    if (head[1] || head[2] > rec_cap) return;      // a label out of range, or records that did not fit: the rows stay as they are
    __shared__ rg_u64 s_sum[2];
    __shared__ uint32_t s_surface;      // (SURFACE only: without a use it takes no LDS)
    if (threadIdx.x < 2u) s_sum[threadIdx.x] = 0ull;
    if constexpr (Rule::SURFACE) { if (threadIdx.x == 2u) s_surface = 0u; }
    __syncthreads();
    const uint32_t n = *total, waves = gridDim.x * (blockDim.x >> 6);
    const bool write = rows != nullptr && (uint64_t)n <= row_cap;
    const uint64_t bmask = (1ull << kb) - 1ull;
    uint64_t pairs = 0ull, close = 0ull;      // (lane 0's count)
    uint32_t surface = 0u;
    for (uint32_t e = BIX * (blockDim.x >> 6) + (threadIdx.x >> 6); e < n; e += waves) {      // (wave-uniform)
        typename Rule::Acc acc;
        Rule::empty(acc);
        for (uint32_t r = ustart[e] + (uint32_t)lane_id(), r1 = uend[e]; r < r1; r += 64u) {
            typename Rule::Acc t;
            Rule::get(rec + (size_t)vals[r] * Rule::WORDS, t);
            Rule::merge(acc, t);
        }
        Rule::wave_merge(acc);
        if (lane_id() == 0) {
            const uint64_t k = ukey[e];
            if (write) rule.finish((uint32_t)(k >> kb), (uint32_t)(k & bmask), acc, &rows[e]);
            pairs += Rule::pairs(acc); close += Rule::close(acc);
            if constexpr (Rule::SURFACE) surface += Rule::close(acc) != 0u ? 1u : 0u;
        }
    }
    if (lane_id() == 0) {
        if (pairs) atomicAdd(&s_sum[0], (rg_u64)pairs);
        if (close) atomicAdd(&s_sum[1], (rg_u64)close);
        if constexpr (Rule::SURFACE) { if (surface) atomicAdd(&s_surface, surface); }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        if (s_sum[0]) atomicAdd(reinterpret_cast<rg_u64*>(head + 4), s_sum[0]);
        if (s_sum[1]) atomicAdd(reinterpret_cast<rg_u64*>(head + 6), s_sum[1]);
        if constexpr (Rule::SURFACE) { if (s_surface) atomicAdd(&head[3], s_surface); }
        if (BIX == 0u) head[0] = n;
    }
}
