// f3ds_contacts.inc -- the device path of the region contacts (f3ds_region_contacts, include/f3ds.h; the rules are in f3ds_contacts.h; DESIGN.md section 19):
// ContactRule over the pair skeleton (f3ds_pairs.inc, which describes the kernels, the records and the head).
// Included by f3ds_hip.hip after f3ds_pairs.inc.
//
//   d_pair_init       (f3ds_pairs.inc)
//   d_contact_accum   pair_accum_span over ContactRule: the one pass over the images; a record is a key and seven words
//   (the radix sort of the record keys with the record index as value, d_evl_heads and the scan of its flags, d_track_runs: run e = the e-th distinct key)
//   d_contact_finish  pair_finish over ContactRule: ct_merge, ct_finish per run
// Every field is a count, a minimum or an integer sum (f3ds_contacts.h): arrival order does not matter, so integer atomics in LDS give the bits of the host
// function.  No float atomics.

constexpr int RGC_SLOT_BITS = 8, RGC_SLOTS = 1 << RGC_SLOT_BITS;      // LDS table: 256 slots of a key + a CtAcc (36 B), 9 KiB; slot k is thread k's at the flush
constexpr uint32_t RGC_TRIPS = 8;      // trips of a workgroup the grid is sized for: longer spans, fewer records of the same pair
constexpr uint32_t RGC_FIRST_CAP = 32768;      // records the first run has room for (a coherent 1M-pixel frame has a few thousand); F3DS_RGC_FIRST_CAP (development) replaces it
constexpr uint32_t RGC_FIRST_ROWS = 2048;      // rows of a host caller that ride with the head; a frame with more gets a second download

// the LDS table of a workgroup: field-major, as RgTable
struct CtTable { rg_u64 key[RGC_SLOTS]; uint32_t w[CT_W][RGC_SLOTS]; rg_u64 s[RGC_SLOTS]; };

struct ContactRule {
    using Acc = CtAcc; using Table = CtTable; using Row = f3ds_region_contact;
    struct Point {};      // a contact needs the two depths only
    static constexpr int SLOT_BITS = RGC_SLOT_BITS, SLOTS = RGC_SLOTS, BLOCK = RGC_SLOTS, WORDS = CT_WORDS;
    static constexpr bool SURFACE = false;
    __device__ static void empty(CtAcc& a) { ct_empty(a); }
    __device__ static void table_reset(CtTable& t, uint32_t k) {
#pragma unroll
        for (int f = 0; f < 4; ++f) t.w[f][k] = 0u;
        t.w[4][k] = CT_NONE;
        t.s[k] = 0ull;
    }
    __device__ static void point(const PairArgs&, uint32_t, uint32_t, float, Point&) {}
    __device__ static void pair(const PairArgs& a, uint32_t p, bool horizontal, uint32_t, uint32_t, uint32_t lp, float zp, const Point&, uint32_t lq, float zq, uint32_t& ra,
                                uint32_t& rb, CtAcc& acc) {
        ct_pair(p, horizontal, lp, zp, lq, zq, a.depth_tol, ra, rb, acc);
    }
    __device__ static void wave_merge(CtAcc& a) {
#pragma unroll
        for (int f = 0; f < 4; ++f) a.w[f] = rg_wave_u32(a.w[f], RgAdd{});
        a.w[4] = rg_wave_u32(a.w[4], RgMin{});
        a.s = rg_wave_add_u64(a.s);
    }
    __device__ static void wave_sum(CtAcc& a, uint64_t) { wave_merge(a); }
    __device__ static void lds_add(CtTable& t, int slot, const CtAcc& a) {
#pragma unroll
        for (int k = 0; k < 4; ++k) if (a.w[k]) atomicAdd(&t.w[k][slot], a.w[k]);
        atomicMin(&t.w[4][slot], a.w[4]);
        atomicAdd(&t.s[slot], (rg_u64)a.s);
    }
    __device__ static void table_get(const CtTable& t, int slot, CtAcc& a) {
#pragma unroll
        for (int f = 0; f < CT_W; ++f) a.w[f] = t.w[f][slot];
        a.s = t.s[slot];
    }
    __device__ static void put(uint32_t* r, const CtAcc& a) {
#pragma unroll
        for (int k = 0; k < CT_W; ++k) r[k] = a.w[k];
        r[CT_W] = (uint32_t)a.s; r[CT_W + 1] = (uint32_t)(a.s >> 32);
    }
    __device__ static void get(const uint32_t* r, CtAcc& a) {
#pragma unroll
        for (int f = 0; f < CT_W; ++f) a.w[f] = r[f];
        a.s = ((uint64_t)r[CT_W + 1] << 32) | r[CT_W];
    }
    __device__ static void merge(CtAcc& a, const CtAcc& b) { ct_merge(a, b); }
    __device__ static uint32_t pairs(const CtAcc& a) { return a.w[0]; }
    __device__ static uint32_t close(const CtAcc& a) { return a.w[1]; }
    __device__ void finish(uint32_t ra, uint32_t rb, const CtAcc& a, f3ds_region_contact* row) const { ct_finish(ra, rb, a, row); }
};

struct d_contact_accum {
    static constexpr int BLOCK = RGC_SLOTS;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, PairArgs a, uint64_t* keys, uint32_t* rec, uint32_t* head) const {
        __shared__ CtTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ uint32_t s_base;
        if (a.depth_f32) pair_accum_span<ContactRule, true>(depth, label, a, keys, rec, head, tab, &s_base);
        else pair_accum_span<ContactRule, false>(depth, label, a, keys, rec, head, tab, &s_base);
    }
};
struct d_contact_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* ukey, const uint32_t* ustart, const uint32_t* uend, const uint32_t* total, const uint32_t* vals, const uint32_t* rec,
                               int kb, uint32_t rec_cap, uint32_t* head, f3ds_region_contact* rows, uint64_t row_cap) const {
        pair_finish<ContactRule>(ContactRule{}, ukey, ustart, uend, total, vals, rec, kb, rec_cap, head, rows, row_cap);
    }
};
