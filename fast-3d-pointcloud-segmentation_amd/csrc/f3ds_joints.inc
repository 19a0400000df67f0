// f3ds_joints.inc -- the device path of the region joints (f3ds_region_joints, include/f3ds.h; the rules are in f3ds_joints.h; DESIGN.md section 24): JointRule
// over the pair skeleton (f3ds_pairs.inc, which describes the kernels, the records and the head).
// Included by f3ds_hip.hip after f3ds_boxes.inc.  In front of these kernels the call records the three kernels of the shapes as they are (f3ds_shapes.inc).
//
//   d_pair_init      (f3ds_pairs.inc)
//   d_joint_accum    pair_accum_span over JointRule: a border lane deprojects its own pixel and the neighbour's; a CLOSE pair adds two sh_pixel contributions
//                    (f3ds_shapes.h) to the LDS slot of its (a, b), next to the contacts' two counts.  A record is a key and 34 words.
//   (the radix sort of the record keys with the record index as value, d_evl_heads and the scan of its flags, d_track_runs: run e = the e-th distinct key)
//   d_joint_finish   pair_finish over JointRule: jt_merge, and lane 0 runs jt_finish -- sh_finish on the samples and the join with shapes[a] and shapes[b], the
//                    K shape rows d_shape_finish wrote earlier in the same flush; the rows with a close pair are counted into head[3] (n_surface)
// Every field that meets more than one pixel is a count or a sum of 64-bit integers: arrival order does not matter, so integer atomics in LDS (ds_add_u64)
// give the bits of the host function.  No float atomics.

constexpr int RGJ_SLOT_BITS = 7, RGJ_SLOTS = 1 << RGJ_SLOT_BITS;      // LDS table: 128 slots of a key, two counts and fifteen sums (136 B), 17 KiB (DESIGN.md section 24: why not 256)
constexpr int RGJ_BLOCK = 256;
constexpr uint32_t RGJ_TRIPS = 8;      // trips of a workgroup the grid is sized for (the contacts' figure)
constexpr uint32_t RGJ_FIRST_CAP = 32768;      // records the first run has room for (4.3 MiB); F3DS_RGJ_FIRST_CAP (development) replaces it
constexpr uint32_t RGJ_FIRST_ROWS = 2048;      // rows of a host caller that ride with the head; a frame with more gets a second download

// the LDS table of a workgroup: field-major, as CtTable and ShTable
struct JtTable { rg_u64 key[RGJ_SLOTS]; uint32_t w[2][RGJ_SLOTS]; rg_u64 s[SH_S][RGJ_SLOTS]; };

struct JointRule {
    using Acc = JtAcc; using Table = JtTable; using Row = f3ds_region_joint;
    struct Point { float p[3]; };      // the lane's own pixel in space
    static constexpr int SLOT_BITS = RGJ_SLOT_BITS, SLOTS = RGJ_SLOTS, BLOCK = RGJ_BLOCK, WORDS = JT_WORDS;
    static constexpr bool SURFACE = true;
    const f3ds_region_shape* shapes; f3ds_joint_params prm;      // (the finish only)
    __device__ static void empty(JtAcc& a) { jt_empty(a); }
    __device__ static void table_reset(JtTable& t, uint32_t k) {
        t.w[0][k] = t.w[1][k] = 0u;
#pragma unroll
        for (int f = 0; f < SH_S; ++f) t.s[f][k] = 0ull;
    }
    __device__ static void point(const PairArgs& a, uint32_t u, uint32_t v, float z, Point& P) { n_deproject(u, v, true, z, a.fx, a.fy, a.cx, a.cy, P.p[0], P.p[1], P.p[2]); }
    __device__ static void pair(const PairArgs& a, uint32_t p, bool horizontal, uint32_t u, uint32_t v, uint32_t lp, float zp, const Point& P, uint32_t lq, float zq, uint32_t& ra,
                                uint32_t& rb, JtAcc& acc) {
        float Q[3];
        n_deproject(horizontal ? u + 1u : u, horizontal ? v : v + 1u, true, zq, a.fx, a.fy, a.cx, a.cy, Q[0], Q[1], Q[2]);
        jt_pair(p, horizontal, lp, zp, lq, zq, a.depth_tol, P.p, Q, ra, rb, acc);
    }
    // every lane with a pair holds n_pairs = 1 and n_close = 0 or 1: the counts are popcounts, and the fifteen 64-bit reductions are paid only where some
    // pair is close
    __device__ static void wave_sum(JtAcc& a, uint64_t m) {
        a.n_pairs = (uint32_t)__popcll(m);
        const uint64_t cm = __ballot(a.n_close != 0u);
        a.n_close = (uint32_t)__popcll(cm);
        a.sh.n = 2u * a.n_close;
        if (cm != 0ull) {
#pragma unroll
            for (int f = 0; f < SH_S; ++f) a.sh.s[f] = rg_wave_add_u64(a.sh.s[f]);
        }
    }
    __device__ static void wave_merge(JtAcc& a) {
        a.n_pairs = rg_wave_u32(a.n_pairs, RgAdd{});
        a.n_close = rg_wave_u32(a.n_close, RgAdd{});
        a.sh.n = 2u * a.n_close;      // (two samples a close pair: what every record's word [2] adds up to)
        if (a.n_close != 0u) {      // (wave-uniform)
#pragma unroll
            for (int f = 0; f < SH_S; ++f) a.sh.s[f] = rg_wave_add_u64(a.sh.s[f]);
        }
    }
    // a into its slot; a pair that is not close has no sample: one atomic
    __device__ static void lds_add(JtTable& t, int slot, const JtAcc& a) {
        atomicAdd(&t.w[0][slot], a.n_pairs);
        if (a.n_close == 0u) return;
        atomicAdd(&t.w[1][slot], a.n_close);
#pragma unroll
        for (int k = 0; k < SH_S; ++k) atomicAdd(&t.s[k][slot], (rg_u64)a.sh.s[k]);
    }
    __device__ static void table_get(const JtTable& t, int slot, JtAcc& a) {
        a.n_pairs = t.w[0][slot]; a.n_close = t.w[1][slot]; a.sh.n = 2u * a.n_close; a.sh.pad = 0u;
#pragma unroll
        for (int f = 0; f < SH_S; ++f) a.sh.s[f] = t.s[f][slot];
    }
    // the record of jt_to_words / jt_from_words, as 8-byte words (JT_WORDS * 4 is a multiple of 8)
    __device__ static void put(uint32_t* rec, const JtAcc& a) {
        uint2* r = reinterpret_cast<uint2*>(rec);
        r[0] = make_uint2(a.n_pairs, a.n_close); r[1] = make_uint2(a.sh.n, 0u);
#pragma unroll
        for (int k = 0; k < SH_S; ++k) r[2 + k] = make_uint2((uint32_t)a.sh.s[k], (uint32_t)(a.sh.s[k] >> 32));
    }
    __device__ static void get(const uint32_t* rec, JtAcc& a) {
        const uint2* r = reinterpret_cast<const uint2*>(rec);
        const uint2 c = r[0];
        a.n_pairs = c.x; a.n_close = c.y; a.sh.n = 2u * c.y; a.sh.pad = 0u;      // (word [2] is 2 * n_close: not read)
#pragma unroll
        for (int f = 0; f < SH_S; ++f) { const uint2 t = r[2 + f]; a.sh.s[f] = ((uint64_t)t.y << 32) | t.x; }
    }
    __device__ static void merge(JtAcc& a, const JtAcc& b) { jt_merge(a, b); }
    __device__ static uint32_t pairs(const JtAcc& a) { return a.n_pairs; }
    __device__ static uint32_t close(const JtAcc& a) { return a.n_close; }
    __device__ void finish(uint32_t ra, uint32_t rb, const JtAcc& a, f3ds_region_joint* row) const { jt_finish(ra, rb, a, shapes[ra], shapes[rb], prm, row); }
};

struct d_joint_accum {
    static constexpr int BLOCK = RGJ_BLOCK;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, PairArgs a, uint64_t* keys, uint32_t* rec, uint32_t* head) const {
        __shared__ JtTable tab;      // (here and not in the template: one table for the kernel, not one per instantiation)
        __shared__ uint32_t s_base;
        if (a.depth_f32) pair_accum_span<JointRule, true>(depth, label, a, keys, rec, head, tab, &s_base);
        else pair_accum_span<JointRule, false>(depth, label, a, keys, rec, head, tab, &s_base);
    }
};
struct d_joint_finish {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* ukey, const uint32_t* ustart, const uint32_t* uend, const uint32_t* total, const uint32_t* vals, const uint32_t* rec,
                               const f3ds_region_shape* shapes, f3ds_joint_params prm, int kb, uint32_t rec_cap, uint32_t* head, f3ds_region_joint* rows, uint64_t row_cap) const {
        pair_finish<JointRule>(JointRule{shapes, prm}, ukey, ustart, uend, total, vals, rec, kb, rec_cap, head, rows, row_cap);
    }
};
