// f3ds_track.inc -- the device path of the label tracker (f3ds_tracker_update, include/f3ds.h; the rules are in f3ds_track.h; DESIGN.md section 17).
// Included by f3ds_hip.hip after f3ds_eval_levels.inc.
//
//   d_track_keys    one pixel per lane and trip: depth and label in, the point (n_depth_to_z / n_deproject), its place in the previous frame (tk_transform,
//                   tk_project), the vote (tk_votes: two gathers into the previous state) -> one 64-bit key per pixel, (i << jb) | j for a labelled pixel
//                   (j = Kp: a no-vote), the hole key for every other one; the pixel's new slot and depth go to the OTHER state buffer
//   (the stage-0 radix sort on the keys alone, then d_evl_heads and the scan of its flags: entry e = the e-th distinct key, in (i, j) order)
//   d_track_runs    where each entry's run of equal keys starts and ends in the sorted keys: its count is the difference.  (d_evl_reduce adds one per element
//                   with an atomic; a 1M-pixel frame has some forty entries, and a million adds onto forty words took 8 ms: DESIGN.md section 17)
//   d_track_pack    the entries as (i, j, c) triples behind a four-word head (entries, bad-label flag): what the one download of an update carries
//   d_track_apply   track_ids[p] = id[label[p]] (F3DS_NO_LABEL stays), after the host's assignment
// Every loop is a grid-stride loop over a flat index; grids come from grid_for(), so F3DS_GRID_CAP narrows them.

struct TrackArgs {
    uint32_t width, height, n;         // n = width * height
    uint32_t depth_pitch;              // bytes per depth row (never 0 here)
    int depth_f32, has_pose, has_prev; // has_prev == 0: the first update, or the one after a reset -- every labelled pixel is a no-vote and the state is not read
    uint32_t Kc, Kp;                   // regions of this frame, slots of the previous one
    int jb;                            // tk_bits(Kp)
    float depth_scale, fx, fy, cx, cy, depth_tol;
    float pose[12];
};
constexpr uint32_t TRK_HEAD = 4;       // words in front of the packed entries: [0] entries, [1] 1 if a label was >= Kc, [2] [3] spare

template <bool DEPTH_F32>
__device__ inline void track_keys_loop(const unsigned char* depth, const uint32_t* label, const uint32_t* prev_slot, const float* prev_z, const TrackArgs& a,
                                       uint64_t* keys, uint32_t* new_slot, float* new_z, uint32_t* bad_label) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t sv = stride / a.width, su = stride - sv * a.width;      // a trip moves every lane this many rows and columns on (as d_deproject)
    uint32_t i = BIX * blockDim.x + threadIdx.x;
    uint32_t v = i / a.width, u = i - v * a.width;
    const uint64_t hole = tk_hole(a.Kc, a.jb);
    for (; i < a.n; i += stride) {
        float z = 0.0f;
        const bool valid = li_read_depth<DEPTH_F32>(depth, a.depth_pitch, a.depth_scale, u, v, z);
        const uint32_t l = label[i];
        float x, y, zo;
        n_deproject(u, v, valid, z, a.fx, a.fy, a.cx, a.cy, x, y, zo);
        const bool bad = l != TK_NONE && l >= a.Kc;
        const bool labelled = valid && l < a.Kc;      // (Kc <= TK_MAX_REGIONS: TK_NONE is never below it)
        uint64_t key = hole;
        if (labelled) {
            uint32_t j = a.Kp;
            if (a.has_prev) {
                float xp, yp, zp;
                tk_transform(a.has_pose ? a.pose : nullptr, x, y, zo, xp, yp, zp);
                const int32_t q = tk_project(xp, yp, zp, a.fx, a.fy, a.cx, a.cy, a.width, a.height);
                if (q >= 0) {
                    const uint32_t s = prev_slot[q];
                    const float zq = prev_z[q];
                    if (s < a.Kp && tk_votes(s, zp, zq, a.depth_tol)) j = s;      // (s < Kp or TK_NONE: the state only ever holds checked labels)
                }
            }
            key = tk_key(l, j, a.jb);
        }
        if (bad) *bad_label = 1u;      // (every writer stores the same word)
        keys[i] = key;
        new_slot[i] = labelled ? l : TK_NONE;
        new_z[i] = zo;                 // (n_deproject: quiet NaN for an invalid pixel)
        u += su; v += sv;
        if (u >= a.width) { u -= a.width; ++v; }
    }
}
struct d_track_keys {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const unsigned char* depth, const uint32_t* label, const uint32_t* prev_slot, const float* prev_z, TrackArgs a, uint64_t* keys,
                               uint32_t* new_slot, float* new_z, uint32_t* bad_label) const {
        if (a.depth_f32) track_keys_loop<true>(depth, label, prev_slot, prev_z, a, keys, new_slot, new_z, bad_label);
        else track_keys_loop<false>(depth, label, prev_slot, prev_z, a, keys, new_slot, new_z, bad_label);
    }
};

// Sorted keys -> the distinct keys below `limit` (holes never start an entry), each with the range [ustart, uend) of its run.  incl = the inclusive scan of
// d_evl_heads' flags: every element of a run reads its entry's number there, the first writes the key and the start, the last the end.  No atomics.
struct d_track_runs {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* keys, uint32_t n, uint64_t limit, const uint32_t* incl, uint64_t* ukey, uint32_t* ustart, uint32_t* uend, uint32_t* total) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const uint64_t k = keys[i];
            if (k < limit) {
                const uint32_t e = incl[i] - 1u;      // (>= 1 here: the run's head is at or before i; e < n)
                if (i == 0u || keys[i - 1u] != k) { ukey[e] = k; ustart[e] = i; }
                if (i == n - 1u || keys[i + 1u] != k) uend[e] = i + 1u;
            }
            if (i == n - 1u) *total = incl[i];
        }
    }
};

// out: TRK_HEAD words, then up to cap triples (i, j, c).  More entries than cap: the head says so and the host asks again with room for all of them.
struct d_track_pack {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* ukey, const uint32_t* ustart, const uint32_t* uend, const uint32_t* total, const uint32_t* bad_label, int jb, uint32_t cap,
                               uint32_t* out) const {
        const uint32_t n = *total, m = n < cap ? n : cap;
        const uint64_t jmask = (1ull << jb) - 1ull;
        for (uint32_t e = BIX * blockDim.x + threadIdx.x; e < m; e += gridDim.x * blockDim.x) {
            const uint64_t k = ukey[e];
            uint32_t* o = out + TRK_HEAD + (size_t)e * 3u;
            o[0] = (uint32_t)(k >> jb); o[1] = (uint32_t)(k & jmask); o[2] = uend[e] - ustart[e];
        }
        if (BIX == 0u && threadIdx.x == 0u) { out[0] = n; out[1] = *bad_label; out[2] = 0u; out[3] = 0u; }
    }
};

struct d_track_apply {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint32_t* label, uint32_t n, const uint32_t* id, uint32_t Kc, uint32_t* track_ids) const {
        for (uint32_t p = BIX * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
            const uint32_t l = label[p];
            track_ids[p] = l < Kc ? id[l] : TK_NONE;      // (a label >= Kc other than F3DS_NO_LABEL never gets here: the update stops at the flag)
        }
    }
};
