// f3ds_levels.inc -- hierarchy levels: the labels of K thresholds t_l <= T from the merge log of one cluster run to T
// (f3ds_labels_at_thresholds, include/f3ds.h; the rules are in f3ds_levels.h).  Included by f3ds_hip.hip after f3ds_kernels.inc.
//
//   d_level_log     one lane per logged merge i = (a, b, w): into[b] = a, at[b] = i (at[] was filled with LV_NOT_ABSORBED; a supervoxel
//                   is absorbed at most once, so no atomics)
//   d_level_prefix  one workgroup per frame: p_l = the first i with !(w_i < t_l), a wave-wide min per level; ord[] = the levels by ascending p
//   d_level_labels  the level tables in LDS (every workgroup builds them, as d_relabel does) + the grid-stride point pass, when
//                   (S0 + 1) * Kp * 4 bytes fit LV_LDS_BYTES for every frame of the batch;
//   d_level_tables + d_level_points  the same with the tables in global memory otherwise (F3DS_LEVELS_GLOBAL=1 forces this form).
// Table layout: tab[h * Kp + l] = id of the region that holds supervoxel h at level l (Kp = K rounded up to 4), so a point fetches all
// of its levels with Kp / 4 16-byte reads; each level is its own contiguous n-word row of the output, written with coalesced stores.

// LDS budget of the fused form: the 48 KB of d_relabel's table.  Three 256-thread workgroups then fit the 160 KB of a CU (12 waves),
// enough to keep the point pass -- a streaming gather / store loop -- fed; a 64 KB table would leave two (8 waves).
constexpr uint32_t LV_LDS_BYTES = 48u * 1024u;

struct d_level_log {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t nm, uint32_t S0, const uint32_t* merges, uint32_t* into, uint32_t* at) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
            const uint32_t a = merges[(size_t)i * 3], b = merges[(size_t)i * 3 + 1];
            if (a <= S0 && b <= S0) { into[b] = a; at[b] = i; }
        }
    }
};

struct d_level_prefix {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t nm, const uint32_t* merges, uint32_t K, const float* thr, uint32_t* pfx, uint32_t* ord) const {
        __shared__ uint32_t lp_min[4];
        if (BIX) return;
        const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x >> 6;
        for (uint32_t l = 0; l < K; ++l) {
            const float t = thr[l];
            uint32_t first = nm;      // this lane's first stopping index (its indices ascend)
            for (uint32_t i = threadIdx.x; i < nm; i += 256u)
                if (lv_stops(m_from_bitsf(merges[(size_t)i * 3 + 2]), t)) { first = i; break; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)first, off); first = o < first ? o : first; }
            if (lane == 0u) lp_min[w] = first;
            __syncthreads();
            if (threadIdx.x == 0) {
                uint32_t m = lp_min[0];
                for (uint32_t k = 1; k < 4u; ++k) m = lp_min[k] < m ? lp_min[k] : m;
                pfx[l] = m;
            }
            __syncthreads();
        }
        if (threadIdx.x == 0)      // (insertion sort of the K prefixes, once per frame: pass 2 of the tables walks every chain once for all levels)
            for (uint32_t l = 0; l < K; ++l) {
                const uint32_t p = pfx[l];
                uint32_t j = l;
                while (j > 0u && pfx[ord[j - 1u]] > p) { ord[j] = ord[j - 1u]; --j; }
                ord[j] = l;
            }
    }
};

// The tables of one frame, by ONE workgroup (into LDS or global memory):
//   pass 1  per level, the surviving supervoxels (lv_alive) in ascending h -> ids: __ballot + mbcnt inside a wave, the four wave totals
//           through LDS, a running carry across the 256-label chunks (relabel_tables' scan); `writer` stores the level's region count;
//   pass 2  every other supervoxel walks to its root (lv_root) and takes the root's id, levels in ascending p (ord): the walk of a longer
//           prefix continues the walk of a shorter one along the same chain, so a chain is walked once for all K levels.  A root's entry of
//           level l is only read there, a non-root's only written, each by the one thread that owns it.
__device__ inline void level_tables(uint32_t S0, uint32_t K, uint32_t Kp, const unsigned char* alive0, const uint32_t* into, const uint32_t* at,
                                    const uint32_t* pfx, const uint32_t* ord, uint32_t* tab, bool writer, uint32_t* nreg) {
    __shared__ uint32_t lt_wtot[4];
    const uint32_t lane = (uint32_t)lane_id(), w = threadIdx.x >> 6;
    for (uint32_t l = 0; l < K; ++l) {
        const uint32_t p = pfx[l];
        uint32_t carry = 0;
        for (uint32_t base = 0; base <= S0; base += 256u) {
            const uint32_t h = base + threadIdx.x;
            const bool alive = h > 0u && h <= S0 && lv_alive(alive0[h] != 0, at[h], p);
            const uint64_t mask = __ballot(alive);
            const uint32_t within = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (lane == 0u) lt_wtot[w] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) { const uint32_t t = lt_wtot[k]; total += t; if (k < w) before += t; }
            if (h <= S0) tab[(size_t)h * Kp + l] = alive ? carry + before + within : F3DS_NO_LABEL;
            carry += total;
            __syncthreads();
        }
        if (writer && threadIdx.x == 0) nreg[l] = carry;
    }
    for (uint32_t h = threadIdx.x; h <= S0; h += 256u) {
        uint32_t r = h;
        for (uint32_t j = 0; j < K; ++j) {
            const uint32_t l = ord[j];
            r = lv_root(into, at, r, pfx[l]);
            if (r != h) tab[(size_t)h * Kp + l] = tab[(size_t)r * Kp + l];
        }
    }
    __syncthreads();
}
// Every point reads pt_voxel and owner once and writes all K levels: labels[l * n + i].
__device__ inline void level_points(uint32_t n, uint32_t K, uint32_t Kp, const int* pt_voxel, const uint32_t* owner, const uint32_t* tab, uint32_t* labels) {
    for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int v = pt_voxel[i];
        const uint32_t o = owner[v >= 0 ? v : 0];          // (unconditional, as in relabel_points)
        const bool has = v >= 0 && o;
        const uint4* row = reinterpret_cast<const uint4*>(tab + (size_t)(has ? o : 0u) * Kp);
        for (uint32_t q = 0; q < Kp; q += 4u) {
            const uint4 x = row[q >> 2];
            const uint32_t e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
                if (q + j < K) labels[(size_t)(q + j) * n + i] = has ? e[j] : F3DS_NO_LABEL;
        }
    }
}
struct d_level_labels {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, const int* pt_voxel, const uint32_t* owner, uint32_t S0, uint32_t K, uint32_t Kp, const unsigned char* alive0,
                               const uint32_t* into, const uint32_t* at, const uint32_t* pfx, const uint32_t* ord, uint32_t* labels, uint32_t* nreg) const {
        extern __shared__ uint4 lv_tab[];
        if (BIX > 0 && BIX * blockDim.x >= n) return;
        level_tables(S0, K, Kp, alive0, into, at, pfx, ord, reinterpret_cast<uint32_t*>(lv_tab), BIX == 0, nreg);
        level_points(n, K, Kp, pt_voxel, owner, reinterpret_cast<const uint32_t*>(lv_tab), labels);
    }
};
struct d_level_tables {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t S0, uint32_t K, uint32_t Kp, const unsigned char* alive0, const uint32_t* into, const uint32_t* at, const uint32_t* pfx,
                               const uint32_t* ord, uint32_t* tab, uint32_t* nreg) const {
        if (BIX) return;
        level_tables(S0, K, Kp, alive0, into, at, pfx, ord, tab, true, nreg);
    }
};
struct d_level_points {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t n, uint32_t K, uint32_t Kp, const int* pt_voxel, const uint32_t* owner, const uint32_t* tab, uint32_t* labels) const {
        level_points(n, K, Kp, pt_voxel, owner, tab, labels);
    }
};
