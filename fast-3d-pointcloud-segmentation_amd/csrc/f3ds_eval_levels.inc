// f3ds_eval_levels.inc -- the device scorer of hierarchy levels: the seven scores of f3ds_evaluate for K thresholds t_l <= T of one cluster
// run, from sparse contingency tables (f3ds_evaluate_levels, include/f3ds.h; the rules are in f3ds_eval_levels.h; DESIGN.md section 15).
// Included by f3ds_hip.hip after f3ds_levels.inc.
//
//   d_evl_ghosts      the live ghost leaves of the frame as a list (any order: every use below compares supervoxel ids, not list positions)
//   d_evl_base_keys   one key (h = owner[v], j = tlab[v]) per voxel; sorted (radix sort of stage 0) and reduced (d_evl_heads, scan, d_evl_reduce)
//                     they are the BASE TABLE of the frame: the level-independent entries (supervoxel, truth label, count)
//   d_evl_level_keys  per level l every base entry becomes (l, i = tab[h * Kp + l], j) with its count, every ghost leaf that is not "seen" at that
//                     level (d_contingency_ghost's rule over region ids) an entry of count 1; ssize[l][i] gathers both.  One sort + reduce of all
//                     levels of a frame gives every level's table in (i, j) order: the order evl_scores adds the mutual information in
//   d_evl_col_keys    the reduced entries re-keyed (l, j, i); a stable sort on (l, j) alone gives every level's columns, rows ascending
//   d_evl_ht          h_t of the frame (level-independent): the terms lane-parallel, then one lane adds them in evl_scores' order
//   d_evl_score       one workgroup per (frame, level): h_s and mi (terms lane-parallel, one lane adds), the matching (serial over the visited
//                     labels, each column's argmax across the workgroup: evl_better / evl_match_column), the sums over the matched labels
// Key layouts (the field widths are the batch's: every frame records the same sort passes):
//   base  (h << jb) | j                      level  (l << (ib + jb)) | (i << jb) | j                      column  (l << (ib + jb)) | (j << ib) | i
// A key whose top field holds one past its largest value (h = S0 + 1, l = K) is a hole: it sorts behind every entry and d_evl_heads drops it.

// ---- sorted (key, value) pairs -> distinct keys with summed values --------------------------------------------------------------------
// flags[i] = 1 where a new key starts (holes -- keys >= limit -- never start one)
struct d_evl_heads {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* keys, uint32_t n, uint64_t limit, uint32_t* flags) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const uint64_t k = keys[i];
            flags[i] = (k < limit && (i == 0u || keys[i - 1u] != k)) ? 1u : 0u;
        }
    }
};
// incl = the inclusive scan of the flags: entry incl[i] - 1 receives key i; the counts are integers, so their order is free (ucnt starts at zero)
struct d_evl_reduce {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* keys, const uint32_t* vals, uint32_t n, uint64_t limit, const uint32_t* incl, uint64_t* ukey, uint32_t* ucnt,
                               uint32_t* total) const {
        for (uint32_t i = BIX * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
            const uint64_t k = keys[i];
            if (k < limit) {
                const uint32_t e = incl[i] - 1u;
                if (i == 0u || keys[i - 1u] != k) ukey[e] = k;
                atomicAdd(&ucnt[e], vals[i]);
            }
            if (i == n - 1u) *total = incl[i];
        }
    }
};

// ---- the base table ---------------------------------------------------------------------------------------------------------------------
struct d_evl_ghosts {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t S0, const unsigned char* ghost_active, uint32_t* glist, uint32_t* n_ghosts) const {
        for (uint32_t h = 1u + BIX * blockDim.x + threadIdx.x; h <= S0; h += gridDim.x * blockDim.x)
            if (ghost_active[h]) glist[atomicAdd(n_ghosts, 1u)] = h;      // (at most S0 of them: glist holds S0 + 1 words)
    }
};
struct d_evl_base_keys {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t V, uint32_t S0, uint32_t M, const uint32_t* owner, const uint32_t* tlab, int jb, uint64_t* keys, uint32_t* vals) const {
        for (uint32_t v = BIX * blockDim.x + threadIdx.x; v < V; v += gridDim.x * blockDim.x) {
            const uint32_t o = owner[v], j = tlab[v];
            const bool ok = o != 0u && o <= S0 && j < M;
            keys[v] = ((uint64_t)(ok ? o : S0 + 1u) << jb) | (ok ? j : 0u);
            vals[v] = 1u;
        }
    }
};

// ---- the level tables -------------------------------------------------------------------------------------------------------------------
// entry e of level l goes to keys[l * (Eb + G) + e]: e < Eb the base entries, then the G ghost leaves.  tab / Kp: d_level_tables' (f3ds_levels.inc).
struct d_evl_level_keys {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t Eb, uint32_t G, uint32_t K, uint32_t Kp, uint32_t S0, uint32_t M, uint32_t V, const uint64_t* bkey, const uint32_t* bcnt,
                               const uint32_t* glist, const int* ghost_vox, const uint32_t* owner, const uint32_t* tlab, const uint32_t* tab, int ib, int jb,
                               uint64_t* keys, uint32_t* vals, uint32_t* ssize) const {
        const uint32_t ne = Eb + G;
        const uint64_t hole = (uint64_t)K << (ib + jb);
        for (uint32_t e = BIX * blockDim.x + threadIdx.x; e < ne; e += gridDim.x * blockDim.x) {
            uint32_t h, j, c, v = 0u;
            const bool ghost = e >= Eb;
            if (!ghost) { const uint64_t k = bkey[e]; h = (uint32_t)(k >> jb); j = (uint32_t)(k & ((1ull << jb) - 1ull)); c = bcnt[e]; }
            else { h = glist[e - Eb]; v = (uint32_t)ghost_vox[h]; j = v < V ? tlab[v] : M; c = 1u; }      // (v >= V cannot be for a live ghost leaf: such an entry is dropped below)
            const uint32_t ov = ghost && v < V ? owner[v] : 0u;
            for (uint32_t l = 0; l < K; ++l) {
                const uint32_t i = h <= S0 ? tab[(size_t)h * Kp + l] : F3DS_NO_LABEL;
                bool keep = h <= S0 && i <= S0 && j < M;      // (a supervoxel that holds voxels is in a region at every level: this only keeps a broken table inside the buffers)
                if (keep) atomicAdd(&ssize[(size_t)l * (S0 + 1u) + i], c);      // a ghost leaf always adds to its segment's size ...
                if (keep && ghost) {                                          // ... and to the intersection only if its voxel is not in that segment yet (d_contingency_ghost)
                    bool seen = ov != 0u && tab[(size_t)ov * Kp + l] == i;
                    for (uint32_t q = 0; q < G && !seen; ++q) { const uint32_t g = glist[q]; seen = g < h && (uint32_t)ghost_vox[g] == v && tab[(size_t)g * Kp + l] == i; }
                    keep = !seen;
                }
                keys[(size_t)l * ne + e] = keep ? (((uint64_t)l << (ib + jb)) | ((uint64_t)i << jb) | j) : hole;
                vals[(size_t)l * ne + e] = c;
            }
        }
    }
};
struct d_evl_col_keys {
    static constexpr int BLOCK = 256;
    __device__ void operator()(const uint64_t* ukey, const uint32_t* ucnt, const uint32_t* n_dev, int ib, int jb, uint64_t* keys, uint32_t* vals) const {
        const uint32_t n = *n_dev;
        for (uint32_t e = BIX * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
            const uint64_t k = ukey[e];
            const uint64_t j = k & ((1ull << jb) - 1ull), i = (k >> jb) & ((1ull << ib) - 1ull), l = k >> (ib + jb);
            keys[e] = (l << (ib + jb)) | (j << ib) | i;
            vals[e] = ucnt[e];
        }
    }
};

// ---- sums in the header's order ---------------------------------------------------------------------------------------------------------
// acc -= terms[0], terms[1], ... (SUB) or += in index order, by thread 0; the terms pass through LDS in chunks the whole workgroup loads, so that the
// one adding lane reads LDS and not global memory.  Every thread must call it; the result is valid in thread 0.
constexpr uint32_t EVL_CHUNK = 2048;
template <bool SUB>
__device__ inline float evl_ordered_sum(const float* terms, uint32_t n, float acc, float* chunk) {
    for (uint32_t base = 0; base < n; base += EVL_CHUNK) {
        const uint32_t m = n - base < EVL_CHUNK ? n - base : EVL_CHUNK;
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < m; k += blockDim.x) chunk[k] = terms[base + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (uint32_t k = 0; k < m; ++k) { if (SUB) acc -= chunk[k]; else acc += chunk[k]; }
    }
    return acc;
}
__device__ inline uint32_t evl_lower_bound(const uint64_t* keys, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < key) lo = mid + 1u; else hi = mid; }
    return lo;
}

// h_t = -sum over the labels ascending of evl_entropy_term(tsize[j]) (evl_scores' second loop)
struct d_evl_ht {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t M, const uint32_t* tsize, uint32_t V, float* terms, float* ht) const {
        __shared__ float chunk[EVL_CHUNK];
        if (BIX) return;
        const float N = (float)V;
        for (uint32_t j = threadIdx.x; j < M; j += blockDim.x) terms[j] = evl_entropy_term((float)tsize[j], N, evl_m_logf{});
        __syncthreads();
        const float s = evl_ordered_sum<true>(terms, M, 0.0f, chunk);
        if (threadIdx.x == 0) *ht = s;
    }
};

// One workgroup per level (BIX = l).  rkey / rcnt: the frame's reduced entries in (l, i, j) order; ckey / ccnt: the same in (l, j, i) order; U their count.
// order[0 .. nvis): the visited labels (evl_visit_order), rank[k]: order[k]'s position among them by ascending label, bylabel[q]: the visited label of rank q.  Scratch of this level: used (K_l
// bytes, zeroed), hterm (K_l floats), mterm (as many floats as the level has entries, indexed like rkey), slot (4 * nvis words).
// out: 8 words per level: the seven scores and the region count.
struct d_evl_score {
    static constexpr int BLOCK = 256;
    __device__ void operator()(uint32_t K, uint32_t S0, uint32_t V, const uint32_t* nreg, const uint32_t* ssize_all, const uint32_t* tsize,
                               const uint64_t* rkey, const uint32_t* rcnt, const uint64_t* ckey, const uint32_t* ccnt, const uint32_t* n_entries, int ib, int jb,
                               const uint32_t* order, const uint32_t* rank, const uint32_t* bylabel, uint32_t nvis, const float* ht, unsigned char* used_all, float* hterm_all,
                               float* mterm, uint32_t* slot_all, uint32_t* out) const {
        __shared__ float chunk[EVL_CHUNK];
        __shared__ uint32_t red_c[4], red_i[4];
        const uint32_t l = BIX;
        if (l >= K) return;
        const uint32_t Kl = nreg[l], U = *n_entries, tid = threadIdx.x, lane = (uint32_t)lane_id(), w = tid >> 6;
        const uint32_t* ssize = ssize_all + (size_t)l * (S0 + 1u);
        unsigned char* used = used_all + (size_t)l * (S0 + 1u);
        float* hterm = hterm_all + (size_t)l * (S0 + 1u);
        uint32_t* slot_row = slot_all + (size_t)l * nvis * 4u;      // per level: matched row and its count by label rank, then the column range of every visited label
        uint32_t* slot_in = slot_row + nvis;
        uint32_t* col_lo = slot_in + nvis;
        uint32_t* col_hi = col_lo + nvis;
        const float N = (float)V;
        const uint64_t jmask = (1ull << jb) - 1ull, imask = (1ull << ib) - 1ull;
        // h_s: evl_scores' first loop
        for (uint32_t i = tid; i < Kl; i += 256u) hterm[i] = evl_entropy_term((float)ssize[i], N, evl_m_logf{});
        __syncthreads();
        const float h_s = evl_ordered_sum<true>(hterm, Kl, 0.0f, chunk);
        // mi: evl_scores' third loop over this level's entries, which are in (i, j) order
        const uint32_t r0 = evl_lower_bound(rkey, U, (uint64_t)l << (ib + jb)), r1 = evl_lower_bound(rkey, U, (uint64_t)(l + 1u) << (ib + jb));
        for (uint32_t e = r0 + tid; e < r1; e += 256u) {
            const uint64_t k = rkey[e];
            const uint32_t i = (uint32_t)((k >> jb) & imask), j = (uint32_t)(k & jmask);
            mterm[e] = evl_mi_term(N, (float)rcnt[e], (float)ssize[i], (float)tsize[j], evl_m_logf{});
        }
        __syncthreads();
        const float mi = evl_ordered_sum<false>(mterm + r0, r1 - r0, 0.0f, chunk);
        // the matching: evl_match_column per visited label, the column's argmax (evl_better) across the workgroup.  The columns' ranges first, all labels at
        // once: the serial loop below then has no dependent searches in it
        for (uint32_t k = tid; k < nvis; k += 256u) {
            const uint64_t cbase = ((uint64_t)l << (ib + jb)) | ((uint64_t)order[k] << ib);
            col_lo[k] = evl_lower_bound(ckey, U, cbase); col_hi[k] = evl_lower_bound(ckey, U, cbase + (1ull << ib));
        }
        __syncthreads();
        for (uint32_t k = 0; k < nvis; ++k) {
            const uint32_t c0 = col_lo[k], c1 = col_hi[k];
            uint32_t best = EVL_UNMATCHED, bc = 0;
            for (uint32_t e = c0 + tid; e < c1; e += 256u) {
                const uint32_t i = (uint32_t)(ckey[e] & imask), c = ccnt[e];
                if (!used[i] && (best == EVL_UNMATCHED || evl_better(c, i, bc, best))) { best = i; bc = c; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t oi = (uint32_t)__shfl_xor((int)best, off), oc = (uint32_t)__shfl_xor((int)bc, off);
                if (oi != EVL_UNMATCHED && (best == EVL_UNMATCHED || evl_better(oc, oi, bc, best))) { best = oi; bc = oc; }
            }
            if (lane == 0u) { red_i[w] = best; red_c[w] = bc; }
            __syncthreads();
            if (tid == 0u) {
                for (uint32_t q = 1; q < 4u; ++q)
                    if (red_i[q] != EVL_UNMATCHED && (best == EVL_UNMATCHED || evl_better(red_c[q], red_i[q], bc, best))) { best = red_i[q]; bc = red_c[q]; }
                if (c0 == c1) { best = used[0] ? EVL_UNMATCHED : 0u; bc = 0u; }      // the empty column: row 0 if it is free
                if (best != EVL_UNMATCHED) used[best] = 1;
                slot_row[rank[k]] = best; slot_in[rank[k]] = best == EVL_UNMATCHED ? 0u : bc;
            }
            __syncthreads();      // (used[] is read by every thread at the next label)
        }
        // evl_scores' last loop.  Unvisited and unmatched labels only add their size to fn; r, fp and fn are sums of integers below 2^24 (the host refuses
        // larger frames), so every partial sum is exact in float and integer arithmetic gives the same bits.  p and w run over the matched labels ascending.
        if (tid == 0u) {
            float p = 0, wv = 0;
            uint32_t r = 0, fp = 0;
            for (uint32_t q = 0; q < nvis; ++q) {
                const uint32_t i = slot_row[q];
                if (i == EVL_UNMATCHED) continue;
                const uint32_t j = bylabel[q], in = slot_in[q];
                const float inj = (float)in, g = (float)tsize[j], s = (float)ssize[i];
                p += evl_p_term(inj, g, s); r += in; fp += ssize[i] - in;
                wv += evl_w_term(inj, g, ssize[i], tsize[j], in);
            }
            const uint32_t fn = V - r;      // sum of tsize = V: every label adds its size, a matched one less its intersection
            const f3ds_performance pf = evl_finish(h_s, *ht, mi, p, (float)r, (float)fp, (float)fn, wv, N);
            out[(size_t)l * 8u + 0u] = __float_as_uint(pf.voi); out[(size_t)l * 8u + 1u] = __float_as_uint(pf.precision); out[(size_t)l * 8u + 2u] = __float_as_uint(pf.recall);
            out[(size_t)l * 8u + 3u] = __float_as_uint(pf.fscore); out[(size_t)l * 8u + 4u] = __float_as_uint(pf.wov); out[(size_t)l * 8u + 5u] = __float_as_uint(pf.fpr);
            out[(size_t)l * 8u + 6u] = __float_as_uint(pf.fnr); out[(size_t)l * 8u + 7u] = Kl;
        }
    }
};
