// Kernel probe (test infrastructure only: tests/test_kernprobe_gpu.py).  The wave- and workgroup-level building blocks of csrc/f3ds_kernels.inc,
// each behind a thin __global__ wrapper, compiled for gfx950 with the product's own flags (the Makefile asks csrc/Makefile for them).  The product's
// headers and f3ds_kernels.inc are included unchanged; the functors run through kp_call<>, launched with the grid widths the host layer
// (scan_u32, radix_sort, seg_sort, seg_labels, seg_sweeps_on in f3ds_hip.hip) gives them.
//
// Every kp_* entry point takes host pointers, checks the primitive's preconditions BEFORE any HIP call (KP_EARG: nothing is launched, no device is
// touched -- tests/test_kernprobe_cpu.py calls them without a GPU), allocates zero-filled device buffers, copies in, launches, synchronises, copies
// back, frees, and returns the HIP error code (0 = hipSuccess).  No wrapper has an unbounded loop of its own, and the checked preconditions bound
// every loop and every address of the code under test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "f3ds.h"
#include "f3ds_algo.h"
#include "f3ds_glasbey.h"
#include "f3ds_eval.h"
#include "f3ds_dev.h"
#include "f3ds_levels.h"
#include "f3ds_eval_levels.h"

using namespace f3ds;

#ifndef KP_KERNELS_INC
#define KP_KERNELS_INC "f3ds_kernels.inc"
#endif
#include KP_KERNELS_INC

namespace {

constexpr int KP_EARG = -2;      // a precondition does not hold: nothing was launched

template <class K, class... A>
__global__ __launch_bounds__(K::BLOCK) void kp_call(A... a) { K{}(a...); }

// the same with the register budget the host layer's launcher gives a kernel that asks for one (f3ds_hip.hip: waves_per_simd, k_batched): kp_sweeps
template <class K, class = void> struct kp_wps { static constexpr int v = 1; };
template <class K> struct kp_wps<K, std::void_t<decltype(K::WAVES_PER_SIMD)>> { static constexpr int v = K::WAVES_PER_SIMD; };
template <class K, class... A>
__global__ __launch_bounds__(K::BLOCK, kp_wps<K>::v) void kp_call_w(A... a) { K{}(a...); }

// ---- wave primitives: one wave per workgroup, one case (64 words) per workgroup -------------------------------------------------------
enum { KP_WAVE_SCAN = 0, KP_WAVE_SCAN_DPP = 1, KP_WAVE_MIN = 2, KP_ROW_MIN = 3, KP_ROW_SORT16 = 4 };
__global__ __launch_bounds__(64) void kp_wave_k(int op, const uint32_t* in, uint32_t* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const uint32_t v = in[i];
    uint32_t r = 0;
    if (op == KP_WAVE_SCAN) r = wave_incl_scan(v);
    else if (op == KP_WAVE_SCAN_DPP) r = wave_incl_scan_dpp(v);
    else if (op == KP_WAVE_MIN) r = wave_min_u32(v);
    else if (op == KP_ROW_MIN) r = row_min_u32(v);
    else r = row_sort16(v, threadIdx.x & 15u);
    out[i] = r;
}
// run_of_lane: in = 3 x 64 words per case (valid, w0, w1), out = 3 x 64 (head, head_lane, run_len)
__global__ __launch_bounds__(64) void kp_run_of_lane_k(const uint32_t* in, uint32_t* out) {
    const uint32_t b = blockIdx.x * 192u, l = threadIdx.x;
    bool head; int hl; uint32_t len;
    run_of_lane(in[b + l] != 0u, in[b + 64u + l], in[b + 128u + l], &head, &hl, &len);
    out[b + l] = head ? 1u : 0u; out[b + 64u + l] = (uint32_t)hl; out[b + 128u + l] = len;
}
// ---- workgroup scans: one case (256 words, or 2 x 256) per workgroup ----------------------------------------------------------------
__global__ __launch_bounds__(256) void kp_block_incl_k(const uint32_t* in, uint32_t* out) {      // out: 256 prefixes, then the total as every thread got it
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    uint32_t tot;
    const uint32_t inc = block_incl_scan<256>(in[b * 256u + t], &tot);
    out[b * 512u + t] = inc; out[b * 512u + 256u + t] = tot;
}
__global__ __launch_bounds__(256) void kp_block_excl2_k(const uint32_t* in, uint32_t* out) {     // in: a[256] b[256]; out: ea, eb, ta, tb (256 each)
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    uint32_t ea, eb, ta, tb;
    block_excl_scan2(in[b * 512u + t], in[b * 512u + 256u + t], &ea, &eb, &ta, &tb);
    uint32_t* o = out + b * 1024u;
    o[t] = ea; o[256u + t] = eb; o[512u + t] = ta; o[768u + t] = tb;
}
// ---- helper_tile_list: one wave per workgroup, one helper per workgroup ---------------------------------------------------------------
__global__ __launch_bounds__(64) void kp_tile_list_k(const uint32_t* tl, const uint32_t* cnt, const int* gv, uint32_t* srt_out, int* ret) {
    __shared__ uint32_t srt[64];
    const uint32_t b = blockIdx.x, l = threadIdx.x;
    srt[l] = 0xFFFFFFFFu;
    wave_lds_sync();
    const int r = helper_tile_list(tl + (size_t)b * HT_CAP, cnt[b], gv[b], srt);
    wave_lds_sync();
    srt_out[b * 64u + l] = srt[l];
    if (l == 0u) ret[b] = r;
}
// ---- row_leaves: one wave, four helpers (one per 16-lane row); tables as d_centroid::quad holds them -----------------------------------
constexpr uint32_t KP_QL = 64;      // = d_centroid::QL: the leaf table has cap + 32 entries, the spare entry is cap + 31
__global__ __launch_bounds__(64) void kp_row_leaves_k(const uint32_t* owner, uint32_t V, const uint32_t* hs, const uint32_t* tids, const int* gvs, uint32_t cap,
                                                      uint32_t* qt_out, uint32_t* ql_out, uint32_t* scal) {
    __shared__ __attribute__((aligned(16))) uint32_t qt[4][16];
    __shared__ __attribute__((aligned(16))) uint32_t ql[4][KP_QL + 32];
    const uint32_t l = threadIdx.x, row = l >> 4, l16 = l & 15u;
    qt[row][l16] = 0xFFFFFFFFu;
    for (uint32_t i = l16; i < KP_QL + 32u; i += 16u) ql[row][i] = 0xFFFFFFFFu;
    wave_lds_sync();
    uint32_t nd, kept;
    const uint32_t count = row_leaves(owner, V, hs[row], tids[l], gvs[row], qt, ql[row], cap, cap + 31u, &nd, &kept);
    wave_lds_sync();
    qt_out[l] = qt[row][l16];
    for (uint32_t i = l16; i < KP_QL + 32u; i += 16u) ql_out[row * (KP_QL + 32u) + i] = ql[row][i];
    // (count, nd, kept) as every lane of the row got them: 3 x 64 words
    scal[l] = count; scal[64u + l] = nd; scal[128u + l] = kept;
}
// ---- f3ds_vblock: which (frame, virtual block) a workgroup of a (gx, nf) launch works on ------------------------------------------------
__global__ __launch_bounds__(64) void kp_vblock_k(uint32_t* out) {
    uint32_t f, x;
    f3ds_vblock(&f, &x);
    const uint32_t lin = blockIdx.y * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) { out[2u * lin] = f; out[2u * lin + 1u] = x; out[2u * gridDim.x * gridDim.y + 2u * lin] = f3ds_frame(); out[2u * gridDim.x * gridDim.y + 2u * lin + 1u] = BIX; }
}

// device buffers of one call: freed when the call returns, whatever it returns (hipMalloc: 256-byte aligned, so every buffer can take 16-byte loads)
struct Bufs {
    void* p[64];
    int n = 0;
    hipError_t err = hipSuccess;
    ~Bufs() { for (int i = 0; i < n; ++i) (void)hipFree(p[i]); }
    void* make(size_t bytes, const void* src) {          // a buffer of `bytes` (at least 64: a zero-length array still gives a valid address), zeroed, then filled from src
        if (err != hipSuccess || n >= 64) { if (err == hipSuccess) err = hipErrorOutOfMemory; return nullptr; }
        void* d = nullptr;
        const size_t cap = bytes < 64 ? 64 : bytes;
        err = hipMalloc(&d, cap);
        if (err != hipSuccess) return nullptr;
        p[n++] = d;
        err = hipMemset(d, 0, cap);
        if (err == hipSuccess && src && bytes) err = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    template <class T> T* mk(size_t count, const T* src = nullptr) { return (T*)make(count * sizeof(T), src); }
    void sync() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    template <class T> void back(T* dst, const T* src, size_t count) {
        if (err == hipSuccess && count) err = hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost);
    }
};

// the grid widths of the host layer (f3ds_hip.hip: grid_for with its default cap, grid_wide)
uint32_t kp_grid_for(size_t work, int block) { size_t g = (work + block - 1) / block; return (uint32_t)(g < 1 ? 1 : (g > 2048 ? 2048 : g)); }
constexpr size_t KP_MAX_N = 1u << 22;      // elements / cases a call may ask for

// scan_u32 as the host records it; extra = workgroups beyond what n needs (a batched launch is as wide as its widest frame)
void kp_scan_u32_on(Bufs& B, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t extra) {
    const uint32_t nt = n ? (n + SCAN_TILE - 1) / SCAN_TILE : 1u;
    uint32_t* tiles = B.mk<uint32_t>((size_t)nt + extra);
    if (B.err != hipSuccess) return;
    hipLaunchKernelGGL((kp_call<d_scan_tiles, const uint32_t*, uint32_t*, uint32_t*, uint32_t>), dim3(nt + extra, 1), dim3(d_scan_tiles::BLOCK), 0, 0, in, out, tiles, n);
    hipLaunchKernelGGL((kp_call<d_scan_single, uint32_t*, uint32_t>), dim3(1, 1), dim3(d_scan_single::BLOCK), 0, 0, tiles, nt);
    hipLaunchKernelGGL((kp_call<d_scan_add, uint32_t*, const uint32_t*, uint32_t>), dim3(nt + extra, 1), dim3(d_scan_add::BLOCK), 0, 0, out, (const uint32_t*)tiles, n);
}
bool radix_args_ok(uint32_t n, int shift, int bits, long long n_dev) {
    return n <= KP_MAX_N && bits >= 1 && bits <= RS_MAXBITS && shift >= 0 && shift + bits <= 64 && n_dev >= -1 && n_dev <= 0xFFFFFFFFll;
}
uint32_t radix_nb(uint32_t n) { return n ? (n + RS_TILE - 1) / RS_TILE : 1u; }

}  // namespace

extern "C" {

int kp_const(int which) {
    switch (which) {
        case 0: return (int)HT_CAP; case 1: return SCAN_TILE; case 2: return RS_TILE; case 3: return RS_MAXBITS; case 4: return (int)RL_LDS_CAP;
        case 5: return (int)KP_QL; case 6: return (int)sizeof(DevCounters); case 7: return KP_EARG; case 8: return (int)F3DS_NO_LABEL;
    }
    return -1;
}

// op: KP_WAVE_SCAN .. KP_ROW_SORT16; in / out: ncases x 64 words
int kp_wave(int op, const uint32_t* in, uint32_t* out, size_t ncases) {
    if (op < 0 || op > KP_ROW_SORT16 || !in || !out || ncases > KP_MAX_N / 64) return KP_EARG;
    if (ncases == 0) return 0;
    Bufs B;
    const uint32_t* din = B.mk<uint32_t>(ncases * 64, in);
    uint32_t* dout = B.mk<uint32_t>(ncases * 64);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL(kp_wave_k, dim3((unsigned)ncases), dim3(64), 0, 0, op, din, dout);
    B.sync(); B.back(out, dout, ncases * 64);
    return (int)B.err;
}
int kp_run_of_lane(const uint32_t* in, uint32_t* out, size_t ncases) {
    if (!in || !out || ncases > KP_MAX_N / 192) return KP_EARG;
    if (ncases == 0) return 0;
    Bufs B;
    const uint32_t* din = B.mk<uint32_t>(ncases * 192, in);
    uint32_t* dout = B.mk<uint32_t>(ncases * 192);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL(kp_run_of_lane_k, dim3((unsigned)ncases), dim3(64), 0, 0, din, dout);
    B.sync(); B.back(out, dout, ncases * 192);
    return (int)B.err;
}
// two = 0: block_incl_scan<256> (in 256, out 512 per case); 1: block_excl_scan2 (in 512, out 1024 per case)
int kp_block(int two, const uint32_t* in, uint32_t* out, size_t ncases) {
    if ((two != 0 && two != 1) || !in || !out || ncases > KP_MAX_N / 1024) return KP_EARG;
    if (ncases == 0) return 0;
    Bufs B;
    const size_t ni = two ? 512 : 256, no = two ? 1024 : 512;
    const uint32_t* din = B.mk<uint32_t>(ncases * ni, in);
    uint32_t* dout = B.mk<uint32_t>(ncases * no);
    if (B.err != hipSuccess) return (int)B.err;
    if (two) hipLaunchKernelGGL(kp_block_excl2_k, dim3((unsigned)ncases), dim3(256), 0, 0, din, dout);
    else hipLaunchKernelGGL(kp_block_incl_k, dim3((unsigned)ncases), dim3(256), 0, 0, din, dout);
    B.sync(); B.back(out, dout, ncases * no);
    return (int)B.err;
}
// d_scan_single alone: data[m] in place.  cap = words of the buffer (>= m)
int kp_scan_single(uint32_t* data, uint32_t m, size_t cap) {
    if (!data || m > cap || cap > KP_MAX_N) return KP_EARG;
    Bufs B;
    uint32_t* d = B.mk<uint32_t>(cap, data);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL((kp_call<d_scan_single, uint32_t*, uint32_t>), dim3(1, 1), dim3(d_scan_single::BLOCK), 0, 0, d, m);
    B.sync(); B.back(data, d, cap);
    return (int)B.err;
}
// d_scan_tiles + d_scan_single + d_scan_add; out has cap >= n words (the words behind n come back zero)
int kp_scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, size_t cap, uint32_t extra_blocks) {
    if (!in || !out || n > cap || cap > KP_MAX_N || extra_blocks > 64) return KP_EARG;
    Bufs B;
    const uint32_t* din = B.mk<uint32_t>(cap, in);
    uint32_t* dout = B.mk<uint32_t>(cap);
    if (B.err != hipSuccess) return (int)B.err;
    kp_scan_u32_on(B, din, dout, n, extra_blocks);
    B.sync(); B.back(out, dout, cap);
    return (int)B.err;
}
// d_radix_hist: hist[(1 << bits) * nb], nb from n as radix_sort computes it.  n_dev = -1: no device-side count
int kp_radix_hist(const uint64_t* keys, uint32_t n, int shift, int bits, long long n_dev, uint32_t* hist) {
    if (!keys || !hist || !radix_args_ok(n, shift, bits, n_dev)) return KP_EARG;
    const uint32_t nb = radix_nb(n);
    Bufs B;
    const uint64_t* dk = B.mk<uint64_t>(n, keys);
    uint32_t* dh = B.mk<uint32_t>((size_t)RS_BINS * nb);
    const uint32_t ndv = (uint32_t)n_dev;
    const uint32_t* dn = n_dev >= 0 ? B.mk<uint32_t>(1, &ndv) : nullptr;
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL((kp_call<d_radix_hist, const uint64_t*, uint32_t, int, int, uint32_t*, uint32_t, const uint32_t*>), dim3(nb, 1), dim3(RS_THREADS), 0, 0, dk, n, shift, bits, dh, nb, dn);
    B.sync(); B.back(hist, dh, ((size_t)1 << bits) * nb);
    return (int)B.err;
}
// d_radix_scatter (vals != null) / d_radix_scatter_k (vals == null; n_dev must be -1) with the caller's scanned histogram.  The histogram is checked
// against the keys before the launch: every tile's digit range has to end inside the output (so no position can leave it, whatever the ranks inside).
int kp_radix_scatter(const uint64_t* keys, const uint32_t* vals, uint32_t n, int shift, int bits, long long n_dev, const uint32_t* hist_scanned,
                     uint64_t* keys_out, uint32_t* vals_out) {
    if (!keys || !hist_scanned || !keys_out || !radix_args_ok(n, shift, bits, n_dev) || (vals && !vals_out) || (!vals && n_dev >= 0)) return KP_EARG;
    const uint32_t nb = radix_nb(n), ne = n_dev >= 0 && (uint32_t)n_dev < n ? (uint32_t)n_dev : n, mask = (1u << bits) - 1u;
    std::vector<uint32_t> c((size_t)(1u << bits) * nb, 0u);
    for (uint32_t i = 0; i < ne; ++i) c[(size_t)((uint32_t)(keys[i] >> shift) & mask) * nb + i / RS_TILE]++;
    for (size_t j = 0; j < c.size(); ++j) if ((uint64_t)hist_scanned[j] + c[j] > ne) return KP_EARG;
    Bufs B;
    const uint64_t* dk = B.mk<uint64_t>(n, keys);
    const uint32_t* dv = vals ? B.mk<uint32_t>(n, vals) : nullptr;
    uint64_t* dko = B.mk<uint64_t>(n);
    uint32_t* dvo = vals ? B.mk<uint32_t>(n) : nullptr;
    uint32_t* dh = B.mk<uint32_t>((size_t)RS_BINS * nb);
    if (B.err == hipSuccess) B.err = hipMemcpy(dh, hist_scanned, c.size() * 4, hipMemcpyHostToDevice);
    const uint32_t ndv = (uint32_t)n_dev;
    const uint32_t* dn = n_dev >= 0 ? B.mk<uint32_t>(1, &ndv) : nullptr;
    if (B.err != hipSuccess) return (int)B.err;
    if (vals) hipLaunchKernelGGL((kp_call<d_radix_scatter, const uint64_t*, const uint32_t*, uint64_t*, uint32_t*, uint32_t, int, int, const uint32_t*, uint32_t, const uint32_t*>),
                                 dim3(nb, 1), dim3(RS_THREADS), 0, 0, dk, dv, dko, dvo, n, shift, bits, (const uint32_t*)dh, nb, dn);
    else hipLaunchKernelGGL((kp_call<d_radix_scatter_k, const uint64_t*, uint64_t*, uint32_t, int, int, const uint32_t*, uint32_t>), dim3(nb, 1), dim3(RS_THREADS), 0, 0, dk, dko, n, shift, bits, (const uint32_t*)dh, nb);
    B.sync(); B.back(keys_out, dko, n);
    if (vals) B.back(vals_out, dvo, n);
    return (int)B.err;
}
// the pass sequence of radix_sort (f3ds_hip.hip), buffers ping-ponged as there; keys_out / vals_out = the arrays the last pass left the result in
int kp_radix_sort(const uint64_t* keys, const uint32_t* vals, uint32_t n, int total_bits, int base_shift, long long n_dev, uint64_t* keys_out, uint32_t* vals_out) {
    if (!keys || !keys_out || n > KP_MAX_N || total_bits < 0 || base_shift < 0 || base_shift + total_bits > 64 || n_dev < -1 || n_dev > 0xFFFFFFFFll || (vals && !vals_out) || (!vals && n_dev >= 0))
        return KP_EARG;
    Bufs B;
    uint64_t *k0 = B.mk<uint64_t>(n, keys), *k1 = B.mk<uint64_t>(n);
    uint32_t *v0 = vals ? B.mk<uint32_t>(n, vals) : nullptr, *v1 = vals ? B.mk<uint32_t>(n) : nullptr;
    const uint32_t nb = radix_nb(n);
    uint32_t* hist = B.mk<uint32_t>((size_t)RS_BINS * nb);
    const uint32_t ndv = (uint32_t)n_dev;
    const uint32_t* dn = n_dev >= 0 ? B.mk<uint32_t>(1, &ndv) : nullptr;
    if (B.err != hipSuccess) return (int)B.err;
    if (total_bits > 0) {
        const int passes = (total_bits + RS_MAXBITS - 1) / RS_MAXBITS;
        const int per = (total_bits + passes - 1) / passes;
        int shift = 0;
        for (int p = 0; p < passes; ++p) {
            const int bits = (total_bits - shift) < per ? (total_bits - shift) : per;
            hipLaunchKernelGGL((kp_call<d_radix_hist, const uint64_t*, uint32_t, int, int, uint32_t*, uint32_t, const uint32_t*>), dim3(nb, 1), dim3(RS_THREADS), 0, 0,
                               (const uint64_t*)k0, n, base_shift + shift, bits, hist, nb, dn);
            hipLaunchKernelGGL((kp_call<d_scan_single, uint32_t*, uint32_t>), dim3(1, 1), dim3(d_scan_single::BLOCK), 0, 0, hist, (uint32_t)((1u << bits) * nb));
            if (v0) hipLaunchKernelGGL((kp_call<d_radix_scatter, const uint64_t*, const uint32_t*, uint64_t*, uint32_t*, uint32_t, int, int, const uint32_t*, uint32_t, const uint32_t*>),
                                       dim3(nb, 1), dim3(RS_THREADS), 0, 0, (const uint64_t*)k0, (const uint32_t*)v0, k1, v1, n, base_shift + shift, bits, (const uint32_t*)hist, nb, dn);
            else hipLaunchKernelGGL((kp_call<d_radix_scatter_k, const uint64_t*, uint64_t*, uint32_t, int, int, const uint32_t*, uint32_t>), dim3(nb, 1), dim3(RS_THREADS), 0, 0,
                                    (const uint64_t*)k0, k1, n, base_shift + shift, bits, (const uint32_t*)hist, nb);
            std::swap(k0, k1); std::swap(v0, v1);
            shift += bits;
        }
    }
    B.sync(); B.back(keys_out, k0, n);
    if (vals) B.back(vals_out, v0, n);
    return (int)B.err;
}
// the segment table of sorted keys.  chain 0: d_heads + scan_u32 + d_segstart; chain 1: d_seg_count + d_scan_single + d_seg_write.
// seg_start[n + 1], counters[2] = (segments, valid keys); all pre-zeroed, as the host leaves them
int kp_seg_table(int chain, const uint64_t* keys, uint32_t n, uint64_t limit, int shift, uint32_t* seg_start, uint32_t* counters) {
    if ((chain != 0 && chain != 1) || !keys || !seg_start || !counters || n > KP_MAX_N || shift < 0 || shift > 63) return KP_EARG;
    Bufs B;
    const uint64_t* dk = B.mk<uint64_t>(n, keys);
    uint32_t* ds = B.mk<uint32_t>((size_t)n + 1);
    uint32_t* dc = B.mk<uint32_t>(2);
    if (chain == 0) {
        uint32_t *flags = B.mk<uint32_t>(n), *incl = B.mk<uint32_t>(n);
        if (B.err != hipSuccess) return (int)B.err;
        const uint32_t gx = kp_grid_for(n, 256);
        hipLaunchKernelGGL((kp_call<d_heads, const uint64_t*, uint32_t, uint64_t, uint32_t*, int>), dim3(gx, 1), dim3(256), 0, 0, dk, n, limit, flags, shift);
        kp_scan_u32_on(B, flags, incl, n, 0);
        if (B.err != hipSuccess) return (int)B.err;
        hipLaunchKernelGGL((kp_call<d_segstart, const uint64_t*, const uint32_t*, const uint32_t*, uint32_t, uint64_t, uint32_t*, uint32_t*, uint32_t*, int>), dim3(gx, 1), dim3(256), 0, 0,
                           dk, (const uint32_t*)flags, (const uint32_t*)incl, n, limit, ds, dc, dc + 1, shift);
    } else {
        const uint32_t nt = n ? (n + SCAN_TILE - 1) / SCAN_TILE : 1u;
        uint32_t* tiles = B.mk<uint32_t>(nt);
        if (B.err != hipSuccess) return (int)B.err;
        hipLaunchKernelGGL((kp_call<d_seg_count, const uint64_t*, uint32_t, uint64_t, int, uint32_t*>), dim3(nt, 1), dim3(SCAN_THREADS), 0, 0, dk, n, limit, shift, tiles);
        hipLaunchKernelGGL((kp_call<d_scan_single, uint32_t*, uint32_t>), dim3(1, 1), dim3(d_scan_single::BLOCK), 0, 0, tiles, nt);
        hipLaunchKernelGGL((kp_call<d_seg_write, const uint64_t*, uint32_t, uint64_t, int, const uint32_t*, uint32_t*, uint32_t*, uint32_t*>), dim3(nt, 1), dim3(SCAN_THREADS), 0, 0,
                           dk, n, limit, shift, (const uint32_t*)tiles, ds, dc, dc + 1);
    }
    B.sync(); B.back(seg_start, ds, (size_t)n + 1); B.back(counters, dc, 2);
    return (int)B.err;
}
// relabel.  parent[S0 + 1] (every entry <= S0, every chain reaches a root: checked), ralive[S0 + 1].
// n == 0 and pt_voxel == null: relabel_tables through d_region_ids, rank_or_labels = rank[S0 + 1].
// otherwise d_relabel (S0 + 1 <= RL_LDS_CAP) with gx as seg_labels computes it: pt_voxel[n] in [-1, V), owner[V] in [0, S0], rank_or_labels = labels[n].
int kp_relabel(uint32_t S0, const uint32_t* parent, const unsigned char* ralive, uint32_t n, const int* pt_voxel, const uint32_t* owner, uint32_t V,
               uint32_t* rank_or_labels, uint32_t* root_out, uint32_t* incl_out, uint32_t* n_regions) {
    if (!parent || !ralive || !rank_or_labels || !root_out || !incl_out || !n_regions || S0 >= KP_MAX_N || n > KP_MAX_N || V > KP_MAX_N) return KP_EARG;
    for (uint32_t h = 0; h <= S0; ++h) if (parent[h] > S0) return KP_EARG;
    for (uint32_t h = 0; h <= S0; ++h) {
        uint32_t r = h, steps = 0;
        while (parent[r] != r) { r = parent[r]; if (++steps > S0) return KP_EARG; }      // a cycle
    }
    const bool points = pt_voxel != nullptr;
    if (points) {
        if (!owner || V < 1 || S0 + 1u > RL_LDS_CAP) return KP_EARG;
        for (uint32_t i = 0; i < n; ++i) if (pt_voxel[i] < -1 || (pt_voxel[i] >= 0 && (uint32_t)pt_voxel[i] >= V)) return KP_EARG;
        for (uint32_t v = 0; v < V; ++v) if (owner[v] > S0) return KP_EARG;
    } else if (n != 0) return KP_EARG;
    Bufs B;
    const uint32_t* dp = B.mk<uint32_t>((size_t)S0 + 1, parent);
    const unsigned char* da = B.mk<unsigned char>((size_t)S0 + 1, ralive);
    uint32_t *droot = B.mk<uint32_t>((size_t)S0 + 1), *dincl = B.mk<uint32_t>((size_t)S0 + 1);
    DevCounters* dc = B.mk<DevCounters>(1);
    uint32_t* dout = B.mk<uint32_t>(points ? n : (size_t)S0 + 1);
    const int* dpv = points ? B.mk<int>(n, pt_voxel) : nullptr;
    const uint32_t* down = points ? B.mk<uint32_t>(V, owner) : nullptr;
    if (B.err != hipSuccess) return (int)B.err;
    if (points) {
        const uint32_t gx = std::min(kp_grid_for(n, 256), kp_grid_for(n, 4096));
        hipLaunchKernelGGL((kp_call<d_relabel, uint32_t, const int*, const uint32_t*, uint32_t, const uint32_t*, const unsigned char*, uint32_t*, uint32_t*, uint32_t*, DevCounters*>),
                           dim3(gx, 1), dim3(256), (S0 + 1u) * 4u, 0, n, dpv, down, S0, dp, da, droot, dincl, dout, dc);
    } else {
        hipLaunchKernelGGL((kp_call<d_region_ids, uint32_t, const uint32_t*, const unsigned char*, uint32_t*, uint32_t*, uint32_t*, DevCounters*>), dim3(1, 1), dim3(256), 0, 0,
                           S0, dp, da, dout, droot, dincl, dc);
    }
    B.sync();
    B.back(rank_or_labels, dout, points ? n : (size_t)S0 + 1); B.back(root_out, droot, (size_t)S0 + 1); B.back(incl_out, dincl, (size_t)S0 + 1);
    DevCounters h;
    memset(&h, 0, sizeof h);
    B.back(&h, dc, 1);
    *n_regions = h.n_regions;
    return (int)B.err;
}
// helper_tile_list on ncases helpers: tl[ncases x HT_CAP], cnt <= HT_CAP + 1, gv = -1 or a voxel; srt_out[ncases x 64] (0xFFFFFFFF where nothing was written), ret[ncases]
int kp_tile_list(const uint32_t* tl, const uint32_t* cnt, const int* gv, size_t ncases, uint32_t* srt_out, int* ret) {
    if (!tl || !cnt || !gv || !srt_out || !ret || ncases > KP_MAX_N / HT_CAP) return KP_EARG;
    for (size_t i = 0; i < ncases; ++i) if (cnt[i] > HT_CAP + 1u || gv[i] < -1) return KP_EARG;
    if (ncases == 0) return 0;
    Bufs B;
    const uint32_t* dtl = B.mk<uint32_t>(ncases * HT_CAP, tl);
    const uint32_t* dcnt = B.mk<uint32_t>(ncases, cnt);
    const int* dgv = B.mk<int>(ncases, gv);
    uint32_t* dsrt = B.mk<uint32_t>(ncases * 64);
    int* dret = B.mk<int>(ncases);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL(kp_tile_list_k, dim3((unsigned)ncases), dim3(64), 0, 0, dtl, dcnt, dgv, dsrt, dret);
    B.sync(); B.back(srt_out, dsrt, ncases * 64); B.back(ret, dret, ncases);
    return (int)B.err;
}
// row_leaves on one wave: owner[V], hs[4], tids[64] (0xFFFFFFFF or a tile with tile * 64 < V), gvs[4] (-1 or a voxel < V), cap <= QL.
// qt_out[64] (the four rows' tile tables), ql_out[4 x (QL + 32)] (0xFFFFFFFF where nothing was written), scal[3 x 64] = count, nd, kept of every lane
int kp_row_leaves(const uint32_t* owner, uint32_t V, const uint32_t* hs, const uint32_t* tids, const int* gvs, uint32_t cap, uint32_t* qt_out, uint32_t* ql_out, uint32_t* scal) {
    if (!owner || !hs || !tids || !gvs || !qt_out || !ql_out || !scal || V < 1 || V > KP_MAX_N || cap < 1 || cap > KP_QL) return KP_EARG;
    for (int l = 0; l < 64; ++l) if (tids[l] != 0xFFFFFFFFu && (uint64_t)tids[l] * 64u >= V) return KP_EARG;
    for (int r = 0; r < 4; ++r) if (gvs[r] < -1 || (gvs[r] >= 0 && (uint32_t)gvs[r] >= V)) return KP_EARG;
    Bufs B;
    const uint32_t* down = B.mk<uint32_t>(V, owner);
    const uint32_t* dh = B.mk<uint32_t>(4, hs);
    const uint32_t* dt = B.mk<uint32_t>(64, tids);
    const int* dg = B.mk<int>(4, gvs);
    uint32_t *dqt = B.mk<uint32_t>(64), *dql = B.mk<uint32_t>(4 * (KP_QL + 32)), *ds = B.mk<uint32_t>(192);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL(kp_row_leaves_k, dim3(1), dim3(64), 0, 0, down, V, dh, dt, dg, cap, dqt, dql, ds);
    B.sync(); B.back(qt_out, dqt, 64); B.back(ql_out, dql, 4 * (KP_QL + 32)); B.back(scal, ds, 192);
    return (int)B.err;
}
// out[2 x gx x nf x 2]: (frame, vbx) of every workgroup in linear order from f3ds_vblock, then the same from f3ds_frame() / BIX
int kp_vblock(uint32_t gx, uint32_t nf, uint32_t* out) {
    if (!out || gx < 1 || nf < 1 || gx > 4096 || nf > 4096) return KP_EARG;
    Bufs B;
    uint32_t* d = B.mk<uint32_t>((size_t)4 * gx * nf);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL(kp_vblock_k, dim3(gx, nf), dim3(64), 0, 0, d);
    B.sync(); B.back(out, d, (size_t)4 * gx * nf);
    return (int)B.err;
}

// d_centroid at sweep t = 0 on a hand-built SweepFrame.  Arrays by label have S0 + 1 entries, by voxel V; tl has (S0 + 1) x HT_CAP.  In and out:
// ghost_active, ghost_done, hcount, tcnt, tl, hc[(S0 + 1) x 12].  ctl = {n_changed, thr, sweep_marks, sweep_idle, gx (0: as seg_sweeps_on)}.
// Every other pointer member of the frame points at a zero-filled buffer of its product size (none is null); the state must be one in which
// nothing marks tiles (the neighbour tables are all zero): !(n_changed <= thr && sweep_marks == 1).
int kp_centroid(uint32_t S0, uint32_t V, const uint32_t* owner, const float* vf, unsigned char* ghost_active, unsigned char* ghost_done, const int* ghost_vox,
                const uint32_t* hlo, const uint32_t* hhi, uint32_t* hcount, uint32_t* tl, uint32_t* tcnt, float* hc, const uint32_t* ctl) {
    if (!owner || !vf || !ghost_active || !ghost_done || !ghost_vox || !hlo || !hhi || !hcount || !tl || !tcnt || !hc || !ctl) return KP_EARG;
    if (V < 1 || V > KP_MAX_N || S0 > 65536) return KP_EARG;
    const uint32_t n_changed = ctl[0], thr = ctl[1], marks = ctl[2], idle = ctl[3];
    if (n_changed <= thr && marks == 1u) return KP_EARG;
    const uint32_t gx = ctl[4] ? ctl[4] : kp_grid_for((size_t)S0 * 64u, 256);
    if (gx > 2048) return KP_EARG;
    for (uint32_t h = 0; h <= S0; ++h) {
        if (tcnt[h] > HT_CAP + 1u) return KP_EARG;
        for (uint32_t i = 0; i < tcnt[h] && i < HT_CAP; ++i) if ((uint64_t)tl[(size_t)h * HT_CAP + i] * 64u >= V) return KP_EARG;
        if (ghost_vox[h] < -1 || (ghost_vox[h] >= 0 && (uint32_t)ghost_vox[h] >= V)) return KP_EARG;
        if (hlo[h] > hhi[h] || hhi[h] >= V) return KP_EARG;
    }
    const uint32_t T = (V + 63u) / 64u, NT = (V + NT_TILE - 1) / NT_TILE;
    Bufs B;
    const size_t L = (size_t)S0 + 1;
    uint32_t* down = B.mk<uint32_t>(V, owner);
    const float* dvf = B.mk<float>((size_t)V * 12, vf);
    float* ddist = B.mk<float>(V);
    float* dhc = B.mk<float>(L * 12, hc);
    uint32_t *dghead = B.mk<uint32_t>(V), *dgnext = B.mk<uint32_t>(L);
    DevCounters hdc;
    memset(&hdc, 0, sizeof hdc);
    hdc.n_changed = n_changed; hdc.sweep_marks = marks; hdc.sweep_idle = idle;
    DevCounters* ddc = B.mk<DevCounters>(1, &hdc);
    const int* dnbrT = B.mk<int>((size_t)27 * V);
    const int* dnbr = B.mk<int>((size_t)27 * V);
    SweepFrame a;
    a.sv = SweepView{(int)V, dnbrT, dvf, down, ddist, dhc, dghead, dgnext, ddc ? &ddc->n_ghosts : nullptr, 0.2f, 1.0f, 1.0f, 1.0f, dnbr};
    a.R = B.mk<unsigned char>(V); a.ownR = B.mk<uint32_t>(V); a.owner_out = down; a.dist_out = ddist;
    a.ghost_done = B.mk<unsigned char>(L, ghost_done); a.ghost_active = B.mk<unsigned char>(L, ghost_active); a.ghost_vox = B.mk<int>(L, ghost_vox);
    a.ghost_head = dghead; a.ghost_next = dgnext;
    a.hlo = B.mk<uint32_t>(L, hlo); a.hhi = B.mk<uint32_t>(L, hhi); a.hcount = B.mk<uint32_t>(L, hcount); a.hc = dhc; a.dc = ddc; a.S0 = S0;
    uint32_t* tiles4 = B.mk<uint32_t>((size_t)4 * T);
    a.tR0 = tiles4; a.tR1 = tiles4 + T; a.tC0 = tiles4 + 2 * (size_t)T; a.tC1 = tiles4 + 3 * (size_t)T;
    a.tRr = B.mk<uint32_t>((size_t)(F3DS_R_ROUNDS > 1 ? F3DS_R_ROUNDS - 1 : 1) * T); a.hD = B.mk<uint32_t>(L); a.T = T;
    a.tl = B.mk<uint32_t>(L * HT_CAP, tl); a.tcnt = B.mk<uint32_t>(L, tcnt);
    a.wl = B.mk<uint32_t>(V); a.wl2 = B.mk<uint32_t>(V); a.tmask = B.mk<uint32_t>(V);
    a.thr = thr;
    a.tile_n1 = B.mk<uint32_t>(NT); a.tile_ord = B.mk<uint32_t>((size_t)NT * NT_RING1); a.tile_slots = B.mk<uint32_t>((size_t)NT * SW_SLOT_WORDS * NT_TILE);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL((kp_call<d_centroid, SweepFrame, uint32_t>), dim3(gx, 1), dim3(d_centroid::BLOCK), 0, 0, a, 0u);
    B.sync();
    B.back(ghost_active, (const unsigned char*)a.ghost_active, L); B.back(ghost_done, (const unsigned char*)a.ghost_done, L);
    B.back(hcount, (const uint32_t*)a.hcount, L); B.back(tl, (const uint32_t*)a.tl, L * HT_CAP); B.back(tcnt, (const uint32_t*)a.tcnt, L); B.back(hc, (const float*)dhc, L * 12);
    return (int)B.err;
}

// d_sv_fill on the states d_centroid left, launched as seg_supervoxels does.  loff[S0 + 2] = exclusive prefix of hcount.  Checked before the launch: hcount[h] is
// the number of leaves the kernel will find for h (its payload rows are written at loff[h] + 0 .. count - 1), and every helper's rows end inside the buffers.
// Out: rows[(V + S0 + 1) x 12], row_voxel[V + S0 + 1], rcnt0, ralive0 (pre-zeroed), *n_alive; in and out: racc0[(S0 + 1) x 12], rrec0[(S0 + 1) x 16] (the host does not clear them).
int kp_sv_fill(uint32_t S0, uint32_t V, const uint32_t* owner, const float* vf, const unsigned char* ghost_active, const int* ghost_vox, const uint32_t* hlo, const uint32_t* hhi,
               const uint32_t* hcount, const uint32_t* loff, const float* hc, const uint32_t* tl, const uint32_t* tcnt,
               float* rows, int* row_voxel, float* racc0, uint32_t* rcnt0, float* rrec0, unsigned char* ralive0, uint32_t* n_alive) {
    if (!owner || !vf || !ghost_active || !ghost_vox || !hlo || !hhi || !hcount || !loff || !hc || !tl || !tcnt || !rows || !row_voxel || !racc0 || !rcnt0 || !rrec0 || !ralive0 || !n_alive)
        return KP_EARG;
    if (V < 1 || V > KP_MAX_N || S0 > 65536) return KP_EARG;
    const size_t L = (size_t)S0 + 1, NR = (size_t)V + S0 + 1;
    for (uint32_t h = 0; h <= S0; ++h) {
        if (tcnt[h] > HT_CAP + 1u) return KP_EARG;
        for (uint32_t i = 0; i < tcnt[h] && i < HT_CAP; ++i) if ((uint64_t)tl[(size_t)h * HT_CAP + i] * 64u >= V) return KP_EARG;
        if (ghost_vox[h] < -1 || (ghost_vox[h] >= 0 && (uint32_t)ghost_vox[h] >= V)) return KP_EARG;
        if (hlo[h] > hhi[h] || hhi[h] >= V) return KP_EARG;
    }
    if (loff[0] != 0u) return KP_EARG;
    for (uint32_t h = 1; h <= S0; ++h) {
        // the leaves d_sv_fill will find: the voxels h owns (and its ghost leaf) in the distinct tiles of its list, or in hlo..hhi when the list overflowed
        const int gv = ghost_active[h] ? ghost_vox[h] : -1;
        std::vector<uint32_t> tiles;
        bool window = tcnt[h] > HT_CAP;
        if (!window) {
            tiles.assign(tl + (size_t)h * HT_CAP, tl + (size_t)h * HT_CAP + tcnt[h]);
            if (gv >= 0) tiles.push_back((uint32_t)gv >> 6);
            const size_t raw = tiles.size();
            std::sort(tiles.begin(), tiles.end());
            tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
            if (raw > 64 && tiles.size() > 64) window = true;
        }
        if (window) { tiles.clear(); for (uint32_t t = hlo[h] >> 6; t <= hhi[h] >> 6; ++t) tiles.push_back(t); }
        uint32_t count = 0;
        for (uint32_t t : tiles) for (uint32_t v = t * 64u; v < t * 64u + 64u && v < V; ++v) count += owner[v] == h || (int)v == gv;
        if (count != hcount[h] || loff[h] != loff[h - 1] + hcount[h - 1] || (size_t)loff[h] + count > NR) return KP_EARG;
    }
    Bufs B;
    const uint32_t* down = B.mk<uint32_t>(V, owner);
    const float* dvf = B.mk<float>((size_t)V * 12, vf);
    const unsigned char* dga = B.mk<unsigned char>(L, ghost_active);
    const int* dgv = B.mk<int>(L, ghost_vox);
    const uint32_t *dlo = B.mk<uint32_t>(L, hlo), *dhi = B.mk<uint32_t>(L, hhi), *dcnt = B.mk<uint32_t>(L, hcount), *dloff = B.mk<uint32_t>(L + 1, loff);
    const float* dhc = B.mk<float>(L * 12, hc);
    const uint32_t *dtl = B.mk<uint32_t>(L * HT_CAP, tl), *dtc = B.mk<uint32_t>(L, tcnt);
    float* drows = B.mk<float>(NR * 12); int* drv = B.mk<int>(NR);
    float* dracc = B.mk<float>(L * 12, racc0); uint32_t* drcnt = B.mk<uint32_t>(L); float* drrec = B.mk<float>(L * 16, rrec0); unsigned char* dral = B.mk<unsigned char>(L);
    DevCounters* ddc = B.mk<DevCounters>(1);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL((kp_call<d_sv_fill, const float*, const uint32_t*, uint32_t, const uint32_t*, const uint32_t*, const int*, const unsigned char*, const uint32_t*, const uint32_t*,
                                const float*, float*, int*, float*, uint32_t*, float*, unsigned char*, DevCounters*, const uint32_t*, const uint32_t*, uint32_t>),
                       dim3(S0 ? (S0 + 3u) / 4u : 1u, 1), dim3(d_sv_fill::BLOCK), 0, 0,
                       dvf, down, S0, dlo, dhi, dgv, dga, dcnt, dloff, dhc, drows, drv, dracc, drcnt, drrec, dral, ddc, dtl, dtc, V);
    B.sync();
    B.back(rows, (const float*)drows, NR * 12); B.back(row_voxel, (const int*)drv, NR); B.back(racc0, (const float*)dracc, L * 12); B.back(rcnt0, (const uint32_t*)drcnt, L);
    B.back(rrec0, (const float*)drrec, L * 16); B.back(ralive0, (const unsigned char*)dral, L);
    DevCounters hd;
    memset(&hd, 0, sizeof hd);
    B.back(&hd, (const DevCounters*)ddc, 1);
    *n_alive = hd.n_alive;
    return (int)B.err;
}

// ---- the seed stage (d_chunkbox + d_seed_grow; d_cell_hash + d_seed_nn; d_cell_hash + d_seed_filter), launched with the widths seg_seed_grid / seg_seeds give them.
// d_seed_grow on vf[V x 12] (xyz finite: checked).  Its loop ends: every trip moves the cursor forward or sets the error, and a_seed_grow stops at depth 22.
// ints[7 + 5 x F3DS_MAX_SEED_EVENTS] = n_events, error, defined, depth, off[3], then (trigger, depth, off[3]) per event; dbls[7 + 3 x F3DS_MAX_SEED_EVENTS] = res, min[3], max[3], then min[3] per event;
// dc_out[2] = the sdepth and the error d_seed_grow left in the counters
int kp_seed_grow(const float* vf, uint32_t V, float seed_res, int* ints, double* dbls, int* dc_out) {
    if (!vf || !ints || !dbls || !dc_out || V < 1 || V > KP_MAX_N || !(seed_res > 0.0f) || !std::isfinite(seed_res)) return KP_EARG;
    for (size_t v = 0; v < V; ++v) for (int a = 0; a < 3; ++a) if (!std::isfinite(vf[v * 12 + a])) return KP_EARG;
    const uint32_t nchunks = (V + SEED_CHUNK - 1) / SEED_CHUNK;
    Bufs B;
    const float* dvf = B.mk<float>((size_t)V * 12, vf);
    float* boxes = B.mk<float>((size_t)nchunks * 6);
    DevCounters hdc;
    memset(&hdc, 0, sizeof hdc);
    hdc.n_voxels = V;
    DevCounters* ddc = B.mk<DevCounters>(1, &hdc);
    SeedGrid* dg = B.mk<SeedGrid>(1);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL((kp_call<d_chunkbox, const float*, const DevCounters*, float*>), dim3(nchunks, 1), dim3(d_chunkbox::BLOCK), 0, 0, dvf, (const DevCounters*)ddc, boxes);
    hipLaunchKernelGGL((kp_call<d_seed_grow, const float*, const float*, DevCounters*, float, SeedGrid*>), dim3(1, 1), dim3(d_seed_grow::BLOCK), 0, 0, dvf, (const float*)boxes, ddc, seed_res, dg);
    B.sync();
    SeedGrid g;
    memset(&g, 0, sizeof g);
    B.back(&g, (const SeedGrid*)dg, 1); B.back(&hdc, (const DevCounters*)ddc, 1);
    if (B.err != hipSuccess) return (int)B.err;
    ints[0] = g.n_events; ints[1] = g.error; ints[2] = g.defined; ints[3] = g.depth;
    dbls[0] = g.res;
    for (int a = 0; a < 3; ++a) { ints[4 + a] = (int)g.off[a]; dbls[1 + a] = g.min[a]; dbls[4 + a] = g.max[a]; }
    for (int e = 0; e < F3DS_MAX_SEED_EVENTS; ++e) {
        const bool live = e < g.n_events;
        ints[7 + 5 * e] = live ? g.ev[e].trigger : 0; ints[8 + 5 * e] = live ? g.ev[e].depth : 0;
        for (int a = 0; a < 3; ++a) { ints[9 + 5 * e + a] = live ? (int)g.ev[e].off[a] : 0; dbls[7 + 3 * e + a] = live ? g.ev[e].min[a] : 0.0; }
    }
    dc_out[0] = hdc.sdepth; dc_out[1] = hdc.error;
    return 0;
}
}  // extern "C"
namespace {
// the cell tables of seg_seeds: sorted_vox[n] (voxels < V), cell_start[C + 1] (0 = first, ascending strictly: no empty cell, last = n), ckey[V x 3] below 2^21 - 1 (a
// neighbour's key still packs), one key per cell and no key twice.  The hash has pow2_ge(2 C + 16) slots, so every probe sequence meets an empty one.
bool seed_tables_ok(const float* vf, uint32_t V, const uint32_t* ckey, const uint32_t* sorted_vox, uint32_t n, const uint32_t* cell_start, uint32_t C, const double* grid) {
    if (!vf || !ckey || !sorted_vox || !cell_start || !grid || V < 1 || V > KP_MAX_N || n < 1 || n > V || C < 1 || C > n) return false;
    if (!(grid[0] > 0.0) || !std::isfinite(grid[0]) || !std::isfinite(grid[1]) || !std::isfinite(grid[2]) || !std::isfinite(grid[3])) return false;
    if (cell_start[0] != 0u || cell_start[C] != n) return false;
    std::vector<uint64_t> keys;
    for (uint32_t c = 0; c < C; ++c) {
        if (cell_start[c] >= cell_start[c + 1] || cell_start[c + 1] > n) return false;
        for (uint32_t i = cell_start[c]; i < cell_start[c + 1]; ++i) {
            const uint32_t v = sorted_vox[i], v0 = sorted_vox[cell_start[c]];
            if (v >= V) return false;
            for (int a = 0; a < 3; ++a) if (ckey[v * 3 + a] >= (1u << 21) - 1u || ckey[v * 3 + a] != ckey[v0 * 3 + a]) return false;
        }
        const uint32_t v0 = sorted_vox[cell_start[c]];
        keys.push_back(n_pack_key(ckey[v0 * 3], ckey[v0 * 3 + 1], ckey[v0 * 3 + 2]));
    }
    std::sort(keys.begin(), keys.end());
    return std::adjacent_find(keys.begin(), keys.end()) == keys.end();
}
uint32_t kp_pow2_ge(size_t x) { uint32_t p = 1; while (p < x) p <<= 1; return p; }
struct SeedTables { const float* vf; const uint32_t *ckey, *sorted_vox, *cell_start, *hvals; const uint64_t* hkeys; const DevCounters* dc; const SeedGrid* grid; uint32_t hmask; };
// copies the tables in and builds the hash with d_cell_hash, as seg_seeds does; extra = cells' worth of workgroups beyond what C needs
SeedTables seed_tables_on(Bufs& B, const float* vf, uint32_t V, const uint32_t* ckey, const uint32_t* sorted_vox, uint32_t n, const uint32_t* cell_start, uint32_t C, const double* grid) {
    SeedTables t;
    memset(&t, 0, sizeof t);
    t.vf = B.mk<float>((size_t)V * 12, vf); t.ckey = B.mk<uint32_t>((size_t)V * 3, ckey); t.sorted_vox = B.mk<uint32_t>(n, sorted_vox); t.cell_start = B.mk<uint32_t>((size_t)C + 1, cell_start);
    const uint32_t ccap = kp_pow2_ge((size_t)C * 2 + 16);
    uint64_t* hk = B.mk<uint64_t>(ccap); uint32_t* hv = B.mk<uint32_t>(ccap);
    if (B.err == hipSuccess) B.err = hipMemset(hk, 0xFF, (size_t)ccap * 8);
    DevCounters hdc;
    memset(&hdc, 0, sizeof hdc);
    hdc.n_voxels = V; hdc.n_cells = C;
    SeedGrid g;
    memset(&g, 0, sizeof g);
    g.defined = 1; g.res = grid[0];
    for (int a = 0; a < 3; ++a) g.min[a] = grid[1 + a];
    t.dc = B.mk<DevCounters>(1, &hdc); t.grid = B.mk<SeedGrid>(1, &g);
    t.hkeys = hk; t.hvals = hv; t.hmask = ccap - 1u;
    if (B.err != hipSuccess) return t;
    hipLaunchKernelGGL((kp_call<d_cell_hash, const uint32_t*, const uint32_t*, const uint32_t*, const DevCounters*, uint64_t*, uint32_t*, uint32_t>), dim3(kp_grid_for(C, 256), 1), dim3(d_cell_hash::BLOCK), 0, 0,
                       t.ckey, t.sorted_vox, t.cell_start, t.dc, hk, hv, ccap - 1u);
    return t;
}
}  // namespace
extern "C" {
// d_seed_nn on hand-built cell tables (seed_tables_ok).  grid[4] = res, min[3] of the seed grid.  seed_orig[C + 4 extra]: the words behind C come back as they went in
// (-1), whatever the extra workgroups do (extra: workgroups beyond (C + 3) / 4, as a batched launch has them)
int kp_seed_nn(const float* vf, uint32_t V, const uint32_t* ckey, const uint32_t* sorted_vox, uint32_t n, const uint32_t* cell_start, uint32_t C, const double* grid, uint32_t extra, int* seed_orig) {
    if (!seed_orig || extra > 64 || !seed_tables_ok(vf, V, ckey, sorted_vox, n, cell_start, C, grid)) return KP_EARG;
    Bufs B;
    const SeedTables t = seed_tables_on(B, vf, V, ckey, sorted_vox, n, cell_start, C, grid);
    std::vector<int> init((size_t)C + 4u * extra, -1);
    int* dso = B.mk<int>(init.size(), init.data());
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL((kp_call<d_seed_nn, const float*, const uint32_t*, const uint32_t*, const uint32_t*, const DevCounters*, const SeedGrid*, const uint64_t*, const uint32_t*, uint32_t, int*>),
                       dim3((C + 3u) / 4u + extra, 1), dim3(d_seed_nn::BLOCK), 0, 0, t.vf, t.ckey, t.sorted_vox, t.cell_start, t.dc, t.grid, t.hkeys, t.hvals, t.hmask, dso);
    B.sync(); B.back(seed_orig, (const int*)dso, init.size());
    return (int)B.err;
}
// d_seed_filter on the same tables and seed_orig[C] (every entry a voxel < V: checked).  keep[C + 4 extra]: 0 / 1, and 0xFFFFFFFF behind C
int kp_seed_filter(const float* vf, uint32_t V, const uint32_t* ckey, const uint32_t* sorted_vox, uint32_t n, const uint32_t* cell_start, uint32_t C, const double* grid, uint32_t extra,
                   const int* seed_orig, float r2, float min_points, uint32_t* keep) {
    if (!seed_orig || !keep || extra > 64 || !std::isfinite(r2) || !std::isfinite(min_points) || !seed_tables_ok(vf, V, ckey, sorted_vox, n, cell_start, C, grid)) return KP_EARG;
    for (uint32_t c = 0; c < C; ++c) if (seed_orig[c] < 0 || (uint32_t)seed_orig[c] >= V) return KP_EARG;
    Bufs B;
    const SeedTables t = seed_tables_on(B, vf, V, ckey, sorted_vox, n, cell_start, C, grid);
    const int* dso = B.mk<int>(C, seed_orig);
    std::vector<uint32_t> init((size_t)C + 4u * extra, 0xFFFFFFFFu);
    uint32_t* dk = B.mk<uint32_t>(init.size(), init.data());
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL((kp_call<d_seed_filter, const float*, const uint32_t*, const uint32_t*, const uint32_t*, const DevCounters*, const SeedGrid*, const uint64_t*, const uint32_t*, uint32_t, const int*, float, float, uint32_t*>),
                       dim3((C + 3u) / 4u + extra, 1), dim3(d_seed_filter::BLOCK), 0, 0, t.vf, t.ckey, t.sorted_vox, t.cell_start, t.dc, t.grid, t.hkeys, t.hvals, t.hmask, dso, r2, min_points, dk);
    B.sync(); B.back(keep, (const uint32_t*)dk, init.size());
    return (int)B.err;
}
}  // extern "C"
namespace {
constexpr uint32_t KP_MAX_SWEEPS = 140;
// The start-of-run contract of kp_sweeps: the state createSupervoxelHelpers / reseedSupervoxels / a finished run of sweeps could have left, as far as the sweep kernels
// read it.  Arrays by voxel have V entries, by label S0 + 1 (row 0 is nobody's: no leaf, no ghost, empty books).
//   owner <= S0;  dist = FLT_MAX where owner is 0, finite and >= 0 elsewhere;  hc and the nine feature words of every voxel finite;
//   nbr[v][k] is -1 or a voxel, slot 13 is v itself, and u = nbr[v][k] has v in its slot 26 - k (the marks of the dirty-tile scheme go to N(v) and are meant for the
//   voxels that have v in theirs: the table of a lattice, and of d_neighbors);
//   a helper has at most one ghost leaf (ghost_active 0 | 1; ghost_vox a voxel whose owner has a HIGHER label -- createSupervoxelHelpers' last seed owns -- or -1);
//   hcount = voxels owned + the ghost leaf;  hlo <= every leaf <= hhi < V (0, 0 for a helper without leaves);  tcnt <= HT_CAP lists tiles below T, among them every tile
//   the helper owns a voxel in (d_helper_init: the seed's tile, nothing for a ghost seed; d_centroid: exactly those tiles), or tcnt = HT_CAP + 1: the ordinal window.
bool sweep_state_ok(uint32_t V, uint32_t S0, const int* nbr, const float* vf, const uint32_t* owner, const float* dist, const float* hc, const uint32_t* hcount, const uint32_t* hlo,
                    const uint32_t* hhi, const uint32_t* tl, const uint32_t* tcnt, const int* ghost_vox, const unsigned char* ghost_active) {
    const size_t L = (size_t)S0 + 1;
    const uint32_t T = (V + 63u) / 64u;
    for (uint32_t v = 0; v < V; ++v) {
        for (int k = 0; k < 27; ++k) {
            const int u = nbr[(size_t)v * 27 + k];
            if (u < -1 || (u >= 0 && (uint32_t)u >= V)) return false;
            if (u >= 0 && nbr[(size_t)u * 27 + (26 - k)] != (int)v) return false;
        }
        if (nbr[(size_t)v * 27 + 13] != (int)v) return false;
        for (int k = 0; k < 9; ++k) if (!std::isfinite(vf[(size_t)v * 12 + k])) return false;
        if (owner[v] > S0) return false;
        if (owner[v] == 0u) { const float fmax = F3DS_FLT_MAX; if (memcmp(&dist[v], &fmax, 4) != 0) return false; }
        else if (!std::isfinite(dist[v]) || !(dist[v] >= 0.0f)) return false;
    }
    for (size_t i = 0; i < L * 12; ++i) if (!std::isfinite(hc[i])) return false;
    std::vector<uint32_t> cnt(L, 0u), lo(L, 0xFFFFFFFFu), hi(L, 0u);
    auto leaf = [&](uint32_t h, uint32_t v) { cnt[h]++; if (v < lo[h]) lo[h] = v; if (v > hi[h]) hi[h] = v; };
    for (uint32_t v = 0; v < V; ++v) if (owner[v]) leaf(owner[v], v);
    for (uint32_t h = 0; h <= S0; ++h) {
        if (ghost_active[h] > 1) return false;
        if (!ghost_active[h]) { if (ghost_vox[h] != -1) return false; continue; }
        if (h == 0u || ghost_vox[h] < 0 || (uint32_t)ghost_vox[h] >= V || owner[ghost_vox[h]] <= h) return false;
        leaf(h, (uint32_t)ghost_vox[h]);
    }
    if (cnt[0] != 0u) return false;
    std::vector<std::vector<uint32_t>> listed(L);
    for (uint32_t h = 0; h <= S0; ++h) {
        if (hcount[h] != cnt[h]) return false;
        if (cnt[h] ? !(hlo[h] <= lo[h] && hi[h] <= hhi[h] && hhi[h] < V) : (hlo[h] != 0u || hhi[h] != 0u)) return false;
        if (tcnt[h] > HT_CAP + 1u) return false;
        if (tcnt[h] > HT_CAP) continue;
        for (uint32_t i = 0; i < tcnt[h]; ++i) { if (tl[(size_t)h * HT_CAP + i] >= T) return false; listed[h].push_back(tl[(size_t)h * HT_CAP + i]); }
        std::sort(listed[h].begin(), listed[h].end());
    }
    for (uint32_t v = 0; v < V; ++v) {
        const uint32_t h = owner[v];
        if (h && tcnt[h] <= HT_CAP && !std::binary_search(listed[h].begin(), listed[h].end(), v >> 6)) return false;
    }
    return true;
}
}  // namespace
extern "C" {
// The sweep kernels of sweeps 0 .. n - 1 in the order seg_sweeps_on (f3ds_hip.hip) records them, from the caller's start-of-run state (sweep_state_ok above; anything
// else is refused before a device is touched), with the state copied back after every sweep.  Everything private to the device -- stamps, hD, ownR, the memo R, work
// lists, thief masks, ghost chains, the counters -- starts zeroed, as seg_sweeps_on fills it or as sweeps 0 and 1, which are full by construction, rebuild it.
//   in[12] = nbr[V x 27] (row-major; nbrT is derived here), vf[V x 12], owner, dist, hc[(S0 + 1) x 12], hcount, hlo, hhi, tl[(S0 + 1) x HT_CAP], tcnt, ghost_vox, ghost_active
//   w[4] = seed_res, w_normal, w_color, w_spatial
//   ctl[5] = n (<= 140), inc_shift + 1 (0: every sweep full; thr = a_sweep_thr(V, inc_shift), the library's F3DS_INC_SHIFT), r_rounds (1 .. F3DS_R_ROUNDS, its
//            F3DS_R_ROUNDS_RUN), tiles (0: tile_n1 = nullptr, the global-gather path; 1: the tables d_normals_t<384> builds from vf and nbr, as seg_normals launches it --
//            the caller's normals are put back afterwards), gx_cap (0: the widths of grid_for; 1 or 3: every launch wider than that is that wide, as F3DS_GRID_CAP)
//   out[10], per sweep: owner[n x V], dist, hc[n x (S0 + 1) x 12], hcount, ghost_active, ghost_done, tcnt, n_changed[n] (as the claim pass left it);  at the end:
//            sweep_stats[4], tile_n1[(V + 127) / 128] (0xFFFFFFFF: a tile on the global path; all of them with tiles = 0)
int kp_sweeps(uint32_t V, uint32_t S0, const void* const* in, const float* w, const uint32_t* ctl, void* const* out) {
    if (!in || !w || !ctl || !out) return KP_EARG;
    for (int i = 0; i < 12; ++i) if (!in[i]) return KP_EARG;
    for (int i = 0; i < 10; ++i) if (!out[i]) return KP_EARG;
    const uint32_t n = ctl[0], r_rounds = ctl[2], tiles = ctl[3], gx_cap = ctl[4];
    const int inc_shift = (int)ctl[1] - 1;
    if (V < 1 || V > (1u << 20) || S0 > 65536 || n > KP_MAX_SWEEPS || ctl[1] > 33u || r_rounds < 1 || r_rounds > (uint32_t)F3DS_R_ROUNDS || tiles > 1 || (gx_cap != 0 && gx_cap != 1 && gx_cap != 3)) return KP_EARG;
    for (int i = 0; i < 4; ++i) if (!std::isfinite(w[i]) || w[i] < 0.0f) return KP_EARG;
    if (!(w[0] > 0.0f)) return KP_EARG;
    const int* nbr = (const int*)in[0]; const float* vf = (const float*)in[1]; const uint32_t* owner = (const uint32_t*)in[2]; const float* dist = (const float*)in[3];
    const float* hc = (const float*)in[4]; const uint32_t *hcount = (const uint32_t*)in[5], *hlo = (const uint32_t*)in[6], *hhi = (const uint32_t*)in[7], *tl = (const uint32_t*)in[8],
                                          *tcnt = (const uint32_t*)in[9];
    const int* ghost_vox = (const int*)in[10]; const unsigned char* ghost_active = (const unsigned char*)in[11];
    if (!sweep_state_ok(V, S0, nbr, vf, owner, dist, hc, hcount, hlo, hhi, tl, tcnt, ghost_vox, ghost_active)) return KP_EARG;
    const size_t L = (size_t)S0 + 1;
    const uint32_t T = (V + 63u) / 64u, NT = (V + NT_TILE - 1) / NT_TILE;
    std::vector<int> nbrT((size_t)27 * V);
    for (uint32_t v = 0; v < V; ++v) for (int k = 0; k < 27; ++k) nbrT[(size_t)k * V + v] = nbr[(size_t)v * 27 + k];
    auto width = [&](size_t work, int block) { const uint32_t g = kp_grid_for(work, block); return gx_cap && g > gx_cap ? gx_cap : g; };
    Bufs B;
    float* dvf = B.mk<float>((size_t)V * 12, vf);
    const int* dnbr = B.mk<int>((size_t)27 * V, nbr);
    const int* dnbrT = B.mk<int>((size_t)27 * V, nbrT.data());
    uint32_t* down = B.mk<uint32_t>(V, owner);
    float* ddist = B.mk<float>(V, dist);
    float* dhc = B.mk<float>(L * 12, hc);
    uint32_t *dghead = B.mk<uint32_t>(V), *dgnext = B.mk<uint32_t>(L);
    DevCounters hdc;
    memset(&hdc, 0, sizeof hdc);
    hdc.n_voxels = V;
    DevCounters* ddc = B.mk<DevCounters>(1, &hdc);
    SweepFrame a;
    a.sv = SweepView{(int)V, dnbrT, dvf, down, ddist, dhc, dghead, dgnext, ddc ? &ddc->n_ghosts : nullptr, w[0], w[1], w[2], w[3], dnbr};
    a.R = B.mk<unsigned char>(V); a.ownR = B.mk<uint32_t>(V); a.owner_out = down; a.dist_out = ddist;
    a.ghost_done = B.mk<unsigned char>(L); a.ghost_active = B.mk<unsigned char>(L, ghost_active); a.ghost_vox = B.mk<int>(L, ghost_vox);
    a.ghost_head = dghead; a.ghost_next = dgnext;
    a.hlo = B.mk<uint32_t>(L, hlo); a.hhi = B.mk<uint32_t>(L, hhi); a.hcount = B.mk<uint32_t>(L, hcount); a.hc = dhc; a.dc = ddc; a.S0 = S0;
    uint32_t* tiles4 = B.mk<uint32_t>((size_t)4 * T);
    a.tR0 = tiles4; a.tR1 = tiles4 + T; a.tC0 = tiles4 + 2 * (size_t)T; a.tC1 = tiles4 + 3 * (size_t)T;
    a.tRr = B.mk<uint32_t>((size_t)(F3DS_R_ROUNDS > 1 ? F3DS_R_ROUNDS - 1 : 1) * T); a.hD = B.mk<uint32_t>(L); a.T = T;
    a.tl = B.mk<uint32_t>(L * HT_CAP, tl); a.tcnt = B.mk<uint32_t>(L, tcnt);
    a.wl = B.mk<uint32_t>(V); a.wl2 = B.mk<uint32_t>(V); a.tmask = B.mk<uint32_t>(V);
    a.thr = a_sweep_thr(V, inc_shift);
    std::vector<uint32_t> none(NT, SW_TILE_NONE);
    uint32_t* dtn1 = B.mk<uint32_t>(NT, none.data());
    uint32_t* dtord = B.mk<uint32_t>((size_t)NT * NT_RING1);
    uint32_t* dtslots = B.mk<uint32_t>((size_t)NT * SW_SLOT_WORDS * NT_TILE);
    a.tile_n1 = tiles ? dtn1 : nullptr; a.tile_ord = dtord; a.tile_slots = dtslots;
    if (B.err != hipSuccess) return (int)B.err;
    if (tiles) {
        hipLaunchKernelGGL((kp_call_w<d_normals_t<384>, float*, const int*, const DevCounters*, uint32_t*, uint32_t*, uint32_t*, uint32_t>), dim3(NT, 1), dim3(384), 0, 0,
                           dvf, dnbr, (const DevCounters*)ddc, dtn1, dtord, dtslots, 0u);
        B.sync();
        if (B.err == hipSuccess) B.err = hipMemcpy(dvf, vf, (size_t)V * 48, hipMemcpyHostToDevice);      // the caller's normals, not the ones the kernel computed on the way
        if (B.err != hipSuccess) return (int)B.err;
    }
    for (uint32_t t = 0; t < n; ++t) {
        if (a_sweep_needs_clear(t)) B.err = hipMemset(a.R, 0, V);
        if (B.err != hipSuccess) return (int)B.err;
        const unsigned char tag = a_sweep_tag(t);
        hipLaunchKernelGGL((kp_call_w<d_sweep_begin, SweepFrame, uint32_t>), dim3(1, 1), dim3(d_sweep_begin::BLOCK), 0, 0, a, t);
        const uint32_t nrounds = inc_shift >= 0 && t >= 2u ? r_rounds : 0u;      // (as seg_sweeps_on: sweeps 0 and 1 are full by construction)
        hipLaunchKernelGGL((kp_call_w<d_sweep_R_first, SweepFrame, unsigned char, uint32_t, uint32_t>), dim3(width(V, 256), 1), dim3(d_sweep_R_first::BLOCK), 0, 0, a, tag, t, nrounds);
        for (uint32_t r = 1; r < nrounds; ++r)
            hipLaunchKernelGGL((kp_call_w<d_sweep_R_round, SweepFrame, uint32_t, uint32_t, uint32_t>), dim3(width(V, 256), 1), dim3(d_sweep_R_round::BLOCK), 0, 0, a, t, r, nrounds);
        for (uint32_t pass = 0; pass < F3DS_R_PASSES; ++pass)
            hipLaunchKernelGGL((kp_call_w<d_sweep_R, SweepFrame, unsigned char, uint32_t, uint32_t>), dim3(pass == 0 ? width(V, 256) : (gx_cap ? gx_cap : 64u), 1), dim3(d_sweep_R::BLOCK), 0, 0, a, tag, t, pass);
        hipLaunchKernelGGL((kp_call_w<d_sweep_R_tail, SweepFrame, unsigned char, uint32_t>), dim3(1, 1), dim3(d_sweep_R_tail::BLOCK), 0, 0, a, tag, t);
        hipLaunchKernelGGL((kp_call_w<d_sweep_claim, SweepFrame, uint32_t>), dim3(width(V, 256), 1), dim3(d_sweep_claim::BLOCK), 0, 0, a, t);
        hipLaunchKernelGGL((kp_call_w<d_centroid, SweepFrame, uint32_t>), dim3(width((size_t)S0 * 64u, 256), 1), dim3(d_centroid::BLOCK), 0, 0, a, t);
        B.sync();
        B.back((uint32_t*)out[0] + (size_t)t * V, (const uint32_t*)down, V); B.back((float*)out[1] + (size_t)t * V, (const float*)ddist, V);
        B.back((float*)out[2] + (size_t)t * L * 12, (const float*)dhc, L * 12); B.back((uint32_t*)out[3] + (size_t)t * L, (const uint32_t*)a.hcount, L);
        B.back((unsigned char*)out[4] + (size_t)t * L, (const unsigned char*)a.ghost_active, L); B.back((unsigned char*)out[5] + (size_t)t * L, (const unsigned char*)a.ghost_done, L);
        B.back((uint32_t*)out[6] + (size_t)t * L, (const uint32_t*)a.tcnt, L);
        B.back(&hdc, (const DevCounters*)ddc, 1);
        if (B.err != hipSuccess) return (int)B.err;      // (nothing more is launched after an error)
        ((uint32_t*)out[7])[t] = hdc.n_changed;
        if (hdc.r_overflow) return KP_EARG - 1;          // the tail made no progress: cannot happen
    }
    B.back(&hdc, (const DevCounters*)ddc, 1); B.back((uint32_t*)out[9], (const uint32_t*)dtn1, NT);
    if (B.err != hipSuccess) return (int)B.err;
    memcpy(out[8], hdc.sweep_stats, sizeof hdc.sweep_stats);
    if (!tiles) for (uint32_t i = 0; i < NT; ++i) ((uint32_t*)out[9])[i] = SW_TILE_NONE;
    return 0;
}

}  // extern "C"
