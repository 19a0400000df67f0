// The dispatch table of devprobe_fns.h as device code for gfx950, compiled with the product's own flags (tests/devprobe/Makefile reads them
// from csrc/Makefile), plus wave-shaped kernels for the device-only restatements of csrc/f3ds_quad.h, each beside its one-lane original in
// the same launch.  Test infrastructure only (tests/test_devprobe_gpu.py).  The kernels are elementwise with bounded loops; every host entry
// point allocates, copies, launches, synchronises, copies back, frees and returns the HIP error code.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "devprobe_fns.h"

using namespace f3ds;

namespace {
#include "../../fast-3d-pointcloud-segmentation_amd/csrc/f3ds_quad.h"

constexpr int ROWS_BLOCK = 256;
constexpr int MAX_GRID = 8192;

// one row per lane, grid-stride; LDS: the f64 constants through m_lds over an LDS copy of the table, as the merge kernel has them
template <bool LDS>
__global__ void __launch_bounds__(ROWS_BLOCK) dp_rows(int fn, const uint32_t* in, uint32_t* out, size_t n, int ni, int no) {
    __shared__ double s_tab[MC_COUNT];
    if (LDS) { m_table_fill(s_tab, (int)threadIdx.x, ROWS_BLOCK); __syncthreads(); }
    for (size_t r = (size_t)blockIdx.x * ROWS_BLOCK + threadIdx.x; r < n; r += (size_t)gridDim.x * ROWS_BLOCK) {
        if (LDS) dp_eval(fn, in + r * (size_t)ni, out + r * (size_t)no, m_lds_here(s_tab));
        else dp_eval(fn, in + r * (size_t)ni, out + r * (size_t)no, m_lit());
    }
}

// The wave kernels below run one wave per block; a wave's loop is uniform (its bounds depend on the block only), so every lane is active
// inside the lane-parallel functions: a wave past the end repeats the last row and does not store.

// n_ciede00_quad on every quad of a wave, one colour pair (a DP_CIEDE00 row) per quad.
// out, 27 words per row: n_ciede00 on one lane | the four lanes' results with m_lit | the four lanes' results with m_lds |
//                        the radicands in double (two words each): n_ciede00_sq on one lane | n_ciede00_quad_sq of the four lanes with m_lit | with m_lds
__global__ void __launch_bounds__(64) dp_ciede_quad(const uint32_t* in, uint32_t* out, size_t n) {
    __shared__ double s_tab[MC_COUNT];
    m_table_fill(s_tab, (int)threadIdx.x, 64);
    __syncthreads();
    const int lane = (int)threadIdx.x, q = lane & 3;
    for (size_t base = (size_t)blockIdx.x * 16; base < n; base += (size_t)gridDim.x * 16) {
        const size_t row = base + (size_t)(lane >> 2), r = row < n ? row : n - 1;
        float f[6];
        dp_floats(in + r * 6, f, 6);
        const float one = n_ciede00(f, f + 3);
        const float ql = n_ciede00_quad(f, f + 3, q, m_lit());
        const float qt = n_ciede00_quad(f, f + 3, q, m_lds_here(s_tab));
        const double sone = n_ciede00_sq(f, f + 3);
        const double sl = n_ciede00_quad_sq(f, f + 3, q, m_lit());
        const double st = n_ciede00_quad_sq(f, f + 3, q, m_lds_here(s_tab));
        if (row < n) {
            uint32_t* o = out + row * 27;
            if (q == 0) { o[0] = m_bitsf(one); dp_put_d(o + 9, sone); }
            o[1 + q] = m_bitsf(ql); o[5 + q] = m_bitsf(qt);
            dp_put_d(o + 11 + 2 * q, sl); dp_put_d(o + 19 + 2 * q, st);
        }
    }
}
// edge_weight_quad likewise on DP_EDGE_WEIGHT rows (colour metric 0: the quad version is LAB_CIEDE00 only).
// out, 18 words per row: a_edge_weight on one lane (weight, err) | 4 x (weight, err) with m_lit | 4 x (weight, err) with m_lds
__global__ void __launch_bounds__(64) dp_edge_quad(const uint32_t* in, uint32_t* out, size_t n) {
    __shared__ double s_tab[MC_COUNT];
    m_table_fill(s_tab, (int)threadIdx.x, 64);
    __syncthreads();
    const int lane = (int)threadIdx.x, q = lane & 3;
    constexpr int NI = 29 + 2 * DP_CDF;
    for (size_t base = (size_t)blockIdx.x * 16; base < n; base += (size_t)gridDim.x * 16) {
        const size_t row = base + (size_t)(lane >> 2), r = row < n ? row : n - 1;
        const uint32_t* w = in + r * NI;
        float f[24], cc[DP_CDF], cg[DP_CDF];
        dp_floats(w, f, 24); dp_floats(w + 29, cc, DP_CDF); dp_floats(w + 29 + DP_CDF, cg, DP_CDF);
        const MergeParams p = dp_merge_params(w + 26, 0, (int)w[25], cc, cg);
        int e0 = 0, e1 = 0, e2 = 0;
        const float one = a_edge_weight(p, f, f + 12, &e0);
        const float ql = edge_weight_quad(p, f, f + 12, q, &e1, m_lit());
        const float qt = edge_weight_quad(p, f, f + 12, q, &e2, m_lds_here(s_tab));
        if (row < n) {
            uint32_t* o = out + row * 18;
            if (q == 0) { o[0] = m_bitsf(one); o[1] = (uint32_t)e0; }
            o[2 + 2 * q] = m_bitsf(ql); o[3 + 2 * q] = (uint32_t)e1;
            o[10 + 2 * q] = m_bitsf(qt); o[11 + 2 * q] = (uint32_t)e2;
        }
    }
}

// lanes (of the 64-bit ballot) whose three / four / seven words differ from those of lane `first`
__device__ inline unsigned long long dp_differs(const float* v, int n, int first) {
    bool d = false;
    for (int k = 0; k < n; ++k) d = d || m_bitsf(v[k]) != m_bitsf(__shfl(v[k], first, 64));
    return __ballot(d);
}
// lab_three_lanes on DP_RGB2LAB rows.  rows_per_wave = 1: base = 0, one colour per wave (all 64 lanes compared); 4: base = 16 r, one colour per row
// of 16 lanes (the 16 lanes of the row compared).
// out, 13 words per row: n_rgb2lab on one lane | m_lit: lab[3] of the first lane, mask of the lanes that differ from it (2 words) | m_lds: the same
template <int ROWS_PER_WAVE>
__global__ void __launch_bounds__(64) dp_lab_three(const uint32_t* in, uint32_t* out, size_t n) {
    __shared__ double s_tab[MC_COUNT];
    m_table_fill(s_tab, (int)threadIdx.x, 64);
    __syncthreads();
    const int lane = (int)threadIdx.x;
    const int sub = ROWS_PER_WAVE == 4 ? lane >> 4 : 0, rb = ROWS_PER_WAVE == 4 ? (lane & 48) : 0, l = ROWS_PER_WAVE == 4 ? (lane & 15) : lane;
    const unsigned long long lanes = ROWS_PER_WAVE == 4 ? 0xFFFFull : ~0ull;
    for (size_t base = (size_t)blockIdx.x * ROWS_PER_WAVE; base < n; base += (size_t)gridDim.x * ROWS_PER_WAVE) {
        const size_t row = base + (size_t)sub, r = row < n ? row : n - 1;
        float rgb[3], one[3], a[3], b[3];
        dp_floats(in + r * 3, rgb, 3);
        n_rgb2lab(rgb, one);
        const float mine = l == 0 ? rgb[0] : (l == 1 ? rgb[1] : rgb[2]);
        lab_three_lanes(mine, l, a, m_lit(), rb);
        lab_three_lanes(mine, l, b, m_lds_here(s_tab), rb);
        const unsigned long long da = (dp_differs(a, 3, rb) >> rb) & lanes, db = (dp_differs(b, 3, rb) >> rb) & lanes;
        if (row < n && l == 0) {
            uint32_t* o = out + row * 13;
            dp_put_floats(o, one, 3);
            dp_put_floats(o + 3, a, 3); o[6] = (uint32_t)da; o[7] = (uint32_t)(da >> 32);
            dp_put_floats(o + 8, b, 3); o[11] = (uint32_t)db; o[12] = (uint32_t)(db >> 32);
        }
    }
}
// plane_normal_wave on DP_NORMAL_CEN rows (count >= 3: its contract), one row per wave: lane k < 9 holds sum k (the other lanes repeat the sums).
// out, 25 words per row: n_plane_normal with the centroid as view point on one lane (normal[4], centroid[3]) |
//                        m_lit: normal[4] centroid[3] of lane 0, mask of the lanes that differ from it (2 words) | m_lds: the same
__global__ void __launch_bounds__(64) dp_normal_wave(const uint32_t* in, uint32_t* out, size_t n) {
    __shared__ double s_tab[MC_COUNT];
    m_table_fill(s_tab, (int)threadIdx.x, 64);
    __syncthreads();
    const int lane = (int)threadIdx.x;
    for (size_t row = blockIdx.x; row < n; row += gridDim.x) {
        const uint32_t* w = in + row * 10;
        uint32_t one[7];
        dp_eval(DP_NORMAL_CEN, w, one, m_lit());
        const float acc = dp_f(w[lane % 9]);
        const unsigned count = w[9];
        float a[7], b[7];
        plane_normal_wave(acc, count, lane, a + 4, a, m_lit());
        plane_normal_wave(acc, count, lane, b + 4, b, m_lds_here(s_tab));
        const unsigned long long da = dp_differs(a, 7, 0), db = dp_differs(b, 7, 0);
        if (lane == 0) {
            uint32_t* o = out + row * 25;
            for (int k = 0; k < 7; ++k) o[k] = one[k];
            dp_put_floats(o + 7, a, 7); o[14] = (uint32_t)da; o[15] = (uint32_t)(da >> 32);
            dp_put_floats(o + 16, b, 7); o[23] = (uint32_t)db; o[24] = (uint32_t)(db >> 32);
        }
    }
}
// evl_scores<evl_m_logf> with evl_visit_order / evl_match_column: one table per lane (devprobe_fns.h, dp_evl_one)
__global__ void __launch_bounds__(64) dp_evl(DpEvlArrays A, uint32_t T) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t < T) dp_evl_one(A, t);
}

// device buffers of one call: freed when the call returns, whatever it returns
struct Bufs {
    void* p[16];
    int n = 0;
    hipError_t err = hipSuccess;
    ~Bufs() { for (int i = 0; i < n; ++i) (void)hipFree(p[i]); }
    void* make(size_t bytes, const void* src) {          // a buffer of `bytes`, filled from src (zeroed without one)
        if (err != hipSuccess || n >= 16) return nullptr;
        void* d = nullptr;
        err = hipMalloc(&d, bytes ? bytes : 4);
        if (err != hipSuccess) return nullptr;
        p[n++] = d;
        err = src ? hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) : hipMemset(d, 0, bytes ? bytes : 4);
        return d;
    }
    int finish(void* dst, const void* src, size_t bytes) {      // after the launch: its error, synchronise, copy back
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        if (err == hipSuccess) err = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
        return (int)err;
    }
};
unsigned grid_for(size_t units) { return (unsigned)(units < 1 ? 1 : (units > (size_t)MAX_GRID ? (size_t)MAX_GRID : units)); }

// a wave kernel over n rows of ni words in, no words out
template <class Kern>
int run_wave(Kern kern, const uint32_t* in, uint32_t* out, size_t n, int ni, int no, int rows_per_wave) {
    if (n == 0) return 0;
    Bufs B;
    const uint32_t* din = (const uint32_t*)B.make(n * (size_t)ni * 4, in);
    uint32_t* dout = (uint32_t*)B.make(n * (size_t)no * 4, nullptr);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL(kern, dim3(grid_for((n + rows_per_wave - 1) / rows_per_wave)), dim3(64), 0, 0, din, dout, n);
    return B.finish(out, dout, n * (size_t)no * 4);
}
}  // namespace

extern "C" {

int dp_dev_shape(int fn, int* ni, int* no) { return dp_shape(fn, ni, no) ? 0 : -1; }

// fn < DP_TABLE: constants as literals (m_lit); fn >= DP_TABLE: through m_lds.  Returns the HIP error code (0 = hipSuccess), -1 for an unknown fn.
int dp_dev_run(int fn, const uint32_t* in, uint32_t* out, size_t n) {
    int ni, no;
    if (!dp_shape(fn, &ni, &no)) return -1;
    if (n == 0) return 0;
    Bufs B;
    const uint32_t* din = (const uint32_t*)B.make(n * (size_t)ni * 4, in);
    uint32_t* dout = (uint32_t*)B.make(n * (size_t)no * 4, nullptr);
    if (B.err != hipSuccess) return (int)B.err;
    const dim3 grid(grid_for((n + ROWS_BLOCK - 1) / ROWS_BLOCK)), block(ROWS_BLOCK);
    if (fn >= DP_TABLE) hipLaunchKernelGGL(dp_rows<true>, grid, block, 0, 0, fn - DP_TABLE, din, dout, n, ni, no);
    else hipLaunchKernelGGL(dp_rows<false>, grid, block, 0, 0, fn, din, dout, n, ni, no);
    return B.finish(out, dout, n * (size_t)no * 4);
}
int dp_dev_ciede_quad(const uint32_t* in, uint32_t* out, size_t n) { return run_wave(dp_ciede_quad, in, out, n, 6, 27, 16); }
int dp_dev_edge_quad(const uint32_t* in, uint32_t* out, size_t n) { return run_wave(dp_edge_quad, in, out, n, 29 + 2 * DP_CDF, 18, 16); }
int dp_dev_lab_three(int rows_per_wave, const uint32_t* in, uint32_t* out, size_t n) {
    if (rows_per_wave == 4) return run_wave(dp_lab_three<4>, in, out, n, 3, 13, 4);
    return run_wave(dp_lab_three<1>, in, out, n, 3, 13, 1);
}
int dp_dev_normal_wave(const uint32_t* in, uint32_t* out, size_t n) { return run_wave(dp_normal_wave, in, out, n, 10, 25, 1); }

// as dp_host_evl; ne = the summed entry count of all tables
int dp_dev_evl(uint32_t T, const uint32_t* dims, const uint32_t* ssize, const uint32_t* tsize, const uint32_t* roff, const uint32_t* col, const uint32_t* cnt,
               size_t nk, size_t nm, size_t ne, uint32_t* out) {
    if (T == 0) return 0;
    Bufs B;
    DpEvlArrays A;
    A.dims = (const uint32_t*)B.make((size_t)T * 8 * 4, dims);
    A.ssize = (const uint32_t*)B.make(nk * 4, ssize);
    A.tsize = (const uint32_t*)B.make(nm * 4, tsize);
    A.roff = (const uint32_t*)B.make((nk + T) * 4, roff);
    A.col = (const uint32_t*)B.make(ne * 4, ne ? col : nullptr);
    A.cnt = (const uint32_t*)B.make(ne * 4, ne ? cnt : nullptr);
    A.visited = (unsigned char*)B.make(nm, nullptr);
    A.used = (unsigned char*)B.make(nk, nullptr);
    A.order = (uint32_t*)B.make(nm * 4, nullptr);
    A.match = (uint32_t*)B.make(nm * 4, nullptr);
    A.in = (uint32_t*)B.make(nm * 4, nullptr);
    A.ci = (uint32_t*)B.make(nk * 4, nullptr);
    A.cc = (uint32_t*)B.make(nk * 4, nullptr);
    A.out = (uint32_t*)B.make((size_t)T * 7 * 4, nullptr);
    if (B.err != hipSuccess) return (int)B.err;
    hipLaunchKernelGGL(dp_evl, dim3((T + 63u) / 64u), dim3(64), 0, 0, A, T);
    return B.finish(out, A.out, (size_t)T * 7 * 4);
}

}  // extern "C"
