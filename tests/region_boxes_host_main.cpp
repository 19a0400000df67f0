// f3ds_region_boxes_host (csrc/f3ds_host.cpp) as a stand-alone program for the sanitizers: tests/test_region_boxes_cpu.py builds this file and
// f3ds_host.cpp with -fsanitize=address,undefined and runs it.  Blocks of regions over a tilted plane at fixed sizes, tight and pitched rows, one pixel, single
// rows and columns, a frame that is all invalid; every buffer allocated at exactly its size (a read or write past an end is an error the sanitizer reports):
// the depth image ends at its last pixel, the rows at the last region.  The bit-for-bit comparison against the reference is the Python test's; here the rows
// are checked against the shapes' host function and against what a box has by construction.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/f3ds.h"

namespace {

int failures = 0;
int cur_scene = 0; uint32_t cur_w = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("scene %d, width %u, line %d: %s\n", cur_scene, cur_w, __LINE__, #cond); ++failures; } } while (0)

struct Frame {
    f3ds_rgbd_format fmt;
    std::vector<unsigned char> depth;
    std::vector<uint32_t> labels;
    uint32_t K;
};

// scene 0: blocks of 8 x 8 pixels over a tilted plane, every seventh pixel invalid, every eleventh unlabelled; 1: one region at one depth; 2: all depths invalid;
// 3: every pixel its own region, the last two regions without a pixel.  pad: extra bytes per row
Frame make(int scene, uint32_t w, uint32_t h, bool f32, uint32_t pad) {
    Frame f;
    std::memset(&f.fmt, 0, sizeof f.fmt);
    f.fmt.width = w; f.fmt.height = h; f.fmt.depth_type = f32 ? F3DS_DEPTH_F32 : F3DS_DEPTH_U16; f.fmt.depth_scale = f32 ? 1.0f : 0.001f;
    f.fmt.color_format = 77; f.fmt.color_pitch = 1;      // (not looked at)
    f.fmt.fx = f.fmt.fy = 0.8f * (float)w; f.fmt.cx = ((float)w - 1.0f) / 2.0f; f.fmt.cy = ((float)h - 1.0f) / 2.0f;
    const uint32_t de = f32 ? 4u : 2u;
    const uint32_t dp = w * de + (pad ? (f32 ? 8u : 6u) : 0u);
    if (pad) f.fmt.depth_pitch = dp;
    f.depth.assign((size_t)(h - 1) * dp + (size_t)w * de, 0xA5);      // the last row has no padding: bytes past its last pixel do not exist
    f.labels.assign((size_t)w * h, 0u);
    const uint32_t bx = (w + 7u) / 8u, by = (h + 7u) / 8u;
    f.K = scene == 0 ? bx * by : (scene == 3 ? w * h + 2u : 1u);
    for (uint32_t v = 0; v < h; ++v)
        for (uint32_t u = 0; u < w; ++u) {
            const size_t p = (size_t)v * w + u;
            float mm = scene == 1 ? 1500.0f : 1000.0f + 3.0f * (float)u + 2.0f * (float)v;
            if (scene == 2 || (scene == 0 && p % 7u == 3u)) mm = 0.0f;
            if (f32) { const float d = mm * 0.001f; std::memcpy(&f.depth[(size_t)v * dp + 4u * u], &d, 4); }
            else { const uint16_t d = (uint16_t)mm; std::memcpy(&f.depth[(size_t)v * dp + 2u * u], &d, 2); }
            if (scene == 0) f.labels[p] = p % 11u == 5u ? F3DS_NO_LABEL : (v / 8u) * bx + u / 8u;
            if (scene == 3) f.labels[p] = (uint32_t)p;
        }
    return f;
}

bool all_bytes(const void* p, size_t n, unsigned char b) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < n; ++k) if (c[k] != b) return false;
    return true;
}
uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

void run(int scene, uint32_t w, uint32_t h, bool f32, uint32_t pad) {
    cur_scene = scene; cur_w = w;
    Frame f = make(scene, w, h, f32, pad);
    const uint32_t K = f.K;
    std::vector<f3ds_region_box> rows(K);            // exactly the rows
    std::vector<f3ds_region_shape> shapes(K), want(K);
    std::memset(rows.data(), 0xA5, K * sizeof(f3ds_region_box));
    f3ds_region_boxes_result res; f3ds_region_shapes_result sres;
    int rc = f3ds_region_boxes_host(&f.fmt, f.depth.data(), f.labels.data(), K, 0.01f, rows.data(), shapes.data(), &res);
    EXPECT(rc == F3DS_OK);
    EXPECT(f3ds_region_shapes_host(&f.fmt, f.depth.data(), f.labels.data(), K, want.data(), &sres) == F3DS_OK);
    if (rc != F3DS_OK) return;
    EXPECT(std::memcmp(shapes.data(), want.data(), K * sizeof(f3ds_region_shape)) == 0);
    EXPECT(res.n_regions == K && res.n_nonempty == sres.n_nonempty && res.n_labelled == sres.n_labelled && res.n_clamped == sres.n_clamped);
    uint64_t pixels = 0, inliers = 0; uint32_t nonempty = 0;
    for (uint32_t r = 0; r < K; ++r) {
        const f3ds_region_box& b = rows[r];
        EXPECT(b.n_pixels == want[r].n_pixels && b.n_inliers <= b.n_pixels);
        pixels += b.n_pixels; inliers += b.n_inliers;
        if (!b.n_pixels) { EXPECT(bits(b.center[0]) == 0x7FC00000u && bits(b.mean_abs_residual) == 0x7FC00000u && bits(b.half[2]) == 0x7FC00000u); continue; }
        ++nonempty;
        for (int k = 0; k < 3; ++k) {
            EXPECT(bits(b.axis_n[k]) == bits(want[r].normal[k]) && bits(b.axis_l[k]) == bits(want[r].axis[k]));
            EXPECT(b.lo[k] <= b.hi[k] && b.half[k] >= 0.0f && b.half[k] == (b.hi[k] - b.lo[k]) * 0.5f);
        }
        EXPECT(b.mean_abs_residual >= 0.0f);
        if (b.n_pixels == 1u) EXPECT(b.half[0] == 0.0f && b.half[1] == 0.0f && b.half[2] == 0.0f);
    }
    EXPECT(pixels == res.n_labelled && inliers == res.n_inliers && nonempty == res.n_nonempty);
    if (scene == 2) EXPECT(res.n_labelled == 0 && res.n_nonempty == 0);
    if (scene == 3) EXPECT(res.n_nonempty == w * h && rows[K - 1].n_pixels == 0u);
    // without the shapes and without the result: the same rows
    std::vector<f3ds_region_box> rows2(K);
    EXPECT(f3ds_region_boxes_host(&f.fmt, f.depth.data(), f.labels.data(), K, 0.01f, rows2.data(), nullptr, nullptr) == F3DS_OK);
    EXPECT(std::memcmp(rows.data(), rows2.data(), K * sizeof(f3ds_region_box)) == 0);
    // an infinite tolerance: every pixel an inlier
    EXPECT(f3ds_region_boxes_host(&f.fmt, f.depth.data(), f.labels.data(), K, INFINITY, rows2.data(), nullptr, &res) == F3DS_OK && res.n_inliers == res.n_labelled);
    // a bad label: refused, nothing written
    {
        Frame g = f;
        g.labels.back() = K;
        std::memset(rows2.data(), 0xA5, K * sizeof(f3ds_region_box));
        std::memset(shapes.data(), 0xA5, K * sizeof(f3ds_region_shape));
        f3ds_region_boxes_result r5; std::memset(&r5, 0x5A, sizeof r5);
        EXPECT(f3ds_region_boxes_host(&g.fmt, g.depth.data(), g.labels.data(), K, 0.01f, rows2.data(), shapes.data(), &r5) == F3DS_ERR_ARG);
        EXPECT(all_bytes(rows2.data(), K * sizeof(f3ds_region_box), 0xA5) && all_bytes(shapes.data(), K * sizeof(f3ds_region_shape), 0xA5) && all_bytes(&r5, sizeof r5, 0x5A));
    }
}

}  // namespace

int main() {
    for (int scene = 0; scene < 4; ++scene) {
        run(scene, 97, 61, false, 0);
        run(scene, 67, 45, true, 1);      // pitched rows
        run(scene, 67, 45, false, 1);
        run(scene, 3, 2, false, 0);
        run(scene, 1, 1, true, 0);        // one pixel
        run(scene, 1, 1, false, 1);
        run(scene, 40, 1, false, 0);
        run(scene, 1, 40, true, 1);
    }
    // the argument errors need no frame
    cur_scene = -1; cur_w = 0;
    f3ds_rgbd_format fmt; std::memset(&fmt, 0, sizeof fmt);
    uint16_t d = 1000; uint32_t l = 0; f3ds_region_box row; f3ds_region_shape shape;
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 1, 0.01f, &row, &shape, nullptr) == F3DS_ERR_ARG);      // width 0
    fmt.width = fmt.height = 1; fmt.depth_scale = 0.001f; fmt.fx = fmt.fy = 1.0f;
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 1, 0.01f, &row, &shape, nullptr) == F3DS_OK && row.n_pixels == 1u && row.n_inliers == 1u && shape.n_pixels == 1u);
    EXPECT(row.half[0] == 0.0f && row.half[1] == 0.0f && row.half[2] == 0.0f);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 1, 0.0f, &row, nullptr, nullptr) == F3DS_OK);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 1, 0.01f, nullptr, &shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_boxes_host(&fmt, nullptr, &l, 1, 0.01f, &row, &shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, nullptr, 1, 0.01f, &row, &shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 1, -0.5f, &row, &shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 1, NAN, &row, &shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 0x01000000u, 0.01f, &row, &shape, nullptr) == F3DS_ERR_UNSUPPORTED);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 0x01000000u, NAN, &row, &shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 0, 0.01f, nullptr, nullptr, nullptr) == F3DS_ERR_ARG);      // label 0 >= 0 regions
    l = F3DS_NO_LABEL;
    f3ds_region_boxes_result res;
    EXPECT(f3ds_region_boxes_host(&fmt, &d, &l, 0, 0.01f, nullptr, nullptr, &res) == F3DS_OK && res.n_regions == 0 && res.n_labelled == 0 && res.n_inliers == 0);
    if (failures) { std::printf("region_boxes_host: %d failures\n", failures); return 1; }
    std::printf("region_boxes_host: ok\n");
    return 0;
}
