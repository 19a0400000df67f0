// f3ds_region_table_host (csrc/f3ds_host.cpp) as a stand-alone program for the sanitizers: tests/test_region_table_cpu.py builds this file and
// f3ds_host.cpp with -fsanitize=address,undefined and runs it.  The scenes of that test file at fixed sizes, every colour format and no colour, tight
// and padded rows, every buffer allocated at exactly its size (a read or write past an end is an error the sanitizer reports); the properties that
// need no reference are checked on the way.  The bit-for-bit comparison against numpy is the Python test's.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/f3ds.h"

namespace {

int failures = 0;
int cur_scene = 0; uint32_t cur_w = 0; int cur_color = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("scene %d, width %u, colour %d, line %d: %s\n", cur_scene, cur_w, cur_color, __LINE__, #cond); ++failures; } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

struct Frame {
    f3ds_rgbd_format fmt;
    std::vector<unsigned char> depth, color;
    std::vector<uint32_t> labels;
    uint32_t K;
};

// scene 1 ... 9 at w x h; color: -1 none, else F3DS_COLOR_*; pad: extra bytes per row
Frame make(int scene, uint32_t w, uint32_t h, bool f32, int color, uint32_t pad) {
    Frame f;
    std::memset(&f.fmt, 0, sizeof f.fmt);
    f.fmt.width = w; f.fmt.height = h; f.fmt.depth_type = f32 ? F3DS_DEPTH_F32 : F3DS_DEPTH_U16; f.fmt.depth_scale = scene == 8 ? 4.0f : 0.001f;
    f.fmt.color_format = color < 0 ? 77 : color;      // (not looked at without a colour image)
    f.fmt.fx = f.fmt.fy = 0.8f * (float)w; f.fmt.cx = ((float)w - 1.0f) / 2.0f; f.fmt.cy = ((float)h - 1.0f) / 2.0f;
    if (scene == 7) { f.fmt.fx = f.fmt.fy = 1.0f; f.fmt.cx = f.fmt.cy = 0.0f; if (f32) f.fmt.depth_scale = 1.0f; }      // (f32: z = (2k + 1) / 2^17, x = u * z: ties)
    if (scene == 9) { f.fmt.fx = -f.fmt.fx; f.fmt.cx = (float)(w / 2); }
    const uint32_t de = f32 ? 4u : 2u, ce = color == F3DS_COLOR_RGB8 ? 3u : 4u;
    const uint32_t dp = w * de + (pad ? (f32 ? 8u : 6u) : 0u), cp = w * ce + (pad ? 5u : 0u);
    if (pad) { f.fmt.depth_pitch = dp; f.fmt.color_pitch = color < 0 ? 1u : cp; }
    f.depth.assign((size_t)(h - 1) * dp + (size_t)w * de, 0xA5);      // the last row has no padding: bytes past its last pixel do not exist
    if (color >= 0) f.color.assign((size_t)(h - 1) * cp + (size_t)w * ce, 0);
    f.labels.assign((size_t)w * h, 0u);
    const uint32_t nx = w >= 32 ? 4u : 1u, ny = h >= 24 ? 3u : 1u;
    f.K = scene == 2 ? 1u : scene == 3 ? w * h : scene == 4 ? 7u : scene == 5 ? 1000u : nx * ny;
    for (uint32_t v = 0; v < h; ++v)
        for (uint32_t u = 0; u < w; ++u) {
            const uint32_t p = v * w + u, block = (v * ny / h) * nx + u * nx / w;
            uint32_t lab = scene == 2 ? 0u : scene == 3 ? p : scene == 4 ? p % 7u : block;
            if (scene == 1 && rnd() % 20u == 0u) lab = F3DS_NO_LABEL;
            f.labels[p] = lab;
            bool hole = rnd() % 10u == 0u || (scene == 6 && block == nx * ny - 1u);
            float mm = scene == 8 ? 20000.0f + 300.0f * (float)u : 1000.0f + 200.0f * (float)block + 3.0f * (float)u;
            if (mm > 60000.0f) mm = 60000.0f;
            if (f32) {
                float d = scene == 7 ? (float)(2u * (rnd() % 4096u) + 1u) / 131072.0f : mm;
                if (hole) { const float bad[4] = {0.0f, -1.0f, NAN, INFINITY}; d = bad[rnd() % 4u]; }
                std::memcpy(&f.depth[(size_t)v * dp + 4u * u], &d, 4);
            } else {
                const uint16_t d = hole ? (uint16_t)0 : (uint16_t)mm;
                std::memcpy(&f.depth[(size_t)v * dp + 2u * u], &d, 2);
            }
            if (color >= 0) for (uint32_t k = 0; k < ce; ++k) f.color[(size_t)v * cp + (size_t)ce * u + k] = (unsigned char)rnd();
        }
    return f;
}

void run(int scene, uint32_t w, uint32_t h, bool f32, int color, uint32_t pad) {
    cur_scene = scene; cur_w = w; cur_color = color;
    Frame f = make(scene, w, h, f32, color, pad);
    std::vector<f3ds_region_row> rows(f.K);      // exactly K rows
    f3ds_region_table_result res;
    const int rc = f3ds_region_table_host(&f.fmt, f.depth.data(), color < 0 ? nullptr : f.color.data(), f.labels.data(), f.K, rows.data(), &res);
    EXPECT(rc == F3DS_OK);
    if (rc != F3DS_OK) return;
    uint64_t sum = 0; uint32_t nonempty = 0;
    for (const f3ds_region_row& r : rows) {
        sum += r.n_pixels;
        if (!r.n_pixels) {
            EXPECT(r.first_pixel == 0xFFFFFFFFu && r.u_min == 0xFFFFFFFFu && r.v_min == 0xFFFFFFFFu && r.u_max == 0u && r.v_max == 0u);
            EXPECT(std::isinf(r.lo[0]) && r.lo[0] > 0 && std::isinf(r.hi[2]) && r.hi[2] < 0 && std::isnan(r.centroid[1]) && std::isnan(r.mean_rgb[0]));
            continue;
        }
        ++nonempty;
        const uint32_t fu = r.first_pixel % w, fv = r.first_pixel / w;
        EXPECT(fu >= r.u_min && fu <= r.u_max && fv == r.v_min && fv <= r.v_max && r.u_max < w && r.v_max < h);
        for (int k = 0; k < 3; ++k) {
            EXPECT(r.lo[k] <= r.hi[k]);
            if (scene != 8) EXPECT(r.centroid[k] >= r.lo[k] - 1e-4f && r.centroid[k] <= r.hi[k] + 1e-4f);
            EXPECT(r.mean_rgb[k] >= 0.0f && r.mean_rgb[k] <= 255.0f && (color >= 0 || r.mean_rgb[k] == 0.0f));
        }
    }
    EXPECT(sum == res.n_labelled && nonempty == res.n_nonempty && res.n_regions == f.K);
    EXPECT(scene == 8 ? (res.n_clamped > 0 || res.n_labelled == 0) : res.n_clamped == 0);
    // a bad label: refused, nothing written
    if (f.K < 0x00FFFFFFu) {
        Frame g = f;
        g.labels.back() = f.K;
        std::vector<unsigned char> raw(sizeof(f3ds_region_row) * (size_t)f.K, 0xA5);
        f3ds_region_table_result r2; std::memset(&r2, 0x5A, sizeof r2);
        EXPECT(f3ds_region_table_host(&g.fmt, g.depth.data(), color < 0 ? nullptr : g.color.data(), g.labels.data(), g.K, reinterpret_cast<f3ds_region_row*>(raw.data()), &r2) == F3DS_ERR_ARG);
        bool untouched = r2.n_regions == 0x5A5A5A5Au;
        for (unsigned char b : raw) untouched = untouched && b == 0xA5;
        EXPECT(untouched);
    }
}

}  // namespace

int main() {
    const int colors[4] = {-1, F3DS_COLOR_RGB8, F3DS_COLOR_RGBA8, F3DS_COLOR_PACKED};
    for (int scene = 1; scene <= 9; ++scene)
        for (int ci = 0; ci < 4; ++ci) {
            run(scene, 97, 61, false, colors[ci], 0);
            run(scene, 67, 45, true, colors[ci], 1);
            run(scene, 3, 2, false, colors[ci], 0);
            run(scene, 1, 1, true, colors[ci], 0);
        }
    // the argument errors need no frame
    f3ds_rgbd_format fmt; std::memset(&fmt, 0, sizeof fmt);
    uint16_t d = 1000; uint32_t l = 0; f3ds_region_row row;
    EXPECT(f3ds_region_table_host(&fmt, &d, nullptr, &l, 1, &row, nullptr) == F3DS_ERR_ARG);      // width 0
    fmt.width = fmt.height = 1; fmt.depth_scale = 0.001f; fmt.fx = fmt.fy = 1.0f;
    EXPECT(f3ds_region_table_host(&fmt, &d, nullptr, &l, 1, &row, nullptr) == F3DS_OK && row.n_pixels == 1u);
    EXPECT(f3ds_region_table_host(&fmt, &d, nullptr, &l, 1, nullptr, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_table_host(&fmt, &d, nullptr, &l, 0x01000000u, &row, nullptr) == F3DS_ERR_UNSUPPORTED);
    l = F3DS_NO_LABEL;
    EXPECT(f3ds_region_table_host(&fmt, &d, nullptr, &l, 0, nullptr, nullptr) == F3DS_OK);
    if (failures) { std::printf("region_table_host: %d failures\n", failures); return 1; }
    std::printf("region_table_host: ok\n");
    return 0;
}
