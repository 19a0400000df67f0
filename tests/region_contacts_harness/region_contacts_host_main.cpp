// f3ds_region_contacts_host (csrc/f3ds_host.cpp) as a stand-alone program for the sanitizers: tests/test_region_contacts_cpu.py builds this file and
// f3ds_host.cpp with -fsanitize=address,undefined and runs it.  Scenes of that test file at fixed sizes, tight and padded rows, single rows and columns, every
// buffer allocated at exactly its size (a read or write past an end is an error the sanitizer reports): the depth image ends at its last pixel, the rows
// at the count a first call gave.  The properties that need no reference are checked on the way; the bit-for-bit comparison against numpy is the Python test's.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/f3ds.h"

namespace {

int failures = 0;
int cur_scene = 0; uint32_t cur_w = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("scene %d, width %u, line %d: %s\n", cur_scene, cur_w, __LINE__, #cond); ++failures; } } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 32); }

struct Frame {
    f3ds_rgbd_format fmt;
    std::vector<unsigned char> depth;
    std::vector<uint32_t> labels;
    uint32_t K;
    float tol;
};

// scene 1 ... 6 (the region table's), 7 (three classes on a border) and 9 (depth_tol 0) at w x h; pad: extra bytes per row
Frame make(int scene, uint32_t w, uint32_t h, bool f32, uint32_t pad) {
    Frame f;
    std::memset(&f.fmt, 0, sizeof f.fmt);
    f.fmt.width = w; f.fmt.height = h; f.fmt.depth_type = f32 ? F3DS_DEPTH_F32 : F3DS_DEPTH_U16; f.fmt.depth_scale = 0.001f;
    f.fmt.color_format = 77; f.fmt.color_pitch = 1;      // (not looked at)
    f.fmt.fx = f.fmt.fy = 0.8f * (float)w; f.fmt.cx = ((float)w - 1.0f) / 2.0f; f.fmt.cy = ((float)h - 1.0f) / 2.0f;
    const uint32_t de = f32 ? 4u : 2u;
    const uint32_t dp = w * de + (pad ? (f32 ? 8u : 6u) : 0u);
    if (pad) f.fmt.depth_pitch = dp;
    f.depth.assign((size_t)(h - 1) * dp + (size_t)w * de, 0xA5);      // the last row has no padding: bytes past its last pixel do not exist
    f.labels.assign((size_t)w * h, 0u);
    const uint32_t nx = w >= 32 ? 4u : (w >= 2 ? 2u : 1u), ny = h >= 24 ? 3u : (h >= 2 ? 2u : 1u);
    f.K = scene == 2 ? 1u : scene == 3 ? w * h : scene == 4 ? 7u : scene == 5 ? 1000u : nx * ny;
    f.tol = scene == 9 ? 0.0f : 0.05f;
    for (uint32_t v = 0; v < h; ++v)
        for (uint32_t u = 0; u < w; ++u) {
            const uint32_t p = v * w + u, block = (v * ny / h) * nx + u * nx / w;
            uint32_t lab = scene == 2 ? 0u : scene == 3 ? p : scene == 4 ? p % 7u : block;
            if (scene == 1 && rnd() % 20u == 0u) lab = F3DS_NO_LABEL;
            f.labels[p] = lab;
            const bool hole = (scene != 7 && scene != 9 && rnd() % 10u == 0u) || (scene == 6 && block == nx * ny - 1u);
            float mm = 1000.0f + 200.0f * (float)block + 3.0f * (float)u;
            if (scene == 7) { const float step[3] = {1.0f, 1000.0f, -900.0f}; mm = 2000.0f + (block ? step[(u + v) % 3u] : 0.0f); }
            if (scene == 9) mm = 2000.0f + (block && (u + v) % 2u ? 1.0f : 0.0f);
            if (f32) {
                float d = mm;
                if (hole) { const float bad[4] = {0.0f, -1.0f, NAN, INFINITY}; d = bad[rnd() % 4u]; }
                std::memcpy(&f.depth[(size_t)v * dp + 4u * u], &d, 4);
            } else {
                const uint16_t d = hole ? (uint16_t)0 : (uint16_t)mm;
                std::memcpy(&f.depth[(size_t)v * dp + 2u * u], &d, 2);
            }
        }
    return f;
}

void run(int scene, uint32_t w, uint32_t h, bool f32, uint32_t pad) {
    cur_scene = scene; cur_w = w;
    Frame f = make(scene, w, h, f32, pad);
    size_t count = 12345; f3ds_region_contacts_result res;
    int rc = f3ds_region_contacts_host(&f.fmt, f.depth.data(), f.labels.data(), f.K, f.tol, nullptr, 0, &count, &res);      // count only
    EXPECT(rc == F3DS_OK && count == res.n_contacts && res.n_regions == f.K);
    if (rc != F3DS_OK) return;
    std::vector<f3ds_region_contact> rows(count);      // exactly the rows
    size_t again = 0; f3ds_region_contacts_result res2;
    rc = f3ds_region_contacts_host(&f.fmt, f.depth.data(), f.labels.data(), f.K, f.tol, count ? rows.data() : nullptr, count, &again, &res2);
    EXPECT(rc == F3DS_OK && again == count && res2.n_pairs == res.n_pairs && res2.n_close == res.n_close);
    uint64_t pairs = 0, close = 0, a_front = 0, b_front = 0;
    for (size_t e = 0; e < count; ++e) {
        const f3ds_region_contact& r = rows[e];
        EXPECT(r.a < r.b && r.b < f.K && r.n_pairs >= 1u && (uint64_t)r.n_close + r.n_a_front <= r.n_pairs && r.n_horizontal <= r.n_pairs);
        if (e) EXPECT(rows[e - 1].a < r.a || (rows[e - 1].a == r.a && rows[e - 1].b < r.b));
        EXPECT(r.first_pixel < w * h && (f.labels[r.first_pixel] == r.a || f.labels[r.first_pixel] == r.b));
        EXPECT(r.mean_gap >= 0.0f && std::isfinite(r.mean_gap));
        pairs += r.n_pairs; close += r.n_close; a_front += r.n_a_front; b_front += r.n_pairs - r.n_close - r.n_a_front;
    }
    EXPECT(pairs == res.n_pairs && close == res.n_close);
    if (scene == 2) EXPECT(count == 0);
    if (scene == 7 && w >= 8 && h >= 8) EXPECT(close > 0 && a_front > 0 && b_front > 0);
    if (h == 1) for (const f3ds_region_contact& r : rows) EXPECT(r.n_horizontal == r.n_pairs);
    if (w == 1) for (const f3ds_region_contact& r : rows) EXPECT(r.n_horizontal == 0u);
    // one row too few: refused, no row written, the count and the result are
    if (count) {
        std::vector<unsigned char> raw(sizeof(f3ds_region_contact) * (count - 1), 0xA5);
        size_t c3 = 0; f3ds_region_contacts_result r3; std::memset(&r3, 0x5A, sizeof r3);
        f3ds_region_contact one;      // (a non-NULL pointer for count == 1: nothing may be written through it)
        EXPECT(f3ds_region_contacts_host(&f.fmt, f.depth.data(), f.labels.data(), f.K, f.tol, count > 1 ? reinterpret_cast<f3ds_region_contact*>(raw.data()) : &one, count - 1, &c3, &r3) == F3DS_ERR_CAPACITY);
        bool untouched = c3 == count && r3.n_contacts == count;
        for (unsigned char b : raw) untouched = untouched && b == 0xA5;
        EXPECT(untouched);
    }
    // a bad label: refused, nothing written
    if (f.K < 0x00FFFFFFu) {
        Frame g = f;
        g.labels.back() = f.K;
        std::vector<unsigned char> raw(sizeof(f3ds_region_contact) * count, 0xA5);
        size_t c4 = 777; f3ds_region_contacts_result r4; std::memset(&r4, 0x5A, sizeof r4);
        f3ds_region_contact one;
        EXPECT(f3ds_region_contacts_host(&g.fmt, g.depth.data(), g.labels.data(), g.K, g.tol, count ? reinterpret_cast<f3ds_region_contact*>(raw.data()) : &one, count, &c4, &r4) == F3DS_ERR_ARG);
        bool untouched = c4 == 777 && r4.n_regions == 0x5A5A5A5Au;
        for (unsigned char b : raw) untouched = untouched && b == 0xA5;
        EXPECT(untouched);
    }
}

}  // namespace

int main() {
    const int scenes[8] = {1, 2, 3, 4, 5, 6, 7, 9};
    for (int scene : scenes) {
        run(scene, 97, 61, false, 0);
        run(scene, 67, 45, true, 1);
        run(scene, 3, 2, false, 0);
        run(scene, 1, 1, true, 0);
        run(scene, 40, 1, false, 0);
        run(scene, 1, 40, true, 1);
    }
    // the argument errors need no frame
    cur_scene = 0; cur_w = 0;
    f3ds_rgbd_format fmt; std::memset(&fmt, 0, sizeof fmt);
    uint16_t d = 1000; uint32_t l = 0; f3ds_region_contact row; size_t n = 5;
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 1, 0.05f, &row, 1, &n, nullptr) == F3DS_ERR_ARG);      // width 0
    fmt.width = fmt.height = 1; fmt.depth_scale = 0.001f; fmt.fx = fmt.fy = 1.0f;
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 1, 0.05f, &row, 1, &n, nullptr) == F3DS_OK && n == 0);
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 1, 0.05f, &row, 1, nullptr, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 1, -0.5f, &row, 1, &n, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 1, NAN, &row, 1, &n, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 0x01000000u, 0.05f, &row, 1, &n, nullptr) == F3DS_ERR_UNSUPPORTED);
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 0, 0.05f, nullptr, 0, &n, nullptr) == F3DS_ERR_ARG);      // label 0 >= 0 regions
    l = F3DS_NO_LABEL;
    EXPECT(f3ds_region_contacts_host(&fmt, &d, &l, 0, 0.05f, nullptr, 0, &n, nullptr) == F3DS_OK && n == 0);
    if (failures) { std::printf("region_contacts_host: %d failures\n", failures); return 1; }
    std::printf("region_contacts_host: ok\n");
    return 0;
}
