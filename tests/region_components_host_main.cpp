// f3ds_region_components_host and f3ds_region_components_tiled (csrc/f3ds_host.cpp) as a stand-alone program for the sanitizers:
// tests/test_region_components_cpu.py builds this file and f3ds_host.cpp with -fsanitize=address,undefined and runs it.  The spiral and the comb scenes of
// that test file at fixed sizes, tight and padded rows, single rows and columns, every buffer allocated at exactly its size (a read or write past an end is
// an error the sanitizer reports): the depth image ends at its last pixel, the rows at the count a first call gave.  The sequential run of the device's
// algorithm is compared with the host function word for word at four tile sizes; the bit-for-bit comparison against the reference is the Python test's.
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
    f3ds_component_params prm;
};

// scene 0: the spiral (labels 0 and 1); 1, 2, 3: the comb joined along the bottom row, the top row, the right column; 4: speckles of 1 ... 5 pixels, min_pixels 3.
// pad: extra bytes per row
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
    f.labels.assign((size_t)w * h, scene == 0 ? 1u : F3DS_NO_LABEL);
    f.K = scene == 0 ? 2u : (scene == 4 ? 3u : 1u);
    f3ds_default_component_params(&f.prm);
    if (scene == 4) f.prm.min_pixels = 3u;
    for (uint32_t v = 0; v < h; ++v)
        for (uint32_t u = 0; u < w; ++u) {
            if (f32) { const float d = 1500.0f; std::memcpy(&f.depth[(size_t)v * dp + 4u * u], &d, 4); }
            else { const uint16_t d = 1500; std::memcpy(&f.depth[(size_t)v * dp + 2u * u], &d, 2); }
            const size_t p = (size_t)v * w + u;
            if (scene == 1 && (u % 2u == 0u || v == h - 1u)) f.labels[p] = 0u;
            if (scene == 2 && (u % 2u == 0u || v == 0u)) f.labels[p] = 0u;
            if (scene == 3 && (v % 2u == 0u || u == w - 1u)) f.labels[p] = 0u;
            if (scene == 4) {      // cells of 5 x 4 pixels, speckle k of (k mod 5) + 1 pixels
                const uint32_t cu = u / 5u, cv = v / 4u, k = cv * ((w + 4u) / 5u) + cu, du = u % 5u, dv = v % 4u, size = k % 5u + 1u;
                const bool in = (size == 1u && du == 0u && dv == 0u) || (size == 2u && du < 2u && dv == 0u) || (size == 3u && ((du < 2u && dv == 0u) || (du == 0u && dv == 1u))) ||
                                (size == 4u && du < 2u && dv < 2u) || (size == 5u && ((du == 1u && dv < 3u) || (dv == 1u && du < 3u)));
                if (in) f.labels[p] = k % 3u;
            }
        }
    if (scene == 0) {      // a one-pixel-wide spiral of label 0 from the top left corner inwards, one pixel of room between its arms
        std::vector<unsigned char> seen((size_t)w * h, 0);
        auto at = [&](int64_t a, int64_t b) { return a >= 0 && a < (int64_t)w && b >= 0 && b < (int64_t)h; };
        int64_t u = 0, v = 0, du = 1, dv = 0;
        seen[0] = 1; f.labels[0] = 0u;
        for (int turns = 0; turns < 2;) {
            const int64_t a = u + du, b = v + dv, a2 = u + 2 * du, b2 = v + 2 * dv;
            if (at(a, b) && !seen[(size_t)b * w + a] && !(at(a2, b2) && seen[(size_t)b2 * w + a2])) { u = a; v = b; seen[(size_t)v * w + u] = 1; f.labels[(size_t)v * w + u] = 0u; turns = 0; }
            else { const int64_t t = du; du = -dv; dv = t; ++turns; }
        }
    }
    return f;
}

void run(int scene, uint32_t w, uint32_t h, bool f32, uint32_t pad) {
    cur_scene = scene; cur_w = w;
    Frame f = make(scene, w, h, f32, pad);
    const size_t n = (size_t)w * h;
    std::vector<uint32_t> image(n, 0xA5A5A5A5u);      // exactly the image
    size_t count = 12345; f3ds_region_components_result res;
    int rc = f3ds_region_components_host(&f.fmt, f.depth.data(), f.labels.data(), f.K, &f.prm, image.data(), nullptr, 0, &count, &res);      // no rows
    EXPECT(rc == F3DS_OK && count == res.n_components && res.n_regions == f.K && res.reserved == 0u);
    if (rc != F3DS_OK) return;
    std::vector<f3ds_region_component> rows(count);      // exactly the rows
    std::vector<uint32_t> image2(n, 0x5A5A5A5Au);
    size_t again = 0; f3ds_region_components_result res2;
    rc = f3ds_region_components_host(&f.fmt, f.depth.data(), f.labels.data(), f.K, &f.prm, image2.data(), count ? rows.data() : nullptr, count, &again, &res2);
    EXPECT(rc == F3DS_OK && again == count && image2 == image && std::memcmp(&res, &res2, sizeof res) == 0);
    uint64_t kept = 0;
    for (size_t k = 0; k < count; ++k) {
        const f3ds_region_component& r = rows[k];
        EXPECT(r.region < f.K && r.first_pixel < n && r.n_pixels >= (f.prm.min_pixels > 1u ? f.prm.min_pixels : 1u));
        if (r.first_pixel < n) EXPECT(image[r.first_pixel] == k && f.labels[r.first_pixel] == r.region);
        if (k) EXPECT(rows[k - 1].first_pixel < r.first_pixel);
        kept += r.n_pixels;
    }
    EXPECT(kept == res.n_kept && res.n_kept <= res.n_labelled);
    for (size_t p = 0; p < n; ++p) EXPECT(image[p] == F3DS_NO_LABEL ? true : image[p] < count);
    if (scene == 0 && w >= 8 && h >= 8) EXPECT(count == 2 && res.n_labelled == n);
    if (scene >= 1 && scene <= 3 && w >= 2 && h >= 2) EXPECT(count == 1 && rows[0].first_pixel == 0u && rows[0].n_pixels == res.n_labelled);
    if (scene == 4 && w >= 25 && h >= 4) EXPECT(res.n_dropped > 0 && count > 0);
    // the device's algorithm, sequentially: word for word the host function's answer at every tile size
    const uint32_t tiles[4][2] = {{1, 1}, {2, 2}, {3, 5}, {64, 16}};
    for (const auto& t : tiles) {
        std::vector<uint32_t> image3(n, 0x3C3C3C3Cu);
        std::vector<f3ds_region_component> rows3(count);
        size_t c3 = 0; f3ds_region_components_result res3;
        rc = f3ds_region_components_tiled(&f.fmt, f.depth.data(), f.labels.data(), f.K, &f.prm, t[0], t[1], image3.data(), count ? rows3.data() : nullptr, count, &c3, &res3);
        EXPECT(rc == F3DS_OK && c3 == count && image3 == image && std::memcmp(&res, &res3, sizeof res) == 0);
        EXPECT(count == 0 || std::memcmp(rows.data(), rows3.data(), count * sizeof(f3ds_region_component)) == 0);
    }
    // one row too few: refused, no row written; the image, the count and the result are
    if (count) {
        std::vector<unsigned char> raw(sizeof(f3ds_region_component) * (count - 1), 0xA5);
        std::vector<uint32_t> image4(n, 0u);
        size_t c4 = 0; f3ds_region_components_result r4; std::memset(&r4, 0x5A, sizeof r4);
        f3ds_region_component one;      // (a non-NULL pointer for count == 1: nothing may be written through it)
        EXPECT(f3ds_region_components_host(&f.fmt, f.depth.data(), f.labels.data(), f.K, &f.prm, image4.data(), count > 1 ? reinterpret_cast<f3ds_region_component*>(raw.data()) : &one,
                                           count - 1, &c4, &r4) == F3DS_ERR_CAPACITY);
        bool untouched = c4 == count && r4.n_components == count && image4 == image;
        for (unsigned char b : raw) untouched = untouched && b == 0xA5;
        EXPECT(untouched);
    }
    // a bad label: refused, nothing written
    {
        Frame g = f;
        g.labels.back() = f.K;
        std::vector<unsigned char> raw(sizeof(f3ds_region_component) * count, 0xA5);
        std::vector<uint32_t> image5(n, 0xA5A5A5A5u);
        size_t c5 = 777; f3ds_region_components_result r5; std::memset(&r5, 0x5A, sizeof r5);
        f3ds_region_component one;
        for (int tiled = 0; tiled < 2; ++tiled) {
            f3ds_region_component* out = count ? reinterpret_cast<f3ds_region_component*>(raw.data()) : &one;
            rc = tiled ? f3ds_region_components_tiled(&g.fmt, g.depth.data(), g.labels.data(), g.K, &g.prm, 64, 16, image5.data(), out, count, &c5, &r5)
                       : f3ds_region_components_host(&g.fmt, g.depth.data(), g.labels.data(), g.K, &g.prm, image5.data(), out, count, &c5, &r5);
            bool untouched = rc == F3DS_ERR_ARG && c5 == 777 && r5.n_regions == 0x5A5A5A5Au;
            for (unsigned char b : raw) untouched = untouched && b == 0xA5;
            for (uint32_t x : image5) untouched = untouched && x == 0xA5A5A5A5u;
            EXPECT(untouched);
        }
    }
}

}  // namespace

int main() {
    for (int scene = 0; scene < 5; ++scene) {
        run(scene, 97, 61, false, 0);
        run(scene, 67, 45, true, 1);
        run(scene, 3, 2, false, 0);
        run(scene, 1, 1, true, 0);
        run(scene, 40, 1, false, 0);
        run(scene, 1, 40, true, 1);
        run(scene, 130, 35, false, 1);      // three tile columns and three tile rows of the kernels' tile
    }
    // the argument errors need no frame
    cur_scene = -1; cur_w = 0;
    f3ds_rgbd_format fmt; std::memset(&fmt, 0, sizeof fmt);
    uint16_t d = 1000; uint32_t l = 0, out = 9; f3ds_region_component row; size_t n = 5;
    f3ds_component_params prm; f3ds_default_component_params(&prm);
    EXPECT(prm.depth_tol == 0.05f && prm.min_pixels == 1u);
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, &prm, &out, &row, 1, &n, nullptr) == F3DS_ERR_ARG);      // width 0
    fmt.width = fmt.height = 1; fmt.depth_scale = 0.001f; fmt.fx = fmt.fy = 1.0f;
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, nullptr, &out, &row, 1, &n, nullptr) == F3DS_OK && n == 1 && out == 0u && row.region == 0u && row.first_pixel == 0u && row.n_pixels == 1u);
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, &prm, &out, &row, 1, nullptr, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, &prm, nullptr, &row, 1, &n, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, &prm, &l, &row, 1, &n, nullptr) == F3DS_ERR_ARG);      // comp_labels == labels
    prm.depth_tol = -0.5f;
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, &prm, &out, &row, 1, &n, nullptr) == F3DS_ERR_ARG);
    prm.depth_tol = NAN;
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, &prm, &out, &row, 1, &n, nullptr) == F3DS_ERR_ARG);
    prm.depth_tol = INFINITY;
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 1, &prm, &out, &row, 1, &n, nullptr) == F3DS_OK && n == 1);
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 0x01000000u, &prm, &out, &row, 1, &n, nullptr) == F3DS_ERR_UNSUPPORTED);
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 0, &prm, &out, nullptr, 0, &n, nullptr) == F3DS_ERR_ARG);      // label 0 >= 0 regions
    l = F3DS_NO_LABEL;
    EXPECT(f3ds_region_components_host(&fmt, &d, &l, 0, &prm, &out, nullptr, 0, &n, nullptr) == F3DS_OK && n == 0 && out == F3DS_NO_LABEL);
    EXPECT(f3ds_region_components_tiled(&fmt, &d, &l, 0, &prm, 0, 1, &out, nullptr, 0, &n, nullptr) == F3DS_ERR_ARG);
    if (failures) { std::printf("region_components_host: %d failures\n", failures); return 1; }
    std::printf("region_components_host: ok\n");
    return 0;
}
