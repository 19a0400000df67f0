// f3ds_region_joints_host (csrc/f3ds_host.cpp) as a stand-alone program for the sanitizers: tests/test_region_joints_cpu.py builds this file and
// f3ds_host.cpp with -fsanitize=address,undefined and runs it.  Blocks of regions over a tilted plane with a step in depth at fixed sizes, tight and pitched
// rows, one pixel, single rows and columns, a frame that is all invalid, every pixel its own region; every buffer allocated at exactly its size (a read or
// write past an end is an error the sanitizer reports): the depth image ends at its last pixel, the rows at the last joint, the shapes at the last region.  The
// bit-for-bit comparison against the reference is the Python test's; here the rows are checked against the contacts' and the shapes' host functions and against
// what a joint has by construction.
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

// scene 0: blocks of 8 x 8 pixels over a tilted plane, the right half half a metre further, every seventh pixel invalid, every eleventh unlabelled; 1: one region
// at one depth; 2: all depths invalid; 3: every pixel its own region, the last two regions without a pixel.  pad: extra bytes per row
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
            float mm = scene == 1 ? 1500.0f : 1000.0f + 3.0f * (float)u + 2.0f * (float)v + (u >= w / 2u + 4u ? 500.0f : 0.0f);
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
bool qnan3(const float* x) { return bits(x[0]) == 0x7FC00000u && bits(x[1]) == 0x7FC00000u && bits(x[2]) == 0x7FC00000u; }

void run(int scene, uint32_t w, uint32_t h, bool f32, uint32_t pad) {
    cur_scene = scene; cur_w = w;
    Frame f = make(scene, w, h, f32, pad);
    const uint32_t K = f.K;
    f3ds_joint_params prm; f3ds_default_joint_params(&prm);
    size_t n = 777; f3ds_region_joints_result res;
    EXPECT(f3ds_region_joints_host(&f.fmt, f.depth.data(), f.labels.data(), K, &prm, nullptr, 0, &n, nullptr, &res) == F3DS_OK);      // count only
    if (n == 777) return;
    std::vector<f3ds_region_joint> rows(n);            // exactly the rows
    std::vector<f3ds_region_shape> shapes(K), want(K);
    std::vector<f3ds_region_contact> contacts(n);
    size_t n2 = 0, nc = 0; f3ds_region_joints_result res2; f3ds_region_contacts_result cres;
    const int rc = f3ds_region_joints_host(&f.fmt, f.depth.data(), f.labels.data(), K, &prm, rows.data(), n, &n2, shapes.data(), &res2);
    EXPECT(rc == F3DS_OK && n2 == n && std::memcmp(&res, &res2, sizeof res) == 0);
    EXPECT(f3ds_region_shapes_host(&f.fmt, f.depth.data(), f.labels.data(), K, want.data(), nullptr) == F3DS_OK);
    EXPECT(f3ds_region_contacts_host(&f.fmt, f.depth.data(), f.labels.data(), K, prm.depth_tol, contacts.data(), n, &nc, &cres) == F3DS_OK && nc == n);
    if (rc != F3DS_OK || nc != n) return;
    EXPECT(std::memcmp(shapes.data(), want.data(), K * sizeof(f3ds_region_shape)) == 0);
    EXPECT(res.n_regions == K && res.n_joints == n && res.n_pairs == cres.n_pairs && res.n_close == cres.n_close && res.reserved == 0u);
    uint32_t surface = 0;
    for (size_t e = 0; e < n; ++e) {
        const f3ds_region_joint& r = rows[e];
        const f3ds_region_contact& c = contacts[e];
        EXPECT(r.a == c.a && r.b == c.b && r.n_pairs == c.n_pairs && r.n_close == c.n_close && r.a < r.b && r.b < K);
        const uint32_t kind = r.kind & 0xFFu;
        EXPECT((r.kind & ~0x1FFu) == 0u && kind <= F3DS_JOINT_CONCAVE && (kind == F3DS_JOINT_OCCLUSION) == (r.n_close == 0u));
        if (r.n_close) {
            ++surface;
            EXPECT(r.spread[0] >= 0.0f && r.spread[0] <= r.spread[1] && r.spread[1] <= r.spread[2] && r.centroid[2] > 0.0f);
        } else EXPECT(qnan3(r.centroid) && qnan3(r.direction) && qnan3(r.spread) && bits(r.e_a) == 0x7FC00000u && bits(r.e_b) == 0x7FC00000u);
    }
    EXPECT(surface == res.n_surface);
    if (scene == 1 || scene == 2) EXPECT(n == 0);
    if (scene == 3 && w * h > 1u) EXPECT(n >= w * h - 1u);
    // without the shapes, the result and the parameters: the same rows
    std::vector<f3ds_region_joint> rows2(n);
    EXPECT(f3ds_region_joints_host(&f.fmt, f.depth.data(), f.labels.data(), K, nullptr, rows2.data(), n, &n2, nullptr, nullptr) == F3DS_OK);
    EXPECT(n == 0 || std::memcmp(rows.data(), rows2.data(), n * sizeof(f3ds_region_joint)) == 0);
    // one row short: refused, no row written
    if (n > 0) {
        std::memset(rows2.data(), 0xA5, n * sizeof(f3ds_region_joint));
        EXPECT(f3ds_region_joints_host(&f.fmt, f.depth.data(), f.labels.data(), K, &prm, rows2.data(), n - 1, &n2, nullptr, nullptr) == F3DS_ERR_CAPACITY && n2 == n);
        EXPECT(all_bytes(rows2.data(), n * sizeof(f3ds_region_joint), 0xA5));
    }
    // a bad label: refused, nothing written
    {
        Frame g = f;
        g.labels.back() = K;
        if (n) std::memset(rows2.data(), 0xA5, n * sizeof(f3ds_region_joint));
        std::memset(shapes.data(), 0xA5, K * sizeof(f3ds_region_shape));
        f3ds_region_joints_result r5; std::memset(&r5, 0x5A, sizeof r5);
        n2 = 777;
        EXPECT(f3ds_region_joints_host(&g.fmt, g.depth.data(), g.labels.data(), K, &prm, rows2.data(), n, &n2, shapes.data(), &r5) == F3DS_ERR_ARG && n2 == 777);
        EXPECT(all_bytes(rows2.data(), n * sizeof(f3ds_region_joint), 0xA5) && all_bytes(shapes.data(), K * sizeof(f3ds_region_shape), 0xA5) && all_bytes(&r5, sizeof r5, 0x5A));
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
    uint16_t d[2] = {1000, 1010}; uint32_t l[2] = {0, 1}; f3ds_region_joint row; f3ds_region_shape shape[2]; size_t n = 0;
    f3ds_joint_params prm; f3ds_default_joint_params(&prm);
    EXPECT(prm.depth_tol == 0.05f && prm.plane_tol == 0.01f && prm.cos_coplanar == 0.9659258f);
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 2, &prm, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);      // width 0
    fmt.width = 2; fmt.height = 1; fmt.depth_scale = 0.001f; fmt.fx = fmt.fy = 1.0f;
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 2, &prm, &row, 1, &n, shape, nullptr) == F3DS_OK && n == 1 && row.a == 0u && row.b == 1u && row.n_pairs == 1u && row.n_close == 1u);
    EXPECT(shape[0].n_pixels == 1u && shape[1].n_pixels == 1u && (row.kind & 0xFFu) != F3DS_JOINT_OCCLUSION);
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 2, &prm, &row, 1, nullptr, shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_joints_host(&fmt, nullptr, l, 2, &prm, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_joints_host(&fmt, d, nullptr, 2, &prm, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);
    f3ds_joint_params bad = prm; bad.depth_tol = -1.0f;
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 2, &bad, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);
    bad = prm; bad.plane_tol = NAN;
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 2, &bad, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);
    bad = prm; bad.cos_coplanar = 1.5f;
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 2, &bad, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 0x01000000u, &bad, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 0x01000000u, &prm, &row, 1, &n, shape, nullptr) == F3DS_ERR_UNSUPPORTED);
    EXPECT(f3ds_region_joints_host(&fmt, d, l, 1, &prm, &row, 1, &n, shape, nullptr) == F3DS_ERR_ARG);      // label 1 >= 1 region
    if (failures) { std::printf("region_joints_host: %d failures\n", failures); return 1; }
    std::printf("region_joints_host: ok\n");
    return 0;
}
