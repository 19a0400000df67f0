// track_host_main.cpp -- a stand-alone program around the label tracker's two host functions (f3ds_track_reproject, f3ds_track_assign: csrc/f3ds_host.cpp),
// built by tests/test_track_cpu.py with -fsanitize=address,undefined together with that source file and run as an ordinary executable.  Seeded inputs of
// every shape the functions take (NaN and infinite records, zp <= 0, points on the image border, empty tables, exhausted ids, refused arguments); the program
// checks what must hold of any answer -- a pixel index is -1 or inside the image, no id is handed out twice, nothing is written on an error -- and prints
// "track_host: ok".  What the answers ARE is the business of the Python tests; this one is for the sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../../include/f3ds.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
static float unit() { return (float)(rnd() & 0xFFFFFF) / (float)0x1000000; }
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "track_host: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static int reproject_round(uint32_t w, uint32_t h, bool with_pose) {
    f3ds_rgbd_format f;
    std::memset(&f, 0, sizeof f);
    f.width = w; f.height = h; f.depth_type = F3DS_DEPTH_U16; f.depth_scale = 0.001f; f.color_format = 77;      // (the colour fields are not looked at)
    f.fx = f.fy = 0.8f * (float)w; f.cx = ((float)w - 1.0f) / 2.0f; f.cy = ((float)h - 1.0f) / 2.0f;
    const size_t n = (size_t)w * h + 8;
    std::vector<float> pts(n * 4);
    for (size_t i = 0; i < n; ++i) {
        const float z = 0.5f + 3.0f * unit();
        pts[i * 4 + 0] = (unit() - 0.5f) * 1.5f * z; pts[i * 4 + 1] = (unit() - 0.5f) * 1.5f * z; pts[i * 4 + 2] = z;
        if (rnd() % 10 == 0) pts[i * 4] = pts[i * 4 + 1] = pts[i * 4 + 2] = NAN;
    }
    pts[2] = -1.0f; pts[6] = 0.0f; pts[10] = INFINITY; pts[12] = INFINITY; pts[16] = -f.cx / f.fx * pts[18] - 0.5f / f.fx * pts[18];      // behind, at, beyond, and on the left border
    float pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (with_pose) { const float a = (unit() - 0.5f) * 0.17f; pose[0] = std::cos(a); pose[2] = std::sin(a); pose[8] = -std::sin(a); pose[10] = std::cos(a); pose[3] = 0.2f * (unit() - 0.5f); pose[11] = 0.2f * (unit() - 0.5f); }
    std::vector<int32_t> pixel(n, -7);
    std::vector<float> zp(n, 0.0f);
    CHECK(f3ds_track_reproject(&f, with_pose ? pose : nullptr, pts.data(), n, pixel.data(), zp.data()) == F3DS_OK);
    for (size_t i = 0; i < n; ++i) CHECK(pixel[i] == -1 || (pixel[i] >= 0 && (uint32_t)pixel[i] < w * h));
    CHECK(pixel[0] == -1 && pixel[1] == -1 && pixel[2] == -1);
    CHECK(f3ds_track_reproject(&f, nullptr, pts.data(), 0, pixel.data(), zp.data()) == F3DS_OK);      // no records
    pose[5] = NAN;
    CHECK(f3ds_track_reproject(&f, pose, pts.data(), n, pixel.data(), zp.data()) == F3DS_ERR_ARG);
    f.fx = 0.0f;
    CHECK(f3ds_track_reproject(&f, nullptr, pts.data(), n, pixel.data(), zp.data()) == F3DS_ERR_ARG);
    CHECK(f3ds_track_reproject(nullptr, nullptr, pts.data(), n, pixel.data(), zp.data()) == F3DS_ERR_ARG);
    return 0;
}

static int assign_round(uint32_t K, uint32_t M) {
    std::vector<uint32_t> size(K), prev(M), ent, id(K, 0xABCDEF01u);
    for (uint32_t i = 0; i < K; ++i) size[i] = rnd() % 5 == 0 ? 0u : 1u + rnd() % 60;
    for (uint32_t j = 0; j < M; ++j) prev[j] = 1000u + j * 3u;
    for (uint32_t i = 0; i < K; ++i) for (uint32_t j = 0; j < M; ++j) if (size[i] && rnd() % 6 == 0) { ent.push_back(i); ent.push_back(j); ent.push_back(1u + rnd() % size[i]); }
    f3ds_track_params prm;
    f3ds_default_track_params(&prm);
    prm.min_votes = rnd() % 3 ? 1u : 16u; prm.min_permille = (rnd() % 5) * 250u;
    uint32_t next = 5000u;
    f3ds_track_result res;
    CHECK(f3ds_track_assign(&prm, K ? size.data() : nullptr, K, ent.empty() ? nullptr : ent.data(), ent.size() / 3, M ? prev.data() : nullptr, M, &next, K ? id.data() : nullptr, &res) == F3DS_OK);
    std::set<uint32_t> seen;
    for (uint32_t i = 0; i < K; ++i) {
        CHECK((id[i] == F3DS_NO_LABEL) == (size[i] == 0));
        if (id[i] != F3DS_NO_LABEL) CHECK(seen.insert(id[i]).second);
    }
    CHECK(res.n_matched + res.n_new == res.n_nonempty && res.next_id == next && next == 5000u + res.n_new && res.n_retired + res.n_matched == M);
    // errors write nothing
    std::vector<uint32_t> keep = id;
    uint32_t last = 0xFFFFFFFEu;
    if (K && size[0]) { CHECK(f3ds_track_assign(&prm, size.data(), K, nullptr, 0, nullptr, 0, &last, id.data(), &res) == F3DS_ERR_UNSUPPORTED); CHECK(last == 0xFFFFFFFEu && id == keep); }
    prm.min_permille = 1001u;
    CHECK(f3ds_track_assign(&prm, K ? size.data() : nullptr, K, nullptr, 0, nullptr, 0, &next, K ? id.data() : nullptr, nullptr) == F3DS_ERR_ARG);
    if (K && M) { const uint32_t bad[3] = {K, 0, 1}; prm.min_permille = 300u; CHECK(f3ds_track_assign(&prm, size.data(), K, bad, 1, prev.data(), M, &next, id.data(), nullptr) == F3DS_ERR_ARG && id == keep); }
    return 0;
}

int main() {
    const uint32_t shapes[5][2] = {{160, 120}, {97, 61}, {67, 45}, {3, 2}, {1, 1}};
    for (const auto& s : shapes) for (int p = 0; p < 4; ++p) if (reproject_round(s[0], s[1], p != 0)) return 1;
    for (int k = 0; k < 300; ++k) if (assign_round(rnd() % 41, rnd() % 41)) return 1;
    if (assign_round(0, 0) || assign_round(0, 7) || assign_round(9, 0)) return 1;
    std::puts("track_host: ok");
    return 0;
}
