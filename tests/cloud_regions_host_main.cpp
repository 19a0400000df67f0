// f3ds_cloud_regions_host (csrc/f3ds_host.cpp) as a stand-alone program for the sanitizers: tests/test_cloud_regions_cpu.py builds this file and f3ds_host.cpp
// with -fsanitize=address,undefined and runs it.  The clouds an image cannot reach -- none, one point, one region, hundreds and thousands of regions under
// scattered labels, coordinates that are not finite, signed zeros, coordinates beyond the clamp, negative z with and without the fold, points without a label,
// labels over points that are not finite -- and every argument error in its order; every buffer allocated at exactly its size (a read or write past an end is an
// error the sanitizer reports), the records at an odd address once.  The bit-for-bit comparison against the reference is the Python test's; here the rows are
// checked against what they have by construction.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/f3ds.h"

namespace {

int failures = 0;
const char* cur = "";
#define EXPECT(cond) do { if (!(cond)) { std::printf("%s, line %d: %s\n", cur, __LINE__, #cond); ++failures; } } while (0)

struct Rec { float x, y, z; uint32_t rgba; };
struct Cloud { std::vector<Rec> pts; std::vector<uint32_t> lab; uint32_t K; };

uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
float unit(uint32_t& s) { return (float)(lcg(s) & 0xFFFFu) / 65536.0f; }

// n points on K tilted patches, label = a fixed scatter of i
Cloud patches(uint32_t n, uint32_t K, uint32_t seed) {
    Cloud c; c.K = K; c.pts.resize(n); c.lab.resize(n);
    uint32_t s = seed;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = (uint32_t)(((uint64_t)i * 2654435761ull) % (K ? K : 1u));
        const float a = unit(s) - 0.5f, b = unit(s) - 0.5f;
        c.pts[i] = Rec{(float)(l % 17u) * 0.4f + a, (float)(l % 5u) * 0.7f + b, 2.0f + 0.3f * a - 0.2f * b + (float)(l % 3u), lcg(s) * 256u + 17u};
        c.lab[i] = l;
    }
    return c;
}

bool all_bytes(const void* p, size_t n, unsigned char b) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < n; ++k) if (c[k] != b) return false;
    return true;
}
uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

// the host function on a cloud, with and without boxes; returns the rows.  labelled: how many points the caller expects to count
std::vector<f3ds_cloud_region> run(const char* name, const Cloud& c, int fold, uint64_t labelled, uint64_t clamped) {
    cur = name;
    const uint32_t K = c.K;
    std::vector<f3ds_cloud_region> rows(K), rows2(K);
    std::vector<f3ds_region_box> boxes(K);
    f3ds_cloud_params prm; f3ds_default_cloud_params(&prm);
    EXPECT(prm.plane_tol == 0.01f && prm.fold_negative_z == 0);
    prm.fold_negative_z = fold;
    f3ds_cloud_regions_result res, res2;
    // the records at an address that is no multiple of four: the host function reads them with memcpy
    std::vector<unsigned char> raw(c.pts.size() * sizeof(Rec) + 1u);
    if (!c.pts.empty()) std::memcpy(raw.data() + 1, c.pts.data(), c.pts.size() * sizeof(Rec));
    const uint32_t no_labels = 0u;
    const uint32_t* lab = c.lab.empty() ? &no_labels : c.lab.data();      // (an empty vector has no address, and NULL labels are an error)
    EXPECT(f3ds_cloud_regions_host(raw.data() + 1, c.pts.size(), lab, K, &prm, K ? rows.data() : nullptr, K ? boxes.data() : nullptr, &res) == F3DS_OK);
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), c.pts.size(), lab, K, &prm, K ? rows2.data() : nullptr, nullptr, &res2) == F3DS_OK);
    EXPECT(K == 0 || std::memcmp(rows.data(), rows2.data(), K * sizeof(f3ds_cloud_region)) == 0);
    EXPECT(res.n_regions == K && res.n_labelled == labelled && res.n_clamped == clamped && res2.n_inliers == 0 && res2.n_labelled == labelled);
    uint64_t sum = 0, inl = 0; uint32_t nonempty = 0;
    for (uint32_t r = 0; r < K; ++r) {
        const f3ds_cloud_region& q = rows[r]; const f3ds_region_box& b = boxes[r];
        sum += q.n_points; inl += b.n_inliers; nonempty += q.n_points ? 1u : 0u;
        EXPECT(q.reserved == 0u && b.n_pixels == q.n_points && b.n_inliers <= b.n_pixels);
        if (!q.n_points) {
            EXPECT(q.first_point == 0xFFFFFFFFu && bits(q.lo[0]) == 0x7F800000u && bits(q.hi[2]) == 0xFF800000u && bits(q.centroid[1]) == 0x7FC00000u &&
                   bits(q.mean_rgb[0]) == 0x7FC00000u && bits(q.cov[5]) == 0x7FC00000u && bits(q.curvature) == 0x7FC00000u && bits(b.center[0]) == 0x7FC00000u);
            continue;
        }
        EXPECT(q.first_point < c.pts.size() && c.lab[q.first_point] == r);
        for (int k = 0; k < 3; ++k) {
            EXPECT(q.lo[k] <= q.hi[k] && q.eigenvalue[k] >= 0.0f && q.mean_rgb[k] >= 0.0f && q.mean_rgb[k] <= 255.0f);
            EXPECT(bits(b.axis_n[k]) == bits(q.normal[k]) && bits(b.axis_l[k]) == bits(q.axis[k]) && b.half[k] >= 0.0f);
        }
        EXPECT(q.eigenvalue[0] <= q.eigenvalue[1] && q.eigenvalue[1] <= q.eigenvalue[2] && q.plane_d >= 0.0f);
    }
    EXPECT(sum == labelled && inl == res.n_inliers && nonempty == res.n_nonempty);
    return rows;
}

void errors() {
    cur = "errors";
    Cloud c = patches(65, 5, 3);
    const uint32_t K = c.K;
    std::vector<f3ds_cloud_region> rows(K); std::vector<f3ds_region_box> boxes(K);
    f3ds_cloud_regions_result res;
    auto fill = [&] { std::memset(rows.data(), 0xA5, K * sizeof rows[0]); std::memset(boxes.data(), 0xA5, K * sizeof boxes[0]); std::memset(&res, 0x5A, sizeof res); };
    auto untouched = [&] { return all_bytes(rows.data(), K * sizeof rows[0], 0xA5) && all_bytes(boxes.data(), K * sizeof boxes[0], 0xA5) && all_bytes(&res, sizeof res, 0x5A); };
    f3ds_cloud_params ok{0.01f, 0}, neg{-0.5f, 0}, nan{NAN, 0};
    fill();
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, nullptr, K, &ok, rows.data(), boxes.data(), &res) == F3DS_ERR_ARG && untouched());
    EXPECT(f3ds_cloud_regions_host(nullptr, 65, c.lab.data(), K, &ok, rows.data(), boxes.data(), &res) == F3DS_ERR_ARG && untouched());
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, c.lab.data(), K, &ok, nullptr, boxes.data(), &res) == F3DS_ERR_ARG && untouched());
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, c.lab.data(), K, &neg, rows.data(), boxes.data(), &res) == F3DS_ERR_ARG && untouched());
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, c.lab.data(), K, &nan, rows.data(), nullptr, &res) == F3DS_ERR_ARG && untouched());
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, c.lab.data(), 0x01000000u, &neg, rows.data(), boxes.data(), &res) == F3DS_ERR_ARG && untouched());      // the tolerance first
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, c.lab.data(), 0x01000000u, &ok, rows.data(), boxes.data(), &res) == F3DS_ERR_UNSUPPORTED && untouched());
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), (size_t)0x80000000u, c.lab.data(), K, &ok, rows.data(), boxes.data(), &res) == F3DS_ERR_UNSUPPORTED && untouched());
    Cloud bad = c; bad.lab[64] = K;
    EXPECT(f3ds_cloud_regions_host(bad.pts.data(), 65, bad.lab.data(), K, &ok, rows.data(), boxes.data(), &res) == F3DS_ERR_ARG && untouched());
    EXPECT(f3ds_cloud_regions_host(bad.pts.data(), 65, bad.lab.data(), 0x01000000u, &ok, rows.data(), boxes.data(), &res) == F3DS_ERR_UNSUPPORTED && untouched());      // ... before a label is read
    bad.pts[64].y = NAN;      // the bad label sits on a point that is not finite, and nowhere else
    EXPECT(f3ds_cloud_regions_host(bad.pts.data(), 65, bad.lab.data(), K, &ok, rows.data(), boxes.data(), &res) == F3DS_ERR_ARG && untouched());
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, c.lab.data(), 0, &ok, nullptr, nullptr, &res) == F3DS_ERR_ARG && untouched());      // label 0 >= 0 regions
    // allowed: NULL params, NULL result, NULL points of an empty cloud, no regions under no labels
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, c.lab.data(), K, nullptr, rows.data(), boxes.data(), nullptr) == F3DS_OK && rows[0].n_points > 0);
    EXPECT(f3ds_cloud_regions_host(nullptr, 0, c.lab.data(), K, &ok, rows.data(), boxes.data(), &res) == F3DS_OK && res.n_labelled == 0 && rows[0].n_points == 0);
    std::vector<uint32_t> none(65, F3DS_NO_LABEL);
    EXPECT(f3ds_cloud_regions_host(c.pts.data(), 65, none.data(), 0, &ok, nullptr, nullptr, &res) == F3DS_OK && res.n_regions == 0 && res.n_labelled == 0);
}

}  // namespace

int main() {
    run("empty", Cloud{{}, {}, 4}, 0, 0, 0);
    run("no regions", Cloud{{}, {}, 0}, 0, 0, 0);
    {
        Cloud c{{Rec{0.25f, -1.5f, 2.0f, 0x00804020u}}, {1u}, 2};
        const auto rows = run("one point", c, 0, 1, 0);
        EXPECT(rows[1].n_points == 1 && rows[1].first_point == 0 && rows[1].centroid[1] == -1.5f && rows[1].mean_rgb[0] == 128.0f && rows[1].cov[0] == 0.0f);
    }
    run("one region", patches(500, 1, 11), 0, 500, 0);
    run("K 200", patches(6000, 200, 12), 0, 6000, 0);
    run("K 3000", patches(6000, 3000, 13), 0, 6000, 0);
    {
        Cloud c = patches(40, 3, 14);
        c.pts[1].x = NAN; c.pts[6].y = NAN; c.pts[11].z = NAN; c.pts[16].x = INFINITY; c.pts[21].y = -INFINITY; c.pts[26].z = INFINITY;
        run("one coordinate not finite", c, 0, 34, 0);
    }
    {
        Cloud c{{Rec{-0.0f, 0.0f, 1.0f, 1u}, Rec{0.0f, -0.0f, 1.0f, 2u}, Rec{0.0f, 0.0f, 1.0f, 3u}}, {0u, 0u, 0u}, 1};
        const auto rows = run("signed zero", c, 0, 3, 0);
        EXPECT(bits(rows[0].lo[0]) == 0x80000000u && bits(rows[0].hi[0]) == 0u && bits(rows[0].lo[1]) == 0x80000000u && bits(rows[0].hi[1]) == 0u);
    }
    {
        Cloud c{{Rec{40000.0f, 1.0f, 2.0f, 0u}, Rec{-50000.0f, 1.0f, 2.5f, 0u}, Rec{3.0e38f, -3.0e38f, 32768.0f, 0u}, Rec{1.0f, 2.0f, 3.0f, 0u}}, {0u, 0u, 0u, 0u}, 1};
        const auto rows = run("clamped", c, 0, 4, 3);
        EXPECT(rows[0].hi[0] == 3.0e38f && rows[0].lo[1] == -3.0e38f);
    }
    {
        Cloud c = patches(300, 4, 15);
        for (size_t i = 0; i < c.pts.size(); i += 3) c.pts[i].z = -c.pts[i].z;      // (every third point: every label has some)
        c.pts[7].z = -INFINITY;
        const auto a = run("negative z", c, 0, 299, 0), b = run("negative z folded", c, 1, 299, 0);
        for (uint32_t r = 0; r < 4; ++r) EXPECT(a[r].lo[2] < 0.0f && b[r].lo[2] > 0.0f && a[r].n_points == b[r].n_points);
    }
    {
        Cloud c = patches(60, 2, 16);
        for (size_t i = 0; i < 60; i += 3) c.lab[i] = F3DS_NO_LABEL;
        c.K = 3;
        const auto rows = run("no label over finite points", c, 0, 40, 0);
        EXPECT(rows[2].n_points == 0);
    }
    {
        Cloud c = patches(30, 1, 17);
        c.pts.push_back(Rec{NAN, 0.0f, 1.0f, 1u}); c.lab.push_back(1u);
        c.pts.push_back(Rec{0.0f, INFINITY, 1.0f, 2u}); c.lab.push_back(1u);
        c.pts.push_back(Rec{NAN, NAN, NAN, 3u}); c.lab.push_back(0u);
        c.K = 2;
        const auto rows = run("labels over points that are not finite", c, 0, 30, 0);
        EXPECT(rows[0].n_points == 30 && rows[1].n_points == 0);
    }
    errors();
    if (failures) { std::printf("cloud_regions_host: %d failures\n", failures); return 1; }
    std::printf("cloud_regions_host: ok\n");
    return 0;
}
