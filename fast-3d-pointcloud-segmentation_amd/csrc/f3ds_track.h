// f3ds_track.h -- the rules of the label tracker (f3ds_tracker_update, include/f3ds.h), shared by the HIP kernels
// (f3ds_track.inc) and the two host functions f3ds_track_reproject / f3ds_track_assign (f3ds_host.cpp).
//
// A frame's region labels are ranks (0..K-1) and mean nothing in the next frame.  The tracker keeps, per pixel of the previous frame, the
// region it belonged to (its SLOT) and its depth, reprojects every labelled pixel of the new frame into that image and counts, per
// (region i, previous slot j), the pixels that landed on j at a compatible depth: the VOTES.  One deterministic greedy rule over the counts
// then hands the previous frame's persistent ids on, or gives out new ones.
//   transform  p_prev = R p_cur + t, pose12 row-major 3 x 4; ((r0 x + r1 y) + r2 z) + t, every operation one rounded f32 operation
//   project    uf = (xp fx) / zp + cx, us = uf + 0.5; the pixel is floor(us) when zp > 0 is finite and 0 <= us < width (NaN fails), likewise v
//   vote       slot j of the pixel landed on, iff it has one and |zp - z_prev| <= depth_tol * zp; a labelled pixel that does not vote is a NO-VOTE
//   key        (i << jb) | j, j = Kp (the number of previous slots) for a no-vote, jb = bits(Kp); i = Kc (the number of regions) is the hole
//   eligible   c >= max(min_votes, 1) and c * 1000 >= min_permille * size[i], in 64-bit integers
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_TRACK_H_
#define F3DS_TRACK_H_

#include "f3ds_math.h"

namespace f3ds {

constexpr uint32_t TK_NONE = 0xFFFFFFFFu;         // F3DS_NO_LABEL: a pixel without a slot, a region without an id
constexpr uint32_t TK_MAX_REGIONS = 0x00FFFFFFu;  // regions and slots are 24-bit key fields

F3DS_HD int tk_bits(uint32_t v) { int b = 0; while (b < 32 && (v >> b)) ++b; return b; }

// step 2: pose == nullptr is the identity and does no arithmetic
F3DS_HD void tk_transform(const float* pose, float x, float y, float z, float& xp, float& yp, float& zp) {
    if (!pose) { xp = x; yp = y; zp = z; return; }
    xp = ((pose[0] * x + pose[1] * y) + pose[2] * z) + pose[3];
    yp = ((pose[4] * x + pose[5] * y) + pose[6] * z) + pose[7];
    zp = ((pose[8] * x + pose[9] * y) + pose[10] * z) + pose[11];
}
// step 3: the previous frame's pixel index the point lands on, or -1.  width * height <= 0x7fffffff (f3ds_rgbd.h)
F3DS_HD int32_t tk_project(float xp, float yp, float zp, float fx, float fy, float cx, float cy, uint32_t width, uint32_t height) {
    if (!(zp > 0.0f) || !m_isfinitef(zp)) return -1;
    const float uf = (xp * fx) / zp + cx, vf = (yp * fy) / zp + cy;
    const float us = uf + 0.5f, vs = vf + 0.5f;
    if (!(us >= 0.0f && us < (float)width) || !(vs >= 0.0f && vs < (float)height)) return -1;
    const uint32_t ui = (uint32_t)(int)__builtin_floorf(us), vi = (uint32_t)(int)__builtin_floorf(vs);
    if (ui >= width || vi >= height) return -1;      // (cannot be: the largest float below (float)width is below width; keeps every gather inside the image)
    return (int32_t)(vi * width + ui);
}
// step 4: does a point at depth zp that landed on a pixel of slot j and depth z_prev vote for j?
F3DS_HD bool tk_votes(uint32_t j, float zp, float z_prev, float depth_tol) { return j != TK_NONE && m_absf(zp - z_prev) <= depth_tol * zp; }
// the sort key of a labelled pixel of region i (j = Kp: no-vote) and of everything else
F3DS_HD uint64_t tk_key(uint32_t i, uint32_t j, int jb) { return ((uint64_t)i << jb) | j; }
F3DS_HD uint64_t tk_hole(uint32_t Kc, int jb) { return (uint64_t)Kc << jb; }
// step 5
F3DS_HD bool tk_eligible(uint32_t c, uint32_t size, uint32_t min_votes, uint32_t min_permille) {
    return c >= (min_votes > 1u ? min_votes : 1u) && (uint64_t)c * 1000ull >= (uint64_t)min_permille * size;
}
// what the entry points refuse of f3ds_track_params' fields
F3DS_HD bool tk_params_ok(uint32_t min_permille, float depth_tol) { return min_permille <= 1000u && m_isfinitef(depth_tol) && depth_tol >= 0.0f; }

}  // namespace f3ds
#endif  // F3DS_TRACK_H_
