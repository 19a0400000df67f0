// f3ds_components.h -- the rules of the region components (f3ds_region_components, f3ds_region_components_host, include/f3ds.h), shared
// by the HIP kernels (f3ds_components.inc), the host function and the sequential run of the device's algorithm (f3ds_host.cpp).
//
// The connected components of a label image over a depth image: the output is again a label image, one label per component, and one row per component.
//   point      the family's: pixel p = v * width + u gets z from n_depth_to_z (f3ds_numerics.h); it is LABELLED iff its depth is valid and
//              label[p] != F3DS_NO_LABEL.
//   pairs      the contacts': p with p + 1 (u + 1 < width) and with p + width (v + 1 < height): 4-connectivity.
//   link       a pair is a LINK iff both pixels are labelled, their labels are equal and ct_class(za, zb, depth_tol, g) == CT_CLOSE (f3ds_contacts.h: one rounded
//              f32 subtraction, one rounded f32 product, false on NaN; depth_tol = +inf links every equal-label pair of finite depths).
//   component  a class of the labelled pixels under the transitive closure of the links; its root is its smallest pixel index, its size its pixel count.
//   kept       iff size >= max(min_pixels, 1).
//   numbering  kept components are numbered 0, 1, ... by ascending root.
// Everything is a class of an equivalence relation, a minimum or an integer count: any schedule gives the same bits.
//
// The device's algorithm is a union-find over the pixels whose steps are the functions below, over any memory that can load a word and take an atomic minimum
// (CcPlain here; LDS and global memory in f3ds_components.inc).  Its invariant: parent[x] <= x at every instant, and a stored parent only ever decreases.  So a
// set's root is its smallest index -- which is what makes the result independent of the schedule -- and every walk goes down.
// Float evaluation order is part of the contract: compile with -ffp-contract=off.
#ifndef F3DS_COMPONENTS_H_
#define F3DS_COMPONENTS_H_

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_rgbd.h"
#include "f3ds_regions.h"
#include "f3ds_contacts.h"

namespace f3ds {

constexpr uint32_t CC_NONE = 0xFFFFFFFFu;         // F3DS_NO_LABEL; the parent word of a pixel that is not labelled
constexpr uint32_t CC_MAX_REGIONS = RG_MAX_REGIONS;
constexpr uint32_t CC_TILE_W = 64, CC_TILE_H = 16;      // the kernels' tile: a row of it is one wave
static_assert(sizeof(f3ds_region_component) == 12, "a row is 3 words");

// la, lb: the label of a labelled pixel, CC_NONE for any other; za, zb: their depths
F3DS_HD bool cc_link(uint32_t la, float za, uint32_t lb, float zb, float depth_tol) {
    if (la == CC_NONE || la != lb) return false;
    float g;
    return ct_class(za, zb, depth_tol, g) == CT_CLOSE;
}
F3DS_HD bool cc_kept(uint32_t size, uint32_t min_pixels) { return size >= (min_pixels > 1u ? min_pixels : 1u); }

// plain memory: the sequential run's, and the host's
struct CcPlain {
    uint32_t* p;
    F3DS_HD uint32_t load(uint32_t i) const { return p[i]; }
    F3DS_HD uint32_t fetch_min(uint32_t i, uint32_t v) const { const uint32_t old = p[i]; if (v < old) p[i] = v; return old; }      // atomicMin: returns the word as it was
};

// the root of x.  Terminates: a step is taken only to a word BELOW x, so x strictly decreases; a word >= x ends the walk (== x: a root; > x cannot happen
// under the invariant, and would end the walk all the same).  A stale word is an earlier parent of x: above the current one, in the same set, still below x.
template <class M>
F3DS_HD uint32_t cc_find(const M& m, uint32_t x) {
    for (;;) {
        const uint32_t q = m.load(x);
        if (q >= x) return x;
        x = q;
    }
}
// a and b become one set.  Both roots are found, then the larger root is hung under the smaller one by an atomic minimum.  If the word was no root any more
// (another lane hung it under `old` < b in the meantime) the minimum has kept the lower of the two links, and what is left to do is to unite `old` with a.
// Terminates: every retry follows an atomic that returned a word below b, and goes on with the pair (a, old), both below b: the larger index of the pair
// strictly decreases.  No iteration waits for another lane.
template <class M>
F3DS_HD void cc_unite(const M& m, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(m, a); b = cc_find(m, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = m.fetch_min(b, a);
        if (old == b) return;
        b = old;
    }
}
// lane's run head in a row of up to 64 pixels: bit k of `linked` says that pixel k is linked to pixel k - 1 (bit 0 is never set).  The head is the highest
// pixel at or below `lane` whose bit is clear: no union is needed along a row.
F3DS_HD uint32_t cc_run_head(uint64_t linked, uint32_t lane) {
    const uint64_t heads = ~linked & (lane >= 63u ? ~0ull : ((2ull << lane) - 1ull));      // (bit 0 is among them)
    return 63u - (uint32_t)__builtin_clzll(heads);
}
// Must the pair p = (u, v), q = (u, v + 1) (below) or q = (u + 1, v) unite its two sides?  Only if it is a link, and not if the pair one step earlier along the
// row (the column) does the same work: p' -- p, q' -- q and p' -- q' all links, with p', p in one tile and q', q in one tile (`inner`), whose links the tile
// has resolved or resolves itself.  By induction the first pair of such a chain unites.  pix(u, v, lab, z): the pixel's label (CC_NONE unless labelled) and depth.
template <class Pix>
F3DS_HD bool cc_joins(const Pix& pix, uint32_t u, uint32_t v, bool below, bool inner, float depth_tol) {
    uint32_t lp, lq; float zp, zq;
    pix(u, v, lp, zp);
    pix(below ? u : u + 1u, below ? v + 1u : v, lq, zq);
    if (!cc_link(lp, zp, lq, zq, depth_tol)) return false;
    if (!inner) return true;
    uint32_t lp1, lq1; float zp1, zq1;
    pix(below ? u - 1u : u, below ? v : v - 1u, lp1, zp1);
    pix(below ? u - 1u : u + 1u, below ? v + 1u : v - 1u, lq1, zq1);
    return !(cc_link(lp1, zp1, lp, zp, depth_tol) && cc_link(lq1, zq1, lq, zq, depth_tol) && cc_link(lp1, zp1, lq1, zq1, depth_tol));
}

// What both entry points refuse before they look at a pixel, in ct_check's order: the outputs and li_check's arguments, depth_tol, li_check's region cap; *use =
// the format they work with; *prm = the parameters (the defaults for NULL).  depth_tol may be +inf.
inline int cc_check(const f3ds_rgbd_format* fmt, const void* depth, const uint32_t* labels, uint32_t n_regions, const f3ds_component_params* params,
                    const uint32_t* comp_labels, const size_t* n_out, f3ds_rgbd_format* use, RgbdLayout* lay, f3ds_component_params* prm) {
    if (!comp_labels || !n_out || comp_labels == labels) return F3DS_ERR_ARG;
    const int rc = li_check(fmt, depth, nullptr, labels, n_regions, use, lay);
    if (rc == F3DS_ERR_ARG) return rc;
    if (params) *prm = *params; else { prm->depth_tol = 0.05f; prm->min_pixels = 1u; }
    if (!(prm->depth_tol >= 0.0f)) return F3DS_ERR_ARG;      // (false on NaN)
    return rc;
}

}  // namespace f3ds
#endif  // F3DS_COMPONENTS_H_
