// f3ds_label_image.h -- what the label-image calls share (DESIGN.md "the label-image frame"): the tracker update, the region table, contacts, shapes and
// components all take a depth image plus a label image of an RGB-D frame and return rows.  Shared by the HIP kernels (the .inc files of the family), the
// host functions (f3ds_host.cpp) and the entry points (f3ds_hip.hip).
//   check      li_check: what every call of the family refuses before it looks at a pixel.
//   pixel      li_read_depth: the one read of a depth pixel, through n_depth_to_z (f3ds_numerics.h).  A pixel is LABELLED iff its depth is valid and
//              label[p] != F3DS_NO_LABEL.
//   labels     li_labels_in_range: a label is F3DS_NO_LABEL or below n_regions; the host functions sweep the image before they write anything, the kernels
//              raise word [1] of the head.
//   head       what a region call downloads first: LI_HEAD_WORDS words, [0] the count of rows, [1] 1 if a label was >= n_regions; words 2 ... 7 belong to the
//              call and are documented beside its kernels.  The rows behind the head are 8-byte aligned.
#ifndef F3DS_LABEL_IMAGE_H_
#define F3DS_LABEL_IMAGE_H_

#include <string.h>

#include "../../include/f3ds.h"
#include "f3ds_math.h"
#include "f3ds_numerics.h"
#include "f3ds_rgbd.h"

namespace f3ds {

constexpr uint32_t LI_NONE = 0xFFFFFFFFu;         // F3DS_NO_LABEL
constexpr uint32_t LI_MAX_REGIONS = 0x00FFFFFFu;  // regions are 24-bit key fields in the tracker, and the family follows it
constexpr uint32_t LI_HEAD_WORDS = 8;
constexpr size_t LI_HEAD_BYTES = 4 * LI_HEAD_WORDS;

// The family's checks, in this order: F3DS_ERR_ARG for a missing format, depth image or label image and for a format rgbd_layout refuses, then
// F3DS_ERR_UNSUPPORTED above LI_MAX_REGIONS.  *use = the format the call works with: without a colour image the two colour fields are made neutral and
// not looked at.  A call with tests of its own between the two results (a tolerance, a pose) returns the first at once, makes its tests, then returns this one.
inline int li_check(const f3ds_rgbd_format* fmt, const void* depth, const void* color, const uint32_t* labels, uint32_t n_regions, f3ds_rgbd_format* use, RgbdLayout* lay) {
    if (!fmt || !depth || !labels) return F3DS_ERR_ARG;
    *use = *fmt;
    if (!color) { use->color_format = F3DS_COLOR_RGB8; use->color_pitch = 0; }
    if (const int rc = rgbd_layout(use, lay)) return rc;
    return n_regions > LI_MAX_REGIONS ? F3DS_ERR_UNSUPPORTED : F3DS_OK;
}

inline bool li_labels_in_range(const uint32_t* labels, size_t n, uint32_t n_regions) {
    for (size_t p = 0; p < n; ++p) if (labels[p] != LI_NONE && labels[p] >= n_regions) return false;
    return true;
}

// The staging of a region call over nctx frames, a pure function of the frames' byte counts.  The nctx heads come first, contiguous;
// behind them, at 8-byte aligned offsets, every frame's payload: `fixed[i]` bytes whose size the host knows beforehand (the rows of a table, the image of the
// components) and, for the calls whose row count the device decides, room for `stage_rows[i]` rows of `row_bytes` (stage_rows == NULL: no such rows).  A
// row array of at most `first_rows` rows sits right behind its frame's fixed bytes; the longer ones follow behind ALL of those, so that ONE download of
// *first_bytes from offset 0 brings every head, every fixed payload, every short row array whole and the first `first_rows` rows of the first long one (with
// one frame that is the lone call's download: the head, what is fixed, the first rows).  slot[i].first = the rows of frame i's array that this download
// brings.  Returns the bytes in all.
struct LiSlot { size_t at, rows_at, first; };
inline size_t li_align8(size_t x) { return (x + 7u) & ~(size_t)7u; }
inline size_t li_stage_layout(size_t nctx, const size_t* fixed, const size_t* stage_rows, size_t row_bytes, size_t first_rows, LiSlot* slot, size_t* first_bytes) {
    size_t off = nctx * LI_HEAD_BYTES;
    for (size_t i = 0; i < nctx; ++i) {
        slot[i].at = off; off += li_align8(fixed[i]);
        slot[i].rows_at = off; slot[i].first = 0;
        if (stage_rows && stage_rows[i] <= first_rows) { slot[i].first = stage_rows[i]; off += li_align8(stage_rows[i] * row_bytes); }
    }
    *first_bytes = off;
    bool first_long = true;
    for (size_t i = 0; stage_rows && i < nctx; ++i) {
        if (stage_rows[i] <= first_rows) continue;
        slot[i].rows_at = off;
        if (first_long) { slot[i].first = first_rows; *first_bytes = off + first_rows * row_bytes; first_long = false; }
        off += li_align8(stage_rows[i] * row_bytes);
    }
    return off;
}

// depth pixel (u, v) on the host, read with memcpy: an image row may start anywhere its pitch puts it
inline bool li_read_depth(const f3ds_rgbd_format& fmt, const RgbdLayout& lay, const void* depth, uint32_t u, uint32_t v, float& z) {
    const unsigned char* drow = static_cast<const unsigned char*>(depth) + (size_t)v * lay.depth_pitch;
    if (fmt.depth_type == F3DS_DEPTH_F32) { float d; memcpy(&d, drow + 4u * (size_t)u, 4); return n_depth_to_z(d, fmt.depth_scale, z); }
    uint16_t d; memcpy(&d, drow + 2u * (size_t)u, 2); return n_depth_to_z(d, fmt.depth_scale, z);
}
#if defined(__HIPCC__)
// ... and in a kernel, one typed load of the aligned element (rgbd_layout: the pitch is a multiple of it)
template <bool DEPTH_F32>
__device__ __forceinline__ bool li_read_depth(const unsigned char* depth, uint32_t depth_pitch, float depth_scale, uint32_t u, uint32_t v, float& z) {
    const unsigned char* drow = depth + (size_t)v * depth_pitch;
    if constexpr (DEPTH_F32) return n_depth_to_z(reinterpret_cast<const float*>(drow)[u], depth_scale, z);
    else return n_depth_to_z(reinterpret_cast<const uint16_t*>(drow)[u], depth_scale, z);
}
#endif

}  // namespace f3ds
#endif  // F3DS_LABEL_IMAGE_H_
