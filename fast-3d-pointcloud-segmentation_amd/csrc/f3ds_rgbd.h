// f3ds_rgbd.h -- the one check of an f3ds_rgbd_format (include/f3ds.h), shared by f3ds_deproject (host), the rgbd entry
// points (device) and the frame pipeline: what they refuse with F3DS_ERR_ARG, and the layout they agree on.
#ifndef F3DS_RGBD_H_
#define F3DS_RGBD_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/f3ds.h"
#include "f3ds_math.h"

namespace f3ds {

struct RgbdLayout {
    uint32_t depth_elem, color_elem;      // bytes per pixel
    uint32_t depth_pitch, color_pitch;    // bytes per row, "tightly packed" resolved
    size_t depth_bytes, color_bytes;      // bytes from the first pixel of the image to the end of its last one
    size_t n;                             // pixels
};

inline int rgbd_layout(const f3ds_rgbd_format* f, RgbdLayout* out) {
    if (!f || !f->width || !f->height) return F3DS_ERR_ARG;
    if ((uint64_t)f->width * f->height > 0x7fffffffull) return F3DS_ERR_ARG;
    if (f->depth_type != F3DS_DEPTH_U16 && f->depth_type != F3DS_DEPTH_F32) return F3DS_ERR_ARG;
    if (f->color_format != F3DS_COLOR_RGB8 && f->color_format != F3DS_COLOR_RGBA8 && f->color_format != F3DS_COLOR_PACKED) return F3DS_ERR_ARG;
    if (!m_isfinitef(f->fx) || !m_isfinitef(f->fy) || !m_isfinitef(f->depth_scale) || !m_isfinitef(f->cx) || !m_isfinitef(f->cy)) return F3DS_ERR_ARG;
    if (f->fx == 0.0f || f->fy == 0.0f || !(f->depth_scale > 0.0f)) return F3DS_ERR_ARG;
    RgbdLayout l;
    l.depth_elem = f->depth_type == F3DS_DEPTH_U16 ? 2u : 4u;
    l.color_elem = f->color_format == F3DS_COLOR_RGB8 ? 3u : 4u;
    const uint64_t drow = (uint64_t)f->width * l.depth_elem, crow = (uint64_t)f->width * l.color_elem;
    if (drow > 0xffffffffull || crow > 0xffffffffull) return F3DS_ERR_ARG;      // (a row no pitch could describe)
    if (f->depth_pitch && (f->depth_pitch < drow || f->depth_pitch % l.depth_elem)) return F3DS_ERR_ARG;
    if (f->color_pitch && f->color_pitch < crow) return F3DS_ERR_ARG;
    l.depth_pitch = f->depth_pitch ? f->depth_pitch : (uint32_t)drow;
    l.color_pitch = f->color_pitch ? f->color_pitch : (uint32_t)crow;
    l.depth_bytes = (size_t)(f->height - 1u) * l.depth_pitch + (size_t)drow;
    l.color_bytes = (size_t)(f->height - 1u) * l.color_pitch + (size_t)crow;
    l.n = (size_t)f->width * f->height;
    if (out) *out = l;
    return F3DS_OK;
}

}  // namespace f3ds
#endif  // F3DS_RGBD_H_
