"""Shared by tests/test_rgbd_cpu.py and tests/test_rgbd_gpu.py: RGB-D images made from the seeded synthetic frames, the numpy float32 form of the
deprojection formula (include/f3ds.h, f3ds_rgbd_format), and the image cases both files run.

Images of a synthetic frame (kind 0, width x height pixels): depth = rint(|z| * 1000) as u16, 0 where z is NaN; colour = the low three bytes of rgba;
fx = fy = 0.8 * width, cx = (width - 1) / 2, cy = (height - 1) / 2, depth_scale = 0.001."""
import ctypes

import numpy as np

SIZES = [(160, 120), (67, 45), (3, 2), (1, 1)]
# (depth type, colour format) pairs: u16 + RGB8, f32 + RGBA8, and the packed word with either depth
KINDS = [("u16", "rgb8"), ("f32", "rgba8"), ("u16", "packed"), ("f32", "packed")]
LAYOUTS = ["tight", "padded"]
# padded rows: depth pitch + 6 bytes, colour pitch + 5 bytes.  An f32 depth pitch must be a multiple of 4 (width * 4 + 6 is refused with
# F3DS_ERR_ARG, which test_rgbd_cpu.py asserts), so f32 rows are padded by the next multiple, 8.
DEPTH_PAD = {"u16": 6, "f32": 8}
COLOR_PAD = 5
F32_SPECIALS = [0.0, -1.0, np.nan, np.inf]      # depths that are no measurement: NaN records


def frame_format(P, width, height, depth="u16", color="rgb8", depth_scale=0.001):
    return P.RgbdFormat(width, height, P.DEPTH_U16 if depth == "u16" else P.DEPTH_F32, depth_scale,
                        dict(rgb8=P.COLOR_RGB8, rgba8=P.COLOR_RGBA8, packed=P.COLOR_PACKED)[color], 0, 0,
                        0.8 * width, 0.8 * width, (width - 1) / 2.0, (height - 1) / 2.0)


def frame_images(P, seed, width, height, nan_permille=30):
    """(format, depth (h, w) u16, colour (h, w, 3) u8) of synthetic frame `seed`."""
    pts = P.synth_frame(0, seed, width, height, nan_permille)
    z = pts[:, 2]
    with np.errstate(invalid="ignore"):
        depth = np.where(np.isnan(z), 0.0, np.rint(np.abs(z.astype(np.float64)) * 1000.0))
    assert depth.max() < 65536
    depth = depth.astype(np.uint16).reshape(height, width)
    rgba = pts[:, 3].view(np.uint32)
    color = np.stack([(rgba >> 16) & 255, (rgba >> 8) & 255, rgba & 255], axis=1).astype(np.uint8).reshape(height, width, 3)
    return frame_format(P, width, height), depth, color


def case_images(P, width, height, depth_kind, color_kind, seed=7):
    """(format, depth array, colour array), contiguous, of one case: the synthetic frame's images in the asked element types.  f32 depths are metres
    times 800 under depth_scale 0.00125 (a scale that is not a power of two) and carry every special value of F32_SPECIALS; alpha bytes are seeded noise."""
    _, d16, rgb = frame_images(P, seed, width, height, 100)      # 10 % invalid pixels
    rng = np.random.default_rng(width * 1000 + height)
    if depth_kind == "u16":
        depth, scale = d16, 0.001
    else:
        depth = (d16.astype(np.float32) * np.float32(0.8)).astype(np.float32)
        flat = depth.reshape(-1)
        for k, s in enumerate(F32_SPECIALS):
            flat[(k * 7) % len(flat)] = s      # (1x1: the last one written stays, +inf)
        scale = 0.00125
    if color_kind == "rgb8":
        color = rgb
    else:
        alpha = rng.integers(0, 256, (height, width, 1), dtype=np.uint8)
        rgba8 = np.concatenate([rgb, alpha], axis=2)
        color = rgba8 if color_kind == "rgba8" else expected_words(rgba8)
    return frame_format(P, width, height, depth_kind, color_kind, scale), np.ascontiguousarray(depth), np.ascontiguousarray(color)


def expected_words(color):
    """a << 24 | r << 16 | g << 8 | b of an (h, w, 3 | 4) u8 image (alpha 255 without a fourth byte); a (h, w) u32 image is the words themselves"""
    if color.dtype == np.uint32:
        return color
    c = color.astype(np.uint32)
    a = c[..., 3] if color.shape[-1] == 4 else np.uint32(255)
    return ((a << 24) | (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]).astype(np.uint32)


def numpy_deproject(fmt, depth, color):
    """The (N, 4) float32 records by numpy float32 arithmetic in the operation order of include/f3ds.h: every operation one rounded f32 operation."""
    h, w = int(fmt.height), int(fmt.width)
    f32 = np.float32
    scale, fx, fy, cx, cy = f32(fmt.depth_scale), f32(fmt.fx), f32(fmt.fy), f32(fmt.cx), f32(fmt.cy)
    d = np.asarray(depth)
    with np.errstate(invalid="ignore", over="ignore"):
        if d.dtype == np.uint16:
            valid = d != 0
            z = d.astype(f32) * scale
        else:
            valid = (d > 0) & ~np.isinf(d)
            z = d.astype(f32) * scale
        u = np.arange(w, dtype=np.uint32).astype(f32)[None, :]
        v = np.arange(h, dtype=np.uint32).astype(f32)[:, None]
        x = ((u - cx) * z) / fx
        y = ((v - cy) * z) / fy
    assert x.dtype == f32 and y.dtype == f32 and z.dtype == f32
    out = np.empty((h, w, 4), f32)
    nan = f32(np.nan)
    out[..., 0] = np.where(valid, x, nan)
    out[..., 1] = np.where(valid, y, nan)
    out[..., 2] = np.where(valid, z, nan)
    out[..., 3] = expected_words(np.asarray(color)).view(f32)
    return out.reshape(h * w, 4)


def padded(arr, row_bytes_extra, fill=0xA5):
    """(buffer, pitch): the rows of a contiguous (h, w[, c]) image copied into a byte buffer whose rows are `row_bytes_extra` bytes longer, the padding
    filled with a value no image byte depends on.  The buffer ends with the last row's padding (a full pitch per row)."""
    h = arr.shape[0]
    row = arr.reshape(h, -1).view(np.uint8)
    pitch = row.shape[1] + row_bytes_extra
    buf = np.full((h, pitch), fill, np.uint8)
    buf[:, :row.shape[1]] = row
    return buf, pitch


def laid_out(fmt, depth, color, layout):
    """(format, depth buffer, colour buffer) as raw byte arrays for the C entry points: "tight" or "padded" (DEPTH_PAD / COLOR_PAD)."""
    f = fmt.copy()
    if layout == "tight":
        return f, np.ascontiguousarray(depth).view(np.uint8).reshape(-1), np.ascontiguousarray(color).reshape(-1).view(np.uint8)
    dbuf, f.depth_pitch = padded(depth, DEPTH_PAD["u16" if depth.dtype == np.uint16 else "f32"])
    cbuf, f.color_pitch = padded(color, COLOR_PAD)
    return f, dbuf.reshape(-1), cbuf.reshape(-1)


def c_deproject(P, fmt, depth_buf, color_buf):
    """f3ds_deproject on raw buffers (the pitches of `fmt` as they are); returns (rc, records)."""
    lib = P.load_library()
    out = np.empty((int(fmt.width) * int(fmt.height), 4), np.float32)
    rc = lib.f3ds_deproject(ctypes.byref(fmt), depth_buf.ctypes.data, color_buf.ctypes.data, out.ctypes.data)
    return rc, out
