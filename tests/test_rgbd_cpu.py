"""RGB-D frames, the half that needs no GPU: f3ds_deproject -- the host build of n_depth_to_z / n_deproject (csrc/f3ds_numerics.h), the arithmetic the device
kernel d_deproject runs -- against the numpy float32 form of the formula in include/f3ds.h, bit for bit; every argument the entry points refuse; and the
Python wrappers' handling of row-strided images."""
import ctypes

import numpy as np
import pytest

from conftest import same_bits
from rgbd_common import (COLOR_PAD, F32_SPECIALS, KINDS, LAYOUTS, SIZES, c_deproject, case_images, expected_words, frame_format, frame_images, laid_out,
                         numpy_deproject)


def assert_records(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what                  # NaN positions
    assert same_bits(got, want), what                                           # ... and every other byte
    assert np.array_equal(got[:, 3].view(np.uint32), want[:, 3].view(np.uint32)), what      # the colour word is never a "NaN": all its bits


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("depth_kind,color_kind", KINDS)
@pytest.mark.parametrize("width,height", SIZES)
def test_deproject_equals_the_numpy_formula(P, width, height, depth_kind, color_kind, layout):
    fmt, depth, color = case_images(P, width, height, depth_kind, color_kind)
    f, dbuf, cbuf = laid_out(fmt, depth, color, layout)
    rc, got = c_deproject(P, f, dbuf, cbuf)
    assert rc == 0
    want = numpy_deproject(fmt, depth, color)
    assert_records(got, want, (width, height, depth_kind, color_kind, layout))
    invalid = np.isnan(want[:, 2])
    assert np.isnan(got[invalid][:, :3]).all() and np.isfinite(got[~invalid][:, :3]).all()
    if width * height > 100:
        assert 0.05 < invalid.mean() < 0.2      # the frames are made with 10 % invalid pixels


def test_pixel_order_and_formula_by_hand(P):
    """3 x 2 pixels, numbers small enough to do by hand: pixel (u, v) is record v * width + u."""
    fmt = P.RgbdFormat(3, 2, P.DEPTH_U16, 0.5, P.COLOR_RGB8, 0, 0, 2.0, 4.0, 1.0, 0.5)
    depth = np.array([[2, 0, 4], [6, 8, 10]], np.uint16)
    color = np.arange(18, dtype=np.uint8).reshape(2, 3, 3) + 200
    got = P.deproject(fmt, depth, color)
    z = np.array([1, np.nan, 2, 3, 4, 5], np.float32)
    x = np.array([-1 * 1 / 2.0, np.nan, 1 * 2 / 2.0, -1 * 3 / 2.0, 0.0, 1 * 5 / 2.0], np.float32)
    y = np.array([-0.5 * 1 / 4.0, np.nan, -0.5 * 2 / 4.0, 0.5 * 3 / 4.0, 0.5 * 4 / 4.0, 0.5 * 5 / 4.0], np.float32)
    assert same_bits(got[:, 0], x) and same_bits(got[:, 1], y) and same_bits(got[:, 2], z)
    words = got[:, 3].view(np.uint32)
    assert words[0] == (255 << 24) | (200 << 16) | (201 << 8) | 202 and words[5] == (255 << 24) | (215 << 16) | (216 << 8) | 217
    assert got[1, :3].view(np.uint32).tolist() == [0x7fc00000] * 3      # the quiet NaN, in x, y and z


def test_f32_depths_that_are_no_measurement(P):
    fmt = frame_format(P, len(F32_SPECIALS) + 2, 1, "f32", "packed", 1.0)
    depth = np.array([[1.5] + F32_SPECIALS + [np.float32(1e-40)]], np.float32)      # (a denormal is a positive finite depth)
    color = np.arange(depth.size, dtype=np.uint32).reshape(1, -1) * 0x01020304 + 0x80000000
    got = P.deproject(fmt, depth, color)
    assert np.isnan(got[1:1 + len(F32_SPECIALS), :3]).all()
    assert np.isfinite(got[[0, -1], :3]).all() and got[0, 2] == np.float32(1.5) and got[-1, 2] == np.float32(1e-40)
    assert np.array_equal(got[:, 3].view(np.uint32), color.reshape(-1))             # the colour of an invalid pixel is kept
    assert_records(got, numpy_deproject(fmt, depth, color), "specials")


def test_alpha_rules(P):
    rgb = np.array([[[1, 2, 3], [250, 128, 0]]], np.uint8)
    rgba = np.array([[[1, 2, 3, 0], [250, 128, 0, 77]]], np.uint8)
    depth = np.array([[1000, 2000]], np.uint16)
    w = lambda kind, c: P.deproject(frame_format(P, 2, 1, "u16", kind), depth, c)[:, 3].view(np.uint32).tolist()
    assert w("rgb8", rgb) == [0xFF010203, 0xFFFA8000]                               # no alpha byte: 255
    assert w("rgba8", rgba) == [0x00010203, 0x4DFA8000]                             # carried, 0 included
    assert w("packed", np.array([[0x12345678, 0xFFFFFFFF]], np.uint32)) == [0x12345678, 0xFFFFFFFF]      # the word itself
    assert expected_words(rgba).reshape(-1).tolist() == [0x00010203, 0x4DFA8000]


def _fmt(P, **kw):
    f = P.RgbdFormat(4, 3, P.DEPTH_U16, 0.001, P.COLOR_RGB8, 0, 0, 3.2, 3.1, 1.5, 1.0)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


BAD_FORMATS = [
    ("width 0", dict(width=0)), ("height 0", dict(height=0)),
    ("too many pixels", dict(width=65536, height=32768)),
    ("depth type", dict(depth_type=2)), ("depth type < 0", dict(depth_type=-1)),
    ("colour format", dict(color_format=3)), ("colour format < 0", dict(color_format=-1)),
    ("fx nan", dict(fx=float("nan"))), ("fx inf", dict(fx=float("inf"))), ("fx 0", dict(fx=0.0)), ("fx -0", dict(fx=-0.0)),
    ("fy nan", dict(fy=float("nan"))), ("fy inf", dict(fy=float("-inf"))), ("fy 0", dict(fy=0.0)),
    ("scale nan", dict(depth_scale=float("nan"))), ("scale inf", dict(depth_scale=float("inf"))), ("scale 0", dict(depth_scale=0.0)),
    ("scale < 0", dict(depth_scale=-0.001)),
    ("cx nan", dict(cx=float("nan"))), ("cx inf", dict(cx=float("inf"))), ("cy nan", dict(cy=float("nan"))), ("cy inf", dict(cy=float("-inf"))),
    ("depth pitch short", dict(depth_pitch=6)), ("colour pitch short", dict(color_pitch=11)),
    ("depth pitch odd", dict(depth_pitch=9)),
    ("f32 depth pitch + 6", dict(depth_type=1, depth_pitch=4 * 4 + 6)),
]


@pytest.mark.parametrize("what,fields", BAD_FORMATS, ids=[b[0] for b in BAD_FORMATS])
def test_bad_formats_are_refused(P, what, fields):
    lib = P.load_library()
    f = _fmt(P, **fields)
    buf = np.zeros(4096, np.uint8)      # (never read: the format is checked first; the too-many-pixels case would need 2^31 pixels)
    out = np.zeros(4096, np.uint8)
    assert lib.f3ds_deproject(ctypes.byref(f), buf.ctypes.data, buf.ctypes.data, out.ctypes.data) == P.ERR_ARG, what
    # (the device entry points run the same check, csrc/f3ds_rgbd.h: tests/test_rgbd_gpu.py calls them with a context; without one they refuse at once)
    prm = P.launch_params()
    assert lib.f3ds_segment_rgbd(None, ctypes.byref(f), buf.ctypes.data, buf.ctypes.data, 0, ctypes.byref(prm), out.ctypes.data, 0, None) == P.ERR_ARG, what


def test_good_edge_formats_are_accepted(P):
    lib = P.load_library()
    buf = np.zeros(4096, np.uint8); out = np.zeros(4096, np.uint8)
    for fields in (dict(fx=-3.2), dict(cx=-100.0, cy=1e6), dict(depth_pitch=8), dict(depth_pitch=10), dict(color_pitch=12), dict(color_pitch=13),
                   dict(depth_type=1, depth_pitch=16), dict(depth_type=1, depth_pitch=24), dict(color_format=1, color_pitch=17), dict(depth_scale=1e-30)):
        assert lib.f3ds_deproject(ctypes.byref(_fmt(P, **fields)), buf.ctypes.data, buf.ctypes.data, out.ctypes.data) == 0, fields


def test_null_pointers_are_refused(P):
    lib = P.load_library()
    f = _fmt(P); prm = P.launch_params()
    buf = np.zeros(4096, np.uint8); out = np.zeros(4096, np.uint8)
    b, o = buf.ctypes.data, out.ctypes.data
    assert lib.f3ds_deproject(None, b, b, o) == P.ERR_ARG
    assert lib.f3ds_deproject(ctypes.byref(f), None, b, o) == P.ERR_ARG
    assert lib.f3ds_deproject(ctypes.byref(f), b, None, o) == P.ERR_ARG
    assert lib.f3ds_deproject(ctypes.byref(f), b, b, None) == P.ERR_ARG
    assert lib.f3ds_segment_rgbd(None, ctypes.byref(f), b, b, 0, ctypes.byref(prm), o, 0, None) == P.ERR_ARG
    assert lib.f3ds_segment_rgbd_batch(None, 1, ctypes.byref(f), None, None, 0, ctypes.byref(prm), None, 0, None) == P.ERR_ARG
    assert lib.f3ds_get_points(None, o, 1, 0, None) == P.ERR_ARG
    assert lib.f3ds_stream_submit_rgbd(None, ctypes.byref(f), b, b, ctypes.byref(prm), 0) == P.ERR_ARG


def test_wrappers_pass_row_strided_views_as_pitches(P):
    """A window of a wider image: rows are strided, pixels within a row are not.  The wrappers hand the row stride over as the pitch, no copy."""
    mod = P
    fmt, depth, color = frame_images(P, 7, 67, 45)
    wide_d = np.full((45, 67 + 9), 12345, np.uint16); wide_c = np.full((45, 67 + 9, 3), 99, np.uint8)
    wide_d[:, 4:4 + 67] = depth; wide_c[:, 4:4 + 67] = color
    vd, vc = wide_d[:, 4:4 + 67], wide_c[:, 4:4 + 67]
    assert not vd.flags.c_contiguous and not vc.flags.c_contiguous
    f, d, c = mod._rgbd_images(fmt, vd, vc)
    assert (f.depth_pitch, f.color_pitch) == ((67 + 9) * 2, (67 + 9) * 3)
    assert d.ctypes.data == vd.ctypes.data and c.ctypes.data == vc.ctypes.data          # the views themselves
    assert (fmt.depth_pitch, fmt.color_pitch) == (0, 0)                                   # the caller's format is not written to
    want = numpy_deproject(fmt, depth, color)
    assert_records(P.deproject(fmt, vd, vc), want, "strided views")
    assert_records(P.deproject(fmt, depth, color), want, "contiguous")
    f2, _, _ = mod._rgbd_images(fmt, depth, color)
    assert (f2.depth_pitch, f2.color_pitch) == (0, 0)
    # pixels strided within a row (every second column of a wider image) cannot be a pitch: copied, and right
    dd = np.repeat(depth, 2, axis=1)[:, ::2]; cc = np.repeat(color, 2, axis=1)[:, ::2]
    assert dd.strides[1] != dd.itemsize
    assert_records(P.deproject(fmt, dd, cc), want, "column-strided")
    # an odd colour row stride
    odd = np.full((45, 67 * 3 + COLOR_PAD), 7, np.uint8)
    odd[:, :67 * 3] = color.reshape(45, -1)
    vo = np.lib.stride_tricks.as_strided(odd, shape=(45, 67, 3), strides=(odd.strides[0], 3, 1))
    f3, _, c3 = mod._rgbd_images(fmt, depth, vo)
    assert f3.color_pitch == 67 * 3 + COLOR_PAD and c3.ctypes.data == odd.ctypes.data
    assert_records(P.deproject(fmt, depth, vo), want, "odd colour pitch")
    with pytest.raises(ValueError):
        P.deproject(fmt, depth[:-1], color)
