"""Shared by tests/test_region_table_cpu.py and tests/test_region_table_gpu.py: the numpy reference of the region table (include/f3ds.h, "region table"),
written from the definition -- points from rgbd_common.numpy_deproject, fixed point with np.float64 / np.rint / int64, minima and maxima in the order of
the key, the finishing step in np.float64 -- and the scenes both files run.  Rows are compared bit for bit as u32 words: empty rows hold NaN."""
import numpy as np

import track_common as T
from rgbd_common import COLOR_PAD, DEPTH_PAD, expected_words, frame_format, numpy_deproject, padded

NO = 0xFFFFFFFF
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -7
QNAN = 0x7FC00000
SHAPES = [(97, 61, "u16", "tight"), (67, 45, "f32", "padded"), (3, 2, "u16", "tight"), (1, 1, "f32", "tight")]      # the tracker's
COLORS = ["rgb8", "rgba8", "packed", None]
SCENES = list(range(1, 10))
RESULT_FIELDS = ("n_regions", "n_nonempty", "n_labelled", "n_clamped")
u32, f64, i64 = np.uint32, np.float64, np.int64


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def key(bits):
    bits = np.asarray(bits, u32)
    return bits ^ np.where(bits >> 31 != 0, u32(0xFFFFFFFF), u32(0x80000000))


def unkey(k):
    k = np.asarray(k, u32)
    return k ^ np.where(k >> 31 != 0, u32(0x80000000), u32(0xFFFFFFFF))


def ref_table(P, fmt, depth, labels, n_regions, color=None):
    """(rc, rows (REGION_ROW_DTYPE), result dict) of the definition; rows and result are None unless rc == 0"""
    h, w = int(fmt.height), int(fmt.width)
    K = int(n_regions)
    lab = np.asarray(labels, u32).reshape(-1)
    if ((lab != NO) & (lab >= K)).any():
        return ERR_ARG, None, None
    pts = numpy_deproject(fmt, depth, np.zeros((h, w), u32))
    valid = ~np.isnan(pts[:, 2])
    p = np.flatnonzero(valid & (lab != NO))
    r = lab[p].astype(i64)
    rows = np.zeros(K, P.REGION_ROW_DTYPE)
    n = np.bincount(r, minlength=K).astype(i64)
    rows["n_pixels"] = n
    for name, vals, fn, start in (("first_pixel", p, np.minimum, NO), ("u_min", p % w, np.minimum, NO), ("v_min", p // w, np.minimum, NO),
                                  ("u_max", p % w, np.maximum, 0), ("v_max", p // w, np.maximum, 0)):
        a = np.full(K, start, u32)
        fn.at(a, r, vals.astype(u32))
        rows[name] = a
    xyz = np.ascontiguousarray(pts[p, :3])
    k = key(xyz.view(u32))
    lo = np.full((K, 3), key(np.array(np.inf, np.float32).view(u32)), u32)
    hi = np.full((K, 3), key(np.array(-np.inf, np.float32).view(u32)), u32)
    np.minimum.at(lo, r, k)
    np.maximum.at(hi, r, k)
    rows["lo"] = unkey(lo).view(np.float32)
    rows["hi"] = unkey(hi).view(np.float32)
    a = xyz.astype(f64)
    cl = np.clip(a, -32768.0, 32768.0)
    clamped = (cl != a).any(axis=1)
    fix = np.rint(cl * 65536.0).astype(i64)
    s = np.zeros((K, 3), i64)
    np.add.at(s, r, fix)
    c = np.zeros((K, 3), i64)
    if color is not None:
        words = expected_words(np.asarray(color)).reshape(-1)[p].astype(i64)
        np.add.at(c, r, np.stack([(words >> 16) & 255, (words >> 8) & 255, words & 255], axis=1))
    with np.errstate(all="ignore"):
        nd = n.astype(f64)[:, None]
        cen = ((s.astype(f64) / nd) / 65536.0).astype(np.float32)
        rgb = (c.astype(f64) / nd).astype(np.float32)
    empty = n == 0
    cen.view(u32)[empty] = QNAN
    rgb.view(u32)[empty] = QNAN
    rows["centroid"], rows["mean_rgb"] = cen, rgb
    return OK, rows, dict(n_regions=K, n_nonempty=int((n > 0).sum()), n_labelled=int(len(p)), n_clamped=int(clamped.sum()))


def words_of(rows):
    return np.ascontiguousarray(rows).view(u32).reshape(len(rows), 18)


def assert_rows_equal(P, got, want, what=""):
    g, w = words_of(got), words_of(want)
    if not np.array_equal(g, w):
        i, k = [int(a[0]) for a in np.nonzero(g != w)]
        raise AssertionError("%s row %d word %d: %#x, want %#x\ngot  %r\nwant %r" % (what, i, k, g[i, k], w[i, k], got[i], want[i]))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def make_color(width, height, kind, seed=11):
    """a seeded colour image in one of the three formats, or None"""
    if kind is None:
        return None
    rng = np.random.default_rng(seed * 7919 + width)
    rgba = rng.integers(0, 256, (height, width, 4), dtype=np.uint8)
    if kind == "rgb8":
        return np.ascontiguousarray(rgba[..., :3])
    return rgba if kind == "rgba8" else expected_words(rgba)


def with_color(P, fmt, kind):
    f = fmt.copy()
    f.color_format = dict(rgb8=P.COLOR_RGB8, rgba8=P.COLOR_RGBA8, packed=P.COLOR_PACKED).get(kind, P.COLOR_RGB8)
    return f


def buffers(fmt, depth, color, layout):
    """(format, depth bytes, colour bytes or None) for the C entry points: "tight", or "padded" rows (rgbd_common.DEPTH_PAD / COLOR_PAD)"""
    f = fmt.copy()
    depth = np.ascontiguousarray(depth)
    if layout == "tight":
        return f, depth.view(np.uint8).reshape(-1), None if color is None else np.ascontiguousarray(color).reshape(-1).view(np.uint8)
    dbuf, f.depth_pitch = padded(depth, DEPTH_PAD["u16" if depth.dtype == np.uint16 else "f32"])
    if color is None:
        return f, dbuf.reshape(-1), None
    cbuf, f.color_pitch = padded(np.ascontiguousarray(color), COLOR_PAD)
    return f, dbuf.reshape(-1), cbuf.reshape(-1)


def grid_of(width, height):
    return (max(1, min(4, width // 8)), max(1, min(3, height // 8)))


def scene(P, which, width, height, depth_kind):
    """scene `which` (1 ... 9, the table of the tests' docstrings) at this size: dict(fmt, depth, labels (h, w) u32, n_regions)"""
    w, h, n = width, height, width * height
    rng = np.random.default_rng(100 * which + w)
    fmt = T.track_format(P, w, h, depth_kind)
    nx, ny = grid_of(w, h)
    lab = T.blocks(w, h, nx, ny)
    mm = 1000.0 + 200.0 * lab + 3.0 * np.arange(w)[None, :] + 2.0 * np.arange(h)[:, None]
    holes = rng.random((h, w)) < 0.10
    K = nx * ny
    if which == 1:      # the ordinary path: blocks, 10 % holes, 5 % unlabelled
        mm = np.where(holes, 0.0, mm)
        lab = np.where(rng.random((h, w)) < 0.05, u32(NO), lab).astype(u32)
    elif which == 2:    # one region over the whole image
        lab, K = np.zeros((h, w), u32), 1
    elif which == 3:    # every pixel its own region
        lab, K = np.arange(n, dtype=u32).reshape(h, w), n
        mm = np.where(holes, 0.0, mm)
    elif which == 4:    # runs of length 1
        lab, K = (np.arange(n, dtype=u32) % 7).reshape(h, w), 7
    elif which == 5:    # many empty rows
        mm = np.where(holes, 0.0, mm)
        K = 1000
    elif which == 6:    # labels over invalid depths: scattered ones, and the whole of the last region
        mm = np.where(holes | (lab == K - 1), 0.0, mm)
    elif which == 7:    # ties: x * 65536 and z * 65536 land exactly on .5, towards even in both directions
        fmt = frame_format(P, w, h, "f32", "rgb8", 1.0)
        fmt.fx = fmt.fy = 1.0; fmt.cx = fmt.cy = 0.0
        k = rng.integers(0, 1 << 12, (h, w))
        depth = ((2 * k + 1).astype(np.float32) / np.float32(131072.0)).astype(np.float32)      # z = (2k + 1) / 2^17 exactly; x = u * z
        depth[holes] = 0.0
        return dict(fmt=fmt, depth=depth, labels=lab.astype(u32), n_regions=K)
    elif which == 8:    # the clamp: z up to 240 km, |x| beyond 32768 on all but the smallest frames
        fmt = T.track_format(P, w, h, depth_kind)
        fmt.depth_scale = 4.0
        mm = 20000.0 + 400.0 * lab + 300.0 * np.arange(w)[None, :]
        mm = np.where(holes, 0.0, np.minimum(mm, 60000.0))
    elif which == 9:    # x crosses zero inside the regions; a negative fx makes the centre column -0.0
        fmt.fx = -fmt.fx; fmt.cx = float(w // 2)
        fmt.cy = float(h // 2)
    return dict(fmt=fmt, depth=T.to_depth(mm, depth_kind), labels=np.asarray(lab, u32), n_regions=int(K))


def random_case(P, seed):
    """seeded random scene: (scene dict, colour kind, layout); depth kind, layout and colour format chosen by the seed"""
    rng = np.random.default_rng(5000 + seed)
    w, h = [(67, 45), (97, 61), (40, 30)][seed % 3]
    depth_kind = "u16" if seed % 2 == 0 else "f32"
    K = int(rng.integers(1, 41))
    depth, lab = T.random_scene(rng, w, h, K, depth_kind)
    return dict(fmt=T.track_format(P, w, h, depth_kind), depth=depth, labels=lab, n_regions=K), COLORS[seed % 4], "padded" if (seed // 2) % 2 else "tight"


RANDOM_SEEDS = list(range(24))
