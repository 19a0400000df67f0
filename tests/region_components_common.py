"""Shared by tests/test_region_components_cpu.py and tests/test_region_components_gpu.py: the reference of the region components (include/f3ds.h, "region
components"), written from the definition -- depths and the class of a pair in np.float32 arithmetic (region_contacts_common.depth_z, the contacts' reference),
the links as boolean masks over the pixel pairs, the classes from a plain Python union-find over the links, sizes with np.bincount, the numbering from the
sorted roots -- and the scenes both files run.  It does not call the library.  Image and rows are compared bit for bit as u32 words.

Scenes (by name; every one at every shape of SHAPES):
   table1 ... table6, at depth_tol 0.05 and inf   the region table's scenes as they are; table3 (every pixel its own region) has n components
   spiral              two interleaved one-pixel-wide spirals of labels 0 and 1: the longest chain an image holds, across every seam many times
   comb_bottom / comb_top / comb_right   teeth of one label between unlabelled gaps, joined along one edge only: tiles see separate parts, the seams merge them
   checker / checker_min2   two labels, every pixel a component; with min_pixels = 2 none is kept
   occluder / occluder_invalid   label 0 left and right of a bar of label 1 (0, 1, 0 in first-pixel order) / of invalid depths under label 0 (a label over an invalid depth cuts)
   stripes / stripes_inf   one label over depth stripes at 1 m and 2 m: splits at depth_tol 0.05, one component at inf
   stripes_ulp         the contacts' scene 8: base 2 m, depth_tol 2^-4, the other side on the bound, one ulp nearer, one ulp further: links, links, does not link
   stripes_zero        depth_tol 0: equal depths link, one ulp apart does not
   staircase           diagonals of one label: diagonal touching only, one component per pixel
   speckles            speckles of 1 ... 5 pixels, min_pixels = 3: sizes 3, 4, 5 kept, the numbering without gaps; a 2 x 2 one on the meeting point of four tiles"""
import numpy as np

import region_contacts_common as C
import region_table_common as R
import track_common as T
from rgbd_common import frame_format

NO = 0xFFFFFFFF
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_CAPACITY = 0, -1, -7, -10
SHAPES = C.SHAPES      # 97 x 61 u16 tight, 67 x 45 f32 padded, 3 x 2, 1 x 1, 40 x 1, 1 x 40
TILE_W, TILE_H = 64, 16      # CC_TILE_W, CC_TILE_H of csrc/f3ds_components.h
TILE_SIZES = [(1, 1), (2, 2), (3, 5), (TILE_W, TILE_H)]
INF = float("inf")
SCENES = (["table%d" % k for k in range(1, 7)] + ["table%d_inf" % k for k in range(1, 7)] +
          ["spiral", "comb_bottom", "comb_top", "comb_right", "checker", "checker_min2", "occluder", "occluder_invalid", "stripes", "stripes_inf", "stripes_ulp",
           "stripes_zero", "staircase", "speckles"])
RESULT_FIELDS = ("n_regions", "n_components", "n_dropped", "reserved", "n_labelled", "n_kept")
u32, f32, i64 = np.uint32, np.float32, np.int64
buffers = R.buffers


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------
def links_of(fmt, depth, labels, depth_tol):
    """(p, q): the two pixels of every link of the definition, flat int64 arrays; and the labelled mask"""
    h, w = int(fmt.height), int(fmt.width)
    lab = np.asarray(labels, u32).reshape(-1)
    z, valid = C.depth_z(fmt, depth)
    labelled = valid & (lab != NO)
    pix = np.arange(h * w, dtype=i64).reshape(h, w)
    p = np.concatenate([pix[:, :-1].reshape(-1), pix[:-1, :].reshape(-1)])
    q = np.concatenate([pix[:, :-1].reshape(-1) + 1, pix[:-1, :].reshape(-1) + w])
    za, zb = z[p].astype(f32), z[q].astype(f32)
    with np.errstate(all="ignore"):
        g = np.abs(za - zb)                              # one rounded f32 subtraction
        zn = np.where(za < zb, za, zb)
        bound = f32(depth_tol) * zn                      # one rounded f32 product
        close = g <= bound                               # false on NaN
    assert g.dtype == f32 and bound.dtype == f32
    m = labelled[p] & labelled[q] & (lab[p] == lab[q]) & close
    return p[m], q[m], labelled


def ref_components(P, fmt, depth, labels, n_regions, depth_tol=0.05, min_pixels=1):
    """(rc, image (h, w) uint32, rows (REGION_COMPONENT_DTYPE), result dict) of the definition; all None but rc unless rc == 0"""
    K = int(n_regions)
    h, w = int(fmt.height), int(fmt.width)
    lab = np.asarray(labels, u32).reshape(-1)
    if ((lab != NO) & (lab >= K)).any():
        return ERR_ARG, None, None, None
    if not depth_tol >= 0:
        return ERR_ARG, None, None, None
    p, q, labelled = links_of(fmt, depth, labels, depth_tol)
    parent = list(range(h * w))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(p.tolist(), q.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)      # the root is the smallest index of the class
    root = np.array([find(x) for x in range(h * w)], i64)
    size = np.bincount(root[labelled], minlength=h * w)
    roots = np.nonzero(size > 0)[0]                  # ascending: raster order of the first pixels
    kept = roots[size[roots] >= max(int(min_pixels), 1)]
    number = np.full(h * w, NO, i64)
    number[kept] = np.arange(len(kept))
    image = np.where(labelled, number[root], NO).astype(u32).reshape(h, w)
    rows = np.zeros(len(kept), P.REGION_COMPONENT_DTYPE)
    rows["region"], rows["first_pixel"], rows["n_pixels"] = lab[kept], kept, size[kept]
    res = dict(n_regions=K, n_components=len(kept), n_dropped=len(roots) - len(kept), reserved=0, n_labelled=int(labelled.sum()), n_kept=int(size[kept].sum()))
    return OK, image, rows, res


def words_of(rows):
    return np.ascontiguousarray(rows).view(u32).reshape(len(rows), 3)


def assert_same(got_image, got_rows, want_image, want_rows, what=""):
    gi, wi = np.asarray(got_image, u32).reshape(-1), np.asarray(want_image, u32).reshape(-1)
    assert gi.shape == wi.shape, "%s image of %d words, want %d" % (what, gi.size, wi.size)
    if not np.array_equal(gi, wi):
        i = int(np.nonzero(gi != wi)[0][0])
        raise AssertionError("%s image word %d: %#x, want %#x (%d words differ)" % (what, i, gi[i], wi[i], int((gi != wi).sum())))
    assert len(got_rows) == len(want_rows), "%s %d rows, want %d" % (what, len(got_rows), len(want_rows))
    g, w = words_of(got_rows), words_of(want_rows)
    if not np.array_equal(g, w):
        i, k = [int(a[0]) for a in np.nonzero(g != w)]
        raise AssertionError("%s row %d word %d: %#x, want %#x\ngot  %r\nwant %r" % (what, i, k, g[i, k], w[i, k], got_rows[i], want_rows[i]))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def spiral_labels(w, h):
    """label 0 along a one-pixel-wide rectangular spiral from the top left corner inwards, one pixel of room between its arms; label 1 on the rest"""
    lab = np.ones((h, w), u32)
    seen = np.zeros((h, w), bool)
    u = v = 0
    du, dv = 1, 0
    lab[0, 0] = 0; seen[0, 0] = True

    def free(a, b):
        return 0 <= a < w and 0 <= b < h and not seen[b, a]

    def may_step(a, b, da, db):      # onto a free pixel whose next one along the way is no arm already
        return free(a + da, b + db) and not (0 <= a + 2 * da < w and 0 <= b + 2 * db < h and seen[b + 2 * db, a + 2 * da])
    turns = 0
    while turns < 2:
        if may_step(u, v, du, dv):
            u, v = u + du, v + dv
            lab[v, u] = 0; seen[v, u] = True
            turns = 0
        else:
            du, dv = -dv, du      # right, down, left, up
            turns += 1
    return lab


def speckle_labels(w, h):
    """unlabelled but for speckles of 1, 2, 3, 4, 5 pixels on a grid of 5 x 4 pixel cells, one label each in turn of three; a 2 x 2 speckle on the meeting
    point of four tiles where the image reaches it"""
    shapes = [[(0, 0)], [(0, 0), (1, 0)], [(0, 0), (1, 0), (0, 1)], [(0, 0), (1, 0), (0, 1), (1, 1)], [(1, 0), (0, 1), (1, 1), (2, 1), (1, 2)]]
    lab = np.full((h, w), NO, u32)
    k = 0
    for v0 in range(0, h - 3, 4):
        for u0 in range(0, w - 3, 5):
            if abs(u0 - TILE_W) < 6 and abs(v0 - TILE_H) < 5:
                continue      # (room for the speckle on the tiles' corner)
            for du, dv in shapes[k % 5]:
                lab[v0 + dv, u0 + du] = k % 3
            k += 1
    if w > TILE_W and h > TILE_H:
        lab[TILE_H - 1:TILE_H + 1, TILE_W - 1:TILE_W + 1] = 1
    return lab


def scene(P, name, width, height, depth_kind):
    """scene `name` (the table of this file's docstring) at this size: dict(fmt, depth, labels (h, w) u32, n_regions, depth_tol, min_pixels)"""
    w, h = width, height
    if name.startswith("table"):
        return dict(R.scene(P, int(name[5]), w, h, depth_kind), depth_tol=INF if name.endswith("_inf") else 0.05, min_pixels=1)
    uu, vv = np.meshgrid(np.arange(w), np.arange(h))
    fmt = T.track_format(P, w, h, depth_kind)
    mm = 1500.0 + 0.0 * uu      # a wall at 1.5 m
    tol, minpix, K = 0.05, 1, 2
    if name == "spiral":
        lab = spiral_labels(w, h)
    elif name.startswith("comb"):
        if name == "comb_right":
            lab = np.where((vv % 2 == 0) | (uu == w - 1), 0, NO)
        else:
            lab = np.where((uu % 2 == 0) | (vv == (h - 1 if name == "comb_bottom" else 0)), 0, NO)
        K = 1
    elif name.startswith("checker"):
        lab = (uu + vv) % 2
        minpix = 2 if name == "checker_min2" else 1
    elif name.startswith("occluder"):
        bar = (uu >= w // 3) & (uu < w // 3 + max(1, w // 8))
        if name == "occluder":
            lab = np.where(bar, 1, 0)
        else:
            lab = np.zeros((h, w), u32)
            mm = np.where(bar, 0.0, mm)
    elif name in ("stripes", "stripes_inf"):
        lab, K = np.zeros((h, w), u32), 1
        mm = np.where((uu // 5) % 2 == 0, 1000.0, 2000.0)
        tol = INF if name == "stripes_inf" else 0.05
    elif name in ("stripes_ulp", "stripes_zero"):      # f32 depths in metres: every depth below is exact (as the contacts' scenes 8 and 9)
        fmt = frame_format(P, w, h, "f32", "rgb8", 1.0)
        lab, K = np.zeros((h, w), u32), 1
        if name == "stripes_ulp":      # base 2 m, depth_tol 2^-4: the bound is 0.125 exactly; the odd columns at 2.125 (on it), one ulp nearer, one ulp further
            on = f32(2.125)
            depth = np.where(uu % 2 == 0, f32(2.0), np.choose((uu // 2) % 3, [on, np.nextafter(on, f32(0)), np.nextafter(on, f32(4))])).astype(f32)
            tol = 0.0625
        else:
            depth = np.where((uu // 3) % 2 == 0, f32(2.0), np.nextafter(f32(2.0), f32(4))).astype(f32)
            tol = 0.0
        return dict(fmt=fmt, depth=depth, labels=lab, n_regions=K, depth_tol=tol, min_pixels=1)
    elif name == "staircase":
        lab, K = np.where((uu - vv) % 3 == 0, 0, NO), 1
    elif name == "speckles":
        lab, K, minpix = speckle_labels(w, h), 3, 3
    else:
        raise KeyError(name)
    return dict(fmt=fmt, depth=T.to_depth(mm, depth_kind), labels=np.asarray(lab, np.int64).astype(u32), n_regions=K, depth_tol=tol, min_pixels=minpix)


def random_case(P, seed):
    """seeded random scene: (scene dict, layout, launch width); depth kind, layout, launch width, depth_tol and min_pixels chosen by the seed"""
    rng = np.random.default_rng(9000 + seed)
    w, h = [(67, 45), (97, 61), (40, 30)][seed % 3]
    depth_kind = "u16" if seed % 2 == 0 else "f32"
    K = int(rng.integers(1, 41))
    depth, lab = T.random_scene(rng, w, h, K, depth_kind)
    tol = [0.0, 0.01, 0.05, INF][int(rng.integers(0, 4))]
    minpix = [1, 1, 4, 50][int(rng.integers(0, 4))]
    sc = dict(fmt=T.track_format(P, w, h, depth_kind), depth=depth, labels=lab, n_regions=K, depth_tol=tol, min_pixels=minpix)
    return sc, "padded" if (seed // 2) % 2 else "tight", [0, 0, 1, 3][seed % 4]


RANDOM_SEEDS = list(range(18))
_refs = {}


def reference(P, key, sc):
    """the reference of a scene, computed once and shared"""
    if key not in _refs:
        _refs[key] = ref_components(P, sc["fmt"], sc["depth"], sc["labels"], sc["n_regions"], sc["depth_tol"], sc["min_pixels"])
    return _refs[key]
