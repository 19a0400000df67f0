"""Shared by tests/test_label_image_wide_cpu.py and tests/test_label_image_wide_gpu.py: the label-image calls (the tracker update, f3ds_region_table,
_contacts, _shapes, _boxes, _components) at frames WIDER than a workgroup.  Nothing here is a new reference: the references are those of
region_table_common, region_contacts_common, region_shapes_common, region_boxes_common, region_components_common and track_common, and the scenes are their
generators at new sizes.  What this file adds is the list of cases, each with the classes of control flow it is for, and a CENSUS: the launch arithmetic of
csrc/f3ds_hip.hip and the span arithmetic of label_accum_span / pair_accum_span restated in plain Python from the kernels' constants (KERNEL_CONSTANTS,
compared with the library's own by name), so that a CPU test can assert that every case reaches what it claims.

Shapes (width x height, depth, layout) and what they reach -- a trip of a 256-thread workgroup moves a lane sv = 256 // width rows and su = 256 - sv * width
columns on, with one carry:
    255 x 9, 256 x 9, 257 x 9   u16 tight    sv 1 su 1 / sv 1 su 0 / sv 0 su 256: either side of and exactly one block per row; 257 is five tile columns, the last one pixel wide
    128 x 17                    f32 tight    sv 2 su 0
    512 x 5                     u16 padded   two blocks per row
    321 x 113                   u16 padded   6 x 8 tiles of 64 x 16, the last tile column one pixel wide; 36 273 pixels: 36 workgroups onto 32 accumulator sets
    640 x 61                    f32 tight    10 x 4 tiles, 2.5 blocks per row; 39 workgroups
Scenes: the region table's 1 (ordinary), 2 (one region: copies = 32, every flush onto one region), 3 (every pixel its own region: the LDS tables overflow) and
8 (the clamp); the components' spiral, comb_right, comb_bottom, checker and speckles; two seeded random scenes per shape (track_common.random_scene, K from
1 ... 40).  Scene 3 has K = n, and the boxes' reference takes a pass over the image per region: on the two large shapes scene 3 runs at 321 x 21 and 640 x 17
(two tile rows still, the same widths), which keeps that reference at a second or two; the census says what the shorter frames still reach.

Classes (CLASSES): a case lists the ones it is for, census() says which ones it reaches, and the CPU test asserts that the first is a subset of the second and
that no class is left without a case."""
import ctypes

import numpy as np

import region_boxes_common as B
import region_components_common as C
import region_contacts_common as CT
import region_table_common as R
import track_common as T

NO = 0xFFFFFFFF
INF = float("inf")
COMPONENT_TOLS = (0.05, INF)
CONTACT_TOLS = (0.05, 1.0e30)      # f3ds_region_contacts refuses a depth_tol that is not finite (include/f3ds.h): the second one calls every pair close, as inf would
u32, i64 = np.uint32, np.int64

# ---- the kernels' constants ---------------------------------------------------------------------------------------------------------------------------------
BLOCK = 256                                   # threads of every kernel of the family
LI_SLOTS, LI_PROBES, LI_TRIPS = 128, 8, 4     # csrc/f3ds_regions.inc: the LDS table of label_accum_span, and the trips its grid is sized for
RGC_SLOTS, RGC_TRIPS = 256, 8                 # csrc/f3ds_contacts.inc
RGT_MAX_COPIES, RGT_COPY_BUDGET = 32, 2048    # csrc/f3ds_regions.inc: rgt_copies
CC_TILE_W, CC_TILE_H = 64, 16                 # csrc/f3ds_components.h
GRID_CAP = 2048                               # csrc/f3ds_hip.hip: grid_for()'s cap for a lone frame unless F3DS_GRID_CAP narrows it
KERNEL_CONSTANTS = {       # name of P.constant() -> the value the census assumes
    "LI_SLOTS": LI_SLOTS, "LI_PROBES": LI_PROBES, "LI_TRIPS": LI_TRIPS, "RGT_MAX_COPIES": RGT_MAX_COPIES, "RGT_COPY_BUDGET": RGT_COPY_BUDGET, "RGC_SLOTS": RGC_SLOTS,
    "RGC_TRIPS": RGC_TRIPS, "CC_TILE_W": CC_TILE_W, "CC_TILE_H": CC_TILE_H, "WIDE_CAP": GRID_CAP,
    # the launches the census restates pass the kernel's own BLOCK to grid_for(); d_comp_local takes a tile per workgroup
    "d_region_accum::BLOCK": BLOCK, "d_shape_accum::BLOCK": BLOCK, "d_box_accum::BLOCK": BLOCK, "d_contact_accum::BLOCK": RGC_SLOTS, "d_comp_local::BLOCK": BLOCK,
    "d_comp_seam::BLOCK": BLOCK, "d_track_keys::BLOCK": BLOCK, "CC_TILES_PER_WG": 1,
}
# What the two operators of the span walk decide, by the classes of CLASSES that sit on them from both sides (test_label_image_wide_cpu.py asserts that each class has a
# case): acc += (BIX % copies) * K -- "wrap32" (more workgroups than accumulator sets: 36 and 39 onto 32) against every case of at most 32 workgroups; several workgroups onto
# as many sets or more (no wrap); the carry u >= width -- su = 1 (width 255: u reaches the width exactly, one trip in 255), su = 0 (256 and 128: never) and sv = 0 (257
# and wider: a carry on every trip that crosses a row end, u landing on the width exactly at 512 = two blocks).
OPERATOR_CLASSES = {"BIX % a.copies": ("wrap32", "several_workgroups"), "u >= a.width": ("below_block", "su0_sv1", "su0_sv2", "sv0")}


# ---- the launch and span arithmetic, restated -----------------------------------------------------------------------------------------------------------------
def grid_for(work, block, cap=0):
    """grid_for() of csrc/f3ds_hip.hip for a lone frame; cap: F3DS_GRID_CAP (0: unset)"""
    return min(max((work + block - 1) // block, 1), cap or GRID_CAP)


def accum_grid(n, trips, cap=0):
    """workgroups of d_region_accum / d_shape_accum / d_box_accum (trips = LI_TRIPS) or d_contact_accum (RGC_TRIPS)"""
    return grid_for((n + trips - 1) // trips, BLOCK, cap)


def span_of(n, grid):
    """pixels a workgroup of an accumulate launch holds: workgroup b takes [b * span, min(n, (b + 1) * span))"""
    per = (n + grid - 1) // grid
    return (per + BLOCK - 1) // BLOCK * BLOCK


def rgt_copies(K):
    return min(max(RGT_COPY_BUDGET // max(K, 1), 1), RGT_MAX_COPIES)


def step_of(width):
    """(sv, su): rows and columns a trip moves a lane on"""
    sv = BLOCK // width
    return sv, BLOCK - sv * width


def tiles_of(width, height):
    return (width + CC_TILE_W - 1) // CC_TILE_W, (height + CC_TILE_H - 1) // CC_TILE_H


def most_per_span(pixel, key, span):
    """the largest number of distinct keys among the entries whose pixel lies in one span"""
    if len(pixel) == 0:
        return 0
    pair = np.unique(np.stack([np.asarray(pixel, i64) // span, np.asarray(key, i64)], axis=1), axis=0)
    return int(np.bincount(pair[:, 0]).max())


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(255, 9, "u16", "tight"), (256, 9, "u16", "tight"), (257, 9, "u16", "tight"), (128, 17, "f32", "tight"), (512, 5, "u16", "padded"),
          (321, 113, "u16", "padded"), (640, 61, "f32", "tight")]
SCENE3_HEIGHT = {321: 21, 640: 17}      # scene 3 on the two large shapes (this file's docstring)
SCENES = ["table1", "table2", "table3", "table8", "spiral", "comb_right", "comb_bottom", "checker", "speckles", "random0", "random1"]
ALL_COLORS_AT = (257, 640)              # widths at which the table runs with every colour format; elsewhere with one, in turn
CLASSES = {
    "below_block": "sv == 1 and su == 1: a row one pixel short of the block",
    "su0_sv1": "su == 0 and sv == 1: a row is exactly the block",
    "su0_sv2": "su == 0 and sv == 2",
    "sv0": "sv == 0: a row is wider than the block, the carry acts on every trip that crosses a row end",
    "two_blocks": "a row is two blocks or more",
    "several_workgroups": "the accumulate launches get more than one workgroup at the default width",
    "wrap32": "more workgroups than accumulator sets, with 32 sets: two workgroups flush into one set",
    "tiles5_partial": "five or more tile columns and a partial last one",
    "lds_overflow": "some span of the table's launch meets more distinct labels than the LDS table has slots, at every launch width",
    "pairs_overflow": "some span of the contacts' launch meets more distinct pairs than its LDS table has slots, at every launch width",
    "spiral_seams": "one component crosses at least as many tile seams as there are tiles",
}


class Case:
    def __init__(self, width, height, depth_kind, layout, scene, index):
        self.width, self.height, self.depth_kind, self.layout, self.scene, self.index = width, height, depth_kind, layout, scene, index
        self.n = width * height
        self.id = "%dx%d-%s" % (width, height, scene)
        sv, su = step_of(width)
        tx, _ = tiles_of(width, height)
        many = scene == "table3"      # K = n: one accumulator set
        c = ["sv0" if sv == 0 else {(1, 1): "below_block", (1, 0): "su0_sv1", (2, 0): "su0_sv2"}[(sv, su)]]
        if width >= 2 * BLOCK:
            c.append("two_blocks")
        if accum_grid(self.n, LI_TRIPS) > 1:
            c.append("several_workgroups")
        if accum_grid(self.n, LI_TRIPS) > RGT_MAX_COPIES and not many:
            c.append("wrap32")
        if tx >= 5 and width % CC_TILE_W:
            c.append("tiles5_partial")
        if many:
            c += ["lds_overflow", "pairs_overflow"]
        if scene == "spiral" and self.n > 30000:
            c.append("spiral_seams")
        self.classes = c
        self.colors = list(R.COLORS) if width in ALL_COLORS_AT else [R.COLORS[index % 4]]
        self.min_pixels = [1, 3] if scene == "speckles" else [1]

    def __repr__(self):
        return self.id


def _cases():
    out = []
    for w, h, kind, layout in SHAPES:
        for scene in SCENES:
            out.append(Case(w, SCENE3_HEIGHT.get(w, h) if scene == "table3" else h, kind, layout, scene, len(out)))
    return out


CASES = _cases()
BAD_LABEL_CASE = next(c for c in CASES if c.id == "640x61-table1")
_frames = {}


def frame(P, case):
    """the images of a case, made once and left unchanged: dict(fmt (tight rows), depth, labels (h, w) u32, K, n) and, laid out as the case says (tight or
    padded rows), f (the format with its pitches), dbuf (the depth bytes) and per colour kind (colour array, format, colour bytes) in color[kind]"""
    if case.id not in _frames:
        w, h, kind = case.width, case.height, case.depth_kind
        if case.scene.startswith("random"):
            rng = np.random.default_rng(31000 + 10 * case.index + int(case.scene[6:]))
            K = int(rng.integers(1, 41))
            depth, lab = T.random_scene(rng, w, h, K, kind)
            sc = dict(fmt=T.track_format(P, w, h, kind), depth=depth, labels=lab, n_regions=K)
        else:
            sc = C.scene(P, case.scene, w, h, kind)
        fr = dict(fmt=sc["fmt"], depth=np.ascontiguousarray(sc["depth"]), labels=np.ascontiguousarray(sc["labels"], u32), K=int(sc["n_regions"]), n=w * h, color={})
        fr["f"], fr["dbuf"], _ = R.buffers(fr["fmt"], fr["depth"], None, case.layout)
        for ck in R.COLORS:
            fmt = R.with_color(P, fr["fmt"], ck)
            color = R.make_color(w, h, ck)
            f, _, cbuf = R.buffers(fmt, fr["depth"], color, case.layout)
            fr["color"][ck] = (color, f, cbuf)
        perm = np.random.default_rng(77 + case.index).permutation(fr["K"]).astype(u32)
        fr["permuted"] = np.where(fr["labels"] == NO, u32(NO), perm[np.minimum(fr["labels"], fr["K"] - 1)]).astype(u32)
        _frames[case.id] = fr
    return _frames[case.id]


def depth_view(case, fr):
    """the depth image as a (h, w) array over the laid-out bytes: strided where the rows are padded (the package takes the row stride as the pitch)"""
    dt = np.dtype(np.uint16 if case.depth_kind == "u16" else np.float32)
    pitch = int(fr["f"].depth_pitch) or case.width * dt.itemsize
    return np.ndarray((case.height, case.width), dt, fr["dbuf"], 0, (pitch, dt.itemsize))


def color_view(case, fr, kind):
    """likewise the colour image of one kind, or None"""
    color, f, cbuf = fr["color"][kind]
    if color is None:
        return None
    pitch = int(f.color_pitch) or color.strides[0]
    return np.ndarray(color.shape, color.dtype, cbuf, 0, (pitch,) + color.strides[1:])


# ---- references, computed once per (case, call, parameters) ------------------------------------------------------------------------------------------------
_refs = {}


def reference(P, case, what, *prm):
    """what: "table" (colour kind) -> (rc, rows, result); "boxes" () -> (rc, box rows, shape rows, boxes' result) -- the shapes' result is that without
    n_inliers; "contacts" (depth_tol) -> (rc, rows, result); "components" (depth_tol, min_pixels) -> (rc, image, rows, result); "track" () -> the six updates of
    track_frames() on one RefTracker, [(rc, id image, ids, result)]"""
    key = (case.id, what) + prm
    if key not in _refs:
        fr = frame(P, case)
        a = (fr["fmt"], fr["depth"], fr["labels"], fr["K"])
        if what == "table":
            fmt = R.with_color(P, fr["fmt"], prm[0])
            _refs[key] = R.ref_table(P, fmt, fr["depth"], fr["labels"], fr["K"], fr["color"][prm[0]][0])
        elif what == "boxes":
            _refs[key] = B.ref_boxes(P, *a)
        elif what == "contacts":
            _refs[key] = CT.ref_contacts(P, *a, prm[0])
        elif what == "components":
            _refs[key] = C.ref_components(P, *a, prm[0], prm[1])
        elif what == "track":
            ref = T.RefTracker()
            out = []
            for labels, reset in track_frames(fr):
                if reset:
                    ref.reset()
                out.append(ref.update(fr["fmt"], fr["depth"], labels, fr["K"]))
            _refs[key] = out
        else:
            raise KeyError(what)
    return _refs[key]


def shapes_result(boxes_result):
    return {k: v for k, v in boxes_result.items() if k != "n_inliers"}


def track_frames(fr):
    """[(labels, reset first?)]: the frame, the same again, the same under permuted labels; then a reset and the three once more (the second time round the
    GPU test takes its inputs from device memory)"""
    three = [(fr["labels"], False), (fr["labels"], False), (fr["permuted"], False)]
    return three + [(fr["labels"], True)] + three[1:]


def c_components_tiled(P, case, fr, depth_tol, min_pixels, tile):
    """f3ds_region_components_tiled (the kernels' union-find steps run tile by tile, seam by seam, on the host) on the laid-out buffers: (rc, image, rows, result)"""
    lib = P.load_library()
    lab = fr["labels"].reshape(-1)
    prm = P.ComponentParams(float(depth_tol), int(min_pixels))
    image = np.full(fr["n"], 0xA5A5A5A5, u32)
    rows = np.zeros(fr["n"], P.REGION_COMPONENT_DTYPE)
    n_out, res = ctypes.c_size_t(0), P.RegionComponentsResult()
    rc = lib.f3ds_region_components_tiled(ctypes.byref(fr["f"]), fr["dbuf"].ctypes.data, lab.ctypes.data, fr["K"], ctypes.byref(prm), tile[0], tile[1], image.ctypes.data,
                                          rows.ctypes.data, len(rows), ctypes.byref(n_out), ctypes.byref(res))
    return rc, image.reshape(case.height, case.width), rows[:n_out.value], res


# ---- the census -------------------------------------------------------------------------------------------------------------------------------------------------
CAPS = [0, 1, 2048]      # F3DS_GRID_CAP of the GPU test: unset, one workgroup, as many as the frame allows


def census(P, case):
    """dict: the figures of a case and `reached`, the set of classes whose condition holds"""
    fr = frame(P, case)
    w, h, n, K = case.width, case.height, case.n, fr["K"]
    sv, su = step_of(w)
    tx, ty = tiles_of(w, h)
    out = dict(sv=sv, su=su, tiles_x=tx, tiles_y=ty, copies=rgt_copies(K), workgroups=accum_grid(n, LI_TRIPS), contact_workgroups=accum_grid(n, RGC_TRIPS),
               trips_of_one=span_of(n, 1) // BLOCK)
    reached = set()
    if sv == 1 and su == 1:
        reached.add("below_block")
    if sv == 1 and su == 0:
        reached.add("su0_sv1")
    if sv == 2 and su == 0:
        reached.add("su0_sv2")
    if sv == 0:
        reached.add("sv0")
    if w >= 2 * BLOCK:
        reached.add("two_blocks")
    if out["workgroups"] > 1 and out["contact_workgroups"] > 1:
        reached.add("several_workgroups")
    if out["workgroups"] > out["copies"] and out["copies"] == RGT_MAX_COPIES:
        reached.add("wrap32")
    if tx >= 5 and w % CC_TILE_W:
        reached.add("tiles5_partial")
    # labels and pairs per span, at the widest launch the GPU test runs (the shortest spans): a span of a narrower launch is a union of those
    lab = fr["labels"].reshape(-1)
    _, valid = CT.depth_z(fr["fmt"], fr["depth"])
    p = np.flatnonzero(valid & (lab != NO))
    out["labels_per_span"] = min(most_per_span(p, lab[p], span_of(n, accum_grid(n, LI_TRIPS, cap))) for cap in CAPS)
    pairs = CT.pairs_of(fr["fmt"], fr["depth"], fr["labels"], 0.05)
    out["pairs_per_span"] = min(most_per_span(pairs["p"], pairs["a"] * max(K, 1) + pairs["b"], span_of(n, accum_grid(n, RGC_TRIPS, cap))) for cap in CAPS)
    if out["labels_per_span"] > LI_SLOTS:
        reached.add("lds_overflow")
    if out["pairs_per_span"] > RGC_SLOTS:
        reached.add("pairs_overflow")
    # seams a component crosses: its links whose two pixels lie in different tiles
    lp, lq, _ = C.links_of(fr["fmt"], fr["depth"], fr["labels"], 0.05)
    tile = lambda x: (x // w // CC_TILE_H) * tx + x % w // CC_TILE_W
    cross = tile(lp) != tile(lq)
    image = reference(P, case, "components", 0.05, 1)[1].reshape(-1)
    out["seam_links"] = int(np.bincount(image[lp[cross]].astype(i64)).max()) if cross.any() else 0
    if out["seam_links"] >= tx * ty:
        reached.add("spiral_seams")
    out["reached"] = reached
    return out
