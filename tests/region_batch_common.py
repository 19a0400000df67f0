"""Shared by tests/test_region_batch_cpu.py and tests/test_region_batch_gpu.py: the batches the batch forms of the five region calls run
(f3ds_region_table_batch, _shapes_batch, _boxes_batch, _contacts_batch, _components_batch in include/f3ds.h), their references and one runner for all five.

The reference of every frame is the f3ds_*_host function on that frame (the package's region_*_host): the CPU tests of the five calls pin those to the numpy
references bit for bit, and the numpy reference of the boxes takes a pass over the image per region, too slow at K = 5917.  The frames of a batch share a format
and differ in everything else; scenes are region_table_common.scene and label_image_wide_common.frame:

    one      nctx 1, 97 x 61 u16 tight     scene 1: the batch must be the lone call
    four     nctx 4, 97 x 61 u16 tight     scene 1; scene 3 (every pixel its own region: K = 5917, one accumulator set, more labels in a span than LI_SLOTS, more than
                                           2048 contact and component rows); scene 2 (one region: 32 sets, every flush on one region); scene 6 (labels over invalid
                                           depths, the last region empty)
    five     nctx 5, 67 x 45 f32 padded    scene 1; the same with a depth that is invalid everywhere; n_regions = 0 with every label F3DS_NO_LABEL; scene 5 (K = 1000, many
                                           empty rows); scene 8 (the clamp) -- all five under scene 8's format (its depth scale is what makes the clamp)
    wide     nctx 3, 257 x 9 u16 tight     table1, table3 and spiral of the wide cases: a trip stays inside a row, the last tile column is one pixel wide
    tiny32   nctx 3, 3 x 2 u16 tight       scenes 1, 2, 3
    tiny11   nctx 3, 1 x 1 f32 tight       scenes 1, 2, 3

run() calls the C entry point on raw buffers, host or device, every output prefilled with 0x5A5A5A5A words (n_out and status with 777, results with sevens)."""
import ctypes

import numpy as np

import label_image_wide_common as W
import region_table_common as R

NO = 0xFFFFFFFF
PREFILL = 0x5A5A5A5A
UNSET = 777
CALLS = ("table", "shapes", "boxes", "contacts", "components")
BATCHES = ("one", "four", "five", "wide", "tiny32", "tiny11")
DEPTH_TOL, PLANE_TOL = 0.05, 0.01
FIRST_ROWS = 2048      # RGC_FIRST_ROWS / RGK_FIRST_ROWS of csrc/f3ds_contacts.inc / f3ds_components.inc
u32 = np.uint32


class Batch:
    def __init__(self, name, fmt, kind, layout, frames):
        self.name, self.fmt, self.kind, self.layout, self.frames = name, fmt, kind, layout, frames
        self.width, self.height, self.n, self.nctx = int(fmt.width), int(fmt.height), int(fmt.width) * int(fmt.height), len(frames)


_batches = {}


def _scene(P, which, w, h, kind):
    s = R.scene(P, which, w, h, kind)
    return dict(depth=np.ascontiguousarray(s["depth"]), labels=np.ascontiguousarray(s["labels"], u32), K=int(s["n_regions"]), fmt=s["fmt"])


def batch(P, name):
    """the batch `name`, made once and left unchanged"""
    if name in _batches:
        return _batches[name]
    if name in ("one", "four"):
        w, h, kind, layout = 97, 61, "u16", "tight"
        frames = [_scene(P, k, w, h, kind) for k in ((1,) if name == "one" else (1, 3, 2, 6))]
        fmt = frames[0]["fmt"]
    elif name == "five":
        w, h, kind, layout = 67, 45, "f32", "padded"
        s1, s5, s8 = (_scene(P, k, w, h, kind) for k in (1, 5, 8))
        invalid = dict(s1, depth=np.zeros_like(s1["depth"]))
        none = dict(s1, labels=np.full((h, w), NO, u32), K=0)
        frames, fmt = [s1, invalid, none, s5, s8], s8["fmt"]
    elif name == "wide":
        w, h, kind, layout = 257, 9, "u16", "tight"
        frames = []
        for scene in ("table1", "table3", "spiral"):
            fr = W.frame(P, next(c for c in W.CASES if c.id == "257x9-%s" % scene))
            frames.append(dict(depth=fr["depth"], labels=fr["labels"], K=fr["K"], fmt=fr["fmt"]))
        fmt = frames[0]["fmt"]
    else:
        w, h, kind, layout = dict(tiny32=(3, 2, "u16", "tight"), tiny11=(1, 1, "f32", "tight"))[name]
        frames = [_scene(P, k, w, h, kind) for k in (1, 2, 3)]
        fmt = frames[0]["fmt"]
    if name != "five":      # one format for the batch: the scenes chosen do not touch it
        assert all(bytes(f["fmt"]) == bytes(fmt) for f in frames)
    _batches[name] = Batch(name, fmt, kind, layout, frames)
    return _batches[name]


def color_of(B, i, kind):
    """frame i's colour image of one kind (None: none): seeded by the frame, so the frames of a batch differ"""
    return R.make_color(B.width, B.height, kind, seed=11 + i)


# ---- references: the host functions, once per (batch, frame, call, parameters) --------------------------------------------------------------------------------
_refs = {}


def reference(P, B, i, call, color_kind=None, labels=None, min_pixels=1):
    """frame i's answer of the f3ds_*_host function: ("ok", outputs...) or ("arg",) for a label >= n_regions.  table: rows, result; shapes: rows, result;
    boxes: rows, shape rows, result; contacts: rows, result; components: image, rows, result.  `labels` replaces the frame's (not cached)."""
    key = (B.name, i, call, color_kind, min_pixels)
    if labels is None and key in _refs:
        return _refs[key]
    fr = B.frames[i]
    lab = fr["labels"] if labels is None else labels
    a = (fr["depth"], lab, fr["K"])
    try:
        if call == "table":
            out = P.region_table_host(*a, R.with_color(P, B.fmt, color_kind), color_of(B, i, color_kind))
        elif call == "shapes":
            out = P.region_shapes_host(*a, B.fmt)
        elif call == "boxes":
            out = P.region_boxes_host(*a, B.fmt, PLANE_TOL, want_shapes=True)
        elif call == "contacts":
            out = P.region_contacts_host(*a, B.fmt, DEPTH_TOL)
        else:
            out = P.region_components_host(*a, B.fmt, DEPTH_TOL, min_pixels)
        ans = ("ok",) + tuple(out)
    except P.F3dsError as e:
        assert e.code == P.ERR_ARG, e
        ans = ("arg",)
    if labels is None:
        _refs[key] = ans
    return ans


def row_count(P, B, i, call):
    """rows of frame i's answer (contacts, components)"""
    return len(reference(P, B, i, call)[2 if call == "components" else 1])


# ---- the runner -------------------------------------------------------------------------------------------------------------------------------------------------
def spec(P, call):
    return dict(table=(P.REGION_ROW_DTYPE, P.RegionTableResult), shapes=(P.REGION_SHAPE_DTYPE, P.RegionShapesResult), boxes=(P.REGION_BOX_DTYPE, P.RegionBoxesResult),
                contacts=(P.REGION_CONTACT_DTYPE, P.RegionContactsResult), components=(P.REGION_COMPONENT_DTYPE, P.RegionComponentsResult))[call]


def sevens(res_type):
    return res_type(*([7] * len(res_type._fields_)))


class Buffers:
    """host or device buffers of one run; device tensors are kept alive here"""

    def __init__(self, where):
        self.device = where == "device"
        self.keep = []
        if self.device:
            import torch
            self.torch = torch

    def put(self, arr):
        """an input: its address"""
        arr = np.ascontiguousarray(arr)
        if not self.device:
            self.keep.append(arr)
            return arr.ctypes.data
        t = self.torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()
        self.keep.append(t)
        return t.data_ptr()

    def out(self, words):
        """an output of `words` prefilled words: (address, handle for get())"""
        if not self.device:
            a = np.full(max(int(words), 1), PREFILL, u32)
            return a.ctypes.data, a
        t = self.torch.full((max(int(words), 1),), PREFILL, dtype=self.torch.int32, device="cuda")
        return t.data_ptr(), t

    def sync(self):
        if self.device:
            self.torch.cuda.synchronize()

    def get(self, handle):
        return handle if not self.device else handle.cpu().numpy().view(u32)


def run(P, ctxs, B, call, where="host", color_kind=None, caps=None, labels=None, min_pixels=1, want_shapes=True, want_rows=True, handles=None, fmt=None, n_regions=None,
        depth_tol=DEPTH_TOL, plane_tol=PLANE_TOL, null_rows_at=None, comp_is_labels_at=None, status=True):
    """f3ds_region_<call>_batch on raw buffers.  caps: per-frame row capacities of contacts / components (default: the frame's count + 2); labels: {frame: array}
    replacing a frame's labels; handles: the context pointers (default: those of ctxs).  Returns dict(rc, status (int32 array), frames=[dict(rows, shapes, image
    (u32 word arrays, whole buffers), n_out, res)])."""
    lib = ctxs[0].lib if ctxs else P.load_library()
    k = B.nctx
    vp = ctypes.c_void_p
    dtype, res_type = spec(P, call)
    rw = dtype.itemsize // 4
    buf = Buffers(where)
    f = R.with_color(P, B.fmt if fmt is None else fmt, color_kind) if call == "table" else (B.fmt if fmt is None else fmt).copy()
    dps, cps, lps, outs = [], [], [], []
    Ks = [fr["K"] for fr in B.frames] if n_regions is None else list(n_regions)
    if caps is None and call in ("contacts", "components"):
        caps = [row_count(P, B, i, call) + 2 for i in range(k)]
    for i, fr in enumerate(B.frames):
        ff, dbuf, cbuf = R.buffers(f, fr["depth"], color_of(B, i, color_kind) if call == "table" else None, B.layout)
        if i == 0:
            f = ff
        dps.append(buf.put(dbuf))
        cps.append(None if cbuf is None else buf.put(cbuf))
        lab = fr["labels"] if not (labels and i in labels) else labels[i]
        lps.append(buf.put(np.ascontiguousarray(lab, u32).reshape(-1)))
        o = {}
        if call in ("table", "shapes", "boxes"):
            o["rows"] = buf.out(Ks[i] * rw if Ks[i] < (1 << 24) else 1)
            if call == "boxes":
                o["shapes"] = buf.out(Ks[i] * 21 if Ks[i] < (1 << 24) else 1)
        else:
            o["rows"] = buf.out(caps[i] * rw)
            if call == "components":
                o["image"] = buf.out(B.n)
        outs.append(o)
    buf.sync()
    arr = lambda ptrs: (vp * k)(*[None if p is None else vp(p) for p in ptrs])
    hs = arr([c.handle.value for c in ctxs]) if handles is None else handles
    nr = (ctypes.c_uint32 * k)(*Ks)
    results = (res_type * k)(*[sevens(res_type) for _ in range(k)])
    st = np.full(k, UNSET, np.int32)
    n_out = (ctypes.c_size_t * k)(*[UNSET] * k)
    on = 1 if buf.device else 0
    rows_p = [o["rows"][0] for o in outs]
    if null_rows_at is not None:
        rows_p[null_rows_at] = None
    stp = st.ctypes.data if status else None
    fb = ctypes.byref(f)
    if call == "table":
        rc = lib.f3ds_region_table_batch(hs, k, fb, arr(dps), arr(cps) if color_kind else None, arr(lps), nr, on, arr(rows_p), on, results, stp)
    elif call == "shapes":
        rc = lib.f3ds_region_shapes_batch(hs, k, fb, arr(dps), arr(lps), nr, on, arr(rows_p), on, results, stp)
    elif call == "boxes":
        rc = lib.f3ds_region_boxes_batch(hs, k, fb, arr(dps), arr(lps), nr, plane_tol, on, arr(rows_p), arr([o["shapes"][0] for o in outs]) if want_shapes else None, on, results, stp)
    elif call == "contacts":
        rc = lib.f3ds_region_contacts_batch(hs, k, fb, arr(dps), arr(lps), nr, depth_tol, on, arr(rows_p) if want_rows else None, (ctypes.c_size_t * k)(*caps), on, n_out, results, stp)
    else:
        prm = P.ComponentParams(depth_tol, min_pixels)
        images = [o["image"][0] for o in outs]
        if comp_is_labels_at is not None:
            images[comp_is_labels_at] = lps[comp_is_labels_at]
        rc = lib.f3ds_region_components_batch(hs, k, fb, arr(dps), arr(lps), nr, ctypes.byref(prm), on, arr(images), arr(rows_p) if want_rows else None, (ctypes.c_size_t * k)(*caps), on,
                                              n_out, results, stp)
    buf.sync()
    frames = []
    for i, o in enumerate(outs):
        frames.append(dict(rows=buf.get(o["rows"][1]), shapes=buf.get(o["shapes"][1]) if "shapes" in o else None, image=buf.get(o["image"][1]) if "image" in o else None,
                           n_out=int(n_out[i]), res=results[i], cap=caps[i] if caps else None))
    return dict(rc=rc, status=st, frames=frames)


def untouched(P, call, fr):
    """nothing of a frame was written: every buffer holds the prefill, n_out and the result too"""
    _, res_type = spec(P, call)
    ok = all((fr[k] == PREFILL).all() for k in ("rows", "shapes", "image") if fr[k] is not None) and fr["res"].as_dict() == sevens(res_type).as_dict()
    return ok and (call not in ("contacts", "components") or fr["n_out"] == UNSET)


def words(a):
    return np.ascontiguousarray(a).view(u32).reshape(-1)


def assert_frame(P, call, got, want, what="", want_shapes=True, want_rows=True):
    """frame `got` of run() holds exactly the host function's answer `want` (reference()), and the prefill behind it"""
    assert want[0] == "ok", what
    res = want[-1]
    assert got["res"].as_dict() == res.as_dict(), (what, got["res"].as_dict(), res.as_dict())
    rows = want[2] if call == "components" else want[1]
    w = words(rows) if want_rows else np.zeros(0, u32)
    g = got["rows"]
    if not np.array_equal(g[:len(w)], w):
        j = int(np.flatnonzero(g[:len(w)] != w)[0])
        raise AssertionError("%s: rows word %d (row %d): %#x, want %#x" % (what, j, j // max(rows.dtype.itemsize // 4, 1), g[j], w[j]))
    assert (g[len(w):] == PREFILL).all(), what + ": written behind the rows"
    if call == "boxes":
        s = words(want[2]) if want_shapes else np.zeros(0, u32)
        assert np.array_equal(got["shapes"][:len(s)], s) and (got["shapes"][len(s):] == PREFILL).all(), what + ": shape rows"
    if call == "components":
        assert np.array_equal(got["image"][:len(words(want[1]))], words(want[1])), what + ": image"
    if call in ("contacts", "components"):
        assert got["n_out"] == len(rows), (what, got["n_out"], len(rows))


def assert_batch(P, B, call, out, what="", color_kind=None, **kw):
    """every frame of a run is OK and holds its reference"""
    assert out["rc"] == 0 and (out["status"] == 0).all(), (what, out["rc"], out["status"])
    for i in range(B.nctx):
        assert_frame(P, call, out["frames"][i], reference(P, B, i, call, color_kind), "%s %s frame %d %s" % (B.name, call, i, what), **kw)
