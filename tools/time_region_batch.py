#!/usr/bin/env python3
"""The batch forms of the five region calls against 64 lone calls (f3ds_region_table_batch, _shapes_batch, _boxes_batch, _contacts_batch, _components_batch),
profiler off.  The frames are the bench workload's (1000 x 1000, seeds 1000 ... 1063, -v 0.008 -s 0.08 --AL --CVX -t 0.2) as pinned u16 depth + RGB8 colour, one
context per frame; f3ds_segment_rgbd_batch runs once and its labels stay on the device.  Then, for each of the five calls, every round runs
  (a) lone   the 64 lone calls on their contexts, one after the other
  (b) batch  one batch call
in turn: wall time of each, which ends in the calls' own waits; median and spread (min ... max) of the timed rounds.  Two forms:
  device  every buffer on the GPU: the images, the labels, the rows, the component images
  host    pinned host images and labels in, pinned host rows and images out (bound by the copies over the link: reported, no condition)
and two label images: the segmenter's, and (table, shapes, boxes, contacts; device form) the component image with n_regions = n_components.
Prints one JSON line; "condition_met": in the device form, on the segmenter's labels, the median of the batch call is below the median of the 64 lone calls
of the same run, for each of the five calls.
usage: tools/time_region_batch.py [--frames F] [--reps R] [--warmup W] [--host-reps R]
       tools/time_region_batch.py --trace     one warm-up and one batch call per kind, device form only: the program of the rocprofv3 --kernel-trace --stats run
                                              (microseconds per batched dispatch, beside the lone figures of profiles/region_*_time.txt)"""
import argparse, ctypes, importlib, json, os, sys, time
import numpy as np
import torch        # (first: libf3ds binds to the HIP runtime torch has mapped)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = importlib.import_module("fast-3d-pointcloud-segmentation_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-reps", type=int, default=4)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
if args.trace:
    args.reps, args.warmup = 1, 1
W = H = 1000
N = W * H
NF = args.frames
CONTACT_CAP = COMPONENT_CAP = 1 << 16      # rows a frame has room for (device form; the host form takes 2048, what rides with the heads, when the counts allow)
PLANE_TOL, DEPTH_TOL = 0.01, 0.05
CALLS = ("table", "contacts", "shapes", "boxes", "components")
prm = P.launch_params(voxel_res=0.008, seed_res=0.08)
lib = P.load_library()
fmt = P.RgbdFormat(W, H, P.DEPTH_U16, 0.001, P.COLOR_RGB8, 0, 0, 0.8 * W, 0.8 * W, (W - 1) / 2.0, (H - 1) / 2.0)
cprm = P.ComponentParams(DEPTH_TOL, 1)
vp, sz = ctypes.c_void_p, ctypes.c_size_t
RES = dict(table=P.RegionTableResult, contacts=P.RegionContactsResult, shapes=P.RegionShapesResult, boxes=P.RegionBoxesResult, components=P.RegionComponentsResult)


def pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


depth, color = [], []
for i in range(NF):
    pts = P.synth_frame(0, 1000 + i, W, H, 30)
    z = pts[:, 2]
    d = np.where(np.isnan(z), 0.0, np.rint(np.abs(z.astype(np.float64)) * 1000.0)).astype(np.uint16).reshape(H, W)
    rgba = pts[:, 3].view(np.uint32)
    c = np.stack([(rgba >> 16) & 255, (rgba >> 8) & 255, rgba & 255], axis=1).astype(np.uint8).reshape(H, W, 3)
    depth.append(pinned(d.view(np.uint8))); color.append(pinned(c))

ctxs = [P.Context(0) for _ in range(NF)]
handles = (vp * NF)(*[c.handle for c in ctxs])
d_depth, d_color = [t.cuda() for t in depth], [t.cuda() for t in color]
d_lab = [torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(NF)]
torch.cuda.synchronize()
ptrs = lambda ts: (vp * NF)(*[vp(t.data_ptr()) for t in ts])
seg_res = (P.Result * NF)()
t0 = time.perf_counter()
rc = lib.f3ds_segment_rgbd_batch(handles, NF, ctypes.byref(fmt), ptrs(d_depth), ptrs(d_color), 1, ctypes.byref(prm), ptrs(d_lab), 1, seg_res)
segment_ms = (time.perf_counter() - t0) * 1e3      # (the first call of the process: allocations included)
assert rc == 0, rc
K_SEG = [int(r.n_regions) for r in seg_res]


class Form:
    """the buffers of one form (device / host) over one label image per frame"""

    def __init__(self, on_dev, labels, K, dep, col, contact_cap=CONTACT_CAP, component_cap=COMPONENT_CAP):
        self.contact_cap, self.component_cap = contact_cap, component_cap
        self.on, self.K, self.dep, self.col, self.lab = 1 if on_dev else 0, K, dep, col, labels
        new = (lambda words: torch.empty(max(words, 1), dtype=torch.int32, device="cuda")) if on_dev else (lambda words: torch.empty(max(words, 1), dtype=torch.int32).pin_memory())
        self.rows = dict(table=[new(18 * k) for k in K], shapes=[new(21 * k) for k in K], boxes=[new(24 * k) for k in K], contacts=[new(8 * contact_cap) for _ in K],
                         components=[new(3 * component_cap) for _ in K])
        self.bshapes = [new(21 * k) for k in K]
        self.comp = [new(N) for _ in K]
        self.nr = (ctypes.c_uint32 * NF)(*K)
        self.caps = dict(contacts=(sz * NF)(*[contact_cap] * NF), components=(sz * NF)(*[component_cap] * NF))
        self.n_out = (sz * NF)()
        self.n_lone = [sz() for _ in range(NF)]
        self.res = {c: (RES[c] * NF)() for c in CALLS}
        self.status = np.zeros(NF, np.int32)
        self.p = dict(dep=ptrs(dep), col=ptrs(col), lab=ptrs(labels), comp=ptrs(self.comp), bshapes=ptrs(self.bshapes), **{"rows_" + c: ptrs(self.rows[c]) for c in CALLS})
        torch.cuda.synchronize()

    def lone(self, call):
        f, on = ctypes.byref(fmt), self.on
        for i in range(NF):
            h, d, l, k, r, res = handles[i], self.p["dep"][i], self.p["lab"][i], self.K[i], self.p["rows_" + call][i], ctypes.byref(self.res[call][i])
            if call == "table":
                rc = lib.f3ds_region_table(h, f, d, self.p["col"][i], l, k, on, r, on, res)
            elif call == "shapes":
                rc = lib.f3ds_region_shapes(h, f, d, l, k, on, r, on, res)
            elif call == "boxes":
                rc = lib.f3ds_region_boxes(h, f, d, l, k, PLANE_TOL, on, r, self.p["bshapes"][i], on, res)
            elif call == "contacts":
                rc = lib.f3ds_region_contacts(h, f, d, l, k, DEPTH_TOL, on, r, self.contact_cap, on, ctypes.byref(self.n_lone[i]), res)
            else:
                rc = lib.f3ds_region_components(h, f, d, l, k, ctypes.byref(cprm), on, self.p["comp"][i], r, self.component_cap, on, ctypes.byref(self.n_lone[i]), res)
            assert rc == 0, (call, i, rc)

    def batch(self, call):
        f, on, p, st = ctypes.byref(fmt), self.on, self.p, self.status.ctypes.data
        if call == "table":
            rc = lib.f3ds_region_table_batch(handles, NF, f, p["dep"], p["col"], p["lab"], self.nr, on, p["rows_table"], on, self.res[call], st)
        elif call == "shapes":
            rc = lib.f3ds_region_shapes_batch(handles, NF, f, p["dep"], p["lab"], self.nr, on, p["rows_shapes"], on, self.res[call], st)
        elif call == "boxes":
            rc = lib.f3ds_region_boxes_batch(handles, NF, f, p["dep"], p["lab"], self.nr, PLANE_TOL, on, p["rows_boxes"], p["bshapes"], on, self.res[call], st)
        elif call == "contacts":
            rc = lib.f3ds_region_contacts_batch(handles, NF, f, p["dep"], p["lab"], self.nr, DEPTH_TOL, on, p["rows_contacts"], self.caps[call], on, self.n_out, self.res[call], st)
        else:
            rc = lib.f3ds_region_components_batch(handles, NF, f, p["dep"], p["lab"], self.nr, ctypes.byref(cprm), on, p["comp"], p["rows_components"], self.caps[call], on, self.n_out,
                                                  self.res[call], st)
        assert rc == 0 and not self.status.any(), (call, rc, self.status)

    def snapshot(self, call):
        """what a run of `call` left: results and rows of every frame (rows by the results' counts)"""
        torch.cuda.synchronize()
        count = dict(table=lambda i: 18 * self.K[i], shapes=lambda i: 21 * self.K[i], boxes=lambda i: 24 * self.K[i], contacts=lambda i: 8 * self.res[call][i].n_contacts,
                     components=lambda i: 3 * self.res[call][i].n_components)[call]
        out = [bytes(self.res[call])]
        for i in range(NF):
            out.append(self.rows[call][i][:count(i)].cpu().numpy().tobytes())
            if call == "components":
                out.append(self.comp[i].cpu().numpy().tobytes())
            if call == "boxes":
                out.append(self.bshapes[i][:21 * self.K[i]].cpu().numpy().tobytes())
        return out

    def time(self, call, reps, warmup, calls=("lone", "batch")):
        t = dict(lone=[], batch=[])
        for k in range(warmup + reps):
            for kind in calls:
                t0 = time.perf_counter()
                getattr(self, kind)(call)
                if k >= warmup:
                    t[kind].append((time.perf_counter() - t0) * 1e3)
        return t


def summary(t):
    t = np.array(t)
    return dict(ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3))


def measure(form, reps, calls=CALLS, check=True):
    out = {}
    for call in calls:
        if check and not args.trace:      # the batch leaves what the lone calls leave, byte for byte
            form.lone(call); a = form.snapshot(call)
            form.batch(call); b = form.snapshot(call)
            assert a == b, call + ": the batch call's outputs differ from the lone calls'"
        t = form.time(call, reps, args.warmup, ("batch",) if args.trace else ("lone", "batch"))
        if args.trace:
            continue
        lo, ba = summary(t["lone"]), summary(t["batch"])
        out[call] = dict(lone=lo, batch=ba, lone_over_batch=round(lo["ms_median"] / ba["ms_median"], 3), ms_per_frame_lone=round(lo["ms_median"] / NF, 4),
                         ms_per_frame_batch=round(ba["ms_median"] / NF, 4))
    return out


out = dict(tool="time_region_batch", lib=P.library_stamp(), frames=NF, pixels=N, reps=args.reps, warmup=args.warmup, first_segment_batch_ms=round(segment_ms, 1),
           regions_min=min(K_SEG), regions_max=max(K_SEG))
dev = Form(True, d_lab, K_SEG, d_depth, d_color)
out["device"] = measure(dev, args.reps)
if not args.trace:
    # the component image as the label image (the components ran last above: dev.comp and its results are the batch's)
    K_COMP = [int(r.n_components) for r in dev.res["components"]]
    out["components_min"], out["components_max"] = min(K_COMP), max(K_COMP)
    on_comp = Form(True, dev.comp, K_COMP, d_depth, d_color)
    out["device_on_component_labels"] = measure(on_comp, args.reps, ("table", "contacts", "shapes", "boxes"))
    del on_comp
    h_lab = [pinned(t.cpu().numpy()) for t in d_lab]
    fits = lambda counts: 2048 if max(counts) <= 2048 else 1 << 16
    host = Form(False, h_lab, K_SEG, depth, color, fits([int(r.n_contacts) for r in dev.res["contacts"]]), fits(K_COMP))
    out["host_caps"] = dict(contacts=host.contact_cap, components=host.component_cap)
    out["host"] = measure(host, args.host_reps, check=False)
    out["condition_met"] = bool(all(out["device"][c]["batch"]["ms_median"] < out["device"][c]["lone"]["ms_median"] for c in CALLS))
print(json.dumps(out))
for c in ctxs:
    c.close()
