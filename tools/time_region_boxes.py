#!/usr/bin/env python3
"""The region boxes behind the segmenter and the region shapes (f3ds_region_boxes after f3ds_segment_rgbd and f3ds_region_shapes), lone frames, profiler
off.  The frames are the bench workload's (1000 x 1000, seeds 1000 ... 1009, -v 0.008 -s 0.08 --AL --CVX -t 0.2) as pinned u16 depth + RGB8 colour
(tools/time_region_shapes.py makes the same images).  One process: segment frame k, take the region shapes and then the region boxes (with their shape
rows, plane_tol 0.01) of the same labels, next frame; wall time of each call, median and spread (min ... max) of the timed frames, in two forms:
  host    pinned host images and labels in, pinned host rows out
  device  every buffer on the GPU: the images, the labels f3ds_segment_rgbd writes, the rows
Prints one JSON line; "condition_met": in the device form the median of f3ds_region_boxes is at most THREE times the median of f3ds_region_shapes in the
same run.  The factor is a count of passes, not a measurement: two reads of the image where the shapes make one, plus one for the frame gather and the
extra launches.  The host form is reported beside it with no condition: it is bound by the copies over the link.
usage: tools/time_region_boxes.py [--reps R] [--warmup W]
       tools/time_region_boxes.py --trace     one warm-up and one timed frame, device form only: the program of the rocprofv3 --kernel-trace --stats run
                                              (d_shape_init / accum / finish of both calls, d_box_frame, d_box_accum and d_box_finish per frame)"""
import argparse, ctypes, importlib, json, os, sys, time
import numpy as np
import torch        # (first: libf3ds binds to the HIP runtime torch has mapped)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = importlib.import_module("fast-3d-pointcloud-segmentation_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
if args.trace:
    args.reps, args.warmup = 1, 1
W = H = 1000
N = W * H
NF = 10
MAX_ROWS = 1 << 16
PLANE_TOL = 0.01
prm = P.launch_params(voxel_res=0.008, seed_res=0.08)
lib = P.load_library()
fmt = P.RgbdFormat(W, H, P.DEPTH_U16, 0.001, P.COLOR_RGB8, 0, 0, 0.8 * W, 0.8 * W, (W - 1) / 2.0, (H - 1) / 2.0)
vp = ctypes.c_void_p


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


def run(form):
    """(segment times, shapes times, boxes times, last RegionBoxesResult as a dict) over warmup + reps frames, the ten frames in turn"""
    on_dev = 1 if form == "device" else 0
    ctx = P.Context(0)
    res, sres, bres = P.Result(), P.RegionShapesResult(), P.RegionBoxesResult()

    def buf(words):
        t = torch.empty(words, dtype=torch.int32, device="cuda") if on_dev else torch.empty(words, dtype=torch.int32).pin_memory()
        return t
    if on_dev:
        d_in = [t.cuda() for t in depth]; c_in = [t.cuda() for t in color]
    else:
        d_in, c_in = depth, color
    lab, srows, brows, bshapes = buf(N), buf(MAX_ROWS * 21), buf(MAX_ROWS * 24), buf(MAX_ROWS * 21)
    torch.cuda.synchronize()
    t_seg, t_shp, t_box = [], [], []
    for k in range(args.warmup + args.reps):
        d, c = d_in[k % NF], c_in[k % NF]
        t0 = time.perf_counter()
        rc = lib.f3ds_segment_rgbd(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(c.data_ptr()), on_dev, ctypes.byref(prm), vp(lab.data_ptr()), on_dev, ctypes.byref(res))
        t1 = time.perf_counter()
        assert rc == 0 and res.n_regions <= MAX_ROWS, (rc, res.n_regions)
        rc = lib.f3ds_region_shapes(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(lab.data_ptr()), res.n_regions, on_dev, vp(srows.data_ptr()), on_dev, ctypes.byref(sres))
        t2 = time.perf_counter()
        assert rc == 0, rc
        rc = lib.f3ds_region_boxes(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(lab.data_ptr()), res.n_regions, PLANE_TOL, on_dev, vp(brows.data_ptr()),
                                   vp(bshapes.data_ptr()), on_dev, ctypes.byref(bres))
        t3 = time.perf_counter()
        assert rc == 0 and bres.n_labelled == sres.n_labelled and bres.n_nonempty == sres.n_nonempty and bres.n_inliers <= bres.n_labelled, (rc, bres.as_dict(), sres.as_dict())
        if k >= args.warmup:
            t_seg.append((t1 - t0) * 1e3); t_shp.append((t2 - t1) * 1e3); t_box.append((t3 - t2) * 1e3)
    if on_dev:
        torch.cuda.synchronize()
    K = int(res.n_regions)
    same = bool(torch.equal(srows[:21 * K].cpu(), bshapes[:21 * K].cpu()))      # the boxes' shape rows are the shapes', word for word
    out = dict(bres.as_dict(), shape_rows_equal=same)
    ctx.close()
    return t_seg, t_shp, t_box, out


def summary(t):
    t = np.array(t)
    return dict(ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3))


out = dict(tool="time_region_boxes", lib=P.library_stamp(), pixels=N, reps=args.reps, warmup=args.warmup, plane_tol=PLANE_TOL)
for form in (["device"] if args.trace else ["host", "device"]):
    t_seg, t_shp, t_box, last = run(form)
    s, h, b = summary(t_seg), summary(t_shp), summary(t_box)
    out[form] = dict(segment_rgbd=s, region_shapes=h, region_boxes=b, boxes_over_shapes=round(b["ms_median"] / h["ms_median"], 4), last_boxes=last)
if not args.trace:
    out["condition_met"] = bool(out["device"]["region_boxes"]["ms_median"] <= 3.0 * out["device"]["region_shapes"]["ms_median"])
print(json.dumps(out))
