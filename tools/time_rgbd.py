#!/usr/bin/env python3
"""RGB-D frames in (f3ds_segment_rgbd_batch: u16 depth + RGB8 colour, 5 bytes per pixel) against the same frames as 16-byte records
(f3ds_segment_batch), host buffer in to host labels out, everything pinned, profiler off.  The frames are the bench workload's (1000 x 1000,
seeds 1000 ..., -v 0.008 -s 0.08 --AL --CVX -t 0.2) turned into images: depth = rint(|z| * 1000), colour = the low three bytes of rgba,
fx = fy = 800, cx = cy = 499.5, depth_scale = 0.001; the records are f3ds_deproject's of those images, so both paths segment the same points.
The two calls alternate in one process, both warmed up; wall time of the call, median and spread (min ... max) of the timed batches.
Prints one JSON line; "condition_met": the rgbd median is not above the points median by more than the larger spread.
usage: tools/time_rgbd.py [--batch F] [--reps R] [--warmup W]
       tools/time_rgbd.py --trace [--batch F]     one warm-up and one timed rgbd batch only: the program of the rocprofv3 --kernel-trace --stats run
                                                  (tools/kstats.py <dir> <2 * F> then gives d_deproject and d_bbox per frame)"""
import argparse, ctypes, importlib, json, os, sys, time
import numpy as np
import torch        # (first: libf3ds binds to the HIP runtime torch has mapped)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = importlib.import_module("fast-3d-pointcloud-segmentation_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
if args.trace:
    args.reps, args.warmup = 1, 1
W = H = 1000
N = W * H
F = args.batch
prm = P.launch_params(voxel_res=0.008, seed_res=0.08)
lib = P.load_library()
fmt = P.RgbdFormat(W, H, P.DEPTH_U16, 0.001, P.COLOR_RGB8, 0, 0, 0.8 * W, 0.8 * W, (W - 1) / 2.0, (H - 1) / 2.0)
vp = ctypes.c_void_p


def pinned(a):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


depth, color, records = [], [], []
for i in range(F):
    pts = P.synth_frame(0, 1000 + i, W, H, 30)
    z = pts[:, 2]
    d = np.where(np.isnan(z), 0.0, np.rint(np.abs(z.astype(np.float64)) * 1000.0)).astype(np.uint16).reshape(H, W)
    rgba = pts[:, 3].view(np.uint32)
    c = np.stack([(rgba >> 16) & 255, (rgba >> 8) & 255, rgba & 255], axis=1).astype(np.uint8).reshape(H, W, 3)
    depth.append(pinned(d)); color.append(pinned(c))
    if not args.trace:
        records.append(pinned(P.deproject(fmt, d, c)))
lab_r = [torch.empty(N, dtype=torch.int32).pin_memory() for _ in range(F)]
lab_p = [torch.empty(N, dtype=torch.int32).pin_memory() for _ in range(F)]
ctx_r = [P.Context(0) for _ in range(F)]
ctx_p = [] if args.trace else [P.Context(0) for _ in range(F)]
res = (P.Result * F)()
h_r = (vp * F)(*[c.handle for c in ctx_r]); h_p = (vp * F)(*[c.handle for c in ctx_p])
dp = (vp * F)(*[vp(t.data_ptr()) for t in depth]); cp = (vp * F)(*[vp(t.data_ptr()) for t in color]); pp = (vp * F)(*[vp(t.data_ptr()) for t in records])
lr = (vp * F)(*[vp(t.data_ptr()) for t in lab_r]); lp = (vp * F)(*[vp(t.data_ptr()) for t in lab_p])
cnt = (ctypes.c_size_t * F)(*[N] * F)


def run_rgbd():
    t0 = time.perf_counter()
    rc = lib.f3ds_segment_rgbd_batch(h_r, F, ctypes.byref(fmt), dp, cp, 0, ctypes.byref(prm), lr, 0, res)
    assert rc == 0, rc
    return (time.perf_counter() - t0) * 1e3


def run_points():
    t0 = time.perf_counter()
    rc = lib.f3ds_segment_batch(h_p, F, pp, cnt, 0, ctypes.byref(prm), lp, 0, res)
    assert rc == 0, rc
    return (time.perf_counter() - t0) * 1e3


t_r, t_p = [], []
for k in range(args.warmup + args.reps):
    a = run_rgbd()
    b = run_points() if not args.trace else 0.0
    if k >= args.warmup:
        t_r.append(a); t_p.append(b)


def summary(t, bytes_in):
    t = np.array(t)
    med = float(np.median(t))
    return dict(ms_median=round(med, 2), ms_min=round(float(t.min()), 2), ms_max=round(float(t.max()), 2), Mpoints_per_s=round(F * N / med / 1e3, 1),
                upload_bytes_per_point=bytes_in)


out = dict(tool="time_rgbd", lib=P.library_stamp(), frames=F, reps=args.reps, warmup=args.warmup, rgbd=summary(t_r, 5))
if not args.trace:
    out["points"] = summary(t_p, 16)
    spread = max(out["rgbd"]["ms_max"] - out["rgbd"]["ms_min"], out["points"]["ms_max"] - out["points"]["ms_min"])
    out["spread_ms"] = round(spread, 2)
    out["rgbd_over_points_rate"] = round(out["points"]["ms_median"] / out["rgbd"]["ms_median"], 3)
    out["condition_met"] = bool(out["rgbd"]["ms_median"] <= out["points"]["ms_median"] + spread)
    same = all(bool(torch.equal(a, b)) for a, b in zip(lab_r, lab_p))
    out["labels_equal"] = same
for c in ctx_r + ctx_p:
    c.close()
print(json.dumps(out))
