#!/usr/bin/env python3
"""The region joints behind the segmenter (f3ds_region_joints after f3ds_segment_rgbd), beside the two calls that give the same information in two waits
(f3ds_region_contacts and f3ds_region_shapes), lone frames, profiler off.
The frames are the bench workload's (1000 x 1000, seeds 1000 ... 1009, -v 0.008 -s 0.08 --AL --CVX -t 0.2) as pinned u16 depth + RGB8 colour
(tools/time_region_contacts.py makes the same images).  One process: segment frame k, then the contacts, the shapes and the joints of its labels in turn,
next frame; wall time of each call, median and spread (min ... max) of the timed frames, in two forms:
  host    pinned host images and labels in, pinned host rows out
  device  every buffer on the GPU: the images, the labels f3ds_segment_rgbd writes, the rows
Prints one JSON line; "condition_met": in the device form the joints' median is at most 1.5 times the sum of the medians of f3ds_region_contacts and
f3ds_region_shapes in the same run (the joints do everything those two do and save one wait and one download; the margin pays for the 34-word records
and for one Jacobi finish per row).  The host form is reported beside it with no condition.
usage: tools/time_region_joints.py [--reps R] [--warmup W]
       tools/time_region_joints.py --trace   one warm-up and one timed frame, device form only: the program of the rocprofv3 --kernel-trace --stats run
                                             (the shapes' three kernels, d_pair_init, d_joint_accum, the record sort, d_evl_heads, the scan, d_track_runs
                                             and d_joint_finish)"""
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
    """(segment, contacts, shapes, joints times; the last RegionJointsResult as a dict) over warmup + reps frames, the ten frames in turn"""
    on_dev = 1 if form == "device" else 0
    ctx = P.Context(0)
    res, cres, sres, jres = P.Result(), P.RegionContactsResult(), P.RegionShapesResult(), P.RegionJointsResult()
    n_out = ctypes.c_size_t(0)
    make = (lambda n: torch.empty(n, dtype=torch.int32, device="cuda")) if on_dev else (lambda n: torch.empty(n, dtype=torch.int32).pin_memory())
    if on_dev:
        d_in = [t.cuda() for t in depth]; c_in = [t.cuda() for t in color]
    else:
        d_in, c_in = depth, color
    lab, crows, srows, jrows, jshapes = make(N), make(MAX_ROWS * 8), make(MAX_ROWS * 21), make(MAX_ROWS * 20), make(MAX_ROWS * 21)
    if on_dev:
        torch.cuda.synchronize()
    t_seg, t_con, t_sha, t_joi = [], [], [], []
    for k in range(args.warmup + args.reps):
        d, c = d_in[k % NF], c_in[k % NF]
        t0 = time.perf_counter()
        rc = lib.f3ds_segment_rgbd(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(c.data_ptr()), on_dev, ctypes.byref(prm), vp(lab.data_ptr()), on_dev, ctypes.byref(res))
        t1 = time.perf_counter()
        assert rc == 0 and res.n_regions <= MAX_ROWS, (rc, res.n_regions)
        rc = lib.f3ds_region_contacts(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(lab.data_ptr()), res.n_regions, 0.05, on_dev, vp(crows.data_ptr()), MAX_ROWS, on_dev,
                                      ctypes.byref(n_out), ctypes.byref(cres))
        t2 = time.perf_counter()
        assert rc == 0 and cres.n_contacts == n_out.value, (rc, cres.n_contacts, n_out.value)
        rc = lib.f3ds_region_shapes(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(lab.data_ptr()), res.n_regions, on_dev, vp(srows.data_ptr()), on_dev, ctypes.byref(sres))
        t3 = time.perf_counter()
        assert rc == 0, rc
        rc = lib.f3ds_region_joints(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(lab.data_ptr()), res.n_regions, None, on_dev, vp(jrows.data_ptr()), MAX_ROWS,
                                    vp(jshapes.data_ptr()), on_dev, ctypes.byref(n_out), ctypes.byref(jres))
        t4 = time.perf_counter()
        assert rc == 0 and (jres.n_joints, jres.n_pairs, jres.n_close) == (cres.n_contacts, cres.n_pairs, cres.n_close), (rc, jres.as_dict(), cres.as_dict())
        if k >= args.warmup:
            t_seg.append((t1 - t0) * 1e3); t_con.append((t2 - t1) * 1e3); t_sha.append((t3 - t2) * 1e3); t_joi.append((t4 - t3) * 1e3)
    out = dict(jres.as_dict(), n_nonempty=int(sres.n_nonempty))
    ctx.close()
    return t_seg, t_con, t_sha, t_joi, out


def summary(t):
    t = np.array(t)
    return dict(ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3))


out = dict(tool="time_region_joints", lib=P.library_stamp(), pixels=N, reps=args.reps, warmup=args.warmup)
for form in (["device"] if args.trace else ["host", "device"]):
    t_seg, t_con, t_sha, t_joi, last = run(form)
    s, c, h, j = summary(t_seg), summary(t_con), summary(t_sha), summary(t_joi)
    both = c["ms_median"] + h["ms_median"]
    out[form] = dict(segment_rgbd=s, region_contacts=c, region_shapes=h, region_joints=j, contacts_plus_shapes_ms=round(both, 3), joints_over_both=round(j["ms_median"] / both, 4),
                     last_joints=last)
if not args.trace:
    out["condition_met"] = bool(out["device"]["region_joints"]["ms_median"] <= 1.5 * out["device"]["contacts_plus_shapes_ms"])
print(json.dumps(out))
