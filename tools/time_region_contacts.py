#!/usr/bin/env python3
"""The region contacts behind the segmenter, the tracker and the region table (f3ds_region_contacts after f3ds_segment_rgbd, f3ds_tracker_update and
f3ds_region_table), lone frames, profiler off.
The frames are the bench workload's (1000 x 1000, seeds 1000 ... 1009, -v 0.008 -s 0.08 --AL --CVX -t 0.2) as pinned u16 depth + RGB8 colour
(tools/time_track.py makes the same images).  One process: segment frame k, update the tracker with its labels, take the region table and then the region
contacts of the same labels, next frame; wall time of each call, median and spread (min ... max) of the timed frames, in two forms:
  host    pinned host images and labels in, pinned host ids / rows out
  device  every buffer on the GPU: the images, the labels f3ds_segment_rgbd writes, the ids, the rows
Prints one JSON line; "condition_met": in the device form the contacts' median is not above the median of f3ds_tracker_update in the same run (the update
reads the same depth and label images, does two gathers per pixel and sorts all n 8-byte keys; the contacts read two more labels per pixel, depths only
along borders, and sort only the records of border spans).  No margin.  The host form is reported beside it with no condition: it is the two uploads over
the link.
usage: tools/time_region_contacts.py [--reps R] [--warmup W]
       tools/time_region_contacts.py --trace   one warm-up and one timed frame, device form only: the program of the rocprofv3 --kernel-trace --stats run
                                               (d_pair_init, d_contact_accum, the record sort, d_evl_heads, the scan, d_track_runs and d_contact_finish)"""
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
    """(segment times, update times, table times, contacts times, last RegionContactsResult as a dict) over warmup + reps frames, the ten frames in turn"""
    on_dev = 1 if form == "device" else 0
    ctx, trk = P.Context(0), P.Tracker(0)
    res, tres, rres, cres = P.Result(), P.TrackResult(), P.RegionTableResult(), P.RegionContactsResult()
    n_out = ctypes.c_size_t(0)
    if on_dev:
        d_in = [t.cuda() for t in depth]; c_in = [t.cuda() for t in color]
        lab, ids = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.int32, device="cuda")
        rows = torch.empty(MAX_ROWS * 18, dtype=torch.int32, device="cuda")
        crows = torch.empty(MAX_ROWS * 8, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
    else:
        d_in, c_in = depth, color
        lab, ids = torch.empty(N, dtype=torch.int32).pin_memory(), torch.empty(N, dtype=torch.int32).pin_memory()
        rows = torch.empty(MAX_ROWS * 18, dtype=torch.int32).pin_memory()
        crows = torch.empty(MAX_ROWS * 8, dtype=torch.int32).pin_memory()
    t_seg, t_upd, t_tab, t_con = [], [], [], []
    for k in range(args.warmup + args.reps):
        d, c = d_in[k % NF], c_in[k % NF]
        t0 = time.perf_counter()
        rc = lib.f3ds_segment_rgbd(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(c.data_ptr()), on_dev, ctypes.byref(prm), vp(lab.data_ptr()), on_dev, ctypes.byref(res))
        t1 = time.perf_counter()
        assert rc == 0 and res.n_regions <= MAX_ROWS, (rc, res.n_regions)
        rc = lib.f3ds_tracker_update(trk.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(lab.data_ptr()), res.n_regions, on_dev, None, vp(ids.data_ptr()), on_dev, ctypes.byref(tres))
        t2 = time.perf_counter()
        assert rc == 0, rc
        rc = lib.f3ds_region_table(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(c.data_ptr()), vp(lab.data_ptr()), res.n_regions, on_dev, vp(rows.data_ptr()), on_dev,
                                   ctypes.byref(rres))
        t3 = time.perf_counter()
        assert rc == 0 and rres.n_labelled == tres.n_labelled, (rc, rres.n_labelled, tres.n_labelled)
        rc = lib.f3ds_region_contacts(ctx.handle, ctypes.byref(fmt), vp(d.data_ptr()), vp(lab.data_ptr()), res.n_regions, 0.05, on_dev, vp(crows.data_ptr()), MAX_ROWS, on_dev,
                                      ctypes.byref(n_out), ctypes.byref(cres))
        t4 = time.perf_counter()
        assert rc == 0 and cres.n_contacts == n_out.value, (rc, cres.n_contacts, n_out.value)
        if k >= args.warmup:
            t_seg.append((t1 - t0) * 1e3); t_upd.append((t2 - t1) * 1e3); t_tab.append((t3 - t2) * 1e3); t_con.append((t4 - t3) * 1e3)
    out = dict(cres.as_dict(), n_nonempty=int(rres.n_nonempty))
    trk.close(); ctx.close()
    return t_seg, t_upd, t_tab, t_con, out


def summary(t):
    t = np.array(t)
    return dict(ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3))


out = dict(tool="time_region_contacts", lib=P.library_stamp(), pixels=N, reps=args.reps, warmup=args.warmup)
for form in (["device"] if args.trace else ["host", "device"]):
    t_seg, t_upd, t_tab, t_con, last = run(form)
    s, u, t, c = summary(t_seg), summary(t_upd), summary(t_tab), summary(t_con)
    out[form] = dict(segment_rgbd=s, tracker_update=u, region_table=t, region_contacts=c, contacts_over_update=round(c["ms_median"] / u["ms_median"], 4), last_contacts=last)
if not args.trace:
    out["condition_met"] = bool(out["device"]["region_contacts"]["ms_median"] <= out["device"]["tracker_update"]["ms_median"])
print(json.dumps(out))
