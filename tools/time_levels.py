#!/usr/bin/env python3
"""Hierarchy levels (f3ds_labels_at_thresholds) against K reclusters, on the bench workload's frame (seed 1000, 1M points, -v 0.008 -s 0.08
--AL --CVX -t 0.2).  Prints one JSON line:
  lone   per K in {1, 4, 8, 16}: device time of one f3ds_labels_at_thresholds call (labels_on_device) and of K f3ds_recluster calls
         (labels_on_device), and the K = 8 call over ONE recluster (the "< 1" goal);
  batch  64 such frames (seeds 1000..1063), K = 8, one f3ds_labels_at_thresholds_batch call: device time, algorithmic bytes
         (per point K x 4 B written + 4 B pt_voxel + 4 B owner gather, plus per frame the tables written and read once: (S0 + 1) x Kp x 4 B x 2),
         their rate and its share of the 8 TB/s HBM peak.
Device time = torch.cuda events around the call on the stream the contexts run on (f3ds_set_stream), median of the repeats.
usage: tools/time_levels.py [--quick] [--reps R] [--batch F]   (--quick: K = 8 only, 8 frames: the program of the kernel-trace run)"""
import argparse, ctypes, importlib, json, os, sys
import numpy as np
import torch        # (first: libf3ds binds to the HIP runtime torch has mapped)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
P = importlib.import_module("fast-3d-pointcloud-segmentation_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
if args.quick:
    args.batch, args.reps = 8, 3
HBM_PEAK = 8.0e12
W = H = 1000
N = W * H
prm = P.launch_params(voxel_res=0.008, seed_res=0.08)
stream = torch.cuda.Stream()
lib = P.load_library()


def device_ms(fn, reps):
    fn()                                                        # warm-up (scratch grows once)
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            fn()
            b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def thresholds(K):
    return np.linspace(0.0, prm.threshold, K).astype(np.float32)[::-1].copy()      # (the first level is T itself)


ctx = P.Context(0)
ctx.set_stream(stream.cuda_stream)
pts = P.synth_frame(0, 1000, W, H, 30)
ctx.segment(pts, prm)
S0 = int(ctx.result.n_supervoxels)
lone = dict(n_points=N, n_supervoxels=S0, n_merges=int(ctx.result.n_merges), K={})
dev = torch.empty(16 * N, dtype=torch.int32, device="cuda")
res = P.Result()


def recluster_once():
    rc = lib.f3ds_recluster(ctx.handle, ctypes.byref(prm), ctypes.c_void_p(dev.data_ptr()), 1, ctypes.byref(res))
    assert rc == 0, rc


ms_recluster = device_ms(recluster_once, args.reps)
lone["ms_one_recluster"] = round(ms_recluster, 4)
for K in ([8] if args.quick else [1, 4, 8, 16]):
    ts = thresholds(K)
    ms = device_ms(lambda: ctx.labels_at_thresholds(ts, out=dev, on_device=True), args.reps)
    lone["K"][K] = dict(ms_levels=round(ms, 4), ms_K_reclusters=round(K * ms_recluster, 3), speedup=round(K * ms_recluster / ms, 1))
got = dev[:N].cpu().numpy().view(np.uint32)
assert np.array_equal(got, ctx.recluster(prm)), "level 0 (t = T) differs from the frame's labels"
lone["levels8_over_one_recluster"] = round(lone["K"][8]["ms_levels"] / ms_recluster, 5)
ctx.close()

# ---- batch of F frames, K = 8
F, K = args.batch, 8
Kp = (K + 3) // 4 * 4
ts = thresholds(K)
ctxs = [P.Context(0) for _ in range(F)]
for c in ctxs:
    c.set_stream(stream.cuda_stream)
for g in range(0, F, 16):
    group = ctxs[g:g + 16]
    P.segment_batch(group, [P.synth_frame(0, 1000 + g + i, W, H, 30) for i in range(len(group))], prm)
outs = [torch.empty(K * N, dtype=torch.int32, device="cuda") for _ in range(F)]
ms = device_ms(lambda: P.labels_at_thresholds_batch(ctxs, ts, out=outs, on_device=True), args.reps)
s0 = [int(c.result.n_supervoxels) for c in ctxs]
point_bytes = F * N * (K * 4 + 8)
table_bytes = sum((s + 1) * Kp * 4 * 2 for s in s0)
rate = (point_bytes + table_bytes) / (ms * 1e-3)
lds_form = all((s + 1) * Kp * 4 <= 48 * 1024 for s in s0)
batch = dict(frames=F, K=K, ms_levels=round(ms, 4), bytes=point_bytes + table_bytes, GBps=round(rate / 1e9, 1), hbm_peak_share=round(rate / HBM_PEAK, 4),
             floor_ms_at_peak=round((point_bytes + table_bytes) / HBM_PEAK * 1e3, 4), table_form="lds" if lds_form else "global",
             supervoxels_min_max=[min(s0), max(s0)])
for c in ctxs:
    c.close()
print(json.dumps(dict(tool="time_levels", lib=P.library_stamp(), lone=lone, batch=batch)))
