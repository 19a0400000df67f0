#!/usr/bin/env python3
"""Scores of hierarchy levels (f3ds_evaluate_levels) against f3ds_auto_threshold, on the bench workload's frame (seed 1000, 1M points,
-v 0.008 -s 0.08 --AL --CVX), truth = synthetic_truth (the dense path of f3ds_auto_threshold accepts it at every level).  Prints one JSON line:
  lone   the grid (0.0, 0.2, 0.005) = 41 thresholds after a recluster to 0.2: wall time (host clock around the synchronous call, warmed up, median)
         of f3ds_evaluate_levels and of f3ds_auto_threshold on the same frame and grid, alternating the two; f3ds_recluster alone (the baseline
         includes one merge run) and the ratio (auto_threshold - recluster) / evaluate_levels; the six log-free fields of the two agree bit for bit;
         truth labels M and entries per level (min, mean, max over the levels, from the level labels);
  batch  F such frames (seeds 1000 ...), K = 8 and K = 41, one f3ds_evaluate_levels_batch call each: wall time.  With F3DS_DEV=1 F3DS_HOST_PROF=1
         the library prints M / base entries / entries per level (min / mean / max over the frames) on stderr.
usage: tools/time_eval_levels.py [--quick] [--reps R] [--batch F]   (--quick: 8 frames, 3 repeats: the program of the kernel-trace run)"""
import argparse, importlib, json, os, sys, time
import numpy as np
import torch        # (first: libf3ds binds to the HIP runtime torch has mapped)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
P = importlib.import_module("fast-3d-pointcloud-segmentation_amd")
from golden_cases import synthetic_truth

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
if args.quick:
    args.batch, args.reps = 8, 3
W = H = 1000
prm = P.launch_params(voxel_res=0.008, seed_res=0.08)
FIELDS = ("precision", "recall", "fscore", "wov", "fpr", "fnr")


def wall_ms(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


grid = [np.float32(0.0)]
while np.float32(grid[-1] + np.float32(0.005)) <= np.float32(0.2):
    grid.append(np.float32(grid[-1] + np.float32(0.005)))
grid = np.array(grid, np.float32)

ctx = P.Context(0)
pts = P.synth_frame(0, 1000, W, H, 30)
truth = synthetic_truth(pts)
ctx.segment(pts, prm)
top = prm.copy(); top.threshold = float(grid[-1])
t_lv, t_at, t_rc = [], [], []
for rep in range(args.reps + 1):                               # (the first round warms up: scratch grows once)
    ctx.recluster(top)
    ms, (scores, nreg) = wall_ms(lambda: ctx.evaluate_levels(truth, grid))
    ms2, (bt, bp, table, _) = wall_ms(lambda: ctx.auto_threshold(prm, truth, 0.0, 0.2, 0.005))
    ms3, _ = wall_ms(lambda: ctx.recluster(top))
    if rep:
        t_lv.append(ms); t_at.append(ms2); t_rc.append(ms3)
assert [float(t) for t in grid] == list(table), "the two sweeps took different thresholds"
for l, t in enumerate(table):
    for f in FIELDS:
        assert np.float32(getattr(scores[l], f)).tobytes() == np.float32(table[t][f]).tobytes(), (t, f)
    assert abs(scores[l].voi - table[t]["voi"]) <= 1e-5
best = P.best_level(grid, scores)
assert float(grid[best]) == bt
# entries per level, from public outputs: the region of every voxel per level x its truth label (ghost leaves aside)
from eval_levels_common import voxel_truth_labels
ctx.recluster(top)
pv = ctx.debug("POINT_VOXEL")
tl = voxel_truth_labels(pv, ctx.debug("VOXEL_COUNT"), truth, P)
M = int(tl.max()) + 1
labels, _ = ctx.labels_at_thresholds(grid)
ok = pv >= 0
entries = []
for l in range(len(grid)):
    lab = labels[l][ok].astype(np.int64)
    own = lab != 0xFFFFFFFF
    entries.append(len(np.unique(lab[own] * M + tl[pv[ok][own]])))
med = lambda x: float(np.median(x))
lone = dict(levels=len(grid), regions_first_last=[int(nreg[0]), int(nreg[-1])], truth_labels=M, entries_per_level=[min(entries), round(float(np.mean(entries)), 1), max(entries)],
            ms_evaluate_levels=round(med(t_lv), 3), ms_auto_threshold=round(med(t_at), 3), ms_recluster=round(med(t_rc), 3),
            ratio_auto_minus_recluster_over_levels=round((med(t_at) - med(t_rc)) / med(t_lv), 2), best_threshold=float(grid[best]))
ctx.close()

F = args.batch
ctxs = [P.Context(0) for _ in range(F)]
truths = []
for g in range(0, F, 16):
    group = ctxs[g:g + 16]
    frames = [P.synth_frame(0, 1000 + g + i, W, H, 30) for i in range(len(group))]
    truths += [synthetic_truth(f) for f in frames]
    P.segment_batch(group, frames, prm)
batch = dict(frames=F, table_form="global")
for K, ts in ((8, np.linspace(0.0, 0.2, 8).astype(np.float32)), (41, grid)):
    times = []
    for rep in range(args.reps + 1):
        ms, _ = wall_ms(lambda: P.evaluate_levels_batch(ctxs, truths, ts))
        if rep:
            times.append(ms)
    batch["K%d_ms" % K] = round(med(times), 3)
for c in ctxs:
    c.close()
print(json.dumps(dict(tool="time_eval_levels", lib=P.library_stamp(), lone=lone, batch=batch)))
