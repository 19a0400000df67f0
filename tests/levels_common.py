"""Shared by tests/test_levels_cpu.py and tests/test_levels_gpu.py: the threshold set the hierarchy-level tests take for a merge log,
and the host harness that replays a log through csrc/f3ds_levels.h."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

HARNESS_SRC = os.path.join(ROOT, "tests", "levels_harness", "levels_harness.cpp")


def level_thresholds(weights, T):
    """0, just below the first merge, quantiles of the logged weights, several logged weights exactly, T (all float32, all <= T)."""
    w = np.asarray(weights, np.float32)
    T = np.float32(T)
    ts = [np.float32(0.0)]
    if len(w):
        ts.append(np.nextafter(w[0], np.float32(-np.inf), dtype=np.float32))
        for q in np.quantile(w.astype(np.float64), [0.1, 0.25, 0.5, 0.75, 0.9]):
            ts.append(min(np.float32(q), T))
        for i in sorted({0, len(w) // 3, len(w) // 2, len(w) - 1, int(np.argmin(w)), int(np.argmax(w))}):
            ts.append(w[i])
    ts.append(T)
    return np.array([t for t in ts if t <= T], np.float32)


def build_harness(directory):
    out = os.path.join(str(directory), "liblevels_harness.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, HARNESS_SRC], check=True)
    lib = ctypes.CDLL(out)
    vp = ctypes.c_void_p
    lib.lv_replay.argtypes = [ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
    lib.lv_replay.restype = ctypes.c_int
    return lib


def replay(lib, S0, alive0, merges, thresholds, point_sv):
    """(k, n) labels and (k,) region counts of the log `merges` (n_merges x 3 uint32) at `thresholds`."""
    merges = np.ascontiguousarray(merges, np.uint32).reshape(-1, 3)
    alive0 = np.ascontiguousarray(alive0, np.uint8)
    t = np.ascontiguousarray(thresholds, np.float32)
    psv = np.ascontiguousarray(point_sv, np.uint32)
    labels = np.zeros((len(t), len(psv)), np.uint32)
    nreg = np.zeros(len(t), np.uint32)
    rc = lib.lv_replay(int(S0), alive0.ctypes.data, merges.ctypes.data, len(merges), t.ctypes.data, len(t), len(psv), psv.ctypes.data,
                       labels.ctypes.data, nreg.ctypes.data)
    assert rc == 0, "malformed merge log"
    return labels, nreg


def oracle_frame(handle):
    """(S0, alive0, merge log, supervoxel of every point) of an oracle run (handle of CpuChecker.segment)."""
    log = handle.get("MERGES").reshape(-1, 3)
    svl = handle.get("SV_LABELS")
    S0 = int(max(svl.max(initial=0), log[:, :2].max(initial=0)))
    alive0 = np.zeros(S0 + 1, np.uint8)
    alive0[svl] = 1
    pv = handle.get("POINT_VOXEL")
    vsv = handle.get("VOXEL_SVLABEL")
    point_sv = np.where(pv >= 0, vsv[np.clip(pv, 0, None)] if len(vsv) else 0, 0).astype(np.uint32)
    return S0, alive0, log, point_sv
