"""Shared by test_sweep_control_cpu.py and test_sweep_control_gpu.py: the emulation's sweep counts on the golden cases."""
import ctypes
import os

import numpy as np

from golden_cases import case_params, case_points

SWEEP_STATS = 22      # F3DS_DBG_SWEEP_STATS: sweeps that were full from their start, incremental, fallback, idle
FALLBACK_CASES = ["rgbd_160x120", "rgbd_320x240_ghosts", "rgbd_320x240_large_supervoxels", "fixture_launch_flags"]


def emul_sweep_stats(handle):
    buf = np.zeros(4, np.uint32); nb = ctypes.c_size_t()
    assert handle.chk.fn("get")(handle.h, SWEEP_STATS, ctypes.c_void_p(buf.ctypes.data), ctypes.c_size_t(16), ctypes.byref(nb)) == 0 and nb.value == 16
    return tuple(int(x) for x in buf)


_runs = {}


def emul_run(P, emul, name, inc_shift=None):
    """(rc, sweeps, stats) of the emulation on a golden case with F3DS_EMUL_INC_SHIFT = inc_shift (None: unset), run once per session."""
    key = (name, inc_shift)
    if key not in _runs:
        old = os.environ.pop("F3DS_EMUL_INC_SHIFT", None)
        try:
            if inc_shift is not None:
                os.environ["F3DS_EMUL_INC_SHIFT"] = inc_shift
            rc, labels, res, h = emul.segment(case_points(P, name), case_params(P, name))
        finally:
            os.environ.pop("F3DS_EMUL_INC_SHIFT", None)
            if old is not None:
                os.environ["F3DS_EMUL_INC_SHIFT"] = old
        _runs[key] = (rc, int(res.sweeps), emul_sweep_stats(h) if rc == 0 else None)
    return _runs[key]
