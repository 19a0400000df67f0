"""Sweep control without a GPU.  The five words that steer a label-propagation sweep are decided by a_sweep_begin (csrc/f3ds_algo.h),
the one definition that d_sweep_begin and the CPU emulation of the sweeps (tests/emul) both call: its decision table is written out
here from the rule, and the emulation -- which now takes the device's paths: idle sweeps, the thief-mask pre-pass and a_eval_R_mask in
full sweeps (cross-checked against a_eval_R inside the emulation, an error on any difference), a_eval_R on every voxel in sweeps whose
R rounds did not converge -- is checked to have taken them on the golden cases."""
import ctypes
import json
import os

import pytest

from conftest import ALL_DEBUG, ROOT, sha_of
from golden_cases import GOLDEN_CASES, case_params, case_points
from sweep_control_common import FALLBACK_CASES, emul_run, emul_sweep_stats

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")))


def begin(emul, words, t, n_ghosts, thr):
    w = (ctypes.c_uint32 * 5)(*words)
    f = emul.fn("sweep_begin"); f.restype = ctypes.c_int
    runs = f(w, ctypes.c_uint32(t), ctypes.c_uint32(n_ghosts), ctypes.c_uint32(thr))
    return runs, list(w)


# (n_changed, sweep_full, sweep_pre, sweep_marks, sweep_idle) before, t, ghosts, thr  ->  returns, the five words after.  A word holds t + 1 while its
# statement is true of sweep t.  The rule: t == 0 resets marks and idle; a sweep t >= 2 after one that changed nothing, with no ghost leaf, is idle and nothing
# else is decided; full (and full from its start) with a ghost leaf, at t == 0, when the previous sweep changed more than thr voxels or was not marking; marking
# at t >= 1 when the previous sweep changed at most 4 thr (always from thr = 2^30 on, where 4 thr no longer fits a word); n_changed restarts at 0.
TABLE = [
    # t = 0: full whatever the words left by an earlier run say, no marking yet, stale marks / idle reset
    ((777, 5, 5, 9, 9), 0, 0, 100, 1, [0, 1, 1, 0, 0]),
    ((0, 0, 0, 0, 0), 0, 0, 0xFFFFFFFF, 1, [0, 1, 1, 0, 0]),
    ((0, 17, 17, 17, 17), 0, 3, 100, 1, [0, 1, 1, 0, 0]),
    # t = 1: full (sweep 0 was not marking), starts marking when sweep 0 changed little enough; never idle
    ((50, 1, 1, 0, 0), 1, 0, 100, 1, [0, 2, 2, 2, 0]),
    ((0, 1, 1, 0, 0), 1, 0, 100, 1, [0, 2, 2, 2, 0]),
    ((401, 1, 1, 0, 0), 1, 0, 100, 1, [0, 2, 2, 0, 0]),
    # t >= 2, the sweep before changed nothing, no ghost leaf: idle, the other words stay
    ((0, 2, 2, 2, 0), 2, 0, 100, 0, [0, 2, 2, 2, 3]),
    ((0, 2, 2, 0, 0), 7, 0, 0, 0, [0, 2, 2, 0, 8]),
    # ... the same with a ghost leaf: full, not idle
    ((0, 2, 2, 2, 0), 2, 1, 100, 1, [0, 3, 3, 3, 0]),
    # the sweep before was marking: incremental up to prev == thr, full above
    ((100, 2, 2, 2, 0), 2, 0, 100, 1, [0, 2, 2, 3, 0]),
    ((101, 2, 2, 2, 0), 2, 0, 100, 1, [0, 3, 3, 3, 0]),
    ((1, 2, 2, 2, 0), 2, 0, 0, 1, [0, 3, 3, 2, 0]),
    # the sweep before was not marking (sweep_marks != t): full however little it changed
    ((50, 3, 3, 2, 0), 3, 0, 100, 1, [0, 4, 4, 4, 0]),
    ((50, 2, 2, 0, 0), 2, 0, 100, 1, [0, 3, 3, 3, 0]),
    # marking: prev <= 4 thr against prev > 4 thr
    ((400, 2, 2, 2, 0), 2, 0, 100, 1, [0, 3, 3, 3, 0]),
    ((401, 2, 2, 2, 0), 2, 0, 100, 1, [0, 3, 3, 2, 0]),
    # thr from 2^30 on: always marking; thr = 2^32 - 1 (shift 32): no count is above it
    ((0xFFFFFFF0, 2, 2, 2, 0), 2, 0, 0x40000000, 1, [0, 3, 3, 3, 0]),
    ((5000, 2, 2, 2, 0), 2, 0, 0xFFFFFFFF, 1, [0, 2, 2, 3, 0]),
    ((0xFFFFFFFF, 5, 5, 5, 0), 5, 0, 0xFFFFFFFF, 1, [0, 5, 5, 6, 0]),
]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_begin_decision_table(emul, row):
    words, t, ghosts, thr, runs, after = TABLE[row]
    assert begin(emul, words, t, ghosts, thr) == (runs, after)


def test_threshold_from_the_shift(emul):
    f = emul.fn("sweep_thr"); f.restype = ctypes.c_uint32
    thr = lambda V, shift: f(ctypes.c_uint32(V), ctypes.c_int(shift))
    assert thr(76859, -1) == 0 and thr(76859, -7) == 0
    assert thr(76859, 6) == 1200 and thr(63, 6) == 0 and thr(64, 6) == 1
    assert thr(76859, 0) == 76859 and thr(0xFFFFFFFF, 31) == 1
    assert thr(76859, 32) == 0xFFFFFFFF and thr(0, 32) == 0xFFFFFFFF and thr(76859, 40) == 0xFFFFFFFF


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_emulation_counts_every_sweep_and_runs_the_mask_walker(P, emul, name):
    rc, sweeps, (full, incremental, fallback, idle) = emul_run(P, emul, name)
    assert rc == 0 and full + incremental + fallback + idle == sweeps
    assert full >= 1      # sweep 0 at the least: the thief-mask pre-pass and a_eval_R_mask ran (and agreed with a_eval_R, else rc != 0)


def test_emulation_skips_the_sweeps_behind_a_fixed_point(P, emul):
    rc, sweeps, stats = emul_run(P, emul, "rgbd_320x240_large_supervoxels")
    assert rc == 0 and sweeps == 56 and stats[3] > 0, stats


@pytest.mark.parametrize("name", FALLBACK_CASES)
def test_emulation_fallback_of_rounds_that_do_not_converge(P, emul, monkeypatch, name):
    """One R round, every sweep from the third on incremental: any word the round changes turns the sweep full, and a_eval_R derives R for
    every voxel as d_sweep_R's fallback does.  The arrays are still the oracle's (tests/golden/oracle_golden.json)."""
    monkeypatch.setenv("F3DS_EMUL_R_ROUNDS", "1")
    monkeypatch.setenv("F3DS_EMUL_INC_SHIFT", "32")
    rc, labels, res, h = emul.segment(case_points(P, name), case_params(P, name))
    assert rc == 0
    stats = emul_sweep_stats(h)
    assert sum(stats) == res.sweeps and stats[2] > 0, stats
    g = GOLD[name]
    for w in ALL_DEBUG:
        assert sha_of(h.get(w)) == g["sha256"][w], w
    assert sha_of(labels) == g["labels_sha256"]
