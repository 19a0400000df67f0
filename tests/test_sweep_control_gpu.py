"""Sweep control on the device against the CPU emulation, which runs the same protocol (a_sweep_begin and its predicates, csrc/f3ds_algo.h):
per golden case and F3DS_INC_SHIFT setting the device's F3DS_DBG_SWEEP_STATS and the emulation's counts name the same sweeps full from their start
and the same sweeps idle.  Incremental and fallback sweeps are compared as their sum: whether the last R round of an incremental sweep still changes a
word depends on how the rounds interleave -- a device round may see a neighbour's newer word, the emulation's rounds are Jacobi, the least favourable
order -- and either way the sweep ends in the same bits."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from sweep_control_common import FALLBACK_CASES, emul_run

ARRAYS = ("VOXEL_SVLABEL", "VOXEL_DIST", "SV_CENTROID")


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [None, "32"], ids=["default", "shift32"])
def test_device_and_emulation_decide_the_same_sweeps(P, emul, shift):
    """(F3DS_INC_SHIFT is read when the library is loaded, hence one fresh child process per setting.)"""
    code = (
        "import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import conftest; from golden_cases import case_points, case_params\n"
        "P = conftest.pkg(); ctx = P.Context(0); out = {}\n"
        "for n in %r:\n"
        "    lab = ctx.segment(case_points(P, n), case_params(P, n))\n"
        "    out[n] = dict(labels=conftest.sha_of(lab), stats=ctx.sweep_stats(), sweeps=int(ctx.result.sweeps), **{w: conftest.sha_of(ctx.debug(w)) for w in %r})\n"
        "print(json.dumps(out))\n") % (ROOT, os.path.join(ROOT, "tests"), FALLBACK_CASES, ARRAYS)
    env = dict(os.environ)
    env.pop("F3DS_INC_SHIFT", None)
    if shift is not None:
        env["F3DS_INC_SHIFT"] = shift
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")))
    for n in FALLBACK_CASES:
        rc, sweeps, (full, incremental, fallback, idle) = emul_run(P, emul, n, shift)
        d_full, d_incremental, d_fallback, d_idle = got[n]["stats"]
        print(n, shift, "device", got[n]["stats"], "emulation", (full, incremental, fallback, idle))
        assert rc == 0 and got[n]["sweeps"] == sweeps == full + incremental + fallback + idle, n
        assert d_full == full, (n, shift, got[n]["stats"])
        assert d_idle == idle, (n, shift, got[n]["stats"])
        assert d_incremental + d_fallback == incremental + fallback, (n, shift, got[n]["stats"])
        assert got[n]["labels"] == gold[n]["labels_sha256"], (n, shift)
        for w in ARRAYS:
            assert got[n][w] == gold[n]["sha256"][w], (n, w, shift)
