"""The sweep kernels (d_sweep_begin, d_sweep_R_first / _pre / _round, d_sweep_R, d_sweep_R_tail, d_sweep_claim, d_centroid) from hand-built start states, through the
kernel probe's kp_sweeps, against the literal restatement of expand_loop (tests/sweep_states_common.py): every per-sweep array of every case, word for word, on the
LDS tile path and on the global-gather path; sweep_stats against the emulation's; one case per family also one and three workgroups wide and with one and two R
rounds.  A failure names the case, the first differing sweep, the array, the index and both words in hex.  The hc rows of helpers the reference has erased are not
compared: such a row is stale on the device by design."""
import numpy as np
import pytest

import sweep_states_common as S
from test_kernprobe_cpu import kp_built  # noqa: F401  (fixture)
from test_kernprobe_gpu import kp  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def check(kp, emul, case, tiles, gx_cap=0, r_rounds=None):  # noqa: F811
    run = S.Run.of(emul, case)
    rr = case.r_rounds if r_rounds is None else r_rounds
    em = run.emul if rr == case.r_rounds else S.emul_from(emul, case.state, case.n, case.inc_shift, rr)
    rc, got, stats, tn1 = kp.sweeps(case.state, case.n, inc_shift=case.inc_shift, r_rounds=rr, tiles=tiles, gx_cap=gx_cap)
    what = "tiles=%d gx_cap=%d r_rounds=%d" % (tiles, gx_cap, rr)
    assert rc == 0, "case '%s' (%s): kp_sweeps returned %d" % (case.name, what, rc)
    diff = S.first_difference(got, run.ref, run.ref["hcount"])
    assert diff is None, S.describe(case.name + "' (" + what + ")", diff)
    assert stats.tolist() == em.stats.tolist(), "case '%s' (%s): sweep_stats %s, the emulation's %s" % (case.name, what, stats.tolist(), em.stats.tolist())
    staged = int((tn1 != 0xFFFFFFFF).sum())
    assert staged == (len(tn1) if tiles else 0), "case '%s' (%s): %d of %d tiles on the LDS path" % (case.name, what, staged, len(tn1))      # (no lattice here overflows a one-ring table)


@pytest.mark.parametrize("tiles", (1, 0))
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_device_equals_the_literal_reference(kp, emul, case, tiles):  # noqa: F811
    check(kp, emul, case, tiles)


@pytest.mark.parametrize("gx_cap", (1, 3))
@pytest.mark.parametrize("case", [c for c in S.CASES if c.lead], ids=lambda c: c.name)
def test_narrow_launches(kp, emul, case, gx_cap):  # noqa: F811
    check(kp, emul, case, 1, gx_cap=gx_cap)
    check(kp, emul, case, 0, gx_cap=gx_cap)


@pytest.mark.parametrize("r_rounds", (1, 2))
@pytest.mark.parametrize("case", [c for c in S.CASES if c.lead] + [S.CASE["E 130 default sweeps"]], ids=lambda c: c.name)
def test_fewer_r_rounds(kp, emul, case, r_rounds):  # noqa: F811
    """with fewer rounds recorded a sweep whose last round still changed a word falls back to the chain walker: same bits"""
    check(kp, emul, case, 1, r_rounds=r_rounds)
