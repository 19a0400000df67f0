"""The sweeps from hand-built start states, without a GPU (tests/sweep_states_common.py): the literal restatement of expand_loop equals the emulation of the
device's reformulation on every snapshot of every case, word for word; every case meets the condition it was built for (census from the emulation); the kernel
probe refuses every breach of the start-state contract before it touches a device; the constants the cases are sized by are the kernels'."""
import os

import numpy as np
import pytest

import sweep_states_common as S
from conftest import ROOT, same_bits
from test_kernprobe_cpu import EARG, kp_built, kp_nogpu  # noqa: F401  (fixtures)


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_literal_reference_equals_the_emulation_and_the_case_meets_its_condition(emul, case):
    run = S.Run.of(emul, case)
    diff = S.first_difference(run.emul.snap, run.ref, run.ref["hcount"])
    assert diff is None, S.describe(case.name, diff, who="emulation")
    alive = run.ref["hcount"] > 0
    assert same_bits(run.emul.snap["hc"][alive], run.ref["hc"][alive])
    assert int(run.emul.stats.sum()) == case.n
    if case.cond is not None:
        why = case.cond(run)
        assert why is None, "case '%s' does not reach what it was built for: %s (sweep_stats %s, r_deep %d, cold %d, rounds %s)" % (
            case.name, why, run.emul.stats.tolist(), run.emul.r_deep, run.emul.r_deep_cold, run.emul.rounds.tolist())


def test_every_family_has_a_lead_case_and_no_case_is_large():
    assert {c.family for c in S.CASES} == set("ABCDE")
    assert sorted(c.family for c in S.CASES if c.lead) == list("ABCDE")
    for c in S.CASES:
        big = c.name == "D raw list overflows"          # (a list cannot overflow under HT_CAP * 64 voxels: the one case above 4 200)
        assert (c.state.V <= 4200 or (big and c.state.V < 20000)) and (c.n <= 8 or c.family == "E") and c.n <= 140, c.name


def test_start_states_are_in_the_convention_of_the_kernel_probe_inputs():
    """the books of a State are what d_centroid's reference (kernprobe_inputs.ref_centroid) leaves on them"""
    import kernprobe_inputs as K
    for name in ("A block V=257 S0=2", "C one ghost", "D 16 and 17 list entries"):
        st = S.CASE[name].state
        hs = K.HelperState(st.S0, st.V)
        for k in ("owner", "vf", "ghost_active", "ghost_vox", "hlo", "hhi", "hcount", "tl", "tcnt", "hc"):
            setattr(hs, k, getattr(st, k).copy())
        new = K.ref_centroid(hs)
        assert np.array_equal(new.hcount, st.hcount) and np.array_equal(new.tcnt, st.tcnt), name
        for h in range(1, st.S0 + 1):
            assert np.array_equal(new.tl[h, :st.tcnt[h]], st.tl[h, :st.tcnt[h]]), (name, h)


def test_probe_refuses_every_breach_of_the_start_state_contract(kp_nogpu):
    good = S.violations()[0][1].copy()
    good.owner[5] = 1
    # (a state inside the contract passes the checks and goes on to the device: not tried here.  Each breach differs from it in one respect)
    for what, st in S.violations():
        rc = kp_nogpu.sweeps(st, 2)[0]
        assert rc == EARG, "%s: kp_sweeps returned %d" % (what, rc)
    for bad in S.BAD_CONTROLS:
        kw = dict(n=2); kw.update(bad)
        rc = kp_nogpu.sweeps(good, **kw)[0]
        assert rc == EARG, "%s: kp_sweeps returned %d" % (bad, rc)


def test_python_restates_the_probes_contract():
    """every start state of a case passes a restatement of sweep_state_ok, and every breach fails it: the cases stay inside the contract the kernels are launched under"""
    for c in S.CASES:
        assert contract_breach(c.state) is None, (c.name, contract_breach(c.state))
    for what, st in S.violations():
        if what not in ("seed_res 0", "negative weight"):
            assert contract_breach(st) is not None, what


def contract_breach(st):
    V, S0 = st.V, st.S0
    T = (V + 63) // 64
    nbr = st.nbr
    if ((nbr < -1) | (nbr >= V)).any() or (nbr[:, 13] != np.arange(V)).any():
        return "neighbour table"
    for k in range(27):
        u = nbr[:, k]
        ok = u >= 0
        if (nbr[u[ok], 26 - k] != np.flatnonzero(ok)).any():
            return "neighbour symmetry"
    if not np.isfinite(st.vf[:, :9]).all() or not np.isfinite(st.hc).all():
        return "features"
    if (st.owner > S0).any():
        return "owner"
    un = st.owner == 0
    if (st.dist[un].view(np.uint32) != S.FLT_MAX.view(np.uint32)).any() or not (np.isfinite(st.dist[~un]) & (st.dist[~un] >= 0)).all():
        return "dist"
    for h in range(S0 + 1):
        ga, gv = int(st.ghost_active[h]), int(st.ghost_vox[h])
        if ga > 1 or (not ga and gv != -1) or (ga and (h == 0 or not 0 <= gv < V or st.owner[gv] <= h)):
            return "ghost of %d" % h
        own = np.flatnonzero(st.owner == h) if h else np.zeros(0, np.int64)
        leaves = np.union1d(own, [gv] if ga else []).astype(np.int64)
        if st.hcount[h] != len(leaves):
            return "hcount of %d" % h
        if len(leaves) and not (st.hlo[h] <= leaves.min() and leaves.max() <= st.hhi[h] < V):
            return "window of %d" % h
        if not len(leaves) and (st.hlo[h] or st.hhi[h]):
            return "window of %d" % h
        if st.tcnt[h] > S.HT_CAP + 1:
            return "tcnt of %d" % h
        if st.tcnt[h] <= S.HT_CAP:
            listed = st.tl[h, :st.tcnt[h]]
            if (listed >= T).any() or not np.isin(own >> 6, listed).all():
                return "tile list of %d" % h
    return None


def test_kernel_constants_the_cases_are_sized_by(P):
    need = {"HT_CAP": S.HT_CAP, "R_STACK": S.R_STACK, "R_ROUNDS": S.R_ROUNDS, "NT_TILE": S.NT_TILE, "HT_ROW": S.HT_ROW, "QL": S.QL, "BY_WAVE_RATIO": S.BY_WAVE_RATIO}
    for name, want in need.items():
        assert P.constant(name) == want, (name, P.constant(name), want)
    assert (S.HT_CAP, S.R_STACK, S.R_ROUNDS, S.NT_TILE, S.HT_ROW, S.QL, S.BY_WAVE_RATIO) == (256, 24, 4, 128, 16, 64, 48)
    # the emulation's census names the same limits
    text = open(os.path.join(ROOT, "tests", "emul", "f3ds_emul.cpp")).read()
    assert "EM_HT_CAP = %d, EM_ROW_LIST = %d, EM_ROW_LEAVES = %d, EM_WAVE_RATIO = %d, EM_LIST_TILES = 64;" % (S.HT_CAP, S.HT_ROW, S.QL, S.BY_WAVE_RATIO) in text
