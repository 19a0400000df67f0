"""d_chunkbox + d_seed_grow, d_cell_hash + d_seed_nn and d_cell_hash + d_seed_filter through the kernel probe, on the hand-built tables of tests/kernprobe_inputs.py, bit
for bit against the brute-force references of seed_clouds_common.py: the grid (events, depths, key shifts and the cube's corners as doubles), the nearest voxel of every
cell, the filter's verdicts.  The tables are the lattice cases' voxels taken as they are -- no voxelisation, no sort in front of the kernel under test -- and family D's
cell pairs at 600 m and at 0 m go to d_seed_nn directly, a cell per wave.  Each launch is repeated with workgroups beyond what the cells need, as a batched launch has
them: nothing may be written behind the last cell."""
import os

import numpy as np
import pytest

import kernprobe_inputs as K
import seed_clouds_common as S
from test_kernprobe_cpu import PROBE_DIR, cases_of, kp_built  # noqa: F401  (kp_built: fixture)
from test_seed_probe_cpu import NE, SeedProbe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="session")
def sp(kp_built, P):  # noqa: F811
    if P.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    return SeedProbe(os.path.join(PROBE_DIR, "libf3ds_kernprobe.so"))


def test_seed_grow(sp):
    for c in cases_of("seed_grow"):
        rc, ints, dbls, dc = sp.seed_grow(K.vf_rows(c.xyz), c.seed_res)
        assert rc == 0, (c.name, rc)
        g = K.ref_seed_grow(c)
        ev = g.events
        assert (int(ints[0]), int(ints[1]), int(ints[2]), int(ints[3])) == (len(ev), 0, 1, g.depth), (c.name, ints[:4], len(ev), g.depth)
        assert (int(dc[0]), int(dc[1])) == (g.depth, 0), (c.name, dc)
        assert dbls[0] == g.res and dbls[1:4].tobytes() == np.asarray(g.min, np.float64).tobytes(), (c.name, dbls[:4], g.min)
        top = np.asarray(g.min, np.float64) + ((float(1 << g.depth) * g.res - S.FLT_EPS) if len(ev) > 1 else 2.0 * g.res)
        assert np.allclose(dbls[4:7], top, rtol=0, atol=4e-16 * max(1.0, float(np.abs(top).max()))), (c.name, dbls[4:7].tolist(), top.tolist())      # (the first cube's top is min + res / 2 + res + res / 2: an ulp of double)
        assert ints[4:7].tolist() == list(ev[-1].off), (c.name, ints[4:7], ev[-1].off)
        for k, e in enumerate(ev):
            assert ints[7 + 5 * k:12 + 5 * k].tolist() == [e.trigger, e.depth] + list(e.off), (c.name, k, ints[7 + 5 * k:12 + 5 * k], e)
            assert dbls[7 + 3 * k:10 + 3 * k].tobytes() == np.asarray(e.min, np.float64).tobytes(), (c.name, k, dbls[7 + 3 * k:10 + 3 * k], e.min)
        assert not ints[7 + 5 * len(ev):].any() and len(ev) <= NE


@pytest.mark.parametrize("extra", [0, 3])
def test_seed_nn(sp, extra):
    for c in cases_of("seed_nn"):
        t = c.table
        rc, got = sp.seed_nn(t, extra=extra)
        assert rc == 0, (c.name, rc)
        want = K.ref_seed_nn(t)
        bad = np.nonzero(got[:t.C] != want)[0]
        assert len(bad) == 0, "%s: %d of %d cells differ, first cell %d: voxel %d, the nearest is %d" % (c.name, len(bad), t.C, bad[0], got[bad[0]], want[bad[0]])
        assert (got[t.C:] == -1).all(), c.name


@pytest.mark.parametrize("extra", [0, 3])
def test_seed_filter(sp, extra):
    for c in cases_of("seed_filter"):
        t = c.table
        rc, got = sp.seed_filter(t, t.ref.seed_orig, extra=extra)
        assert rc == 0, (c.name, rc)
        want = K.ref_seed_filter(t)
        bad = np.nonzero(got[:t.C] != want)[0]
        assert len(bad) == 0, "%s: %d of %d cells differ, first cell %d: kept %d, %d voxels inside the radius against min_points %r" % (
            c.name, len(bad), t.C, bad[0], got[bad[0]], t.ref.num[bad[0]], t.min_points)
        assert (got[t.C:] == 0xFFFFFFFF).all(), c.name
