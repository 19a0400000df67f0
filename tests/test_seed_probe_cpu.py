"""The seed-stage entry points of the kernel probe (kp_seed_grow, kp_seed_nn, kp_seed_filter) without a GPU: the hand-built tables of tests/kernprobe_inputs.py reach the
edge classes they are named for (the census of seed_clouds_common.py says so), the references agree with a second formulation -- the growth loop point by point, and the
search over the 27 cells around a cell against the search over all voxels --, the probe holds the three entry points and the kernels behind them, and bad arguments are
refused before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

import kernprobe_inputs as K
import seed_clouds_common as S
from test_kernprobe_cpu import EARG, PROBE_DIR, cases_of, kp_built  # noqa: F401  (kp_built: fixture)

VP = ctypes.c_void_p
C32 = ctypes.c_uint32
U32 = np.uint32
F = np.float32
NE = K.MAX_SEED_EVENTS


def _p(a):
    return VP(a.ctypes.data) if a is not None else VP(0)


class SeedProbe:
    """ctypes wrapper of the three seed entry points of libf3ds_kernprobe.so: every method returns (return code, outputs...)"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for nm in ("seed_grow", "seed_nn", "seed_filter"):
            getattr(self.lib, "kp_" + nm).restype = ctypes.c_int

    def seed_grow(self, vf, seed_res, V=None):
        vf = None if vf is None else np.ascontiguousarray(vf, F)
        ints = np.zeros(7 + 5 * NE, np.int32); dbls = np.zeros(7 + 3 * NE, np.float64); dc = np.zeros(2, np.int32)
        rc = self.lib.kp_seed_grow(_p(vf), C32(len(vf) if V is None else V), ctypes.c_float(seed_res), _p(ints), _p(dbls), _p(dc))
        return rc, ints, dbls, dc

    def _tables(self, t, **over):
        a = dict(vf=t.vf, V=t.V, ckey=t.ckey, sorted_vox=t.sorted_vox, n=len(t.sorted_vox), cell_start=t.cell_start, C=t.C, grid=t.grid)
        a.update(over)
        return [_p(a["vf"]), C32(a["V"]), _p(a["ckey"]), _p(a["sorted_vox"]), C32(a["n"]), _p(a["cell_start"]), C32(a["C"]), _p(a["grid"])]

    def seed_nn(self, t, extra=0, **over):
        out = np.full(t.C + 4 * extra, -2, np.int32)
        return self.lib.kp_seed_nn(*self._tables(t, **over), C32(extra), _p(out)), out

    def seed_filter(self, t, seed_orig, extra=0, r2=None, min_points=None, **over):
        out = np.full(t.C + 4 * extra, 7, U32)
        so = np.ascontiguousarray(seed_orig, np.int32)
        rc = self.lib.kp_seed_filter(*self._tables(t, **over), C32(extra), _p(so), ctypes.c_float(t.r2 if r2 is None else r2),
                                     ctypes.c_float(t.min_points if min_points is None else min_points), _p(out))
        return rc, out


@pytest.fixture(scope="session")
def sp_nogpu(kp_built):  # noqa: F811
    return SeedProbe(os.path.join(kp_built, "libf3ds_kernprobe.so"))


def test_probe_holds_the_seed_entry_points(kp_built):  # noqa: F811
    blob = open(os.path.join(kp_built, "libf3ds_kernprobe.so"), "rb").read()
    for sym in ("kp_seed_grow", "kp_seed_nn", "kp_seed_filter", "d_chunkbox", "d_seed_grow", "d_cell_hash", "d_seed_nn", "d_seed_filter"):
        assert sym.encode() in blob, sym
    src = open(os.path.join(kp_built, "kernprobe.hip")).read()
    for launch in ("dim3((C + 3u) / 4u + extra, 1), dim3(d_seed_nn::BLOCK)", "dim3((C + 3u) / 4u + extra, 1), dim3(d_seed_filter::BLOCK)", "dim3(1, 1), dim3(d_seed_grow::BLOCK)",
                   "dim3(nchunks, 1), dim3(d_chunkbox::BLOCK)"):
        assert launch in src, launch


def _census_run(c, xyz, seed_res, voxel_res, ref=None):
    prm = type("Prm", (), dict(leaf_order=0, seed_res=seed_res, voxel_res=voxel_res))()
    case = S.Case(c.name, "probe", None, {}, c.cond)
    return S.Run(case, None, prm, None, None, None, S.census(xyz, seed_res, voxel_res, ref), 0.0)


@pytest.mark.parametrize("prim", ["seed_grow", "seed_nn", "seed_filter"])
def test_tables_reach_the_classes_they_are_named_for(prim):
    """The condition of the cloud case a table was taken from holds on the table itself (the census is taken from the table's voxels, in the table's order)."""
    seen = 0
    for c in cases_of(prim):
        if c.cond is None or c.cond[0] in ("all_dropped", "lower_events", "second_trip"):
            continue
        if prim == "seed_grow":
            S.check_condition(_census_run(c, c.xyz, c.seed_res, S.RD))
        else:
            t = c.table
            S.check_condition(_census_run(c, t.xyz, t.seed_res, t.voxel_res, t.ref))
            assert t.cell_start[0] == 0 and t.cell_start[-1] == t.V and (np.diff(t.cell_start.astype(np.int64)) > 0).all()
            assert (t.ref.cell_of[t.sorted_vox][t.cell_start[:-1]] == np.arange(t.C)).all()
        seen += 1
    assert seen >= 7


def test_growth_references_agree():
    for c in cases_of("seed_grow"):
        g = K.ref_seed_grow(c)
        mn, depth, keys, ev = K.slow_seed_grow(c)
        assert g.depth == depth and [(e.trigger, e.depth) for e in g.events] == ev, c.name
        assert np.array_equal(g.min, np.array(mn)) and np.array_equal(g.keys, keys), c.name
        assert len(ev) <= NE and (g.keys >= 0).all() and (g.keys < (1 << depth)).all(), c.name


def test_nearest_voxel_and_filter_references_agree():
    """The search over all voxels and the search over the 27 cells around a cell give the same seeds and the same verdicts: the restriction is sound on these tables."""
    for c in cases_of("seed_nn") + cases_of("seed_filter"):
        t = c.table
        assert np.array_equal(K.ref_seed_nn(t), K.slow_seed_nn(t)), c.name
        assert np.array_equal(K.ref_seed_filter(t), K.slow_seed_filter(t, t.ref.seed_orig)), c.name


def test_seed_entry_points_refuse_bad_arguments_without_a_gpu(sp_nogpu):
    sp = sp_nogpu
    t = cases_of("seed_nn")[0].table
    vf = t.vf
    bad = vf.copy(); bad[1, 2] = np.nan
    for rc in (sp.seed_grow(None, 0.1, V=4)[0], sp.seed_grow(vf, 0.0)[0], sp.seed_grow(vf, -1.0)[0], sp.seed_grow(vf, float("nan"))[0], sp.seed_grow(vf, 0.1, V=0)[0],
               sp.seed_grow(vf, 0.1, V=(1 << 22) + 1)[0], sp.seed_grow(bad, 0.1)[0]):
        assert rc == EARG
    cs = t.cell_start.copy(); cs[1] = cs[0]                       # an empty cell
    cs2 = t.cell_start.copy(); cs2[-1] += 1                       # the last cell ends behind the list
    sv = t.sorted_vox.copy(); sv[0] = t.V                         # a voxel that does not exist
    ck = t.ckey.copy(); ck[t.sorted_vox[0], 0] = (1 << 21) - 1    # a key whose neighbour does not pack
    ck2 = t.ckey.copy(); ck2[:] = ck2[0]                          # every cell the same key
    g0 = t.grid.copy(); g0[0] = 0.0
    g1 = t.grid.copy(); g1[2] = np.inf
    for over in (dict(vf=None), dict(ckey=None), dict(sorted_vox=None), dict(cell_start=None), dict(grid=None), dict(V=0), dict(n=0), dict(n=t.V + 1), dict(C=0), dict(C=t.V + 1),
                 dict(cell_start=cs), dict(cell_start=cs2), dict(sorted_vox=sv), dict(ckey=ck), dict(ckey=ck2), dict(grid=g0), dict(grid=g1)):
        assert sp.seed_nn(t, **over)[0] == EARG, over
        assert sp.seed_filter(t, t.ref.seed_orig, **over)[0] == EARG, over
    assert sp.seed_nn(t, extra=65)[0] == EARG and sp.seed_filter(t, t.ref.seed_orig, extra=65)[0] == EARG
    so = t.ref.seed_orig.copy(); so[0] = t.V
    so2 = t.ref.seed_orig.copy(); so2[-1] = -1
    assert sp.seed_filter(t, so)[0] == EARG and sp.seed_filter(t, so2)[0] == EARG
    assert sp.seed_filter(t, t.ref.seed_orig, r2=float("nan"))[0] == EARG and sp.seed_filter(t, t.ref.seed_orig, min_points=float("inf"))[0] == EARG
