"""refineSupervoxels on the lattice clouds of vccs_clouds_common.py: the case list, and a census of what every reseed of the oracle's refine run meets.

Plain numpy, no GPU.  reseed_census() reads the oracle's arrays alone (VOXEL_XYZ and the centroids / labels oracle.refine(k - 1) returns) and restates a_sqdist's three
rounded adds in float32: how many helpers have their least distance at more than one voxel (d_reseed's tie rule decides their seed), how many of those ties are decided by
the `ob < mb` clause of d_reseed's LDS reduction and not by a thread's scan order, how many helpers reseed onto a voxel another helper reseeds onto (the reseed makes a ghost
leaf), how many helpers are empty when the reseed starts.  The one fact the oracle cannot give -- helpers with ghost_active set when an iteration starts -- comes from the
emulation (f3ds_emul_refine_ghosts).  tests/test_refine_clouds_cpu.py asserts the conditions the case list has to meet, that the emulation's refine equals the oracle's
on every case, and that the table below is what the census gives; tests/test_refine_clouds_gpu.py runs the cases through the HIP kernels.

The census (census_line() of every case; test_refine_clouds_cpu.py keeps these lines and the census itself equal).  Per case and iteration k: ties [of them cross-thread, decided
by the reduction's tie clause, with two tied voxels in one thread] / collisions / helpers erased on entry (S0 minus the live ones) / ghosts alive on entry (of them with
a higher label than the owner of the voxel they hold).  A frame
without sweeps never ran updateCentroid: every centroid is still the zero it started as, and every helper reseeds onto the voxel nearest the origin.
  r-tiny-supervoxels-desc        V  1601, S0   401,   2 sweeps:  k=1 314[3,291,0]/0/1/0(0)   k=2 11[1,6,0]/0/202/0(0)   k=3 34[0,22,0]/0/204/0(0)
  r-helpers-of-64-and-65-leaves  V   678, S0    55,  13 sweeps:  k=1 40[0,40,0]/0/7/0(0)   k=2 40[0,40,0]/0/7/0(0)   k=3 40[0,40,0]/0/7/0(0)
  d-deep-chain-cold              V  1450, S0  1064,   2 sweeps:  k=1 6[0,2,0]/1/761/2(2)   k=2 5[0,1,0]/0/830/0(0)   k=3 5[0,1,0]/0/849/0(0)
  d-deep-chain-desc              V  1450, S0  1034,   2 sweeps:  k=1 5[0,2,0]/0/755/0(0)   k=2 1[0,1,0]/0/800/0(0)   k=3 4[0,2,0]/0/817/0(0)
  r-every-voxel-a-seed-12287     V 12287, S0 12287,   0 sweeps:  k=1 0[0,0,0]/12286/0/0(0)
  r-every-voxel-a-seed-12288     V 12288, S0 12288,   0 sweeps:  k=1 0[0,0,0]/12287/0/0(0)   k=2 0[0,0,0]/12287/0/12287(0)
  r-every-voxel-a-seed-12289     V 12289, S0 12289,   0 sweeps:  k=1 0[0,0,0]/12288/0/0(0)
  w-corridor-ratio40             V   256, S0     1,  71 sweeps:  k=1 0[0,0,0]/0/0/0(0)   k=2 0[0,0,0]/0/0/0(0)   k=3 0[0,0,0]/0/0/0(0)
  w-corridor-ratio72             V   342, S0     1, 128 sweeps:  k=1 0[0,0,0]/0/0/0(0)   k=2 0[0,0,0]/0/0/0(0)   k=3 0[0,0,0]/0/0/0(0)
  n-ring1-456-over               V  4914, S0    64,   8 sweeps:  k=1 0[0,0,0]/0/0/0(0)   k=2 0[0,0,0]/0/3/0(0)   k=3 0[0,0,0]/0/3/0(0)
  n-ring2-901-over               V  4105, S0    48,   8 sweeps:  k=1 0[0,0,0]/0/0/0(0)   k=2 0[0,0,0]/0/0/0(0)   k=3 0[0,0,0]/0/0/0(0)
  r-tile-lists-of-15-and-17      V  3456, S0    72,   7 sweeps:  k=1 0[0,0,0]/0/0/0(0)   k=2 1[0,0,0]/0/4/0(0)   k=3 0[0,0,0]/0/5/0(0)
  t-plane24                      V   577, S0     9,  13 sweeps:  k=1 1[0,0,0]/0/0/0(0)   k=2 1[0,1,0]/0/0/0(0)   k=3 0[0,0,0]/0/0/0(0)
  v-transform                    V  1502, S0    28,   8 sweeps:  k=1 0[0,0,0]/0/0/0(0)   k=2 0[0,0,0]/0/0/0(0)   k=3 0[0,0,0]/0/0/0(0)
  s-chunk-straddle               V    65, S0    11,   8 sweeps:  k=1 0[0,0,0]/0/4/0(0)   k=2 0[0,0,0]/0/4/0(0)   k=3 0[0,0,0]/0/4/0(0)
  n-line-V127                    V   127, S0    26,   8 sweeps:  k=1 1[0,1,0]/0/1/0(0)   k=2 1[0,1,0]/0/1/0(0)   k=3 1[0,1,0]/0/1/0(0)
  s-voxel-of-256-points          V   145, S0     9,   8 sweeps:  k=1 1[0,1,0]/0/0/0(0)   k=2 0[0,0,0]/0/0/0(0)   k=3 0[0,0,0]/0/0/0(0)
  g-seed-ghosts-one-sweep        V  1450, S0  1203,   1 sweeps:  k=1 22[2,8,0]/1/833/11(11)   k=2 6[0,1,0]/0/944/0(0)   k=3 7[0,1,0]/0/960/0(0)
  g-seed-ghosts-no-sweep         V  2041, S0  1948,   0 sweeps:  k=1 0[0,0,0]/1947/0/8(0)   k=2 0[0,0,0]/1947/0/1947(0)   k=3 0[0,0,0]/1947/0/1947(0)
  g-seed-ghosts-two-sweeps       V  2030, S0  1679,   2 sweeps:  k=1 11[0,7,0]/13/210/13(0)   k=2 11[0,6,0]/13/220/13(0)   k=3 11[0,7,0]/13/224/13(0)
  r-holes-same-thread-tie        V  2843, S0   784,   2 sweeps:  k=1 253[44,153,1]/0/164/0(0)   k=2 37[3,19,0]/0/370/0(0)   k=3 31[2,18,0]/0/398/0(0)
"""
import collections
import ctypes

import numpy as np

import vccs_clouds_common as C
from conftest import first_mismatch, same_bits

RESEED_BLOCK = 256      # d_reseed::BLOCK: thread t scans the voxels t, t + 256, ...; the reduction halves 256 threads down to one
REFINE_KEYS = ("voxel_label", "label", "n_voxels", "voxel_normal", "xyz", "rgb", "normal")      # the seven arrays of a refine call


# ------------------------------------------------------------------------------------------------ the cases
RCase = collections.namedtuple("RCase", "name ks build params why")
# ks: the iteration counts the case is refined with (the oracle's reseed is O(S0 V): the every-voxel cases stop at 2 or at 1);  build / params: None for a case of
# vccs_clouds_common.CASES, else as there;  why: what the case is in the list for
CASES = []
K_ALL = (1, 2, 3)


def rcase(name, why, ks=K_ALL, build=None, **params):
    if build is None:
        assert name in C.CASE and not params, name
        CASES.append(RCase(name, ks, None, None, why))
    else:
        assert name not in C.CASE, name
        p = dict(voxel_res=C.R, seed_res=5 * C.R, use_transform=0)
        p.update(params)
        CASES.append(RCase(name, ks, build, p, why))


rcase("r-tiny-supervoxels-desc", "hundreds of exact ties in one reseed, some decided across threads; half of the helpers erased from iteration 2 on")
rcase("r-helpers-of-64-and-65-leaves", "40 ties in every reseed")
rcase("d-deep-chain-cold", "a reseed collision followed by two sweeps: a reseed-made ghost leaf in d_sweep_begin's chains and a_claim's ghost paths; a quarter of the helpers erased")
rcase("d-deep-chain-desc", "ties and erased helpers under the transform, descending leaves")
for _s in (12287, 12288, 12289):
    rcase("r-every-voxel-a-seed-%d" % _s, "every helper but one reseeds onto ONE voxel, no sweep: d_reseed_own's atomicMax winner, tcnt = 0 of ghosts, supervoxels_of over ghost-only helpers",
          ks=(1, 2) if _s == 12288 else (1,))      # (a reseed is 150 M distances, in the oracle, in the emulation and in the census: a second iteration for one of the three)
rcase("w-corridor-ratio40", "71 sweeps per iteration: each iteration restarts at t = 0 and goes past the memo-tag wrap")
rcase("w-corridor-ratio72", "128 sweeps per iteration: past the wrap twice")
rcase("n-ring1-456-over", "a tile whose one-ring overflowed d_normals_t's table: the refine sweeps gather globally there")
rcase("n-ring2-901-over", "... whose two-ring did")
rcase("r-tile-lists-of-15-and-17", "tile lists on both sides of the row path, V = 48 S0")
rcase("t-plane24", "exact ties between helpers in the sweeps after a reseed")
rcase("v-transform", "the single-camera transform")
rcase("s-chunk-straddle", "V = 65 < 256: most threads of d_reseed see no voxel")
rcase("n-line-V127", "V = 127 < 256")
rcase("s-voxel-of-256-points", "V = 145 < 256")
# Ghost leaves of the SEED stage still active when refine starts.  Two seed cells resolve to one voxel where a cell's own voxels lie further from its centre than a
# neighbouring cell's: on the noisy sheets of the deep-chain cases that happens a dozen times once a seed cell is no larger than two voxels, and the frame then has at most two
# sweeps, too few for every lower helper to win its seed voxel (d-deep-chain-cold keeps 2 of its 24 ghosts).  A scan of three such sheets at seed_res / voxel_res = 1, 1.2,
# 1.5, 2, 2.3, with and without the transform, in both leaf orders, gave the three kinds below; no lattice cloud of vccs_clouds_common.CASES has a ghost when its sweeps end.
def _sheet(seed):
    def build():
        from conftest import pkg
        return pkg().synth_frame(0, seed, 60, 40, 0)      # (as vccs_clouds_common._noisy_sheet: a 60 x 40 RGB-D frame without holes)
    return build


rcase("g-seed-ghosts-one-sweep", "11 seed-stage ghosts alive when refine starts, each with a HIGHER label than its voxel's owner (a third helper claimed the voxel): d_refine_ghost_L "
      "changes L and d_refine_normals computes the voxel's normal for a helper that does not own it; one sweep per iteration", build=_sheet(300328), voxel_res=0.03, seed_res=0.045, use_transform=1)
rcase("g-seed-ghosts-no-sweep", "8 seed-stage ghosts alive when refine starts, all below their voxel's owner; no sweep: a mass collision as in the every-voxel cases, on a noisy sheet, for three iterations",
      build=_sheet(300328), voxel_res=0.03, seed_res=0.03)
rcase("g-seed-ghosts-two-sweeps", "13 helpers whose only leaf is a voxel a higher helper owns: they reseed onto it again in every iteration, and two sweeps carry the ghost leaves",
      build=_sheet(2), voxel_res=0.03, seed_res=0.06)


# Two tied voxels in ONE thread of d_reseed (ordinals a multiple of 256 apart): only there does the ascending scan of a thread decide.  Neighbouring voxels of a full
# plane are 1, 2, 171, 342, ... ordinals apart in Morton order, never a multiple of 256; a tenth of the cells taken out at random shifts the ranks.  Of 48 planes of 40 ..
# 64 cells a side with 0 .. 30 % holes at seed / voxel = 2 and 3, three had such a tie, and in this one the seed it decides changes the refined labels.
def _plane_with_holes():
    cells = C.block(56, 56, 1)
    return C.cloud(cells[np.random.default_rng(2).random(len(cells)) >= 0.1], C.R)


rcase("r-holes-same-thread-tie", "a tie between two voxels 256 m ordinals apart: the scan order of one thread decides the seed", build=_plane_with_holes, seed_res=2 * C.R)

CASE = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
EVERY_VOXEL = [n for n in NAMES if n.startswith("r-every-voxel-a-seed-")]
WRAP_CASES = ["w-corridor-ratio40", "w-corridor-ratio72"]
OVERFLOW_CASES = ["n-ring1-456-over", "n-ring2-901-over"]
GHOST_CASES = ["d-deep-chain-cold", "g-seed-ghosts-one-sweep", "g-seed-ghosts-no-sweep", "g-seed-ghosts-two-sweeps"]      # ghost leaves, seed-made and reseed-made (the every-voxel cases have thousands, but no sweep)


def frame_of(name):
    c = CASE[name]
    if c.build is None:
        return C.frame_of(name)
    if name not in _frames:
        pts = c.build()
        pts.setflags(write=False)
        _frames[name] = pts
    return _frames[name]


def params_of(P, name):
    c = CASE[name]
    return C.params_of(P, name) if c.build is None else P.launch_params(**c.params)


_frames, _runs, _refined, _emul_runs, _emul_refined, _censuses = {}, {}, {}, {}, {}, {}


def oracle_run(oracle, P, name):
    """The oracle's run of a case (a vccs_clouds_common.Run), shared with the vccs_clouds modules where the case is theirs."""
    c = CASE[name]
    if c.build is None:
        return C.oracle_run(oracle, P, name)
    if name not in _runs:
        pts, prm = frame_of(name), params_of(P, name)
        rc, labels, res, h = oracle.segment(pts, prm)
        assert rc == 0, "the oracle refuses case %s: %d" % (name, rc)
        _runs[name] = C.Run(c, pts, prm, labels, res, h, C.census(P, h, res), 0.0)
    return _runs[name]


def oracle_refine(oracle, P, name, k):
    """oracle.refine(k) of a case, made once per process and shared read-only."""
    if (name, k) not in _refined:
        _refined[(name, k)] = oracle_run(oracle, P, name).h.refine(k)
    return _refined[(name, k)]


def emul_run(emul, P, name):
    if CASE[name].build is None:
        return C.emul_run_of(emul, P, name)
    if name not in _emul_runs:
        _emul_runs[name] = C.emul_run(emul, frame_of(name), params_of(P, name))
    return _emul_runs[name]


EmulRefine = collections.namedtuple("EmulRefine", "arrays ghosts above seeds")


def emul_refine(emul, P, name, k):
    """The emulation's refine(k) of a case: the seven arrays, and per iteration the helpers with ghost_active set on entry and the seeds d_reseed gave."""
    if (name, k) not in _emul_refined:
        er = emul_run(emul, P, name)
        assert er.rc == 0
        arrays = er.h.refine(k)
        S0 = int(er.res.n_seeds)
        ghosts, above, seeds = [], [], []
        fg, fs = emul.fn("refine_ghosts"), emul.fn("refine_seeds")
        fg.restype = fs.restype = ctypes.c_int
        for it in range(k):
            ghosts.append(int(fg(er.h.h, ctypes.c_int(it), ctypes.c_int(0))))
            above.append(int(fg(er.h.h, ctypes.c_int(it), ctypes.c_int(1))))
            s = np.full(S0, -2, np.int32)
            assert fs(er.h.h, ctypes.c_int(it), ctypes.c_void_p(s.ctypes.data), ctypes.c_size_t(S0)) == S0
            seeds.append(s)
        assert fg(er.h.h, ctypes.c_int(k), ctypes.c_int(0)) == -1
        _emul_refined[(name, k)] = EmulRefine(arrays, ghosts, above, seeds)
    return _emul_refined[(name, k)]


def ghosts_above_owner_on_entry(emul, P, name, k):
    """... of them, those with a higher label than the owner of the voxel they hold: refineNormals of such a helper writes that voxel's normal last (d_refine_ghost_L)."""
    return emul_refine(emul, P, name, k).above[k - 1]


def ghosts_alive_on_entry(emul, P, name, k):
    """Helpers with ghost_active set when iteration k (1, 2, ...) of the case's refine starts, by the emulation.  k = 1: ghost leaves of the seed stage that the frame's
    own sweeps left active."""
    return emul_refine(emul, P, name, k).ghosts[k - 1]


def refine_mismatch(want, got):
    """None when the seven arrays of two refine calls are the same bits, the first difference otherwise."""
    for key in REFINE_KEYS:
        if want[key].shape != got[key].shape:
            return "%s: shape %s vs %s" % (key, want[key].shape, got[key].shape)
        if not same_bits(want[key], got[key]):
            return first_mismatch(key, want[key], got[key])
    return None


# ------------------------------------------------------------------------------------------------ the census
ReseedCensus = collections.namedtuple("ReseedCensus", "live ties cross_thread_ties reduction_ties same_thread_ties collisions erased seeds")
# ties: helpers whose least distance is attained by more than one voxel, w = their ordinals, ascending.  cross_thread_ties: w[0] has not the least w % 256 among them (the
# lowest ordinal does not sit in the lowest thread).  reduction_ties: the reduction without its `ob < mb` clause would end on another voxel than w[0] -- the ties that
# clause decides; it is neither implied by cross_thread_ties nor implies it, since the reduction's own preference among threads is not the lowest thread (see
# reduction_winner_without_tie_clause).  same_thread_ties: two of w fall to one thread: only there does the ascending scan of a thread decide.


def sqdist32(cen, xyz):
    """a_sqdist of every row of cen against every row of xyz, in float32 with its roundings: r = 0 + d0 d0, r += d1 d1, r += d2 d2 (no fused multiply-add)."""
    cen = np.asarray(cen, np.float32); xyz = np.asarray(xyz, np.float32)
    r = np.zeros((len(cen), len(xyz)), np.float32)
    for a in range(3):
        d = cen[:, a, None] - xyz[None, :, a]
        r = r + d * d
    assert r.dtype == np.float32
    return r


def reseed_census_of(xyz, S0, labels, centroids, block=RESEED_BLOCK):
    """The census of one reseed from the voxel positions and the live helpers' labels (1 .. S0, ascending) and centroids.  seeds: S0 ordinals, the lowest among a helper's
    nearest voxels, -1 for a helper that is not live."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int64); centroids = np.ascontiguousarray(centroids, np.float32).reshape(-1, 3)
    assert len(labels) == len(centroids) and (np.diff(labels) > 0).all() and (len(labels) == 0 or (labels[0] >= 1 and labels[-1] <= S0))
    seeds = np.full(S0, -1, np.int64)
    ties = cross = red = same = 0
    for lo in range(0, len(labels), 64):
        d = sqdist32(centroids[lo:lo + 64], xyz)
        m = d.min(axis=1)
        hit = d == m[:, None]
        seeds[labels[lo:lo + 64] - 1] = hit.argmax(axis=1)      # the first True: the lowest ordinal
        for i in np.nonzero(hit.sum(axis=1) > 1)[0]:
            w = np.nonzero(hit[i])[0]
            ties += 1
            cross += int(w[0] % block != (w % block).min())
            red += int(reduction_winner_without_tie_clause(w, block) != w[0])
            same += int(len(np.unique(w % block)) < len(w))
    live = len(labels)
    return ReseedCensus(live, ties, cross, red, same, live - len(np.unique(seeds[seeds >= 0])), S0 - live, seeds)


def reduction_winner_without_tie_clause(w, block=RESEED_BLOCK):
    """Which of the tied ordinals w (ascending) d_reseed's reduction would end on if it read `od < md` alone.  Every thread brings the lowest of its own; at stride s thread
    t keeps its own against thread t + s's, so the last step (stride 1) prefers the threads with bit 0 clear, the one before those with bit 1 clear, ...: the winner is the
    thread whose number read backwards, bit by bit, is the least -- not the lowest thread, and the lowest ordinal only by accident."""
    bits = block.bit_length() - 1
    assert block == 1 << bits
    first = {}
    for o in w:
        first.setdefault(int(o) % block, int(o))
    return first[min(first, key=lambda t: int(format(t, "0%db" % bits)[::-1], 2))]


def reseed_census(oracle, P, name, k):
    """The census of iteration k's reseed (k = 1, 2, ...) of a case, from the oracle's outputs alone: the helpers and centroids are those of oracle.refine(k - 1)."""
    if (name, k) not in _censuses:
        r = oracle_run(oracle, P, name)
        prev = oracle_refine(oracle, P, name, k - 1)
        _censuses[(name, k)] = reseed_census_of(r.h.get("VOXEL_XYZ"), int(r.res.n_seeds), prev["label"], prev["xyz"])
    return _censuses[(name, k)]


def census_row(oracle, emul, P, name, k):
    c = reseed_census(oracle, P, name, k)
    return (c.ties, c.cross_thread_ties, c.reduction_ties, c.same_thread_ties, c.collisions, c.erased, ghosts_alive_on_entry(emul, P, name, k), ghosts_above_owner_on_entry(emul, P, name, k))


def census_line(oracle, emul, P, name):
    r = oracle_run(oracle, P, name)
    cols = ["k=%d %d[%d,%d,%d]/%d/%d/%d(%d)" % ((k,) + census_row(oracle, emul, P, name, k)) for k in CASE[name].ks]
    return "  %-30s V %5d, S0 %5d, %3d sweeps:  %s" % (name, r.census.V, r.census.S0, r.census.sweeps, "   ".join(cols))

