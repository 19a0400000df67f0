"""The kernel probe without a GPU (tests/kernprobe/, tests/kernprobe_inputs.py): the wave- and workgroup-level building blocks of
csrc/f3ds_kernels.inc behind thin __global__ wrappers are run by tests/test_kernprobe_gpu.py.  Checked here: the probe is cross-compiled for
gfx950 with the product's flags; every edge class a primitive has to meet is populated by its cases; the plain references agree with a second,
slower formulation on every case; and the host-side precondition checks of the kp_* entry points refuse bad arguments before any HIP call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kernprobe_inputs as K
from conftest import ROOT, _make, same_bits

F = np.float32
U32 = np.uint32
U64 = np.uint64
PROBE_DIR = os.path.join(ROOT, "tests", "kernprobe")
VP = ctypes.c_void_p
C32 = ctypes.c_uint32
EARG = -2


def _p(a):
    return VP(a.ctypes.data)


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


class KernProbe:
    """ctypes wrapper of libf3ds_kernprobe.so: every method returns (return code, outputs...); rc 0 = hipSuccess, EARG = a precondition failed"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for nm in ("const", "wave", "run_of_lane", "block", "scan_single", "scan_u32", "radix_hist", "radix_scatter", "radix_sort", "seg_table", "relabel", "tile_list",
                   "row_leaves", "vblock", "centroid", "sv_fill", "sweeps"):
            getattr(self.lib, "kp_" + nm).restype = ctypes.c_int

    def const(self, i):
        return self.lib.kp_const(ctypes.c_int(i))

    def wave(self, op, rows):
        rows = _c(rows, U32); out = np.zeros_like(rows)
        return self.lib.kp_wave(ctypes.c_int(op), _p(rows), _p(out), ctypes.c_size_t(len(rows))), out

    def run_of_lane(self, rows):
        rows = _c(rows, U32); out = np.zeros_like(rows)
        return self.lib.kp_run_of_lane(_p(rows), _p(out), ctypes.c_size_t(len(rows))), out

    def block(self, two, rows):
        rows = _c(rows, U32); out = np.zeros((len(rows), 1024 if two else 512), U32)
        return self.lib.kp_block(ctypes.c_int(two), _p(rows), _p(out), ctypes.c_size_t(len(rows))), out

    def scan_single(self, data, m, cap=None):
        data = _c(data, U32).copy()
        return self.lib.kp_scan_single(_p(data), C32(m), ctypes.c_size_t(len(data) if cap is None else cap)), data

    def scan_u32(self, data, n, extra=0, cap=None):
        data = _c(data, U32); out = np.zeros_like(data)
        return self.lib.kp_scan_u32(_p(data), _p(out), C32(n), ctypes.c_size_t(len(data) if cap is None else cap), C32(extra)), out

    def radix_hist(self, keys, shift, bits, n_dev=-1, n=None):
        keys = _c(keys, U64); n = len(keys) if n is None else n
        hist = np.zeros((1 << max(0, min(bits, 9))) * K.radix_nb(len(keys)), U32)
        return self.lib.kp_radix_hist(_p(keys), C32(n), ctypes.c_int(shift), ctypes.c_int(bits), ctypes.c_longlong(n_dev), _p(hist)), hist

    def radix_scatter(self, keys, vals, shift, bits, hist_scanned, n_dev=-1):
        keys = _c(keys, U64); hs = _c(hist_scanned, U32)
        ko = np.zeros(len(keys), U64); vo = np.zeros(len(keys), U32)
        v = None if vals is None else _c(vals, U32)
        rc = self.lib.kp_radix_scatter(_p(keys), _p(v) if v is not None else VP(0), C32(len(keys)), ctypes.c_int(shift), ctypes.c_int(bits), ctypes.c_longlong(n_dev), _p(hs),
                                       _p(ko), _p(vo) if v is not None else VP(0))
        return rc, ko, vo

    def radix_sort(self, keys, vals, total, base=0, n_dev=-1):
        keys = _c(keys, U64)
        ko = np.zeros(len(keys), U64); vo = np.zeros(len(keys), U32)
        v = None if vals is None else _c(vals, U32)
        rc = self.lib.kp_radix_sort(_p(keys), _p(v) if v is not None else VP(0), C32(len(keys)), ctypes.c_int(total), ctypes.c_int(base), ctypes.c_longlong(n_dev),
                                    _p(ko), _p(vo) if v is not None else VP(0))
        return rc, ko, vo

    def seg_table(self, chain, keys, limit, shift):
        keys = _c(keys, U64)
        seg = np.zeros(len(keys) + 1, U32); cnt = np.zeros(2, U32)
        return self.lib.kp_seg_table(ctypes.c_int(chain), _p(keys), C32(len(keys)), ctypes.c_uint64(limit), ctypes.c_int(shift), _p(seg), _p(cnt)), seg, cnt

    def relabel(self, c, points):
        L = c.S0 + 1
        parent = _c(c.parent, U32); alive = _c(c.ralive, np.uint8)
        root = np.zeros(L, U32); incl = np.zeros(L, U32); nreg = np.zeros(1, U32)
        if points:
            pv = _c(c.pt_voxel, np.int32); owner = _c(c.owner, U32)
            out = np.zeros(len(pv), U32)
            rc = self.lib.kp_relabel(C32(c.S0), _p(parent), _p(alive), C32(len(pv)), _p(pv) if len(pv) else VP(pv.ctypes.data or 1), _p(owner), C32(c.V), _p(out), _p(root), _p(incl), _p(nreg))
        else:
            out = np.zeros(L, U32)
            rc = self.lib.kp_relabel(C32(c.S0), _p(parent), _p(alive), C32(0), VP(0), VP(0), C32(0), _p(out), _p(root), _p(incl), _p(nreg))
        return rc, out, root, incl, int(nreg[0])

    def tile_list(self, tl, cnt, gv):
        tl = _c(tl, U32); cnt = _c(cnt, U32); gv = _c(gv, np.int32)
        srt = np.zeros((len(cnt), 64), U32); ret = np.zeros(len(cnt), np.int32)
        return self.lib.kp_tile_list(_p(tl), _p(cnt), _p(gv), ctypes.c_size_t(len(cnt)), _p(srt), _p(ret)), srt, ret

    def row_leaves(self, c):
        owner = _c(c.owner, U32); hs = _c(c.hs, U32); tids = _c(c.tids, U32); gvs = _c(c.gvs, np.int32)
        qt = np.zeros((4, 16), U32); ql = np.zeros((4, K.QL + 32), U32); scal = np.zeros((3, 64), U32)
        return self.lib.kp_row_leaves(_p(owner), C32(c.V), _p(hs), _p(tids), _p(gvs), C32(c.cap), _p(qt), _p(ql), _p(scal)), qt, ql, scal

    def vblock(self, gx, nf):
        out = np.zeros((2, gx * nf, 2), U32)
        return self.lib.kp_vblock(C32(gx), C32(nf), _p(out)), out

    def centroid(self, st, n_changed=0xFFFFFFFF, thr=0, marks=0, idle=0):
        """-> rc, the state the kernel left"""
        o = st.copy()
        ctl = np.array([n_changed, thr, marks, idle, st.gx], U32)
        rc = self.lib.kp_centroid(C32(o.S0), C32(o.V), _p(o.owner), _p(o.vf), _p(o.ghost_active), _p(o.ghost_done), _p(o.ghost_vox), _p(o.hlo), _p(o.hhi), _p(o.hcount),
                                  _p(o.tl), _p(o.tcnt), _p(o.hc), _p(ctl))
        return rc, o

    def sv_fill(self, st, loff):
        S0, V = st.S0, st.V
        loff = _c(loff, U32)
        rows = np.zeros((V + S0 + 1, 12), F); rv = np.zeros(V + S0 + 1, np.int32)
        racc, rrec = K.sv_garbage(S0)
        rcnt = np.zeros(S0 + 1, U32); ral = np.zeros(S0 + 1, np.uint8); na = np.zeros(1, U32)
        rc = self.lib.kp_sv_fill(C32(S0), C32(V), _p(st.owner), _p(st.vf), _p(st.ghost_active), _p(st.ghost_vox), _p(st.hlo), _p(st.hhi), _p(st.hcount), _p(loff), _p(st.hc),
                                 _p(st.tl), _p(st.tcnt), _p(rows), _p(rv), _p(racc), _p(rcnt), _p(rrec), _p(ral), _p(na))
        return rc, rows, rv, racc, rcnt, rrec, ral, int(na[0])

    def sweeps(self, st, n, inc_shift=6, r_rounds=4, tiles=1, gx_cap=0):
        """kp_sweeps on a start-of-run state (tests/sweep_states_common.py: State) -> rc, dict of the per-sweep arrays, sweep_stats[4], tile_n1"""
        V, L = st.V, st.S0 + 1
        ins = [_c(st.nbr, np.int32), _c(st.vf, F), _c(st.owner, U32), _c(st.dist, F), _c(st.hc, F), _c(st.hcount, U32), _c(st.hlo, U32), _c(st.hhi, U32), _c(st.tl, U32),
               _c(st.tcnt, U32), _c(st.ghost_vox, np.int32), _c(st.ghost_active, np.uint8)]
        m = max(n, 1)
        out = dict(owner=np.zeros((m, V), U32), dist=np.zeros((m, V), F), hc=np.zeros((m, L, 12), F), hcount=np.zeros((m, L), U32), ghost_active=np.zeros((m, L), np.uint8),
                   ghost_done=np.zeros((m, L), np.uint8), tcnt=np.zeros((m, L), U32), n_changed=np.zeros(m, U32))
        stats = np.zeros(4, U32); tn1 = np.zeros((V + 127) // 128, U32)
        outs = list(out.values()) + [stats, tn1]
        w = np.array([st.seed_res, st.w_normal, st.w_color, st.w_spatial], F)
        ctl = np.array([n, inc_shift + 1, r_rounds, tiles, gx_cap], np.int64).astype(U32)
        rc = self.lib.kp_sweeps(C32(V), C32(st.S0), (VP * 12)(*[a.ctypes.data for a in ins]), _p(w), _p(ctl), (VP * 10)(*[a.ctypes.data for a in outs]))
        return rc, {k: v[:n] for k, v in out.items()}, stats, tn1


class HostRef:
    """libf3ds_kernprobe_host.so: a_centroid_finish, a_payload_row + a_fold_row + n_rgb2lab from g++"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)

    def centroid_finish(self, sums, counts):
        sums = _c(sums, F); counts = _c(counts, U32)
        rows = np.zeros((len(counts), 12), F)
        assert self.lib.kp_host_centroid_finish(_p(sums), _p(counts), ctypes.c_size_t(len(counts)), _p(rows)) == 0
        return rows

    def sv(self, vf, leaves):
        vf = _c(vf, F); lv = _c(leaves, np.int32)
        rows = np.zeros((len(lv), 12), F); acc = np.zeros(12, F); lab = np.zeros(3, F)
        assert self.lib.kp_host_sv(_p(vf), _p(lv), C32(len(lv)), _p(rows), _p(acc), _p(lab)) == 0
        return rows, acc, lab


@pytest.fixture(scope="session")
def kp_built():
    _make("tests/kernprobe")          # (a no-op when both libraries are newer than their sources)
    return PROBE_DIR


@pytest.fixture(scope="session")
def kp_host(kp_built):
    return HostRef(os.path.join(kp_built, "libf3ds_kernprobe_host.so"))


@pytest.fixture(scope="session")
def kp_nogpu(kp_built):
    """the device library, loaded for its host-side checks only"""
    return KernProbe(os.path.join(kp_built, "libf3ds_kernprobe.so"))


CASES = {"scan64": lambda: K.scan_cases(64), "scan256": lambda: K.scan_cases(256), "minsort": K.minsort_cases, "run_of_lane": K.run_cases, "scan_single": K.scan_single_cases,
         "scan_u32": K.scan_u32_cases, "radix_pass": K.radix_pass_cases, "radix_sort": K.radix_sort_cases, "seg_table": K.seg_cases, "relabel": K.relabel_cases,
         "tile_list": K.tile_list_cases, "row_leaves": K.row_leaves_cases, "centroid": K.centroid_states, "sv_fill": K.sv_fill_states,
         "seed_grow": K.seed_grow_cases, "seed_nn": K.seed_nn_cases, "seed_filter": K.seed_filter_cases}
_cache = {}


def cases_of(prim):
    if prim not in _cache:
        _cache[prim] = CASES[prim]()
    return _cache[prim]


# ---- the build ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_probe_is_compiled_with_the_products_flags():
    flags = subprocess.run(["make", "-s", "--no-print-directory", "-C", os.path.join(ROOT, "fast-3d-pointcloud-segmentation_amd", "csrc"), "print-flags"],
                           check=True, capture_output=True, text=True).stdout.split()
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags and len(flags) >= 5
    out = subprocess.run(["make", "-n", "-B", "-C", PROBE_DIR], check=True, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if "kernprobe.hip" in l and "hipcc" in l]
    assert len(lines) == 1, lines
    words = lines[0].split()
    for w in flags:
        assert w in words, "%s is missing from the probe's compile line: %s" % (w, lines[0])
    assert [w for w in words if w.startswith("-ffp-contract")] == ["-ffp-contract=off"]
    assert not [w for w in words if w.startswith("-D")], "the kernels are compiled as the product compiles them: %s" % lines[0]
    for bad in ("-ffast-math", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fgpu-flush-denormals-to-zero", "-funsafe-math-optimizations", "-Ofast"):
        assert bad not in words, bad


def test_kernel_probe_is_cross_compiled_for_gfx950(kp_built):
    so = os.path.join(kp_built, "libf3ds_kernprobe.so")
    assert os.path.exists(so)
    blob = open(so, "rb").read()
    assert b"gfx950" in blob
    for kern in ("kp_wave_k", "kp_run_of_lane_k", "kp_block_incl_k", "kp_block_excl2_k", "kp_tile_list_k", "kp_row_leaves_k", "kp_vblock_k", "kp_call", "d_centroid", "d_sv_fill",
                 "d_radix_scatter_k", "d_scan_single", "d_seg_write", "d_region_ids", "d_relabel"):
        assert kern.encode() in blob, kern
    for sym in ("wave", "run_of_lane", "block", "scan_single", "scan_u32", "radix_hist", "radix_scatter", "radix_sort", "seg_table", "relabel", "tile_list", "row_leaves", "vblock",
                "centroid", "sv_fill"):
        assert ("kp_" + sym).encode() in blob, sym
    # the probe includes the product's kernel file itself, not a copy
    src = open(os.path.join(kp_built, "kernprobe.hip")).read()
    assert '#define KP_KERNELS_INC "f3ds_kernels.inc"' in src and "#include KP_KERNELS_INC" in src


def test_inputs_use_the_kernels_constants(kp_nogpu):
    got = [kp_nogpu.const(i) for i in range(9)]
    assert got[:6] == [K.HT_CAP, K.SCAN_TILE, K.RS_TILE, K.RS_MAXBITS, K.RL_LDS_CAP, K.QL], got
    assert got[7] == EARG and got[8] & 0xFFFFFFFF == K.NO_LABEL


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prim", sorted(K.REQUIRED))
def test_every_edge_class_is_populated(prim):
    cl = K.classes_of(cases_of(prim))
    for need in K.REQUIRED[prim]:
        assert cl.get(need), "%s: no case of edge class '%s'" % (prim, need)
    names = [c.name for c in cases_of(prim)]
    assert len(set(names)) == len(names), "%s: case names repeat" % prim
    if "random" in K.REQUIRED[prim]:
        assert len(cl["random"]) >= 30, (prim, len(cl["random"]))


def test_edge_classes_say_what_they_claim():
    """spot checks of the builders: the class a case carries describes its data"""
    for c in cases_of("tile_list"):
        ref = K.ref_tile_list(c.tl, c.cnt, c.gv)
        if "more than 64 distinct tiles: -1" in c.classes or "the ghost is the 65th distinct tile: -1" in c.classes or "cnt = HT_CAP + 1 gives -1" in c.classes:
            assert ref is None, c.name
        if "64 plus a ghost: multi-round path" in c.classes:
            assert c.cnt == 64 and c.gv >= 0
        if "64 distinct tiles" in c.classes and "ghost tile new" not in c.classes:
            assert ref is not None and len(ref) == 64, c.name
    for c in cases_of("radix_pass"):
        if "one digit receives all 4096 keys of a tile" in c.classes:
            assert K.ref_radix_hist(c).max() == 4096
        if "index in the low bits" in c.classes:
            assert ((c.keys & U64((1 << c.idx) - 1)) == np.arange(len(c.keys), dtype=U64)).all() and c.shift >= c.idx
    for c in cases_of("seg_table"):
        k = c.keys >> U64(c.shift)
        assert (np.diff(k.astype(np.int64)) >= 0).all(), c.name
        seg, (ns, nv) = K.ref_seg_table(c)
        if "segment boundary at a tile boundary" in c.classes:
            assert 2048 in seg[:ns]
        if "segment boundary at a thread's first item" in c.classes:
            assert 8 in seg[:ns] and (len(k) <= 2056 or 2056 in seg[:ns])
        if "segment boundary at n - 1" in c.classes:
            assert seg[ns - 1] == len(k) - 1
        if "no valid key" in c.classes:
            assert ns == 0 and nv == 0
    for c in cases_of("relabel"):
        depth = np.zeros(c.S0 + 1, int); r = np.arange(c.S0 + 1)
        while (c.parent[r] != r).any():
            depth += c.parent[r] != r; r = c.parent[r].astype(np.int64)
        want = {"chains of length 1": 1, "chains of length 2": 2, "chains of about 50": 50}
        for k, d in want.items():
            if k in c.classes and c.S0 > d + 1:
                assert depth.max() == d, (c.name, depth.max())
        assert not (c.ralive.astype(bool)[1:] & (c.parent[1:] != np.arange(1, c.S0 + 1))).any(), "only roots are alive"
    for c in cases_of("centroid"):
        st = c.state
        assert st.V <= 48 * st.S0, c.name          # the row path; the GPU test pads each to the wave path
    for c in cases_of("row_leaves"):
        for r in range(4):
            t = c.tids[16 * r:16 * r + 16]
            assert ((t == K.NONE) | (t.astype(np.int64) * 64 < c.V)).all()


# ---- reference against a second formulation -------------------------------------------------------------------------------------------------
def test_scan_references_agree():
    for w in ("scan64", "scan256"):
        for c in cases_of(w):
            assert np.array_equal(K.ref_incl_scan(c.v), K.slow_incl_scan(c.v)), c.name
            assert np.array_equal(K.ref_excl_scan(c.v), np.r_[0, K.slow_incl_scan(c.v)[:-1]].astype(U32)), c.name
    for c in cases_of("scan_single") + cases_of("scan_u32"):
        assert np.array_equal(K.ref_incl_scan(c.data), K.slow_incl_scan(c.data)), c.name
        if "total wraps" in c.classes:
            assert int(c.data.astype(np.uint64).sum()) >= 1 << 32


def test_min_sort_run_references_agree():
    for c in cases_of("minsort"):
        assert np.array_equal(K.ref_wave_min(c.v), K.slow_min(c.v, 64)), c.name
        assert np.array_equal(K.ref_row_min(c.v), K.slow_min(c.v, 16)), c.name
        assert np.array_equal(K.ref_row_sort(c.v), K.slow_row_sort(c.v)), c.name
        for k in c.classes:
            if k.startswith("minimum at lane"):
                assert int(np.argmin(c.v)) == int(k.split()[-1]) and (c.v == c.v.min()).sum() == 1
    for c in cases_of("run_of_lane"):
        a = K.ref_run_of_lane(c.valid, c.w0, c.w1); b = K.slow_run_of_lane(c.valid, c.w0, c.w1)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), c.name
        if "run ending at lane 63" in c.classes:
            assert a[1][63] + a[2][63] == 64 and a[2][63] >= 1


def test_radix_references_agree():
    for c in cases_of("radix_pass"):
        assert np.array_equal(K.ref_radix_hist(c), K.slow_radix_hist(c)), c.name
        for x, y in zip(K.ref_radix_scatter(c), K.slow_radix_scatter(c)):
            assert np.array_equal(x, y), c.name
    for c in cases_of("radix_sort"):
        if len(c.keys) > 13000:
            continue          # (the loop formulation is quadratic in nothing, just slow: the largest case is left to the first)
        for x, y in zip(K.ref_radix_sort(c), K.slow_radix_sort(c)):
            assert np.array_equal(x, y), c.name


def test_segment_and_relabel_references_agree():
    for c in cases_of("seg_table"):
        a, b = K.ref_seg_table(c), K.slow_seg_table(c)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), c.name
    for c in cases_of("relabel"):
        a, b = K.ref_relabel(c), K.slow_relabel(c)
        for i in (0, 1, 2, 4):
            assert np.array_equal(a[i], b[i]), (c.name, i)
        assert a[3] == b[3], c.name


def test_tile_list_and_row_leaves_references_agree():
    for c in cases_of("tile_list"):
        assert K.ref_tile_list(c.tl, c.cnt, c.gv) == K.slow_tile_list(c.tl, c.cnt, c.gv), c.name
    for c in cases_of("row_leaves"):
        for r, (a, b) in enumerate(zip(K.ref_row_leaves(c), K.slow_row_leaves(c))):
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3], (c.name, r)


def _brute_leaves(st, h):
    """helper h's leaves by a walk over all voxels"""
    gact = bool(st.ghost_active[h]) and not st.ghost_done[h]
    gv = int(st.ghost_vox[h]) if gact else -1
    cnt = int(st.tcnt[h])
    listed = set(st.tl[h, :cnt].tolist()) | ({gv >> 6} if gv >= 0 else set()) if cnt <= K.HT_CAP else None
    if listed is not None and cnt + (gv >= 0) > 64 and len(listed) > 64:
        listed = None
    out = []
    for v in range(st.V):
        t = v >> 6
        inside = t in listed if listed is not None else (int(st.hlo[h]) >> 6) <= t <= (int(st.hhi[h]) >> 6)
        if inside and (st.owner[v] == h or v == gv):
            out.append(v)
    return out


def test_centroid_and_sv_fill_references_agree(kp_host):
    """leaves by a walk over all voxels; the sums element by element; a_centroid_finish, a_payload_row, a_fold_row from the g++ build of the shared header"""
    for c in cases_of("centroid"):
        st = c.state
        new = K.ref_centroid(st)
        hs = range(1, st.S0 + 1) if st.S0 <= 301 else range(1, st.S0 + 1, 7)
        sums, counts, rows = [], [], []
        for h in hs:
            leaves = K.helper_leaves(st, h)[0]
            assert leaves == _brute_leaves(st, h), (c.name, h)
            s, n = K.slow_centroid_sums(st, h)
            assert n == new.hcount[h]
            if n:
                sums.append(s); counts.append(n); rows.append(new.hc[h])
            else:
                assert same_bits(new.hc[h], st.hc[h])
            owned_tiles = sorted(set((np.flatnonzero(st.owner == h) >> 6).tolist()) & set(v >> 6 for v in leaves))
            assert new.tl[h, :new.tcnt[h]].tolist() == owned_tiles, (c.name, h)
        assert same_bits(kp_host.centroid_finish(np.array(sums, F), np.array(counts, U32)), np.array(rows, F)), c.name
    for c in cases_of("sv_fill"):
        st = c.state
        for h in range(1, st.S0 + 1, 1 if st.S0 < 10 else 11):
            leaves = K.helper_leaves(st, h)[0]
            if not leaves:
                continue
            rows, acc, lab = kp_host.sv(st.vf, leaves)
            srows, sacc = K.slow_sv(st.vf, leaves)
            assert same_bits(rows, srows) and same_bits(acc, sacc), (c.name, h)


# ---- the precondition checks -------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu(kp_nogpu):
    """Every refusal comes back as EARG: the check sits in front of the first HIP call (a check that let the call through would come back with a HIP error
    code on a machine without a GPU, and could fault on one with)."""
    kp = kp_nogpu
    z64 = np.zeros((1, 64), U32)
    assert kp.wave(7, z64)[0] == EARG and kp.wave(-1, z64)[0] == EARG and kp.block(2, np.zeros((1, 512), U32))[0] == EARG
    # counts within buffer sizes
    assert kp.scan_single(np.zeros(10, U32), 11)[0] == EARG
    assert kp.scan_u32(np.zeros(10, U32), 11)[0] == EARG and kp.scan_u32(np.zeros(10, U32), 10, extra=1000)[0] == EARG
    keys = np.arange(100, dtype=U64)
    assert kp.radix_hist(keys, 0, 0)[0] == EARG and kp.radix_hist(keys, 0, 10)[0] == EARG and kp.radix_hist(keys, 60, 8)[0] == EARG and kp.radix_hist(keys, -1, 8)[0] == EARG
    c = K.Case("x", "x", keys=keys, vals=np.arange(100, dtype=U32), shift=0, bits=4, n_dev=-1)
    hs = K.ref_excl_scan(K.ref_radix_hist(c))
    bad = hs.copy(); bad[-1] += 1          # the last digit's range would end one behind the output
    assert kp.radix_scatter(keys, c.vals, 0, 4, bad)[0] == EARG
    bad = hs.copy(); bad[3] = 0xFFFFFFF0
    assert kp.radix_scatter(keys, c.vals, 0, 4, bad)[0] == EARG and kp.radix_scatter(keys, None, 0, 4, bad)[0] == EARG
    assert kp.radix_scatter(keys, None, 0, 4, hs, n_dev=50)[0] == EARG          # the keys-only kernel has no device-side count
    assert kp.radix_sort(keys, None, 65)[0] == EARG and kp.radix_sort(keys, None, 40, base=30)[0] == EARG and kp.radix_sort(keys, None, 9, n_dev=5)[0] == EARG
    assert kp.seg_table(2, keys, 5, 0)[0] == EARG and kp.seg_table(0, keys, 5, 64)[0] == EARG
    # relabel: parents inside the table, no cycle, voxels and owners inside theirs, the LDS table's capacity
    rc = next(c for c in cases_of("relabel") if c.S0 == 64 and len(c.pt_voxel) > 10)
    for mut in ("parent", "cycle", "pt_voxel", "pt_voxel_low", "owner", "V"):
        c = K.Case("bad", "bad", **{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rc.__dict__.items() if k not in ("name", "classes")})
        if mut == "parent":
            c.parent[1] = c.S0 + 1
        elif mut == "cycle":
            c.parent[1] = 2; c.parent[2] = 1
        elif mut == "pt_voxel":
            c.pt_voxel[3] = c.V
        elif mut == "pt_voxel_low":
            c.pt_voxel[3] = -2
        elif mut == "owner":
            c.owner[0] = c.S0 + 1
        else:
            c.V = 0
        assert kp.relabel(c, True)[0] == EARG, mut
        if mut in ("parent", "cycle"):
            assert kp.relabel(c, False)[0] == EARG, mut
    big = K.Case("big", "big", S0=K.RL_LDS_CAP, parent=np.arange(K.RL_LDS_CAP + 1, dtype=U32), ralive=np.ones(K.RL_LDS_CAP + 1, np.uint8), pt_voxel=np.zeros(4, np.int32), owner=np.zeros(4, U32), V=4)
    assert kp.relabel(big, True)[0] == EARG
    # helper_tile_list: cnt <= HT_CAP + 1
    tl = np.zeros((1, K.HT_CAP), U32)
    assert kp.tile_list(tl, [K.HT_CAP + 2], [-1])[0] == EARG and kp.tile_list(tl, [3], [-2])[0] == EARG
    # row_leaves: V >= 1, tile * 64 < V, the ghost inside the frame, cap <= QL
    good = cases_of("row_leaves")[5]

    def rl(**kw):
        c = K.Case("bad", "bad", **{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.__dict__.items() if k not in ("name", "classes")})
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return kp.row_leaves(c)[0]
    T = (good.V + 63) // 64
    assert rl(V=0) == EARG and rl(tids=(5, T)) == EARG and rl(tids=(63, 0xFFFFFFFE)) == EARG and rl(gvs=(2, good.V)) == EARG and rl(gvs=(0, -2)) == EARG
    assert rl(cap=K.QL + 1) == EARG and rl(cap=0) == EARG
    assert kp.vblock(0, 1)[0] == EARG and kp.vblock(1, 0)[0] == EARG and kp.vblock(5000, 1)[0] == EARG
    # d_centroid / d_sv_fill: h <= S0 tables, tiles and ghosts inside the frame, hlo <= hhi < V, no marking state, consistent leaf counts
    st0 = cases_of("centroid")[2].state

    def cen(edit, **ctl):
        st = st0.copy(); edit(st)
        return kp.centroid(st, **ctl)[0]
    assert cen(lambda s: None, n_changed=0, thr=5, marks=1) == EARG          # this state would mark tiles
    assert cen(lambda s: s.tcnt.__setitem__(1, K.HT_CAP + 2)) == EARG
    assert cen(lambda s: (s.tcnt.__setitem__(1, 2), s.tl.__setitem__((1, 1), (s.V + 63) // 64))) == EARG
    assert cen(lambda s: s.ghost_vox.__setitem__(2, s.V)) == EARG and cen(lambda s: s.ghost_vox.__setitem__(2, -5)) == EARG
    assert cen(lambda s: s.hhi.__setitem__(1, s.V)) == EARG and cen(lambda s: (s.hlo.__setitem__(1, 9), s.hhi.__setitem__(1, 8))) == EARG
    assert cen(lambda s: setattr(s, "V", 0)) == EARG and cen(lambda s: setattr(s, "gx", 4096)) == EARG
    sv0 = K.ref_centroid(st0)
    loff = np.r_[0, np.cumsum(sv0.hcount)].astype(U32)

    def svf(edit, lo=loff):
        st = sv0.copy(); edit(st)
        return kp.sv_fill(st, lo)[0]
    assert svf(lambda s: s.hcount.__setitem__(1, s.hcount[1] + 1)) == EARG          # one row more than the helper has leaves
    assert svf(lambda s: s.hcount.__setitem__(2, s.hcount[2] - 1)) == EARG
    shifted = loff.copy(); shifted[2:] += 5
    assert svf(lambda s: None, shifted) == EARG
    assert svf(lambda s: s.owner.__setitem__(np.flatnonzero(s.owner == 0)[:1], 1)) == EARG      # a leaf the count does not know
    assert svf(lambda s: s.ghost_vox.__setitem__(1, s.V)) == EARG and svf(lambda s: s.hhi.__setitem__(1, s.V)) == EARG and svf(lambda s: s.tcnt.__setitem__(1, K.HT_CAP + 2)) == EARG
