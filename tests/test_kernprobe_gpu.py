"""The wave- and workgroup-level building blocks of csrc/f3ds_kernels.inc, one by one, against plain references (tests/kernprobe_inputs.py).

tests/kernprobe/kernprobe.hip includes the product's headers and f3ds_kernels.inc unchanged and puts a thin __global__ wrapper around each
primitive: ballot ranks and DPP lane exchanges (the wave scans, minima, row_sort16, run_of_lane), the workgroup scans, d_scan_single and the
three-kernel scan, the radix sort's histogram / scatter kernels and its pass sequence, the two segment-table chains, the relabel prefix,
helper_tile_list, row_leaves, d_centroid and d_sv_fill on both of their paths (four helpers per wave / a wave per helper), and the batched launches'
block mapping.  Every comparison is exact: integers word for word, floats with conftest.same_bits against float32 arithmetic done sequentially
in the stated order.  No case is skipped; a failure names the primitive, the case, the first differing index and both words in hex."""
import os

import numpy as np
import pytest

import kernprobe_inputs as K
from conftest import same_bits
from test_kernprobe_cpu import PROBE_DIR, KernProbe, cases_of, kp_built, kp_host  # noqa: F401  (kp_built, kp_host: fixtures)

pytestmark = pytest.mark.gpu
U32 = np.uint32
U64 = np.uint64
F = np.float32


@pytest.fixture(scope="session")
def kp(kp_built, P):  # noqa: F811  (kp_built has run make; conftest has imported torch, whose HIP runtime the library binds to)
    if P.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    return KernProbe(os.path.join(PROBE_DIR, "libf3ds_kernprobe.so"))


def _hex(x):
    x = np.asarray(x).reshape(-1)[0]
    return ("%016x" if x.dtype.itemsize == 8 else "%08x") % int(x.view(U64 if x.dtype.itemsize == 8 else U32 if x.dtype.itemsize == 4 else x.dtype))


def same(prim, case, got, want, unit="index", what=""):
    """got == want in every word; the message names the primitive, the case, the first differing index and both words in hex"""
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s, case '%s'%s: shape %s, want %s" % (prim, case, what, got.shape, want.shape)
    if got.dtype.kind == "f":
        got = got.view(U32); want = np.ascontiguousarray(want, F).view(U32)
    else:
        want = want.astype(got.dtype)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    if len(bad):
        i = int(bad[0])
        where = "%s %d" % (unit, i) if got.ndim == 1 else "%s %s" % (unit, tuple(int(x) for x in np.unravel_index(i, got.shape)))
        raise AssertionError("%s, case '%s'%s: %d of %d words differ.  First at %s: got %s, want %s" % (
            prim, case, what, len(bad), got.size, where, _hex(got.reshape(-1)[i]), _hex(want.reshape(-1)[i])))


def ok(rc, prim, case=""):
    assert rc[0] == 0, "%s, case '%s': the probe returned %d" % (prim, case, rc[0])
    return rc[1:] if len(rc) > 2 else rc[1]


# ---- wave and workgroup scans ------------------------------------------------------------------------------------------------------------------
def test_wave_scans(kp):
    """wave_incl_scan and wave_incl_scan_dpp == np.cumsum in uint32, and so each other"""
    cs = cases_of("scan64")
    rows = np.array([c.v for c in cs], U32)
    a = ok(kp.wave(0, rows), "wave_incl_scan"); b = ok(kp.wave(1, rows), "wave_incl_scan_dpp")
    for i, c in enumerate(cs):
        want = K.ref_incl_scan(c.v)
        same("wave_incl_scan", c.name, a[i], want, "lane")
        same("wave_incl_scan_dpp", c.name, b[i], want, "lane")
        same("wave_incl_scan_dpp against wave_incl_scan", c.name, b[i], a[i], "lane")


def test_block_scans(kp):
    """block_incl_scan<256> with its total (as every thread receives it) and block_excl_scan2 == np.cumsum in uint32"""
    cs = cases_of("scan256")
    a = ok(kp.block(0, np.array([c.v for c in cs], U32)), "block_incl_scan<256>")
    b = ok(kp.block(1, np.array([np.r_[c.v, c.v2] for c in cs], U32)), "block_excl_scan2")
    for i, c in enumerate(cs):
        inc, inc2 = K.ref_incl_scan(c.v), K.ref_incl_scan(c.v2)
        same("block_incl_scan<256>", c.name, a[i, :256], inc, "thread")
        same("block_incl_scan<256>", c.name, a[i, 256:], np.full(256, inc[-1], U32), "thread", " (total)")
        same("block_excl_scan2", c.name, b[i, 0:256], K.ref_excl_scan(c.v), "thread", " (a)")
        same("block_excl_scan2", c.name, b[i, 256:512], K.ref_excl_scan(c.v2), "thread", " (b)")
        same("block_excl_scan2", c.name, b[i, 512:768], np.full(256, inc[-1], U32), "thread", " (total of a)")
        same("block_excl_scan2", c.name, b[i, 768:1024], np.full(256, inc2[-1], U32), "thread", " (total of b)")


# ---- minima, the 16-lane sort, runs ------------------------------------------------------------------------------------------------------------
def test_minima_and_row_sort(kp):
    """wave_min_u32 == np.min in every lane; row_min_u32 == np.min per 16-lane row; row_sort16 == np.sort per row (unsigned)"""
    cs = cases_of("minsort")
    rows = np.array([c.v for c in cs], U32)
    wm = ok(kp.wave(2, rows), "wave_min_u32"); rm = ok(kp.wave(3, rows), "row_min_u32"); rs = ok(kp.wave(4, rows), "row_sort16")
    for i, c in enumerate(cs):
        same("wave_min_u32", c.name, wm[i], K.ref_wave_min(c.v), "lane")
        same("row_min_u32", c.name, rm[i], K.ref_row_min(c.v), "lane")
        same("row_sort16", c.name, rs[i], K.ref_row_sort(c.v), "lane")


def test_run_of_lane(kp):
    """head in every lane; head_lane and run_len in the valid lanes (the run a lane belongs to: an invalid lane belongs to none)"""
    cs = cases_of("run_of_lane")
    out = ok(kp.run_of_lane(np.array([np.r_[c.valid, c.w0, c.w1] for c in cs], U32)), "run_of_lane")
    for i, c in enumerate(cs):
        head, hl, ln = K.ref_run_of_lane(c.valid, c.w0, c.w1)
        v = c.valid != 0
        same("run_of_lane", c.name, out[i, 0:64], head, "lane", " (head)")
        same("run_of_lane", c.name, np.where(v, out[i, 64:128], 0), hl, "lane", " (head_lane)")
        same("run_of_lane", c.name, np.where(v, out[i, 128:192], 0), ln, "lane", " (run_len)")


# ---- d_scan_single, scan_u32 -------------------------------------------------------------------------------------------------------------------
def test_scan_single(kp):
    """exclusive np.cumsum in uint32, in place; the 40 words behind m stay as they were"""
    for c in cases_of("scan_single"):
        m = len(c.data)
        buf = np.r_[c.data, np.full(40, 0xDEADBEEF, U32)]
        got = ok(kp.scan_single(buf, m), "d_scan_single", c.name)
        same("d_scan_single", c.name, got, np.r_[K.ref_excl_scan(c.data), buf[m:]])


def test_scan_u32(kp):
    """d_scan_tiles + d_scan_single + d_scan_add as scan_u32 records them == inclusive np.cumsum; nothing is written behind n"""
    for c in cases_of("scan_u32"):
        n = len(c.data)
        buf = np.r_[c.data, np.full(24, 7, U32)]
        got = ok(kp.scan_u32(buf, n, c.extra), "scan_u32", c.name)
        same("scan_u32", c.name, got, np.r_[K.ref_incl_scan(c.data), np.zeros(24, U32)])


# ---- radix sort ----------------------------------------------------------------------------------------------------------------------------------
def test_radix_hist(kp):
    """np.bincount per tile and digit, hist[d * nb + tile]"""
    for c in cases_of("radix_pass"):
        got = ok(kp.radix_hist(c.keys, c.shift, c.bits, c.n_dev), "d_radix_hist", c.name)
        same("d_radix_hist", c.name, got, K.ref_radix_hist(c), "digit * nb + tile")


@pytest.mark.parametrize("kernel", ["d_radix_scatter", "d_radix_scatter_k"])
def test_radix_scatter(kp, kernel):
    """fed the reference's scanned histogram: a stable partition by digit, the other bits carried along; nothing behind the sorted count"""
    for c in cases_of("radix_pass"):
        if kernel == "d_radix_scatter_k" and c.n_dev >= 0:
            continue          # (the keys-only kernel takes no device-side count: not a case of it)
        hs = K.ref_excl_scan(K.ref_radix_hist(c))
        wk, wv = K.ref_radix_scatter(c)
        if kernel == "d_radix_scatter":
            gk, gv = ok(kp.radix_scatter(c.keys, c.vals, c.shift, c.bits, hs, c.n_dev), kernel, c.name)
            same(kernel, c.name, gv, wv, "position", " (values)")
        else:
            gk, _ = ok(kp.radix_scatter(c.keys, None, c.shift, c.bits, hs), kernel, c.name)
        same(kernel, c.name, gk, wk, "position", " (keys)")


def test_radix_sort(kp):
    """the pass sequence of radix_sort == np.argsort(kind="stable") on the masked bits"""
    for c in cases_of("radix_sort"):
        wk, wv = K.ref_radix_sort(c)
        gk, gv = ok(kp.radix_sort(c.keys, c.vals if c.pairs else None, c.total, c.base, c.n_dev), "radix_sort", c.name)
        same("radix_sort", c.name, gk, wk, "position", " (keys)")
        if c.pairs:
            same("radix_sort", c.name, gv, wv, "position", " (values)")


# ---- the segment table -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [0, 1])
def test_segment_table(kp, chain):
    """d_heads + scan_u32 + d_segstart (chain 0) and d_seg_count + d_scan_single + d_seg_write (chain 1) == np.unique on the shifted keys below the limit"""
    prim = ("d_heads + scan_u32 + d_segstart", "d_seg_count + d_scan_single + d_seg_write")[chain]
    for c in cases_of("seg_table"):
        seg, cnt = ok(kp.seg_table(chain, c.keys, c.limit, c.shift), prim, c.name)
        wseg, wcnt = K.ref_seg_table(c)
        same(prim, c.name, cnt, wcnt, "counter", " (segments, valid keys)")
        same(prim, c.name, seg, wseg, "segment", " (seg_start)")


# ---- relabel ---------------------------------------------------------------------------------------------------------------------------------------
def test_region_ids(kp):
    """relabel_tables through d_region_ids: roots in ascending label get ids 0.., every label takes its root's id"""
    for c in cases_of("relabel"):
        rank, root, incl, nreg = ok(kp.relabel(c, False), "d_region_ids", c.name)
        w = K.ref_relabel(c)
        same("d_region_ids", c.name, rank, w[0], "label", " (rank)")
        same("d_region_ids", c.name, root, w[1], "label", " (root_out)")
        same("d_region_ids", c.name, incl, w[2], "label", " (incl_out)")
        assert nreg == w[3], "d_region_ids, case '%s': n_regions %d, want %d" % (c.name, nreg, w[3])


def test_relabel(kp):
    """d_relabel (rank table in LDS, every workgroup builds it, workgroup 0 writes root / incl / n_regions) with the grid width of seg_labels"""
    for c in cases_of("relabel"):
        labels, root, incl, nreg = ok(kp.relabel(c, True), "d_relabel", c.name)
        w = K.ref_relabel(c)
        same("d_relabel", c.name, labels, w[4], "point", " (labels)")
        same("d_relabel", c.name, root, w[1], "label", " (root_out)")
        same("d_relabel", c.name, incl, w[2], "label", " (incl_out)")
        assert nreg == w[3], "d_relabel, case '%s': n_regions %d, want %d" % (c.name, nreg, w[3])


# ---- helper_tile_list, row_leaves ------------------------------------------------------------------------------------------------------------------
def test_helper_tile_list(kp):
    """sorted(set(list + ghost tile)), or -1; the table behind the distinct tiles stays untouched"""
    cs = cases_of("tile_list")
    srt, ret = ok(kp.tile_list(np.array([c.tl for c in cs], U32), [c.cnt for c in cs], [c.gv for c in cs]), "helper_tile_list")
    for i, c in enumerate(cs):
        want = K.ref_tile_list(c.tl, c.cnt, c.gv)
        assert ret[i] == (-1 if want is None else len(want)), "helper_tile_list, case '%s' (cnt %d, gv %d): returned %d, want %d" % (
            c.name, c.cnt, c.gv, ret[i], -1 if want is None else len(want))
        if want is not None:
            same("helper_tile_list", c.name, srt[i], np.r_[np.array(want, U32), np.full(64 - len(want), K.NONE, U32)], "entry")


def test_row_leaves(kp):
    """per row: distinct tiles ascending, leaves (owner == h or the ghost voxel) ascending and cut at cap, the count, the kept bits; every lane of a row gets the same scalars"""
    for c in cases_of("row_leaves"):
        qt, ql, scal = ok(kp.row_leaves(c), "row_leaves", c.name)
        for r, (tiles, count, leaves, kept) in enumerate(K.ref_row_leaves(c)):
            w = " (row %d, h %d, gv %d)" % (r, c.hs[r], c.gvs[r])
            same("row_leaves", c.name, scal[0, 16 * r:16 * r + 16], np.full(16, count, U32), "lane of the row", w + " count")
            same("row_leaves", c.name, scal[1, 16 * r:16 * r + 16], np.full(16, len(tiles), U32), "lane of the row", w + " nd")
            same("row_leaves", c.name, scal[2, 16 * r:16 * r + 16], np.full(16, kept, U32), "lane of the row", w + " kept")
            same("row_leaves", c.name, qt[r, :len(tiles)], tiles, "tile", w + " distinct tiles")
            want = np.full(K.QL + 32, K.NONE, U32)
            want[:min(count, c.cap)] = leaves[:c.cap]
            got = ql[r].copy()
            got[c.cap + 31] = K.NONE          # the spare entry takes the writes of non-leaves and of leaves past cap: any value
            same("row_leaves", c.name, got, want, "leaf", w + " leaves")


# ---- f3ds_vblock -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", K.VBLOCK_NF)
@pytest.mark.parametrize("gx", K.VBLOCK_GX)
def test_vblock(kp, gx, nf):
    """every (frame, vbx) of gx x nf exactly once; in the full groups of 8 frames, 8 consecutive linear ids are 8 distinct frames of one vbx; the rest is the plain mapping"""
    out = ok(kp.vblock(gx, nf), "f3ds_vblock", "gx %d, nf %d" % (gx, nf))
    fv = out[0].astype(np.int64)
    same("f3ds_frame / BIX against f3ds_vblock", "gx %d, nf %d" % (gx, nf), out[1], out[0], "workgroup")
    assert (fv[:, 0] < nf).all() and (fv[:, 1] < gx).all(), "f3ds_vblock, gx %d, nf %d: a workgroup is sent outside the launch: %s" % (gx, nf, fv[(fv[:, 0] >= nf) | (fv[:, 1] >= gx)][0])
    hits = np.bincount(fv[:, 0] * gx + fv[:, 1], minlength=gx * nf)
    assert (hits == 1).all(), "f3ds_vblock, gx %d, nf %d: (frame %d, vbx %d) is hit %d times" % (gx, nf, int(np.argmax(hits != 1)) // gx, int(np.argmax(hits != 1)) % gx, hits[np.argmax(hits != 1)])
    full = nf & ~7
    for lin in range(0, full * gx, 8):
        g = fv[lin:lin + 8]
        assert len(set(g[:, 0].tolist())) == 8 and len(set(g[:, 1].tolist())) == 1 and (g[:, 0] // 8 == g[0, 0] // 8).all(), \
            "f3ds_vblock, gx %d, nf %d: linear ids %d..%d map to frames %s, blocks %s" % (gx, nf, lin, lin + 7, g[:, 0].tolist(), g[:, 1].tolist())
    for lin in range(full * gx, nf * gx):
        assert fv[lin].tolist() == [lin // gx, lin % gx], "f3ds_vblock, gx %d, nf %d: workgroup %d behind the full groups maps to %s" % (gx, nf, lin, fv[lin].tolist())


# ---- d_centroid, d_sv_fill -------------------------------------------------------------------------------------------------------------------------
def _wave_path(st):
    """the same helpers in a frame padded with unowned voxels until V > 48 * S0: d_centroid and d_sv_fill then take a wave per helper"""
    return st.padded(48 * st.S0 + 1 + (st.S0 % 3) * 64, np.random.default_rng(st.V))


def _same_state(prim, name, got, want):
    for field, unit in (("hcount", "helper"), ("tcnt", "helper"), ("ghost_active", "helper"), ("ghost_done", "helper"), ("tl", "(helper, entry)"), ("hc", "(helper, component)")):
        same(prim, name, getattr(got, field), getattr(want, field), unit, " (%s)" % field)
    for field in ("owner", "ghost_vox", "hlo", "hhi"):
        same(prim, name, getattr(got, field), getattr(want, field), "index", " (%s: not to be written)" % field)


@pytest.mark.parametrize("path", ["rows", "waves"])
def test_centroid(kp, path):
    """d_centroid at t = 0 on hand-built helper books, nothing marking tiles: float32 sums of the leaves' feature rows in ascending ordinal, a_centroid_finish step
    by step, the tile list rewritten as the tiles holding an owned leaf, hcount / tcnt / ghost_active / ghost_done.  The same helper states once with
    V <= 48 * S0 (four helpers per wave, big ones sent on to the wave-wide path) and once padded to V > 48 * S0 (a wave per helper): both equal the reference."""
    for c in cases_of("centroid"):
        st = c.state if path == "rows" else _wave_path(c.state)
        assert (st.V <= 48 * st.S0) == (path == "rows")
        rc, got = kp.centroid(st)
        assert rc == 0, "d_centroid (%s), case '%s': the probe returned %d" % (path, c.name, rc)
        _same_state("d_centroid (%s)" % path, c.name, got, K.ref_centroid(st))


def test_centroid_idle_sweep_changes_nothing(kp):
    """sweep_idle == t + 1: the kernel returns at once"""
    st = cases_of("centroid")[8].state
    rc, got = kp.centroid(st, idle=1)
    assert rc == 0
    _same_state("d_centroid (idle)", "300 helpers", got, st)


@pytest.mark.parametrize("path", ["rows", "waves"])
def test_sv_fill(kp, kp_host, path):  # noqa: F811
    """d_sv_fill on the states d_centroid leaves: leaf order from numpy; payload rows, the twelve ordered sums and the Lab of the mean colour from the g++ build of
    a_payload_row / a_fold_row / n_rgb2lab; centroid and normal of the record copied from the helper's row; zeroed records for helpers without leaves"""
    for c in cases_of("sv_fill"):
        st = c.state if path == "rows" else _wave_path(c.state)
        prim = "d_sv_fill (%s)" % path
        loff, rows, rv, racc, rcnt, rrec, ral, alive = K.ref_sv_fill(st, kp_host.sv)
        out = kp.sv_fill(st, loff)
        assert out[0] == 0, "%s, case '%s': the probe returned %d" % (prim, c.name, out[0])
        same(prim, c.name, out[2], rv, "row", " (row_voxel)")
        same(prim, c.name, out[1], rows, "(row, column)", " (payload rows)")
        same(prim, c.name, out[3], racc, "(helper, sum)", " (racc0)")
        same(prim, c.name, out[4], rcnt, "helper", " (rcnt0)")
        same(prim, c.name, out[5], rrec, "(helper, field)", " (rrec0)")
        same(prim, c.name, out[6], ral, "helper", " (ralive0)")
        assert out[7] == alive, "%s, case '%s': n_alive %d, want %d" % (prim, c.name, out[7], alive)
        assert same_bits(out[1], rows) and same_bits(out[3], racc) and same_bits(out[5], rrec)
