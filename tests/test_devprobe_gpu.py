"""Device numerics bit for bit against the host build of the headers (tested directly).

tests/devprobe/ compiles one dispatch table over the per-element functions of csrc/f3ds_math.h, f3ds_numerics.h, f3ds_algo.h and
f3ds_eval_levels.h twice: with g++ (the reference side: the arithmetic tests/test_devprobe_cpu.py ties to the oracle and the emulation)
and with hipcc for gfx950 under the product's own flags.  Here the two run on the rows of tests/devprobe_inputs.py -- known answers and
specials, rows that force each side of every named branch, 200 000 dense rows per function, rows a few ulps around each decision
boundary -- and must agree in every word; a NaN matches a NaN (conftest.same_bits), nothing else is relaxed and no row is dropped.
The lane-parallel restatements that exist only as device code (n_ciede00_quad, edge_weight_quad, lab_three_lanes, plane_normal_wave,
csrc/f3ds_quad.h) run beside their one-lane originals in the same launch, with both providers of the f64 constants (literals, and m_lds
over an LDS copy of the table as the merge kernel has it): lane-parallel == one-lane on the device == host, in every lane."""
import os

import numpy as np
import pytest

import devprobe_inputs as D
from conftest import same_bits
from test_devprobe_cpu import PROBE_DIR, Probe, cases, evl_tables, hostprobe  # noqa: F401  (cases, hostprobe: fixtures)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="session")
def devprobe(hostprobe, P):  # noqa: F811  (hostprobe has run make; conftest has imported torch, whose HIP runtime the library binds to)
    if P.device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible")
    return Probe(os.path.join(PROBE_DIR, "libf3ds_devprobe.so"), "dp_dev")


def _agree(case, what, got, want, kind):
    """got == want in every word of every row (NaN matches NaN); the message names the function, the first differing row, its inputs as
    hex floats and the branches the row belongs to"""
    ok = D.rows_equal(got, want, kind)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        group = [g for g, v in case.groups.items() if i in v]
        raise AssertionError("%s: %d of %d rows differ.  First: %s (group %s)\n  got  %s\n  want %s" % (
            what, int((~ok).sum()), len(ok), case.describe(i), group, " ".join("%08x" % x for x in got[i]), " ".join("%08x" % x for x in want[i])))
    for a, b in zip(D.typed(got, kind), D.typed(want, kind)):
        assert same_bits(a, b), what


@pytest.mark.parametrize("name", D.NAMES)
def test_device_equals_host(cases, hostprobe, devprobe, name):  # noqa: F811
    """One-lane functions: device == host on all groups, constants as literals and through the table (m_lds over LDS on the device,
    m_tab on the host: the device counterpart of test_math.py::test_constants_from_a_table_give_the_same_bits)."""
    c = cases(name)
    want = hostprobe.run(c.fn, c.rows)
    _agree(c, "%s (device, literals) against the host" % name, devprobe.run(c.fn, c.rows), want, D.OUT_KIND[c.fn])
    _agree(c, "%s (host, table) against the host with literals" % name, hostprobe.run(c.fn + 100, c.rows), want, D.OUT_KIND[c.fn])
    _agree(c, "%s (device, m_lds) against the host" % name, devprobe.run(c.fn + 100, c.rows), want, D.OUT_KIND[c.fn])


def test_ciede00_quad(cases, hostprobe, devprobe):  # noqa: F811
    """n_ciede00_quad on every quad of a wave: all four lanes, with m_lit and with m_lds, == n_ciede00 on one lane of the same launch == host;
    the same for the radicand in double (n_ciede00_sq / n_ciede00_quad_sq), where the rounding to float hides nothing"""
    c = cases("n_ciede00")
    want = hostprobe.run(c.fn, c.rows)
    want_sq = hostprobe.run(D.FN["n_ciede00_sq"], c.rows)
    out = devprobe.call("ciede_quad", c.rows, 27)
    _agree(c, "n_ciede00 (one lane, in the quad kernel) against the host", out[:, 0:1], want, "f")
    _agree(c, "n_ciede00_sq (one lane, in the quad kernel) against the host", out[:, 9:11], want_sq, "dd")
    for q in range(4):
        _agree(c, "n_ciede00_quad with m_lit, lane %d of the quad, against the host" % q, out[:, 1 + q:2 + q], want, "f")
        _agree(c, "n_ciede00_quad with m_lds, lane %d of the quad, against the host" % q, out[:, 5 + q:6 + q], want, "f")
        _agree(c, "n_ciede00_quad_sq with m_lit, lane %d of the quad, against the host" % q, out[:, 11 + 2 * q:13 + 2 * q], want_sq, "dd")
        _agree(c, "n_ciede00_quad_sq with m_lds, lane %d of the quad, against the host" % q, out[:, 19 + 2 * q:21 + 2 * q], want_sq, "dd")


def test_edge_weight_quad(cases, hostprobe, devprobe):  # noqa: F811
    """edge_weight_quad (every MERGING mode, EQUALIZATION with an 8-entry cdf table) == a_edge_weight on one lane == host: weight and err"""
    c = cases("a_edge_weight_lab")
    assert (c.rows[:, 24] == 0).all()                    # the generator's contract: LAB_CIEDE00 rows only
    want = hostprobe.run(c.fn, c.rows)
    out = devprobe.call("edge_quad", c.rows, 18)
    _agree(c, "a_edge_weight (one lane, in the quad kernel) against the host", out[:, 0:2], want, "fu")
    for q in range(4):
        _agree(c, "edge_weight_quad with m_lit, lane %d of the quad, against the host" % q, out[:, 2 + 2 * q:4 + 2 * q], want, "fu")
        _agree(c, "edge_weight_quad with m_lds, lane %d of the quad, against the host" % q, out[:, 10 + 2 * q:12 + 2 * q], want, "fu")


@pytest.mark.parametrize("rows_per_wave", [1, 4])
def test_lab_three_lanes(cases, hostprobe, devprobe, rows_per_wave):  # noqa: F811
    """lab_three_lanes with base = 0 (one colour per wave) and base = 16 r (four per wave) == n_rgb2lab on one lane == host, and every
    lane of the wave / of the row of 16 holds the same bits"""
    c = cases("n_rgb2lab")
    want = hostprobe.run(c.fn, c.rows)
    out = devprobe.call("lab_three", c.rows, 13, rows_per_wave)
    _agree(c, "n_rgb2lab (one lane, in the wave kernel) against the host", out[:, 0:3], want, "fff")
    for nm, at in (("m_lit", 3), ("m_lds", 8)):
        _agree(c, "lab_three_lanes with %s, %d colour(s) per wave, against the host" % (nm, rows_per_wave), out[:, at:at + 3], want, "fff")
        bad = np.nonzero((out[:, at + 3] != 0) | (out[:, at + 4] != 0))[0]
        assert len(bad) == 0, "lab_three_lanes with %s: lanes differ from the first lane in %d rows; first: %s, lane mask %08x%08x" % (
            nm, len(bad), c.describe(int(bad[0])), out[bad[0], at + 4], out[bad[0], at + 3])


def test_plane_normal_wave(cases, hostprobe, devprobe):  # noqa: F811
    """plane_normal_wave (count >= 3) == n_plane_normal with the centroid as view point on one lane == host; every lane of the wave holds
    the same normal and centroid; the centroid is sums 6..8 over the count"""
    c = cases("normal_cen")
    assert (c.rows[:, 9] >= 3).all()                     # the generator's contract
    want = hostprobe.run(c.fn, c.rows)
    out = devprobe.call("normal_wave", c.rows, 25)
    _agree(c, "n_plane_normal with the centroid as view point (one lane, in the wave kernel) against the host", out[:, 0:7], want, "f" * 7)
    with np.errstate(all="ignore"):
        cen = (c.rows[:, 6:9].view(F) / c.rows[:, 9:10].astype(F)).view(np.uint32)
    for nm, at in (("m_lit", 7), ("m_lds", 16)):
        _agree(c, "plane_normal_wave with %s against the host" % nm, out[:, at:at + 7], want, "f" * 7)
        _agree(c, "plane_normal_wave with %s: cen against acc[6..8] / count" % nm, out[:, at + 4:at + 7], cen, "fff")
        bad = np.nonzero((out[:, at + 7] != 0) | (out[:, at + 8] != 0))[0]
        assert len(bad) == 0, "plane_normal_wave with %s: lanes differ from lane 0 in %d rows; first: %s, lane mask %08x%08x" % (
            nm, len(bad), c.describe(int(bad[0])), out[bad[0], at + 8], out[bad[0], at + 7])


def test_known_answers_on_the_device(cases, devprobe):  # noqa: F811
    """The reference's 34 CIEDE2000 and 7 rgb_eucl vectors (both argument orders) evaluated by the GPU, within the existing 1e-4"""
    c = cases("n_ciede00")
    idx, want = c.expect["kat"]
    assert len(idx) == 68
    rows = c.rows[idx]
    assert np.abs(devprobe.run(c.fn, rows).view(F)[:, 0] - want).max() < 1e-4
    quad = devprobe.call("ciede_quad", rows, 27).view(F)
    for k in range(9):
        assert np.abs(quad[:, k] - want).max() < 1e-4, k
    c = cases("n_rgb_eucl")
    idx, want = c.expect["kat"]
    assert len(idx) == 16
    assert np.abs(devprobe.run(c.fn, c.rows[idx]).view(F)[:, 0] - want).max() < 1e-4


def test_evl_scores_on_the_device(hostprobe, devprobe):  # noqa: F811
    """evl_scores<evl_m_logf> with evl_visit_order / evl_match_column on the device == the g++ probe in all seven fields, on the 400 random
    tables and the hand-made quirks of tests/test_eval_levels_cpu.py: csrc/f3ds_eval_levels.h's "the same bits from g++ and hipcc"."""
    tabs = evl_tables(many=False)
    pk = D.pack_tables([t[1:] for t in tabs])
    want = hostprobe.evl(pk)
    got = devprobe.evl(pk)
    assert np.isfinite(want).all()
    for t, g, w in zip(tabs, got, want):
        assert g.view(np.uint32).tolist() == w.view(np.uint32).tolist(), "evl_scores, table '%s': device %r, host %r" % (t[0], g, w)
