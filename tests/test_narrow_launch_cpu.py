"""The narrow-launch GPU tests are not vacuous: from the sizes committed with the golden hashes, every family of grid-stride loops gets at least one
(case, width) of tests/test_narrow_launch_gpu.py at which it goes round three times or more and ends on a ragged trip.  No family is exempt: whoever
changes the frames, the widths or a kernel's stride keeps this green."""
import os
import re

import pytest

from conftest import ROOT
from golden_cases import GOLDEN_CASES
from narrow_launch_common import (BATCH_SIZES, BATCH_WIDTHS, ENTRY_CASES, ENTRY_WIDTHS, FAMILIES, LEVEL_CASES, LEVEL_WIDTHS, SINGLE_CASES, STAGE0, SWEEP_VARIANT_CASES,
                                  SWEEP_VARIANT_WIDTH, WIDTHS, golden_sizes, run_covers, trips)


def test_trip_arithmetic():
    assert trips(76800, 256, 1) == (300, False) and trips(76800, 256, 3) == (100, False)      # exact multiples end on a full trip at widths 1 and 3 ...
    assert trips(76800, 256, 8) == (38, True) and trips(19200, 256, 8) == (10, True)          # ... and on half a row of workgroups at width 8
    assert trips(200000, 256, 8) == (98, True)                                                # 781.25 blocks
    assert trips(15830, 4096, 1) == (4, True) and trips(512, 256, 2) == (1, False) and trips(513, 256, 2) == (2, True)
    assert trips(49, 1, 16) == (4, True)


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.name)
def test_every_loop_family_makes_three_ragged_trips_somewhere(family):
    runs = [(name, w) for name, widths in SINGLE_CASES for w in widths if family.only is None or name in family.only]
    good = [(name, w) for name, w in runs if run_covers(family, golden_sizes(name), w)]
    assert good, "%s (%s): none of %r makes three trips with a ragged last one" % (family.name, family.kernels, runs)


def test_worked_examples():
    by = {f.name: f for f in FAMILIES}
    ghosts = golden_sizes("rgbd_320x240_ghosts")
    assert (ghosts["n"], ghosts["V"], ghosts["E"], ghosts["S0"]) == (76800, 15830, 2266, 1492)
    for fam in ("V/256", "V/4096", "V/64", "E/256", "S0/256", "C/256"):
        assert run_covers(by[fam], ghosts, 1), fam
    assert not run_covers(by["points/256"], ghosts, 1) and not run_covers(by["points/256"], ghosts, 3) and run_covers(by["points/256"], ghosts, 8)
    fused = golden_sizes("fused_200k_nan_lambda")
    assert fused["n"] % 256 == 64 and run_covers(by["points/256"], fused, 8)
    assert not run_covers(by["V/16384"], ghosts, 1) and run_covers(by["V/16384"], fused, 1) and run_covers(by["tiles/1"], fused, 1)


def test_case_tables_are_consistent():
    names = [n for n, _ in SINGLE_CASES]
    assert len(set(names)) == len(names) and all(n in GOLDEN_CASES for n in names)
    assert all(set(w) <= set(WIDTHS) for _, w in SINGLE_CASES) and STAGE0 == ("sort", "tiles")
    for n in SWEEP_VARIANT_CASES + ENTRY_CASES + LEVEL_CASES:
        assert n in GOLDEN_CASES
    assert SWEEP_VARIANT_WIDTH in WIDTHS and set(ENTRY_WIDTHS) | set(BATCH_WIDTHS) | set(LEVEL_WIDTHS) <= set(WIDTHS)
    assert all(b % 8 == 1 for b in BATCH_SIZES)                  # full groups of eight and a remainder frame


def test_every_listed_kernel_exists():
    csrc = os.path.join(ROOT, "fast-3d-pointcloud-segmentation_amd", "csrc")
    src = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".inc", ".hip")))      # (wherever a kernel lives)
    for fam in FAMILIES:
        for k in re.findall(r"\bd_\w+", fam.kernels):
            assert re.search(r"struct %s\b" % k, src), (fam.name, k)
