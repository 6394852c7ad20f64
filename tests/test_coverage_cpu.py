"""Area-coverage rasteriser, the part that needs no GPU: the CPU restatement (tests/coverage_oracle.py) against closed-form
areas, `composeTransmission` (pure torch), and the host-only side of the C entry."""
import math
import os

import numpy as np
import pytest
import torch

from helpers import ROOT

import coverage_oracle as CO


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", ROOT, "-j", "8", "all"])
    return _native


@pytest.fixture(scope="module")
def LY():
    from lithographysimulator_amd import layout
    return layout


def rect(xa, ya, xb, yb):
    return np.array([[xa, ya], [xb, ya], [xb, yb], [xa, yb]], dtype=float)


# ---- the restatement, pinned by closed forms -----------------------------------------------------------------------------
def test_rectangle_on_subgrid_lines_gives_exact_area_fractions(LY):
    """pixel 8, s = 4: sub-grid pitch 2.  [10, 38] x [6, 20]: column 1 is covered from 10 to 16 (3/4), columns 2, 3 fully,
    column 4 from 32 to 38 (3/4); row 0 from 6 to 8 (1/4), row 1 fully, row 2 from 16 to 20 (1/2)."""
    c = CO.coverage(LY.polygonEdges([rect(10, 6, 38, 20)]), 6, 0.0, 0.0, 8.0, 4)
    want = np.zeros((6, 6), dtype=np.float32)
    want[0:3, 1:5] = np.outer([0.25, 1.0, 0.5], [0.75, 1.0, 1.0, 0.75])
    assert c.dtype == np.float32 and np.array_equal(c, want)
    assert float(c.astype(np.float64).sum()) * 64.0 == 28.0 * 14.0


def test_overlapping_rectangles_union(LY):
    polys = [rect(4, 4, 30, 26), rect(18, 10, 44, 40)[::-1]]              # the second one clockwise
    c = CO.coverage(LY.polygonEdges(polys), 6, 0.0, 0.0, 8.0, 4)
    union = 26 * 22 + 26 * 30 - 12 * 16
    assert float(c.astype(np.float64).sum()) * 64.0 == float(union)
    assert float(c.max()) == 1.0 and float(c.min()) == 0.0


def test_clockwise_equals_counter_clockwise(LY):
    tri = np.array([[3.0, 2.0], [41.0, 9.0], [17.0, 44.0]])
    a = CO.coverage_counts(LY.polygonEdges([tri]), 6, 0.0, 0.0, 8.0, 8)
    b = CO.coverage_counts(LY.polygonEdges([tri[::-1]]), 6, 0.0, 0.0, 8.0, 8)
    assert np.array_equal(a, b) and 0 < a.sum() < 36 * 64
    # s = 8 at pixel 8: unit sub-cells.  Only a sub-cell that the boundary crosses can differ from its covered area, by less
    # than 1; a segment crosses at most |dx| + |dy| + 1 cells
    area = 0.5 * abs((41 - 3) * (44 - 2) - (17 - 3) * (9 - 2))            # shoelace: 749
    crossed = (38 + 7 + 1) + (24 + 35 + 1) + (14 + 42 + 1)
    print(f"triangle: {int(a.sum())} sub-centres inside, area {area}")
    assert abs(float(a.sum()) - area) <= crossed


def test_whole_pixel_rectangle_and_empty_layout(LY):
    c = CO.coverage(LY.polygonEdges([rect(8, 16, 40, 32)]), 6, 0.0, 0.0, 8.0, 8)
    want = np.zeros((6, 6), dtype=np.float32)
    want[2:4, 1:5] = 1.0
    assert np.array_equal(c, want)
    from oracle import layout_oracle as LO
    assert np.array_equal(c.astype(np.int16), LO.rasterize_edges(LY.polygonEdges([rect(8, 16, 40, 32)]), 6, 0.0, 0.0, 8.0))
    assert not CO.coverage(np.zeros((0, 4)), 5, 0.0, 0.0, 8.0, 4).any()


def test_s1_is_the_binary_raster(LY):
    from oracle import layout_oracle as LO
    e = LY.polygonEdges(CO.random_layout(5, 20, 3.0, 1))
    assert np.array_equal(CO.coverage_counts(e, 20, 0.0, 0.0, 3.0, 1), LO.rasterize_edges(e, 20, 0.0, 0.0, 3.0))


# ---- composeTransmission -------------------------------------------------------------------------------------------------
def test_compose_transmission(LY):
    """Fails on a tree without the feature: there is no composeTransmission."""
    import lithographysimulator_amd as L
    assert "composeTransmission" in L.__all__ and L.composeTransmission is LY.composeTransmission
    gen = torch.Generator().manual_seed(3)
    g1 = (torch.rand(16, 16, generator=gen) < 0.4).to(torch.int16)
    g2 = (torch.rand(16, 16, generator=gen) < 0.4).to(torch.int16)
    v1, v2, bg = 1 + 0j, complex(math.sqrt(0.06)) * -1, 0.25j
    # the override rule of maskFromGDSII(transmissions=...), statement for statement
    want = torch.full((16, 16), bg, dtype=torch.complex64)
    want[g1 != 0] = v1
    want[g2 != 0] = v2
    got = LY.composeTransmission([g1, g2], [v1, v2], background=bg)
    assert got.dtype == torch.complex64 and torch.equal(got, want)
    assert torch.equal(LY.composeTransmission([g1.float(), g2.double()], [v1, v2], bg), want)
    # a half-covered pi shifter over clear glass is dark
    half = torch.full((4, 4), 0.5)
    assert torch.equal(LY.composeTransmission([half], [-1], background=1), torch.zeros(4, 4, dtype=torch.complex64))
    # area average of one layer over the background; the default background is opaque
    quarter = torch.full((2, 2), 0.25)
    assert torch.equal(LY.composeTransmission([quarter], [1j], background=1), torch.full((2, 2), 0.75 + 0.25j, dtype=torch.complex64))
    assert torch.equal(LY.composeTransmission([quarter], [1]), torch.full((2, 2), 0.25 + 0j, dtype=torch.complex64))
    # order matters: the later layer lies on top
    ab = LY.composeTransmission([half, half], [1, -1])
    ba = LY.composeTransmission([half, half], [-1, 1])
    assert torch.equal(ab, torch.full((4, 4), -0.25 + 0j, dtype=torch.complex64)) and torch.equal(ba, -ab)
    with pytest.raises(ValueError):
        LY.composeTransmission([half], [1, 2])
    with pytest.raises(ValueError):
        LY.composeTransmission([], [])
    with pytest.raises(ValueError):
        LY.composeTransmission([half, quarter], [1, 2])


# ---- the host-only side of the C entry ------------------------------------------------------------------------------------
def test_work_bytes_formula_and_bad_arguments(nat):
    wb = nat.rasterize_coverage_work_bytes
    for pn, s, rows in ((33, 4, 1), (33, 4, 7), (33, 4, 33), (2048, 8, 2048), (2048, 16, 5), (32768, 1, 2), (1, 16, 1)):
        assert wb(pn, s, rows) == rows * s * (pn * s + 1) * 4
    assert wb(2048, 8, 2048) == 16384 * 16385 * 4                         # the 1 GiB the banding avoids
    for pn, s, rows in ((33, 3, 1), (33, 0, 1), (33, 32, 1), (33, -4, 1), (0, 4, 1), (-5, 4, 1), (33, 4, 0), (33, 4, -1),
                        (4097, 8, 1), (2049, 16, 1), (32769, 1, 1)):
        assert wb(pn, s, rows) == 0, (pn, s, rows)
    assert "litho_rasterize_coverage" in nat.exported_symbols() and "litho_rasterize_coverage_work_bytes" in nat.exported_symbols()


def test_argument_errors_before_any_gpu_work(nat):
    """Every pointer is NULL or a dummy that a call which got past its checks would fault on: no device is touched."""
    import ctypes
    f = nat.lib().litho_rasterize_coverage
    p = ctypes.c_void_p(8)
    big = 1 << 20
    assert f(p, 1, 8, 0.0, 0.0, 1.0, 3, p, big, p, None) == nat.E_ARG          # s not a supported level
    assert f(p, 1, 8, 0.0, 0.0, 1.0, 32, p, big, p, None) == nat.E_ARG
    assert f(p, 1, 4096, 0.0, 0.0, 1.0, 16, p, big, p, None) == nat.E_ARG      # pn * s > 32768
    assert f(p, 1, 0, 0.0, 0.0, 1.0, 4, p, big, p, None) == nat.E_ARG
    assert f(p, 1, 8, 0.0, 0.0, 1.0, 4, p, big, None, None) == nat.E_ARG       # NULL output
    assert f(p, 1, 8, 0.0, 0.0, 1.0, 4, None, big, p, None) == nat.E_ARG       # NULL workspace
    assert f(None, 1, 8, 0.0, 0.0, 1.0, 4, p, big, p, None) == nat.E_ARG       # NULL edges with n_edges > 0
    assert f(p, 1, 8, 0.0, 0.0, 0.0, 4, p, big, p, None) == nat.E_ARG          # pixel <= 0
    assert f(p, 1, 8, float("nan"), 0.0, 1.0, 4, p, big, p, None) == nat.E_ARG
    assert f(p, 1, 8, 0.0, 0.0, 1.0, 4, p, nat.rasterize_coverage_work_bytes(8, 4, 1) - 1, p, None) == nat.E_WORKSPACE


def test_bad_antialias_is_a_value_error_on_the_host(LY):
    for bad in (0, 3, 32, -2, 2.5):
        with pytest.raises(ValueError):
            LY.rasterizeLayout([rect(0, 0, 4, 4)], 8, 1.0, origin=(0.0, 0.0), antialias=bad)
        with pytest.raises(ValueError):
            LY.maskFromGDSII(LY.GdsLibrary(), 8, 1.0, antialias=bad)
