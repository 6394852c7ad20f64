"""CPU-side checks of the complex-transmission (phase-shift / grey) mask: the C entry's argument checks, the two mask
helpers, and the `Mask(transmission=...)` constructor -- nothing here touches a device."""
import ctypes
import math
import os

import pytest
import torch

from helpers import ROOT

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", ROOT, "-j", "8", "all"])
    return _native


@pytest.fixture(scope="module")
def L():
    import lithographysimulator_amd as L
    return L


def test_library_exports_the_complex_entry(nat):
    assert "litho_mask_spectrum_complex" in nat.exported_symbols()
    assert hasattr(ctypes.CDLL(nat.LIB_PATH), "litho_mask_spectrum_complex")
    text = open(os.path.join(ROOT, "include", "litho_abbe.h")).read()
    assert "int litho_mask_spectrum_complex(const void *transmission" in text


def test_argument_errors_before_any_gpu_work(nat):
    """The same checks, in the same order, as litho_mask_spectrum; every pointer below is either NULL or a dummy that a
    call which got past its checks would fault on."""
    f = nat.lib().litho_mask_spectrum_complex
    g = nat.lib().litho_mask_spectrum
    p = ctypes.c_void_p(8)
    cases = [
        ((None, 64, 1.0, 128, p, p, 0, None), nat.E_ARG),             # NULL transmission
        ((p, 64, 1.0, 128, None, p, 0, None), nat.E_ARG),             # NULL spectrum
        ((p, 63, 1.0, 128, p, p, 0, None), nat.E_ARG),                # odd pn
        ((p, 64, 0.0, 128, p, p, 0, None), nat.E_ARG),                # epsilon <= 0
        ((p, 64, -1.5, 128, p, p, 0, None), nat.E_ARG),
        ((p, 64, float("nan"), 128, p, p, 0, None), nat.E_ARG),
        ((p, 64, 1.0, 100, p, p, 0, None), nat.E_ARG),                # N not a power of two
        ((p, 64, 1.0, 32, p, p, 0, None), nat.E_NSMALL),              # N < pn
        ((p, 64, 1.0, 128, p, None, 0, None), nat.E_WORKSPACE),       # no workspace
        ((p, 64, 1.0, 128, p, p, 16, None), nat.E_WORKSPACE),         # workspace too small
    ]
    for args, want in cases:
        assert f(*args) == want, args
        assert g(*args) == want, args                                 # ... and the int16 entry agrees


def test_attenuated_psm_values(L):
    geo = torch.tensor([[0, 1, 2], [-1, 0, 0]], dtype=torch.int16)
    t = L.attenuatedPSM(geo)
    assert t.dtype == torch.complex64 and t.shape == geo.shape and t.device == geo.device
    a = torch.tensor(math.sqrt(0.06), dtype=torch.float32)
    clear = geo != 0
    assert torch.equal(t[clear], torch.ones(3, dtype=torch.complex64))
    assert torch.equal(t.real[~clear], -a.expand(3)) and torch.equal(t.imag[~clear], torch.zeros(3))   # exact pi: (-a, 0)
    t = L.attenuatedPSM(geo, 0.25, math.pi / 2)
    assert torch.equal(t[~clear], torch.full((3,), 0.5j, dtype=torch.complex64))                       # (0, a) exactly
    t = L.attenuatedPSM(geo, 0.25, 3 * math.pi / 2)
    assert torch.equal(t[~clear], torch.full((3,), -0.5j, dtype=torch.complex64))
    t = L.attenuatedPSM(geo, 1.0, 0.0)
    assert torch.equal(t, torch.ones(2, 3, dtype=torch.complex64))
    t = L.attenuatedPSM(geo, 0.0)                                     # a binary chrome mask
    assert torch.equal(t, clear.to(torch.complex64))
    t = L.attenuatedPSM(geo, 0.09, 1.0)                               # a general phase
    want = torch.tensor(0.3 * complex(math.cos(1.0), math.sin(1.0)), dtype=torch.complex64)
    assert torch.equal(t[~clear], want.expand(3)) and torch.equal(t[clear], torch.ones(3, dtype=torch.complex64))
    assert L.attenuatedPSM(geo.bool()).dtype == torch.complex64       # any dtype with a notion of non-zero
    assert torch.equal(L.attenuatedPSM(geo.float()), L.attenuatedPSM(geo))


def test_alternating_psm_values(L):
    geo = torch.tensor([[1, 1, 0], [1, 0, 1]], dtype=torch.int16)
    sh = torch.tensor([[0, 1, 1], [0, 0, 3]], dtype=torch.int16)
    t = L.alternatingPSM(geo, sh)
    assert t.dtype == torch.complex64 and t.shape == geo.shape
    assert torch.equal(t, torch.tensor([[1, -1, 0], [1, 0, -1]], dtype=torch.complex64))   # imaginary parts exactly 0
    t = L.alternatingPSM(geo, sh, math.pi / 2)
    assert torch.equal(t, torch.tensor([[1, 1j, 0], [1, 0, 1j]], dtype=torch.complex64))
    t = L.alternatingPSM(geo, sh, 0.5)
    e = complex(math.cos(0.5), math.sin(0.5))
    assert torch.equal(t, torch.tensor([[1, e, 0], [1, 0, e]], dtype=torch.complex64))
    with pytest.raises(ValueError):
        L.alternatingPSM(geo, sh[:, :2])


@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), float("inf")])
def test_attenuated_psm_rejects_a_transmittance_outside_0_1(L, bad):
    with pytest.raises(ValueError):
        L.attenuatedPSM(torch.ones(4, 4), bad)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_helpers_reject_a_non_finite_phase(L, bad):
    with pytest.raises(ValueError):
        L.attenuatedPSM(torch.ones(4, 4), 0.06, bad)
    with pytest.raises(ValueError):
        L.alternatingPSM(torch.ones(4, 4), torch.ones(4, 4), bad)


def test_mask_with_transmission_attributes(L):
    geo = torch.zeros(32, 32, dtype=torch.int16)
    geo[4:20, 8:12] = 1
    t = L.attenuatedPSM(geo)
    m = L.Mask(pixelSize=20, device=CPU, transmission=t)
    assert m.transmission.dtype == torch.complex64 and m.transmission.device == CPU and torch.equal(m.transmission, t)
    assert m.geometry.dtype == torch.int16 and torch.equal(m.geometry, torch.ones(32, 32, dtype=torch.int16))   # 6 %: no zero
    assert (m.pixelNumber, m.pixelSize, m.deltaK, m._pixelBound, m._Kbound) == (32, 20, 4 / 32, 320.0, 2.0)
    # a real floating transmission (a grey mask) is taken as it is; the footprint is where it is non-zero
    grey = torch.zeros(16, 16, dtype=torch.float64)
    grey[2:5, 3:9] = 0.375
    m = L.Mask(device=CPU, transmission=grey)
    assert m.transmission.dtype == torch.complex64 and torch.equal(m.transmission, grey.to(torch.complex64))
    assert torch.equal(m.geometry, (grey != 0).to(torch.int16)) and m.pixelNumber == 16 and m.pixelSize == 25
    # the alternating mask: opaque pixels are outside the footprint
    m = L.Mask(device=CPU, transmission=L.alternatingPSM(geo, torch.ones_like(geo)))
    assert torch.equal(m.geometry, geo)


def test_mask_with_transmission_shape_errors(L):
    S = L.imageformation.ShapeError
    sq = torch.ones(8, 8, dtype=torch.complex64)
    for bad in (torch.ones(8, 6), torch.ones(8), torch.ones(2, 8, 8), torch.ones(0, 0), torch.ones(8, 8, dtype=torch.int16),
                torch.ones(8, 8, dtype=torch.bool), [[1.0, 0.0], [0.0, 1.0]], "mask"):
        with pytest.raises(S):
            L.Mask(device=CPU, transmission=bad)
    with pytest.raises(S):
        L.Mask(torch.ones(8, 8, dtype=torch.int16), 25, CPU, transmission=sq)
    with pytest.raises(S):
        L.Mask(torch.ones(8, 8, dtype=torch.int16), 25, CPU, sq)          # ... also positionally


def test_mask_without_transmission_is_what_it_was(L, capsys):
    geo = torch.zeros(32, 32, dtype=torch.float32)
    geo[3:9, 5:7] = 1
    m = L.Mask(geo, 10, CPU)
    assert m.transmission is None
    assert m.geometry.dtype == torch.int16 and torch.equal(m.geometry, geo.to(torch.int16))
    assert (m.pixelNumber, m.pixelSize, m.deltaK, m._pixelBound, m._Kbound) == (32, 10, 4 / 32, 160.0, 2.0)
    # the reference's demo fallback: never raises, prints its notice, 64 x 64 four-bar pattern
    demo = torch.zeros(64, 64, dtype=torch.int16)
    for c0 in (16, 25, 34, 43):
        demo[9:55, c0:c0 + 4] = 1
    capsys.readouterr()
    for bad in (None, torch.ones(8, 6), "mask"):
        m = L.Mask(bad, 25, CPU)
        assert "Using demo instead" in capsys.readouterr().out
        assert m.transmission is None and m.pixelNumber == 64 and torch.equal(m.geometry, demo)
    with pytest.raises(NotImplementedError):
        m.fraunhofer(193.0, False)
    with pytest.raises(RuntimeError):                                  # no CPU fallback, as before
        m.fraunhofer(193.0, True)


def test_transmission_mask_has_no_cpu_fallback_either(L):
    m = L.Mask(device=CPU, transmission=torch.ones(64, 64, dtype=torch.complex64))
    with pytest.raises(RuntimeError):
        m.fraunhofer(193.0, True)


def test_helpers_are_exported(L):
    for name in ("attenuatedPSM", "alternatingPSM"):
        assert name in L.__all__ and callable(getattr(L, name))
