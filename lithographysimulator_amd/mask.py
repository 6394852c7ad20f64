"""Mask: same object API as the reference's mask.py, spectrum computed by HIP kernels."""
import cmath
import math

import torch

from . import _native as nat


def _phasor(phase, what):
    """exp(i phase) with multiples of pi/2 exact: pi -> (-1, 0), not (-1, 1.2e-16)."""
    phase = float(phase)
    if not math.isfinite(phase):
        raise ValueError(f"{what}: the phase must be finite; got {phase}")
    q = phase / (math.pi / 2)
    if abs(q - round(q)) < 1e-12:                                           # 3 * math.pi / 2 is one ulp off 3 quarter turns
        return (1 + 0j, 1j, -1 + 0j, -1j)[int(round(q)) % 4]
    return cmath.exp(1j * phase)


def attenuatedPSM(geometry: torch.Tensor, transmittance: float = 0.06, phase: float = math.pi) -> torch.Tensor:
    """Complex transmission (complex64, geometry's shape and device) of an attenuated phase-shift mask: 1 where
    geometry != 0 (clear), sqrt(transmittance) exp(i phase) elsewhere (the absorber; 6 % and pi: MoSi at 193 nm)."""
    transmittance = float(transmittance)
    if not 0.0 <= transmittance <= 1.0:                                     # NaN fails both comparisons
        raise ValueError(f"attenuatedPSM: the transmittance is an intensity ratio in [0, 1]; got {transmittance}")
    absorber = math.sqrt(transmittance) * _phasor(phase, "attenuatedPSM")
    geometry = torch.as_tensor(geometry)
    t = torch.full(geometry.shape, absorber, dtype=torch.complex64, device=geometry.device)
    t[geometry != 0] = 1
    return t


def alternatingPSM(geometry: torch.Tensor, shifter: torch.Tensor, phase: float = math.pi) -> torch.Tensor:
    """Complex transmission (complex64) of an alternating-aperture mask: clear pixels (geometry != 0) transmit 1, those
    under the shifter (shifter != 0) exp(i phase); everything else is opaque."""
    shifted = _phasor(phase, "alternatingPSM")
    geometry = torch.as_tensor(geometry)
    shifter = torch.as_tensor(shifter).to(geometry.device)
    if shifter.shape != geometry.shape:
        raise ValueError(f"alternatingPSM: geometry {tuple(geometry.shape)} and shifter {tuple(shifter.shape)} differ in shape")
    clear = geometry != 0
    t = torch.zeros(geometry.shape, dtype=torch.complex64, device=geometry.device)
    t[clear] = 1
    t[clear & (shifter != 0)] = shifted
    return t


class Mask:
    """Mirror of reference mask.py:3-90 (class Mask).  `transmission` (no reference counterpart) makes it a phase-shift
    or grey mask: a complex field transmission per pixel instead of the 0 / 1 geometry."""

    def __init__(self, geometry: torch.Tensor = None, pixelSize: int = 25, device: torch.device = None,
                 transmission: torch.Tensor = None):
        self.device = nat.pick_device(device, "mask")                      # mask.py:7-18
        self.transmission = None
        if transmission is not None:
            # a new argument: the reference's "never raises" demo fallback below does not apply to it
            from .imageformation import ShapeError
            if geometry is not None:
                raise ShapeError("Mask takes a geometry or a transmission, not both")
            if (type(transmission) is not torch.Tensor or transmission.dim() != 2
                    or transmission.shape[0] != transmission.shape[1] or transmission.numel() == 0
                    or not (transmission.is_floating_point() or transmission.is_complex())):
                what = (f"{tuple(transmission.shape)} {transmission.dtype}" if type(transmission) is torch.Tensor
                        else type(transmission).__name__)
                raise ShapeError(f"transmission must be a square 2-D floating or complex tensor; got {what}")
            self.transmission = transmission.to(dtype=torch.complex64, device=self.device).contiguous()
            self.geometry = (self.transmission != 0).to(torch.int16)       # the footprint, for plotting
            self.pixelNumber = self.geometry.size()[0]
        elif (geometry is None or type(geometry) is not torch.Tensor) or (
                len(geometry.size()) != 2 or geometry.size()[0] != geometry.size()[1]):
            # mask.py:20-27: never raises, falls back to the 64x64 four-bar demo
            print("Mask not defined or invalid. Check that it is a torch tensor and is square. Using demo instead.")
            self.pixelNumber = 64
            self.geometry = torch.zeros((64, 64), dtype=torch.int16, device=self.device)
            for c0 in (16, 25, 34, 43):
                self.geometry[9:55, c0:c0 + 4] = 1
        else:
            self.geometry = geometry.to(dtype=torch.int16, device=self.device)
            self.pixelNumber = self.geometry.size()[0]
        self.pixelSize = pixelSize
        self._pixelBound = self.pixelNumber / 2 * self.pixelSize
        self.deltaK = 4 / self.pixelNumber                                  # mask.py:34
        self._Kbound = self.pixelNumber / 2 * self.deltaK

    def fraunhofer(self, wavelength, fft: bool) -> torch.Tensor:
        """mask.py:37-40.  Only the FFT formulation is built (the O(pn^4) direct integral of
        mask.py:41-61 is outside the hot path)."""
        if not fft:
            raise NotImplementedError("the direct (non-FFT) Fraunhofer integral is not part of the MI355X engine; "
                                      "call fraunhofer(wavelength, True)")
        epsilon, N = self.calculateEpsilonN(self.deltaK, self.pixelSize, wavelength)
        return self._ffFraunhofer(epsilon, N)

    def _nearest2SqInt(self, input: float):
        """mask.py:63-65."""
        return nat.epsilon_n(1.0, 1.0, float(input))[1]

    def calculateEpsilonN(self, deltaK, pixelSize, wavelength):
        """mask.py:67-72; also callable unbound as Mask.calculateEpsilonN(self=mask, ...)."""
        return nat.epsilon_n(deltaK, pixelSize, wavelength)

    def _ffFraunhofer(self, epsilon, N: int) -> torch.Tensor:
        """mask.py:74-90 as one C-ABI call (bilinear scale, centred forward DFT, crop)."""
        dev = nat.require_gpu(self.device)
        pn = self.pixelNumber
        spec = torch.empty((pn, pn), dtype=torch.complex64, device=dev)
        ws = nat.workspace(dev, pn, N)
        if self.transmission is not None:
            t = self.transmission.contiguous()
            with torch.cuda.device(dev):
                nat.check(nat.lib().litho_mask_spectrum_complex(nat.ptr(t), pn, float(epsilon), int(N), nat.ptr(spec),
                                                                nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)),
                          "litho_mask_spectrum_complex")
            return spec
        geo = self.geometry.contiguous()
        with torch.cuda.device(dev):
            nat.check(nat.lib().litho_mask_spectrum(nat.ptr(geo), pn, float(epsilon), int(N), nat.ptr(spec),
                                                    nat.ptr(ws), ws.numel(), nat.stream_ptr(dev)),
                      "litho_mask_spectrum")
        return spec
