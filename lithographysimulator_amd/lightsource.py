"""LightSource: same object API as the reference's lightsource.py, sampled by a HIP kernel
that reproduces the reference's fp16 sigma-grid arithmetic."""
import ctypes

import torch

from . import _native as nat


class LightSource:
    """Mirror of reference lightsource.py:3-73."""

    def __init__(self, sigmaIn=0, sigmaOut=0.6, pixelNumber: int = 64, NA=0.7, shiftX=0, shiftY=0,
                 device: torch.device = None):
        self.device = nat.pick_device(device, "light source")              # lightsource.py:7-18
        self.pixelNumber = pixelNumber
        self.NA = NA
        self.sigmaInner = sigmaIn
        self.sigmaOuter = sigmaOut
        self.shiftX = shiftX
        self.shiftY = shiftY

    def _bitmap(self, kind, count, rotation):
        dev = nat.require_gpu(self.device)
        pn = int(self.pixelNumber)
        out = torch.empty((pn, pn), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            nat.check(nat.lib().litho_source_bitmap(kind, float(self.sigmaInner), float(self.sigmaOuter), pn,
                                                    float(self.shiftX), float(self.shiftY), int(count),
                                                    float(rotation), nat.ptr(out), nat.stream_ptr(dev)),
                      "litho_source_bitmap")
        return out

    def generateAnnular(self) -> torch.Tensor:
        """lightsource.py:34-50: int64 0/1 bitmap [pn,pn]."""
        return self._bitmap(0, 1, 0.0)

    def generateQuasar(self, count, rotation) -> torch.Tensor:
        """lightsource.py:52-73."""
        return self._bitmap(1, count, rotation)


def _compact_source(lightsource, pixelNumber, weighted, on_host):
    """The compaction under the four functions below: (shifts [pn*pn,2] int32, weights [pn*pn] float32 or None, count), both
    lists at their capacity with the first S rows written.  weighted=False: `lightsource` is the reference's bitmap, taken as
    int64, every non-zero pixel lit (litho_source_compact; no weights).  weighted=True: a real map, taken as float32, the pixels
    with w > 0 lit (litho_source_compact_weighted).  on_host=True: the call waits and count is S as an int; False: no
    read-back, count is the 1-element int32 device tensor that holds S."""
    dev = nat.require_gpu(lightsource.device)
    pn = int(pixelNumber)
    if lightsource.dim() != 2 or lightsource.shape[0] != pn or lightsource.shape[1] != pn:
        # the reference silently mis-shifts when the source grid differs from the mask's
        raise ValueError(f"the source {'map' if weighted else 'bitmap'} must be [{pn},{pn}] (the mask's pixelNumber); got "
                         f"{tuple(lightsource.shape)}")
    if weighted and lightsource.is_complex():
        raise ValueError("a weighted source map holds real intensity weights; got a complex tensor")
    src = lightsource.to(torch.float32 if weighted else torch.int64).contiguous()
    shifts = torch.empty((pn * pn, 2), dtype=torch.int32, device=dev)
    weights = torch.empty(pn * pn, dtype=torch.float32, device=dev) if weighted else None
    scratch = torch.empty(pn + 1, dtype=torch.int32, device=dev)
    S = ctypes.c_int64(0)
    count_host = ctypes.byref(S) if on_host else None
    with torch.cuda.device(dev):
        if weighted:
            nat.check(nat.lib().litho_source_compact_weighted(nat.ptr(src), pn, nat.ptr(shifts), nat.ptr(weights), pn * pn,
                                                              nat.ptr(scratch), count_host, nat.stream_ptr(dev)),
                      "litho_source_compact_weighted")
        else:
            nat.check(nat.lib().litho_source_compact(nat.ptr(src), pn, nat.ptr(shifts), pn * pn, nat.ptr(scratch), count_host,
                                                     nat.stream_ptr(dev)), "litho_source_compact")
    return shifts, weights, S.value if on_host else scratch[pn:pn + 1]


def sourceShiftsAsync(lightsource: torch.Tensor, pixelNumber: int):
    """The same compaction without the host read-back: returns (shifts [pn*pn,2] int32 with only the first S rows
    written, count = 1-element int32 device tensor holding S).  For abbeIntensity(..., count=...)."""
    shifts, _, count = _compact_source(lightsource, pixelNumber, weighted=False, on_host=False)
    return shifts, count


def sourceShifts(lightsource: torch.Tensor, pixelNumber: int) -> torch.Tensor:
    """imageformation.py:59: (argwhere(lightsource) - pn//2).int(), row-major, as int32 [S,2]
    on the bitmap's device."""
    shifts, _, S = _compact_source(lightsource, pixelNumber, weighted=False, on_host=True)
    return shifts[:S]


def sourceWeightsAsync(lightsource: torch.Tensor, pixelNumber: int):
    """Compaction of a WEIGHTED source -- a real map [pn,pn] whose values are per-point intensity weights (lit = w > 0) --
    without a host read-back: (shifts [pn*pn,2] int32, weights [pn*pn] float32, count), only the first S rows written,
    count = 1-element int32 device tensor holding S.  For abbeIntensity(..., weights=..., count=...).  The reference has no
    counterpart: its source is a bitmap (imageformation.py:59)."""
    return _compact_source(lightsource, pixelNumber, weighted=True, on_host=False)


def sourceWeights(lightsource: torch.Tensor, pixelNumber: int):
    """(shifts int32 [S,2], weights float32 [S]) of a weighted source map, row-major like sourceShifts; a map of exact
    0 / 1 values gives sourceShifts' list and weights of one."""
    shifts, weights, S = _compact_source(lightsource, pixelNumber, weighted=True, on_host=True)
    return shifts[:S], weights[:S]
