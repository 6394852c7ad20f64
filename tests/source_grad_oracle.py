"""CPU restatement of the source-gradient definition (include/litho_abbe.h "Source gradients", lithographysimulator_amd/smo.py) in
float64, written from the formula and not from the kernel.  TEST INFRASTRUCTURE ONLY.

    F = O.centred_dft_matrix(pn, N),  E_s = F (torch.roll(P, (dy_s, dx_s), (0, 1)) . M) F^T
    sens[s] = sum_g sum_k sum_q G[g][q] |E_s of pupil g K + k|^2[q]

Tolerance.  The rule of tests/socs_grad_oracle.py, no new number: `sensitivities(..., dtype=complex64)` evaluates the same formula
in torch's CPU single precision and is compared with the float64 chain on exactly the GPU tests' cases (ORACLE_CASES;
test_source_grad_cpu.py::test_fp32_floor_of_the_sensitivity_formula prints and re-checks it).  Errors are normalised by
max_s |sens_s| and ||sens||_2.  Where the floor is below a quarter of helpers.TOL_IMAGE_MAX / TOL_IMAGE_L2 those are the bound,
otherwise four times the floor.  Measured over ORACLE_CASES:
    max_s |d sens| / max_s |sens| <= 7.4e-7,   ||d sens||_2 / ||sens||_2 <= 8.3e-7
(the largest at (256, 256), three groups, and at (1024, 1024)), both below a quarter of helpers.TOL_IMAGE_MAX (5e-6) and TOL_IMAGE_L2 (1.25e-6), so
the sensitivities are held to the project's image tolerances themselves.
G changes sign, so sens is a cancelling sum; relative to the sum without cancellation, sum_q |G| |E_s|^2, the same floor is
    max_s |d sens_s| / (sum_q |G| |E_s|^2) <= 3.8e-8.

Loop tolerances.  The same rule as ILT_FLOOR_LOSS / ILT_FLOOR_UPDATE for optimizeSource's device model: `SmoCase.model(dtype=
complex64)` is this file's whole chain (weights -> image, gradient on the image -> sensitivities) with the same dense matrices in
single precision, and test_source_grad_cpu.py::test_fp32_floor_of_the_source_loop compares the one-iteration loop on it with the
float64 chain on the device tests' cases (SMO_LOOP_CASES).  The resist sigmoid multiplies a relative image error by about
a_r . threshold = 25, so the bound is four times the loop's own floor:
    losses[0], losses[1]  relative 8.1e-8 -> bound 3.2e-7;   (w1 - w0) / (step max w0)  absolute 4.8e-6 -> bound 1.9e-5
(the update is the gradient over its peak, and its floor holds eps32 max(w) / (step max(w)) = 1e-6 from the fp32 subtraction
alone; step 1 / 16).  A structural error -- a roll in the other direction, a
dropped plane, the quotient rule's second term missing -- shows at order 0.1 ... 1."""
import torch

import socs_grad_oracle as GO
from helpers import TOL_IMAGE_L2, TOL_IMAGE_MAX
from oracle import abbe_oracle as O

C128 = torch.complex128
# the measured complex64 floors (see the head of the file) and the bounds chosen from them
FP32_FLOOR_MAX, FP32_FLOOR_L2, FP32_FLOOR_ABS = 7.4e-7, 8.3e-7, 3.8e-8
TOL_SENS_MAX, TOL_SENS_L2 = GO._bound(FP32_FLOOR_MAX, TOL_IMAGE_MAX), GO._bound(FP32_FLOOR_L2, TOL_IMAGE_L2)
SMO_FLOOR_LOSS, SMO_FLOOR_UPDATE = 8.1e-8, 4.8e-6
TOL_SMO_LOSS, TOL_SMO_UPDATE = 4 * SMO_FLOOR_LOSS, 4 * SMO_FLOOR_UPDATE


def _planes(pupils, G, K):
    P = torch.as_tensor(pupils)
    pn = P.shape[-1]
    P = P.reshape(-1, K, pn, pn)
    return P, torch.as_tensor(G).reshape(P.shape[0], 1, pn, pn), pn


def point_intensities(pupils, M, shifts, N, K=1, dtype=C128):
    """|E_s|^2 summed over the K pupils of a plane, one per source point: a generator of [groups,pn,pn] real tensors."""
    P = torch.as_tensor(pupils)
    pn = P.shape[-1]
    P = P.reshape(-1, K, pn, pn).to(dtype)
    F = O.centred_dft_matrix(pn, N, dtype=dtype)
    Mc = torch.as_tensor(M).to(dtype)
    for dy, dx in torch.as_tensor(shifts).tolist():
        E = F @ (torch.roll(P, shifts=(int(dy), int(dx)), dims=(-2, -1)) * Mc) @ F.T
        yield (E.real ** 2 + E.imag ** 2).sum(dim=1)


def sensitivities(pupils, M, shifts, N, G, K=1, dtype=C128, absolute=False):
    """sens [S] of the head of the file (float64, or float32 for dtype complex64); `absolute`: sum_q |G| |E_s|^2 instead."""
    real = torch.float64 if dtype == C128 else torch.float32
    P, G3, pn = _planes(pupils, G, K)
    G3 = G3[:, 0].to(real)
    if absolute:
        G3 = G3.abs()
    return torch.stack([(G3 * I).sum() for I in point_intensities(pupils, M, shifts, N, K, dtype)])


def weighted_image(pupil, M, shifts, weights, N):
    """float64 I_w = sum_s w_s |E_s|^2 from oracle.abbe_oracle's single-point field (field_closed_form, the restatement of the
    reference's calculateFFTAerial on the rolled pupil)."""
    image = torch.zeros(tuple(M.shape), dtype=torch.float64)
    for (dy, dx), w in zip(torch.as_tensor(shifts).tolist(), torch.as_tensor(weights).tolist()):
        E = O.field_closed_form(pupil, M, dy, dx, N)
        image += w * (E.real ** 2 + E.imag ** 2)
    return image


# ---- the loop's arithmetic, from optimizeSource's docstring --------------------------------------------------------------------
def smo_loss(image, target, threshold, dose, resistSteepness):
    """optimizeMask's loss, word for word: GO.ilt_loss."""
    return GO.ilt_loss(image, target, threshold, dose, resistSteepness)


def smo_grad_image(image, target, threshold, dose, resistSteepness):
    return GO.ilt_grad_image(image, target, threshold, dose, resistSteepness)


def normalised_gradient(g, G, image_n, wsum):
    """(g_s - <G, I>) / sum(w) with I the normalised image, float64."""
    return (torch.as_tensor(g).double() - float((torch.as_tensor(G).double() * torch.as_tensor(image_n).double()).sum())) / float(wsum)


def projected_update(w, grad, step):
    """max(w - step max(w) grad / max|grad|, 0), float64."""
    w, grad = torch.as_tensor(w).double(), torch.as_tensor(grad).double()
    return torch.clamp(w - float(step) * w.max() * grad / grad.abs().max(), min=0.0)


# ---- case builders -----------------------------------------------------------------------------------------------------------
def shift_list(pn, n=8):
    """(dy,dx) int32 [n,2]: (0,0); a shift beyond +-pn; negative; +-pn/2; one that wraps the pupil's disc (radius pn/4) around
    the grid; a duplicate of the third; an edge in one axis only; beyond -2 pn."""
    full = [(0, 0), (pn + 5, -pn - 7), (-3, 2), (pn // 2, -pn // 2), (pn // 4 + 3, 1), (-3, 2), (1, -pn // 2), (-2 * pn - 1, 3)]
    return torch.tensor(full[:n], dtype=torch.int32)


_cases = {}


def case(pn, N, groups=1, K=1, points=8):
    """(pupils complex64 [groups K,pn,pn], M complex64 [pn,pn], G fp32 [groups,pn,pn], shifts int32 [points,2]): random complex
    pupils on the disc of radius pn/4 (no symmetry, another one per plane and k), a random complex spectrum that is not
    Hermitian, a G of both signs with a block of exact zeros, another one per group."""
    key = (pn, N, groups, K, points)
    if key not in _cases:
        g = torch.Generator().manual_seed(31 * pn + N + 7 * groups + K)
        r = torch.arange(pn, dtype=torch.float64) - pn // 2
        disc = ((r[:, None] ** 2 + r[None, :] ** 2) <= (pn / 4) ** 2).to(torch.float32)
        P = torch.view_as_complex(torch.randn((groups * K, pn, pn, 2), generator=g, dtype=torch.float32)) * disc
        M = torch.view_as_complex(torch.randn((pn, pn, 2), generator=g, dtype=torch.float32))
        _cases[key] = (P.contiguous(), M.contiguous(), GO.random_G((groups, pn, pn), pn + N + groups), shift_list(pn, points))
    return _cases[key]


# (pn, N, groups, K, points): every line shape of plane_fft.hpp's LineShape -- the one-thread line at 16 (64 lines per workgroup),
# several lines per workgroup (32 ... 512), one workgroup per line (1024) -- and every m = N / pn regime: 1, 1 < m <= pn, m > pn
ORACLE_CASES = [(16, 16, 1, 1, 8), (16, 64, 1, 1, 8), (16, 512, 1, 1, 8), (32, 64, 1, 1, 8), (64, 64, 1, 1, 8), (128, 256, 1, 1, 8),
                (256, 256, 1, 1, 8), (1024, 1024, 1, 1, 2),
                (16, 16, 2, 1, 8), (32, 64, 3, 1, 8), (64, 64, 2, 1, 8), (256, 256, 3, 1, 4),
                (16, 64, 1, 3, 8), (64, 128, 2, 3, 8)]

_refs = {}


def reference(*key):
    """The float64 sensitivities of a case, computed once and shared."""
    if key not in _refs:
        P, M, G, sh = case(*key)
        _refs[key] = sensitivities(P, M, sh, key[1], G, K=key[3])
    return _refs[key]


# ---- the loop on this file's chain ---------------------------------------------------------------------------------------------
SMO_DOSE, SMO_STEP = 1.1, 0.0625
SMO_LOOP_CASES = [(pn, planes, normalize) for pn in (32, 64) for planes in (1, 2) for normalize in (True, False)]
_smo = {}


def smo_candidates(pn):
    """Six candidate pixels in argwhere order, their (dy,dx) = pixel - pn/2 among them: the top row (dy = -pn/2, which wraps the
    pupil's disc of radius pn/4 around the grid), the centre (0,0), the bottom row and off-axis points of both signs."""
    h = pn // 2
    return [(0, h + 1), (h - 3, h + 2), (h, h), (h + 1, pn // 4 - 4), (h + 5, h - 2), (pn - 1, h)]


class SmoCase:
    """One setting of optimizeSource on this file's chain: the six source points of smo_candidates (a wrapping one included),
    random disc pupils (one plane or two), the spectrum of an attenuated phase-shift Bernoulli mask at the 'shrink' pixel size of
    socs_grad_oracle.epsilon_regimes, seeded weights in (0.5, 1.5), a seeded Bernoulli target, the threshold at the median of
    dose . image(w0) (normalised or not), resistSteepness 25 / threshold."""

    def __init__(self, pn, planes, normalize):
        from lithographysimulator_amd.mask import attenuatedPSM
        from lithographysimulator_amd.synthetic import bernoulli_mask
        self.pn, self.planes, self.normalize = pn, planes, normalize
        self.ps, self.eps, self.N = GO.epsilon_regimes(pn)["shrink"]
        pixels = smo_candidates(pn)
        self.pupils = case(pn, self.N, planes, 1, len(pixels))[0]
        self.pupils = self.pupils if planes > 1 else self.pupils[0]
        self.t = attenuatedPSM(bernoulli_mask(pn)).to(torch.complex64)
        self.Pp = GO.postprocess_matrix(pn, self.eps)
        self.n_out = self.Pp.shape[0]
        g = torch.Generator().manual_seed(9000 + 10 * pn + planes)
        self.w0 = (0.5 + torch.rand(len(pixels), generator=g, dtype=torch.float64)).to(torch.float32)
        self.candidates = torch.zeros((pn, pn), dtype=torch.float32)
        for (r, c), w in zip(pixels, self.w0.tolist()):
            self.candidates[r, c] = w
        self.shifts = O.source_shifts(self.candidates != 0, pn)
        assert self.shifts.tolist() == [[r - pn // 2, c - pn // 2] for r, c in pixels]
        self.target = (torch.rand((self.n_out, self.n_out), generator=g, dtype=torch.float64) > 0.5).to(torch.float32)
        self.M = GO.spectrum_complex(self.t, self.eps, self.N).to(torch.complex64)
        if planes > 1:
            # the planes of a focus stack share their dose: each random pupil is scaled to the first one's median image
            med = self.model()[0](self.w0.double()).flatten(1).median(dim=1).values
            self.pupils = (self.pupils * torch.sqrt(med[0] / med).to(torch.float32)[:, None, None]).contiguous()
        image0 = self.model()[0](self.w0.double())
        if normalize:
            image0 = image0 / float(self.w0.double().sum())
        self.threshold = SMO_DOSE * float(image0.median())
        self.a_r = 25.0 / self.threshold
        self._reference = None

    def model(self, dtype=C128):
        """(imager, sensitivity) on the dense chain: w -> Pp (sum_s w_s |E_s|^2) Pp^T per plane; g -> <Pp^T g Pp, |E_s|^2>."""
        real = torch.float64 if dtype == C128 else torch.float32
        Pp = self.Pp.to(real)
        I = torch.stack(list(point_intensities(self.pupils, self.M, self.shifts, self.N, 1, dtype)))     # [S,planes,pn,pn]
        squeeze = self.planes == 1

        def imager(w):
            raw = (torch.as_tensor(w).to(real)[:, None, None, None] * I).sum(dim=0)
            out = Pp @ raw @ Pp.T
            return out[0] if squeeze else out

        def sensitivity(g):
            graw = Pp.T @ torch.as_tensor(g).to(real).reshape(self.planes, self.n_out, self.n_out) @ Pp
            return (graw[None] * I).sum(dim=(1, 2, 3))

        return imager, sensitivity

    def loop(self, imager=None, sensitivity=None, dev=None, **kw):
        """optimizeSource through the public call with this setting, one iteration from w0: on the given hooks, or (dev given) on
        the device model."""
        from lithographysimulator_amd import optimizeSource
        t, P = (None, None) if dev is None else (self.t.to(dev), self.pupils.to(dev))
        return optimizeSource(self.target, t, P, self.candidates, self.ps, 4 / self.pn, 193.0, self.threshold, dose=SMO_DOSE,
                              iterations=1, step=SMO_STEP, normalize=self.normalize, imager=imager, sensitivity=sensitivity, **kw)

    def reference(self):
        if self._reference is None:
            self._reference = self.loop(*self.model())
        return self._reference


def smo_case(pn, planes, normalize):
    key = (pn, planes, normalize)
    if key not in _smo:
        _smo[key] = SmoCase(pn, planes, normalize)
    return _smo[key]


def update_of(case, result):
    """(w1 - w0) / (step max w0) of a one-iteration result whose best iterate is the first update, float64."""
    assert result.best == 1 and result.losses[1] < result.losses[0], result.losses
    return (result.weights.detach().cpu().double() - case.w0.double()) / (SMO_STEP * float(case.w0.max()))
