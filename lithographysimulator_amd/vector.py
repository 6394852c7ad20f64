"""Vector (polarised, high-NA) Hopkins imaging; no reference counterpart (include/litho_abbe.h).

Above NA ~ 0.6 the image is formed by three field components, and the polarisation of every source point decides the contrast.
With direction cosines alpha = NA sigma_x / n, beta = NA sigma_y / n, gamma = sqrt(1 - alpha^2 - beta^2) in the image medium of
index n, the factor M_cj takes polarisation component j in {x, y} at the mask onto field component c in {x, y, z} at the wafer,

    M_xx = 1 - alpha^2/(1+gamma)   M_xy = M_yx = -alpha beta/(1+gamma)   M_yy = 1 - beta^2/(1+gamma)   M_zx = -alpha   M_zy = -beta,

and the six planes of a pupil P are Q_cj = P . M_cj (plane t = 2 c + j; `vectorPupils`, litho_vector_pupils).  A source point
carries a real symmetric 2 x 2 coherency, given as three maps W_xx, W_yy, W_xy on the source grid (`sourcePolarization`).  The
image is a sum of scalar Abbe sums, one per field component and pure polarisation state, so its transmission cross coefficient

    T x = sum_c sum_j Q_cj (*) ( sum_j' W_jj' . (Q_cj' (star) x) )

is a sum of scalar-shaped ones, Hermitian PSD, and factors into SOCS kernels as before: `vectorSocsKernels` returns an ordinary
SOCSKernels, and hopkinsIntensity / hopkinsImage / hopkinsFields / hopkinsGradient / optimizeMask / correctLayout(socs=) run
their K fields with polarisation included.  The operator on the device is litho_tcc_apply_vector: 14 pn^2 transforms per vector.

`vectorAbbeIntensity` is the on-device truth for a UNIFORM polarisation: 3 or 6 effective pupils through the unchanged Abbe
engine.  A resist film stack under the image medium changes only the six planes: film.py (`FilmStack`, `filmPupils`,
`vectorSocsKernels(film=, depths=, depthWeights=)`).  Out of scope: thick-mask polarisation effects, TCC interpolation."""
import ctypes
import math
from functools import partial

import numpy as np
import torch

from . import _native as nat
from . import socs as _socs

MODES = ("x", "y", "te", "tm", "unpolarized")
PLANES = 6


def _check_optics(who, NA, mediumIndex):
    NA, n = float(NA), float(mediumIndex)
    if not (math.isfinite(NA) and math.isfinite(n)) or not 0.0 < NA < n:
        raise ValueError(f"{who}: 0 < NA < mediumIndex is required; got NA {NA}, index {n}")
    return NA, n


def _defocus_list(who, defocus, wavelength):
    """(float64 [planes] or None, given as a list)."""
    if defocus is None:
        return None, False
    if wavelength is None or not float(wavelength) > 0.0:
        raise ValueError(f"{who}: defocus needs a positive wavelength")
    if isinstance(defocus, torch.Tensor):
        defocus = defocus.detach().cpu().numpy()
    z = np.asarray(defocus, dtype=np.float64)
    if z.ndim > 1 or z.size < 1 or not np.isfinite(z).all():
        raise ValueError(f"{who}: defocus must be a finite value or a non-empty list of them (nm)")
    return np.atleast_1d(z).copy(), z.ndim == 1


def _pupil_planes(who, pupilF, zs, as_list):
    if not isinstance(pupilF, torch.Tensor) or pupilF.dim() not in (2, 3) or pupilF.shape[-1] != pupilF.shape[-2]:
        raise ValueError(f"{who}: pupilF must be [pn,pn] or [planes,pn,pn]; got {tuple(getattr(pupilF, 'shape', ()))}")
    pn = int(pupilF.shape[-1])
    pp = int(pupilF.shape[0]) if pupilF.dim() == 3 else 1
    zp = int(zs.shape[0]) if zs is not None else 1
    if pp < 1 or (pp != zp and pp != 1 and zp != 1):
        raise ValueError(f"{who}: {pp} pupil planes and {zp} defocus values: the lengths must agree, or one of them be 1")
    return pn, pp, max(pp, zp), pupilF.dim() == 3 or as_list


def _host_vector_pupils(P, NA, n, radiometric, zs, wavelength):
    """The six planes in float64 torch on the host, complex64 [planes,6,pn,pn].  Only for vectorSocsKernels(applier=) with a
    pupil that does not live on a GPU, where the host algebra needs the planes' support and trace; vectorPupils itself runs
    litho_vector_pupils and nothing else."""
    planes, pn = P.shape[0], P.shape[-1]
    k = torch.arange(pn, dtype=torch.float64) - pn // 2
    a = (NA * (k * 4.0 / pn) / n)[None, :].expand(pn, pn)
    b = (NA * (k * 4.0 / pn) / n)[:, None].expand(pn, pn)
    s = a * a + b * b
    ok = s < 1.0
    g = torch.sqrt(torch.where(ok, 1.0 - s, torch.ones_like(s)))
    d = 1.0 / (1.0 + g)
    M = torch.stack([1.0 - a * a * d, -a * b * d, -a * b * d, 1.0 - b * b * d, -a, -b])
    if radiometric:
        M = M / torch.sqrt(g)
    M = M * ok
    z = torch.from_numpy(np.broadcast_to(zs, (planes,)).copy()) if zs is not None else torch.zeros(planes, dtype=torch.float64)
    phase = torch.exp(2j * math.pi * (n * z / float(wavelength or 1.0))[:, None, None] * (s * d * ok)[None])
    return ((P.to(torch.complex128) * phase)[:, None] * M[None]).to(torch.complex64)


def vectorPupils(pupilF, NA, mediumIndex=1.0, radiometric=False, defocus=None, wavelength=None):
    """The six planes Q_cj = P . M_cj of a pupil function on the device (litho_vector_pupils): complex64 [6,pn,pn], plane
    t = 2 c + j, or [planes,6,pn,pn] for a pupil stack [planes,pn,pn] or a `defocus` list.  `NA` < `mediumIndex`, the index of
    the image medium (1.44 for water at 193 nm).  `radiometric`: every factor times gamma^(-1/2).  `defocus` (nm, a value or one
    per plane; needs `wavelength`): the exact phase exp(+2 pi i n z (1 - gamma) / lambda) on top of whatever the pupil already
    carries.  A pupil stack and a defocus list have the same length, or one of them is a single plane.  pn even, >= 16."""
    NA, n = _check_optics("vectorPupils", NA, mediumIndex)
    zs, as_list = _defocus_list("vectorPupils", defocus, wavelength)
    pn, pp, planes, stacked = _pupil_planes("vectorPupils", pupilF, zs, as_list)
    if pn < 16 or pn & 1:
        raise ValueError(f"vectorPupils: pn must be even and >= 16; got {pn}")
    dev = nat.require_gpu(pupilF.device)
    P = pupilF.detach().to(torch.complex64).reshape(pp, pn, pn).expand(planes, pn, pn).contiguous()
    out = torch.empty((planes, PLANES, pn, pn), dtype=torch.complex64, device=dev)
    z = (ctypes.c_double * planes)(*np.broadcast_to(zs, (planes,)).tolist()) if zs is not None else None
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_vector_pupils(nat.ptr(P), planes, pn, NA, n, 1 if radiometric else 0, z,
                                                float(wavelength) if zs is not None else 0.0, nat.ptr(out), nat.stream_ptr(dev)),
                  "litho_vector_pupils")
    return out if stacked else out[0]


def _degree(who, degree):
    degree = float(degree)
    if not 0.0 <= degree <= 1.0:
        raise ValueError(f"{who}: degree of polarisation must lie in [0, 1]; got {degree}")
    return degree


def _is_map_pair(polarization):
    return (isinstance(polarization, (tuple, list)) and len(polarization) == 2
            and all(isinstance(e, (torch.Tensor, np.ndarray)) and np.ndim(e) == 2 for e in polarization))


def _direction_maps(who, polarization, pn, lit):
    """Unit vector (e_x, e_y) per source-grid point, float64 [pn,pn] each."""
    if isinstance(polarization, str):
        if polarization not in MODES:
            raise ValueError(f"{who}: polarization must be one of {', '.join(MODES)} or a pair of real maps (e_x, e_y); got "
                             f"{polarization!r}")
        k = torch.arange(pn, dtype=torch.float64) - pn // 2
        phi = torch.atan2(k[:, None].expand(pn, pn), k[None, :].expand(pn, pn))        # atan2(0, 0) = 0: TM = x, TE = y at d = 0
        one, zero = torch.ones((pn, pn), dtype=torch.float64), torch.zeros((pn, pn), dtype=torch.float64)
        return {"x": (one, zero), "y": (zero, one), "tm": (torch.cos(phi), torch.sin(phi)),
                "te": (-torch.sin(phi), torch.cos(phi)), "unpolarized": (one, zero)}[polarization]
    if not _is_map_pair(polarization):
        raise ValueError(f"{who}: polarization must be one of {', '.join(MODES)} or a pair of real maps (e_x, e_y)")
    ex, ey = (torch.as_tensor(e).detach().cpu() for e in polarization)
    if tuple(ex.shape) != (pn, pn) or tuple(ey.shape) != (pn, pn) or ex.is_complex() or ey.is_complex():
        raise ValueError(f"{who}: the polarisation maps must be real [{pn},{pn}]; got {tuple(ex.shape)}, {tuple(ey.shape)}")
    ex, ey = ex.to(torch.float64), ey.to(torch.float64)
    norm = torch.hypot(ex, ey)
    if not bool(torch.isfinite(norm).all()) or bool((norm[lit] == 0).any()):
        raise ValueError(f"{who}: a polarisation vector is not finite, or zero at a lit source point")
    norm = torch.where(norm > 0, norm, torch.ones_like(norm))
    return ex / norm, ey / norm


def sourcePolarization(lightsource, mode="unpolarized", degree=1.0):
    """The coherency maps (W_xx, W_yy, W_xy) of a source, float32 [3,pn,pn] on the host: the intensity weight map W (a bitmap
    lights its non-zero pixels with weight 1, a floating map carries the weights; the errors are socsKernels') times the
    coherency  degree . e e^T + (1 - degree)/2 . I  of every point.  `mode`: "x" e = (1,0); "y" e = (0,1); with
    phi = atan2(row - pn/2, col - pn/2), "tm" e = (cos phi, sin phi) and "te" e = (-sin phi, cos phi) (at the centre TM means
    x and TE means y); "unpolarized" is degree 0; or a pair of real maps (e_x, e_y), normalised per point."""
    pn = int(lightsource.shape[-1]) if isinstance(lightsource, torch.Tensor) and lightsource.dim() == 2 else 0
    W = _socs._weight_map(lightsource, pn)
    degree = 0.0 if isinstance(mode, str) and mode == "unpolarized" else _degree("sourcePolarization", degree)
    ex, ey = _direction_maps("sourcePolarization", mode, pn, W > 0)
    iso = (1.0 - degree) / 2.0
    return torch.stack([W * (degree * ex * ex + iso), W * (degree * ey * ey + iso), W * (degree * ex * ey)]).to(torch.float32)


class _VectorOperator:
    """X -> T X on the device (litho_tcc_apply_vector) for the six planes of one pupil, in chunks of vectors whose work buffer
    stays under `apply_bytes` (at least one vector per call).  The vectors are independent: chunking changes no bit."""

    def __init__(self, planes6, w_shifted, apply_bytes):
        self.qh = _socs._device_fft2(planes6.clone())
        self.w = w_shifted
        n = int(planes6.shape[-1])
        self.chunk = max(1, int(apply_bytes) // (PLANES * n * n * 8) - 1)

    def __call__(self, X):
        Y = torch.empty_like(X)
        J, n = int(X.shape[0]), int(X.shape[-1])
        b = min(self.chunk, J)
        lib = nat.lib()
        nbytes = int(lib.litho_tcc_apply_vector_work_bytes(b, n))
        work = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
        with torch.cuda.device(X.device):
            for c0 in range(0, J, b):
                nb = min(b, J - c0)
                nat.check(lib.litho_tcc_apply_vector(nat.ptr(self.qh), nat.ptr(self.w), nat.ptr(X[c0:c0 + nb]), nat.ptr(Y[c0:c0 + nb]),
                                                     nb, n, nat.ptr(work), nbytes, nat.stream_ptr(X.device)),
                          "litho_tcc_apply_vector")
        return Y


def vectorSocsKernels(pupilF, lightsource, NA, polarization="unpolarized", degree=1.0, mediumIndex=1.0, radiometric=False,
                      defocus=None, wavelength=None, kernels=64, oversample=16, iterations=2, seed=0, applier=None,
                      applyBytes=8 << 30, film=None, depths=None, depthWeights=None):
    """SOCS kernels of one optical setting with polarisation: an ordinary SOCSKernels for hopkinsIntensity and every other
    consumer.  `pupilF`, `lightsource`, `kernels`, `oversample`, `iterations`, `seed`, `applier` as socsKernels takes them (pn a
    power of two, 16 ... 4096); `NA`, `mediumIndex`, `radiometric`, `defocus`, `wavelength` as vectorPupils; `polarization`,
    `degree` as sourcePolarization.  A pupil stack or a defocus list is factored plane by plane (socs._factor_plane).

    The rank of the vector T is at most 3 S for a pure state at every lit point (three field components) and 5 S for a mixed
    one (M_xy = M_yx), S the number of lit points; J = min(kernels + oversample, that bound) -- above the rank the surplus
    directions are normalised rounding noise.  The masking box is that of the union support of the six planes.  `trace` is
    sum_jj' (sum W_jj') sum_c <Q_cj', Q_cj>, `captured` = sum_k lambda_k / trace, `weight_sum` = sum W.

    The device operator is litho_tcc_apply_vector, called on chunks of vectors so that its work buffer stays under `applyBytes`
    (48 (chunk + 1) pn^2 bytes; never less than one vector).  The vectors are independent, so chunking changes no bit.

    `film` (a FilmStack; film.py) images into the resist layer of a thin-film stack under the medium `mediumIndex` instead of
    into that medium: the planes are filmPupils' at `depths` (nm below the top of the resist layer, D of them; `wavelength` is
    then required, and `defocus` places best focus relative to the top of the stack).  Without `depthWeights` every (focus
    plane f, depth d) is a plane of the result, at index f D + d.  With `depthWeights` (D non-negative numbers, not all zero) the
    BULK operator X -> sum_d w_d T_d X is factored per focus plane -- support the union over depths, trace sum_d w_d trace_d,
    rank bound (3 or 5) S D, the operator D calls of the unchanged litho_tcc_apply_vector summed in ascending d -- and the
    result is an ordinary SOCSKernels whose image is sum_d w_d I(z_d): K fields per bulk image, not D K.  film=None is the
    code path below, untouched."""
    who = "vectorSocsKernels"
    NA, n = _check_optics(who, NA, mediumIndex)
    zs, as_list = _defocus_list(who, defocus, wavelength)
    if film is not None or depths is not None or depthWeights is not None:
        if film is None:
            raise ValueError(f"{who}: depths and depthWeights belong to a film stack; film is None")
        from .film import _film_socs_kernels
        return _film_socs_kernels(who, pupilF, lightsource, NA, n, polarization, degree, radiometric, zs, as_list, wavelength, film,
                                  depths, depthWeights, applyBytes, kernels=kernels, oversample=oversample, iterations=iterations,
                                  seed=seed, applier=applier)
    pn, pp, planes, stacked = _pupil_planes(who, pupilF, zs, as_list)
    pure = not (isinstance(polarization, str) and polarization == "unpolarized") and float(degree) == 1.0

    def planes_of(W, dev):
        pol = sourcePolarization(lightsource, polarization, degree)
        if dev.type == "cuda":
            Q = vectorPupils(pupilF.reshape(pp, pn, pn), NA, n, radiometric, zs, wavelength)
            Q = Q.expand(planes, PLANES, pn, pn) if Q.shape[0] != planes else Q
        else:
            P = pupilF.detach().to(torch.complex64).reshape(pp, pn, pn).expand(planes, pn, pn)
            Q = _host_vector_pupils(P, NA, n, radiometric, zs, wavelength)
        wsh = torch.fft.ifftshift(pol, dim=(-2, -1)).to(dev).contiguous()
        sxx, syy, sxy = pol.to(torch.float64).sum(dim=(1, 2)).tolist()
        for Qp in Q:
            Qp = Qp.contiguous()
            q = Qp.to(torch.complex128)
            gxx = float((q[0::2].abs() ** 2).sum())
            gyy = float((q[1::2].abs() ** 2).sum())
            gxy = float((q[0::2] * q[1::2].conj()).sum().real)
            yield (Qp != 0).any(dim=0), sxx * gxx + syy * gyy + 2.0 * sxy * gxy, partial(_VectorOperator, Qp, wsh, applyBytes)

    return _socs._factorise(who, pupilF.device, pn, planes, stacked, lightsource, 3 if pure else 5, planes_of, kernels=kernels,
                            oversample=oversample, iterations=iterations, seed=seed, applier=applier)


def _uniform_states(polarization, degree):
    """[(mu, e_x, e_y)] -- the one or two pure states of a coherency that is the same at every source point."""
    who = "vectorAbbeIntensity"
    if isinstance(polarization, str) and polarization in ("x", "y", "unpolarized"):
        ex, ey = (0.0, 1.0) if polarization == "y" else (1.0, 0.0)
        degree = 0.0 if polarization == "unpolarized" else _degree(who, degree)
    elif (isinstance(polarization, (tuple, list)) and len(polarization) == 2
          and all(isinstance(e, (int, float)) for e in polarization)):
        ex, ey = float(polarization[0]), float(polarization[1])
        norm = math.hypot(ex, ey)
        if not norm > 0.0 or not math.isfinite(norm):
            raise ValueError(f"{who}: the polarisation vector must be finite and non-zero")
        ex, ey, degree = ex / norm, ey / norm, _degree(who, degree)
    elif (isinstance(polarization, str) and polarization in MODES) or _is_map_pair(polarization):
        raise ValueError(f"{who}: a polarisation that varies over the source ({polarization if isinstance(polarization, str) else 'maps'}) "
                         "needs the fields, and the Abbe engine keeps |E|^2 only: image it through vectorSocsKernels and "
                         "hopkinsIntensity")
    else:
        raise ValueError(f"{who}: polarization must be 'x', 'y', 'unpolarized' or a pair of numbers (e_x, e_y); got {polarization!r}")
    states = [((1.0 + degree) / 2.0, ex, ey), ((1.0 - degree) / 2.0, -ey, ex)]       # degree e e^T + (1 - degree)/2 I
    return [s for s in states if s[0] > 0.0]


def vectorAbbeIntensity(maskFT, vectorPupils, shifts, N, polarization="unpolarized", degree=1.0, weights=None, out=None, plan=None,
                        options=None):
    """The vector Abbe sum on the device for a UNIFORM polarisation: raw fp32 intensity [pn,pn], or [planes,pn,pn] for
    `vectorPupils` [planes,6,pn,pn] (what vectorPupils returned).  The one or two pure states (mu_m, e_m) of the coherency give
    3 or 6 effective pupils sqrt(mu_m) (e_mx Q_cx + e_my Q_cy); they run as a pupil stack through the unchanged abbeIntensity
    (`shifts`, `weights`, `plan`, `options` as there) and litho_socs_fold sums them, per plane.  `polarization`: "x", "y",
    "unpolarized" or a pair of numbers (e_x, e_y); "te", "tm" and maps raise ValueError -- a per-point state needs the
    fields, which the engine does not keep (vectorSocsKernels images those).  `out`: accumulated into when given."""
    from .imageformation import ShapeError
    states = _uniform_states(polarization, degree)
    Q = vectorPupils
    if not isinstance(Q, torch.Tensor) or Q.dim() not in (3, 4) or Q.shape[-3] != PLANES or Q.shape[-1] != Q.shape[-2]:
        raise ShapeError(f"vectorPupils must be [6,pn,pn] or [planes,6,pn,pn]; got {tuple(getattr(Q, 'shape', ()))}")
    dev = nat.require_gpu(maskFT.device)
    pn, stacked = int(Q.shape[-1]), Q.dim() == 4
    planes = int(Q.shape[0]) if stacked else 1
    out, given = _socs._accumulate_into(out, (planes, pn, pn) if stacked else (pn, pn), torch.float32, dev)
    key = (Q.data_ptr(), Q._version, tuple(Q.shape), tuple(states))
    stack = getattr(plan, "_vector_stack", (None, None))
    if stack[0] != key:                                    # a PlanCache keeps the stack it planned for
        Q4 = Q.to(device=dev, dtype=torch.complex64).reshape(planes, 3, 2, pn, pn)
        eff = torch.stack([math.sqrt(mu) * (ex * Q4[:, :, 0] + ey * Q4[:, :, 1]) for mu, ex, ey in states], dim=1)
        stack = (key, eff.reshape(planes * 3 * len(states), pn, pn).contiguous())
        if plan is not None:
            plan._vector_stack = stack
    _socs._stack_and_fold(maskFT, stack[1], shifts, N, planes, 3 * len(states), out, given, plan=plan, options=options,
                          weights=weights)
    return out
