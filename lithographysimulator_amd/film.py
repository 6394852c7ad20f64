"""Resist film stack for vector imaging; no reference counterpart (include/litho_abbe.h).

`vectorPupils` images into one homogeneous medium.  The image that counts forms inside a resist layer, between a top coat or
water above and a BARC and silicon below: reflection at those interfaces gives standing waves through the depth, swing curves
over thickness, and different transmission for TE and TM.  A film stack changes only the six planes Q_cj of a pupil, so
`filmPupils` (litho_film_pupils: one pointwise kernel in double precision with a thin-film recursion per cell) returns them at
depths inside one layer of a `FilmStack`, and `vectorSocsKernels(film=, depths=)`, `vectorAbbeIntensity`, hopkinsImage,
hopkinsGradient, optimizeMask and correctLayout(socs=) consume them unchanged.

Conventions (the engine's own): a wave advancing by z into the wafer carries exp(-i kappa z), so an absorbing medium (n, k),
k >= 0, enters as n - i k.  In every medium w = sqrt((n - i k)^2 - s), Im w <= 0, with s = NA^2 sigma^2; s- and p-polarisation
are two scalar problems with u and eta-weighted flux continuous (u = E_s, eta = w; u = H_s, eta = w / (n - i k)^2), and

    Q_cj = P . f . [ t_c E_s t_j + (r_c E_rad + zhat_c E_z) r_j ],   r = (alpha, beta) / |(alpha, beta)|,  t = (-r_y, r_x).

With every index equal to the incident one the planes are vectorPupils(defocus=z) . exp(-2 pi i n0 z / lambda).

The depth-averaged ("bulk") image sum_d omega_d I(z_d) has the transmission cross coefficient sum_d omega_d T_d, which is
factored as ONE kernel set (`depthWeights`): a bulk image costs K fields, not D K.

NOT built: absorbed-energy weighting (n k |E|^2 is a constant factor inside one layer), layers with a gradient in index, a
per-depth vectorAbbeIntensity beyond reshaping the planes to [planes D, 6, pn, pn].  Development of the resist from the
per-depth images is develop.py."""
import ctypes
import math
from functools import partial

import numpy as np
import torch

from . import _native as nat
from . import socs as _socs
from . import vector as _vec

MAX_LAYERS = 16


class FilmStack:
    """A thin-film stack under the incident medium: `layers` = [(n, k, thickness_nm), ...] from the top down (1 ... 16 of them,
    n > 0, k >= 0, thickness > 0), `substrate` = (n, k), `resist` = the index of the layer that is sampled."""

    def __init__(self, layers, substrate, resist=0):
        try:
            table = np.array([[float(v) for v in layer] for layer in layers], dtype=np.float64)
            sub = np.array([float(v) for v in substrate], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("FilmStack: layers must be a list of (n, k, thickness_nm) and substrate a pair (n, k)") from None
        if table.ndim != 2 or table.shape[1:] != (3,) or not 1 <= table.shape[0] <= MAX_LAYERS:
            raise ValueError(f"FilmStack: 1 ... {MAX_LAYERS} layers of (n, k, thickness_nm) are required; got shape {table.shape}")
        if sub.shape != (2,):
            raise ValueError("FilmStack: substrate must be a pair (n, k)")
        if not (np.isfinite(table).all() and np.isfinite(sub).all()):
            raise ValueError("FilmStack: a value is not finite")
        if (table[:, 0] <= 0).any() or (table[:, 1] < 0).any() or (table[:, 2] <= 0).any() or sub[0] <= 0 or sub[1] < 0:
            raise ValueError("FilmStack: n > 0, k >= 0 and thickness > 0 are required in every layer, n > 0 and k >= 0 in the substrate")
        if isinstance(resist, bool) or not isinstance(resist, (int, np.integer)) or not 0 <= int(resist) < table.shape[0]:
            raise ValueError(f"FilmStack: resist must be the index of a layer, 0 ... {table.shape[0] - 1}; got {resist!r}")
        self.layers = [tuple(row) for row in table.tolist()]
        self.substrate = (float(sub[0]), float(sub[1]))
        self.resist = int(resist)

    @property
    def thickness(self):
        """Thickness of the sampled layer, nm."""
        return self.layers[self.resist][2]

    def depths(self, count):
        """The midpoints of `count` equal slabs of the resist layer (nm below its top): equal weights are the midpoint rule."""
        count = int(count)
        if count < 1:
            raise ValueError(f"FilmStack.depths: count >= 1 is required; got {count}")
        return [self.thickness * (i + 0.5) / count for i in range(count)]

    def __repr__(self):
        return f"FilmStack(layers={self.layers}, substrate={self.substrate}, resist={self.resist})"


def _depth_list(who, stack, depths):
    if not isinstance(stack, FilmStack):
        raise TypeError(f"{who}: the film stack must be a FilmStack")
    if depths is None:
        raise ValueError(f"{who}: a film stack needs depths (nm below the top of the resist layer)")
    if isinstance(depths, torch.Tensor):
        depths = depths.detach().cpu().numpy()
    z = np.asarray(depths, dtype=np.float64)
    if z.ndim > 1 or z.size < 1 or not np.isfinite(z).all() or (z < 0).any() or (z > stack.thickness).any():
        raise ValueError(f"{who}: depths must be a value or a non-empty list of values in [0, {stack.thickness}] nm, the resist layer")
    return np.atleast_1d(z).copy()


def _root(e_re, e_im, s):
    """sqrt((e_re + i e_im) - s) on the branch Im <= 0 (Re > 0 when Im = 0), complex128."""
    w = torch.sqrt(torch.complex(e_re - s, torch.full_like(s, e_im)))
    return torch.where(w.imag > 0, -w, w)


def _host_film_pupils(P, NA, n, radiometric, zs, wavelength, stack, depths):
    """The planes in float64 torch on the host, complex64 [planes,D,6,pn,pn]: litho_film_pupils restated, in the role
    vector._host_vector_pupils plays -- only for vectorSocsKernels(applier=) with a pupil that does not live on a GPU."""
    planes, pn = P.shape[0], P.shape[-1]
    lam = float(wavelength)
    k = torch.arange(pn, dtype=torch.float64) - pn // 2
    a = (NA * (k * 4.0 / pn) / n)[None, :].expand(pn, pn)
    b = (NA * (k * 4.0 / pn) / n)[:, None].expand(pn, pn)
    s0 = a * a + b * b
    ok = s0 < 1.0
    s0 = torch.where(ok, s0, torch.zeros_like(s0))
    s = n * n * s0
    media = [(n * n, 0.0, 0.0)] + [(ln * ln - lk * lk, -2.0 * ln * lk, d) for ln, lk, d in stack.layers]
    media.append((stack.substrate[0] ** 2 - stack.substrate[1] ** 2, -2.0 * stack.substrate[0] * stack.substrate[1], 0.0))
    res = stack.resist + 1
    w_below = _root(media[-1][0], media[-1][1], s)
    p_below = w_below / complex(media[-1][0], media[-1][1])
    gam = [torch.zeros_like(w_below), torch.zeros_like(w_below)]
    tau = [torch.ones_like(w_below), torch.ones_like(w_below)]
    for m in range(len(media) - 2, -1, -1):
        e_re, e_im, d = media[m]
        w = _root(e_re, e_im, s)
        eta, eta_below = (w, w / complex(e_re, e_im)), (w_below, p_below)
        e = torch.exp(-2j * math.pi * w * (d / lam)) if m > 0 else torch.ones_like(w)
        rho = []
        for q in range(2):
            up, down = eta[q] * (1.0 + gam[q]), eta_below[q] * (1.0 - gam[q])
            rho.append((up - down) / (up + down))
            if m < res:
                tau[q] = tau[q] * (e * (2.0 * eta[q] / (up + down)))
            gam[q] = rho[q] * e * e
        if m == res:
            rho_res, w_res, e_res = rho, w, e
        w_below, p_below = eta
    eps = complex(media[res][0], media[res][1])
    a_s, a_p = tau[0], n * tau[1]
    c_s, c_p = rho_res[0] * a_s * e_res, rho_res[1] * a_p * e_res
    centre = s0 == 0.0
    rn = torch.where(centre, torch.zeros_like(s0), 1.0 / torch.sqrt(torch.where(centre, torch.ones_like(s0), s0)))
    rx, ry = a * rn, b * rn
    out = []
    for z in np.asarray(depths, dtype=np.float64).tolist():
        down = torch.exp(-2j * math.pi * w_res * (z / lam))
        upw = torch.exp(-2j * math.pi * w_res * ((stack.thickness - z) / lam))
        Es = a_s * down + c_s * upw
        H = a_p * down + c_p * upw
        Erad = torch.where(centre, Es, (w_res / eps) * (a_p * down - c_p * upw))
        Ez = -torch.sqrt(s) * H / eps
        diff = Erad - Es
        out.append(torch.stack([Es + rx * rx * diff, rx * ry * diff, rx * ry * diff, Es + ry * ry * diff, rx * Ez, ry * Ez]))
    M = torch.stack(out)                                                                  # [D,6,pn,pn]
    g = torch.sqrt(1.0 - s0)
    if radiometric:
        M = M / torch.sqrt(g)
    M = M * ok
    zf = torch.from_numpy(np.broadcast_to(zs, (planes,)).copy()) if zs is not None else torch.zeros(planes, dtype=torch.float64)
    phase = torch.exp(2j * math.pi * (n * zf / lam)[:, None, None] * (s0 / (1.0 + g))[None])
    return ((P.to(torch.complex128) * phase)[:, None, None] * M[None]).to(torch.complex64)


def _device_film_pupils(P, planes, pn, NA, n, radiometric, zs, wavelength, stack, depths, dev):
    """litho_film_pupils on contiguous complex64 P [planes,pn,pn]: complex64 [planes,D,6,pn,pn]."""
    D, L = int(depths.shape[0]), len(stack.layers)
    if planes * D > 65535:
        raise ValueError(f"filmPupils: {planes} planes times {D} depths exceed 65535")
    out = torch.empty((planes, D, _vec.PLANES, pn, pn), dtype=torch.complex64, device=dev)
    layers = (ctypes.c_double * (3 * L))(*[v for layer in stack.layers for v in layer])
    zd = (ctypes.c_double * D)(*depths.tolist())
    zf = (ctypes.c_double * planes)(*np.broadcast_to(zs, (planes,)).tolist()) if zs is not None else None
    with torch.cuda.device(dev):
        nat.check(nat.lib().litho_film_pupils(nat.ptr(P), planes, pn, NA, n, 1 if radiometric else 0, layers, L, stack.substrate[0],
                                              stack.substrate[1], stack.resist, zd, D, zf, float(wavelength), nat.ptr(out),
                                              nat.stream_ptr(dev)), "litho_film_pupils")
    return out


def _wavelength(who, wavelength):
    if wavelength is None or not (float(wavelength) > 0.0 and math.isfinite(float(wavelength))):
        raise ValueError(f"{who}: a film stack needs a positive wavelength (nm)")
    return float(wavelength)


def filmPupils(pupilF, NA, stack, depths, wavelength, mediumIndex, radiometric=False, defocus=None):
    """The six planes of a pupil function at `depths` (nm below the top of the resist layer of `stack`, a value or a list) on the
    device (litho_film_pupils): complex64 [D,6,pn,pn], plane t = 2 c + j, or [planes,D,6,pn,pn] for a pupil stack [planes,pn,pn]
    or a `defocus` list (vectorPupils' broadcasting rule).  `mediumIndex` is the real index of the incident medium above the
    stack (1.44 for water at 193 nm), `NA` < `mediumIndex`; `radiometric` and `defocus` (nm, in the incident medium: best focus
    relative to the top of the stack) as vectorPupils.  pn even, >= 16.  Reshaped to [planes D, 6, pn, pn] the result is
    vectorAbbeIntensity's input as it is."""
    who = "filmPupils"
    NA, n = _vec._check_optics(who, NA, mediumIndex)
    wavelength = _wavelength(who, wavelength)
    z = _depth_list(who, stack, depths)
    zs, as_list = _vec._defocus_list(who, defocus, wavelength)
    pn, pp, planes, stacked = _vec._pupil_planes(who, pupilF, zs, as_list)
    if pn < 16 or pn & 1:
        raise ValueError(f"{who}: pn must be even and >= 16; got {pn}")
    dev = nat.require_gpu(pupilF.device)
    P = pupilF.detach().to(torch.complex64).reshape(pp, pn, pn).expand(planes, pn, pn).contiguous()
    out = _device_film_pupils(P, planes, pn, NA, n, radiometric, zs, wavelength, stack, z, dev)
    return out if stacked else out[0]


class _BulkOperator:
    """X -> sum_d omega_d T_d X: one unchanged vector._VectorOperator (litho_tcc_apply_vector) per depth, summed in ascending d."""

    def __init__(self, planes6, weights, w_shifted, apply_bytes):
        self.ops = [_vec._VectorOperator(Q, w_shifted, apply_bytes) for Q in planes6]
        self.weights = weights

    def __call__(self, X):
        Y = self.ops[0](X).mul_(self.weights[0])
        for op, omega in zip(self.ops[1:], self.weights[1:]):
            Y.add_(op(X), alpha=omega)
        return Y


def _plane_trace(q, sxx, syy, sxy):
    """trace T of six planes q complex128 [6,pn,pn]: sum_jj' (sum W_jj') sum_c <Q_cj', Q_cj>, as vectorSocsKernels."""
    gxx = float((q[0::2].abs() ** 2).sum())
    gyy = float((q[1::2].abs() ** 2).sum())
    gxy = float((q[0::2] * q[1::2].conj()).sum().real)
    return sxx * gxx + syy * gyy + 2.0 * sxy * gxy


def _film_socs_kernels(who, pupilF, lightsource, NA, n, polarization, degree, radiometric, zs, as_list, wavelength, film, depths,
                       depthWeights, applyBytes, **factor):
    """vectorSocsKernels' film path (its docstring): every (focus plane, depth) a plane of the result, or with `depthWeights`
    one bulk kernel set per focus plane."""
    wavelength = _wavelength(who, wavelength)
    z = _depth_list(who, film, depths)
    D = int(z.shape[0])
    pn, pp, planes, stacked = _vec._pupil_planes(who, pupilF, zs, as_list)
    pure = not (isinstance(polarization, str) and polarization == "unpolarized") and float(degree) == 1.0
    omega = None
    if depthWeights is not None:
        omega = np.asarray(depthWeights.detach().cpu().numpy() if isinstance(depthWeights, torch.Tensor) else depthWeights,
                           dtype=np.float64)
        if omega.shape != (D,) or not np.isfinite(omega).all() or (omega < 0).any() or not (omega > 0).any():
            raise ValueError(f"{who}: depthWeights must be {D} finite non-negative numbers, one per depth and not all zero")
        omega = omega.tolist()

    def planes_of(W, dev):
        pol = _vec.sourcePolarization(lightsource, polarization, degree)
        P = pupilF.detach().to(torch.complex64).reshape(pp, pn, pn).expand(planes, pn, pn)
        if dev.type == "cuda":
            Q = _device_film_pupils(P.contiguous(), planes, pn, NA, n, radiometric, zs, wavelength, film, z, dev)
        else:
            Q = _host_film_pupils(P, NA, n, radiometric, zs, wavelength, film, z)
        wsh = torch.fft.ifftshift(pol, dim=(-2, -1)).to(dev).contiguous()
        sxx, syy, sxy = pol.to(torch.float64).sum(dim=(1, 2)).tolist()
        for Qf in Q:                                                                      # [D,6,pn,pn] of one focus plane
            traces = [_plane_trace(Qd.to(torch.complex128), sxx, syy, sxy) for Qd in Qf]
            if omega is None:
                for Qd, tr in zip(Qf, traces):
                    Qd = Qd.contiguous()
                    yield (Qd != 0).any(dim=0), tr, partial(_vec._VectorOperator, Qd, wsh, applyBytes)
            else:
                yield ((Qf != 0).any(dim=0).any(dim=0), sum(o * t for o, t in zip(omega, traces)),
                       partial(_BulkOperator, [Qd.contiguous() for Qd in Qf], omega, wsh, applyBytes))

    rank = 3 if pure else 5
    if omega is None:
        return _socs._factorise(who, pupilF.device, pn, planes * D, True, lightsource, rank, planes_of, **factor)
    return _socs._factorise(who, pupilF.device, pn, planes, stacked, lightsource, rank * D, planes_of, **factor)
