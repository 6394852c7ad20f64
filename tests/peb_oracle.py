"""CPU restatement (numpy, float64) of the post-exposure bake, written from the definitions in include/litho_abbe.h -- not from
the kernels: exposure, the bake step (Jacobi diffusion without flux, neutralisation, acid loss, the trapezoid of the
amplification integral, in this order and with the header's grouping of every sum), and the slowness after the bake.  Nothing in
the reference computes any of this, so this file is the parity target of tests/test_gpu_peb.py; tests/test_peb_cpu.py pins it by
closed forms."""
import math

import numpy as np

import develop_oracle as DO

MAX_STEPS = 65536


def expose(image, gains, C):
    """image [F, D, n, n] -> h0 = 1 - exp(-(C g) I), float64 [len(gains) F, D, n, n], gain-major; NaN where that is negative or NaN."""
    I = np.asarray(image, dtype=np.float64)
    if I.ndim == 3:
        I = I[None]
    out = []
    for g in gains:
        h0 = 1.0 - np.exp(-((C * float(np.float32(g))) * I))
        with np.errstate(invalid="ignore"):
            out.append(np.where(h0 >= 0.0, h0, np.nan))
    return np.concatenate(out, axis=0)


def lambdas(sigma, vertical_scale, pixel, hz, S):
    """(lambda_xy, lambda_z) = D_s dt / spacing^2 with sigma = sqrt(2 D_s bakeTime), sigma_z = vertical_scale sigma."""
    sz = vertical_scale * sigma
    return sigma * sigma / (2.0 * S * (pixel * pixel)), sz * sz / (2.0 * S * (hz * hz))


def min_steps(sigma_h, sigma_q, vertical_scale, thickness, D, pixel):
    """The smallest S with 4 lambda_xy + 2 lambda_z <= 1 for both species."""
    hz = thickness / D
    S = 1
    while any(4.0 * lxy + 2.0 * lz > 1.0 for lxy, lz in (lambdas(s, vertical_scale, pixel, hz, S) for s in (sigma_h, sigma_q))):
        S += 1
    return S


def step_parameters(k_quench, k_loss, sigma_h, sigma_q, vertical_scale, bake_time, thickness, D, pixel, S):
    """What a step uses, rounded to fp32 as the library hands it to its kernels (returned as Python floats):
    dict(lam_h=(lxy, lz) or None, lam_q=..., beta, fl, half_dt); None: that species does not diffuse."""
    f32 = lambda v: float(np.float32(v))                                         # noqa: E731
    hz, dt = thickness / D, bake_time / S
    lam = lambda s: tuple(f32(v) for v in lambdas(s, vertical_scale, pixel, hz, S)) if s > 0.0 else None   # noqa: E731
    with np.errstate(over="ignore"):
        beta = f32(k_quench * dt)
    return dict(lam_h=lam(sigma_h), lam_q=lam(sigma_q), beta=beta, fl=f32(math.exp(-k_loss * dt)), half_dt=f32(0.5 * dt))


def _neighbour(x, axis, step):
    """The neighbour at `step` (+1 or -1) along `axis`; outside the grid, the cell's mirror image: the cell itself."""
    out = x.copy()
    src, dst = [slice(None)] * x.ndim, [slice(None)] * x.ndim
    if step > 0:
        src[axis], dst[axis] = slice(1, None), slice(None, -1)
    else:
        src[axis], dst[axis] = slice(None, -1), slice(1, None)
    out[tuple(dst)] = x[tuple(src)]
    return out


def diffuse_step(x, lam):
    """x + lxy (((W + E) + (S + N)) - 4 x) + lz ((U + Dn) - 2 x) on [..., D, n, n]; lam None: x itself."""
    if lam is None:
        return x
    lxy, lz = lam
    W, E = _neighbour(x, -1, -1), _neighbour(x, -1, 1)
    S, N = _neighbour(x, -2, -1), _neighbour(x, -2, 1)
    U, Dn = _neighbour(x, -3, -1), _neighbour(x, -3, 1)
    return x + lxy * (((W + E) + (S + N)) - 4.0 * x) + lz * ((U + Dn) - 2.0 * x)


def bake_step(h, q, a, lam_h, lam_q, beta, fl, half_dt):
    """One step on [..., D, n, n]: (h, q, a) after it."""
    hd, qd = diffuse_step(h, lam_h), diffuse_step(q, lam_q)
    with np.errstate(invalid="ignore"):
        if math.isinf(beta):
            R = np.where(hd < qd, hd, qd)
        else:
            R = beta * hd * qd / (1.0 + beta * (hd + qd))
    h_new = (hd - R) * fl
    return h_new, qd - R, a + half_dt * (h + h_new)


def bake(h0, q0, S, lam_h, lam_q, beta, fl, half_dt):
    """S steps from acid h0 [..., D, n, n], uniform quencher q0 and a = 0: (h, q, a), float64."""
    h = np.asarray(h0, dtype=np.float64).copy()
    q = np.full(h.shape, float(q0))
    a = np.zeros(h.shape)
    for _ in range(S):
        h, q, a = bake_step(h, q, a, lam_h, lam_q, beta, fl, half_dt)
    return h, q, a


def rate(a, k_amp, r_max, r_min, qm, m_th, thickness, r0=1.0, delta=1.0):
    """a [..., D, n, n] -> (inhibitor m = exp(-k_amp a), slowness 1 / (Mack's r(m) x the surface factor)); the slowness is NaN
    where 1 - m is negative or NaN."""
    a = np.asarray(a, dtype=np.float64)
    f = DO.surface_factor(thickness, a.shape[-3], r0, delta)[:, None, None]
    m = np.exp(-(k_amp * a))
    with np.errstate(invalid="ignore"):
        s = 1.0 / (DO.rate_of_m(m, r_max, r_min, qm, m_th) * f)
        return m, np.where(1.0 - m >= 0.0, s, np.nan)
