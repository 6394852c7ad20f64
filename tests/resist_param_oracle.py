"""CPU restatement (numpy, float64) of the gradients with respect to the resist's parameters, written from the definitions in
include/litho_abbe.h ("Gradients with respect to the bake's parameters", "... the rate law's parameters") on peb_oracle and
develop_oracle -- not from the kernels: the six step-parameter sums of the bake's backward sweep, their chain to the physical
parameters of a ChemicallyAmplifiedResist, the parameter sums of the rate law and of the exposure, and the rate law's chain.
Nothing in the reference computes any of this; this file is the parity target of tests/test_gpu_resist_param.py, and
tests/test_resist_param_cpu.py pins it to central differences of peb_oracle.bake, of the rate and exposure oracles and of the step
parameters' formulas, and to closed forms."""
import math

import numpy as np

import develop_oracle as DO
import peb_oracle as PO

SLOTS = ("lxy_h", "lz_h", "lxy_q", "lz_q", "beta", "fl")
PHYSICAL = ("kQuench", "kLoss", "acidDiffusionLength", "quencherDiffusionLength", "verticalScale")


def laplacians(x):
    """(((W + E) + (S + N)) - 4 x, (U + Dn) - 2 x) on [..., D, n, n] with the forward's face rule: the cell itself beyond a face."""
    W, E = PO._neighbour(x, -1, -1), PO._neighbour(x, -1, 1)
    S, N = PO._neighbour(x, -2, -1), PO._neighbour(x, -2, 1)
    U, Dn = PO._neighbour(x, -3, -1), PO._neighbour(x, -3, 1)
    return ((W + E) + (S + N)) - 4.0 * x, (U + Dn) - 2.0 * x


def step_terms(h, q, hb, qb, ab, lam_h, lam_q, beta, fl, half_dt):
    """The six per-cell terms of one backward step, [6, ...]: (h, q) the state at the start of the step, (hb, qb) the cotangents
    after it, ab = abar; and the step's (hbar_k, qbar_k)."""
    hd, qd = PO.diffuse_step(h, lam_h), PO.diffuse_step(q, lam_q)
    hp = hb + half_dt * ab
    if math.isinf(beta):
        first = hd < qd
        Rh = np.where(first, 1.0, 0.0)
        Rq = 1.0 - Rh
        R = np.where(first, hd, qd)
        t_beta = np.zeros(h.shape)
    else:
        Dn = 1.0 + beta * (hd + qd)
        Rh = beta * qd * (1.0 + beta * qd) / (Dn * Dn)
        Rq = beta * hd * (1.0 + beta * hd) / (Dn * Dn)
        R = beta * hd * qd / Dn
        t_beta = -(fl * hp + qb) * (hd * qd) / (Dn * Dn)
    f = fl * hp
    u = f * (1.0 - Rh) - qb * Rh
    v = qb * (1.0 - Rq) - f * Rq
    zero = np.zeros(h.shape)
    t = [zero, zero, zero, zero, t_beta, hp * (hd - R)]
    if lam_h is not None:
        lxy, lz = laplacians(h)
        t[0], t[1] = u * lxy, u * lz
    if lam_q is not None:
        lxy, lz = laplacians(q)
        t[2], t[3] = v * lxy, v * lz
    return np.stack(t), PO.diffuse_step(u, lam_h) + half_dt * ab, PO.diffuse_step(v, lam_q)


def bake_param_vjp(h0, q0, S, gh, gq, ga, lam_h, lam_q, beta, fl, half_dt):
    """For h0 [B, D, n, n]: (grad_step [B, 6], the sums of the absolute per-cell, per-step terms [B, 6], hbar_0, qbar_0).  The
    cotangents gh, gq, ga of (h_S, q_S, a_S); None = zero."""
    h = np.asarray(h0, dtype=np.float64).copy()
    assert h.ndim == 4
    q = np.full(h.shape, float(q0))
    a = np.zeros(h.shape)
    states = []
    for _ in range(S):
        states.append((h, q))
        h, q, a = PO.bake_step(h, q, a, lam_h, lam_q, beta, fl, half_dt)
    zero = np.zeros(h.shape)
    hb, qb, ab = (zero if g is None else np.asarray(g, dtype=np.float64) for g in (gh, gq, ga))
    grad, mass = np.zeros((h.shape[0], 6)), np.zeros((h.shape[0], 6))
    for hk, qk in reversed(states):
        t, hb, qb = step_terms(hk, qk, hb, qb, ab, lam_h, lam_q, beta, fl, half_dt)
        grad += t.sum(axis=(2, 3, 4)).T
        mass += np.abs(t).sum(axis=(2, 3, 4)).T
    return grad, mass, hb, qb


def param_chain(thickness, pixel, k_quench, k_loss, sigma_h, sigma_q, vertical_scale, bake_time, D, S, grad_step):
    """grad_step [..., 6] -> [..., 5] = d/d(kQuench, kLoss, acidDiffusionLength, quencherDiffusionLength, verticalScale): the
    analytic derivative of the step parameters' formulas at a fixed step count S."""
    g = np.asarray(grad_step, dtype=np.float64)
    hz, dt = thickness / D, bake_time / S
    dxy = lambda s: s / (S * pixel * pixel)                                      # noqa: E731   d lxy / d sigma = 2 lxy / sigma
    dz = lambda s: vertical_scale * vertical_scale * s / (S * hz * hz)           # noqa: E731   d lz / d sigma = 2 lz / sigma
    dv = lambda s: vertical_scale * s * s / (S * hz * hz)                        # noqa: E731   d lz / d vscale = 2 lz / vscale
    fl = math.exp(-k_loss * dt)
    kq = 0.0 if math.isinf(k_quench) else g[..., 4] * dt
    return np.stack([kq + 0.0 * g[..., 4], g[..., 5] * (-dt * fl), g[..., 0] * dxy(sigma_h) + g[..., 1] * dz(sigma_h),
                     g[..., 2] * dxy(sigma_q) + g[..., 3] * dz(sigma_q), g[..., 1] * dv(sigma_h) + g[..., 3] * dv(sigma_q)], axis=-1)


def step_vector(k_quench, k_loss, sigma_h, sigma_q, vertical_scale, bake_time, thickness, D, pixel, S):
    """The six step parameters in double, unrounded: what param_chain differentiates."""
    hz, dt = thickness / D, bake_time / S
    lh, lq = PO.lambdas(sigma_h, vertical_scale, pixel, hz, S), PO.lambdas(sigma_q, vertical_scale, pixel, hz, S)
    return np.array([lh[0], lh[1], lq[0], lq[1], k_quench * dt, math.exp(-k_loss * dt)])


# ---- the rate law and the exposure -------------------------------------------------------------------------------------------------
RATE_SLOTS = ("kappa", "R", "rmin", "q", "a", "f")
RATE_PARAMETERS = ("kappa", "rMax", "rMin", "q", "mTh", "surfaceRate", "surfaceDepth")


def rate_param_sums(x, gains, kappa, r_max, r_min, q, m_th, thickness, r0, delta, grad_s):
    """x [F, D, n, n], grad_s [len(gains) F, D, n, n] gain-major -> (plane sums [len(gains) F, D, 6], the sums of the absolute
    terms, alike): the header's six derivatives of s = 1 / r times the cotangent, a wall contributing 0."""
    x = np.asarray(x, dtype=np.float64)
    F, D = x.shape[0], x.shape[1]
    gs = np.asarray(grad_s, dtype=np.float64).reshape((len(gains), F) + x.shape[1:])
    f = DO.surface_factor(thickness, D, r0, delta)[None, :, None, None]
    a = DO.mack_a(q, m_th)
    R = r_max * (a + 1.0)
    sums, mass = [], []
    for i, gain in enumerate(gains):
        g = float(np.float32(gain))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            m = np.exp(-((kappa * g) * x))
            b = 1.0 - m
            ok = b >= 0.0
            bs = np.where(ok, b, 0.5)
            X = bs ** q
            r = (R * X / (a + X) + r_min) * f
            s = 1.0 / r
            ssf = s * s * f
            ds = [-ssf * (R * a / (a + X) ** 2) * (q * bs ** (q - 1.0) * ((g * x) * m)),
                  -ssf * X / (a + X),
                  -ssf * np.ones_like(X),
                  np.where(bs > 0.0, -ssf * (R * a / (a + X) ** 2) * X * np.log(np.where(bs > 0.0, bs, 1.0)), 0.0),
                  -ssf * (R / (a + 1.0)) * X * (X - 1.0) / (a + X) ** 2,
                  -s / f * np.ones_like(X)]
            t = np.stack([np.where(ok, np.where(ok, gs[i], 0.0) * d, 0.0) for d in ds], axis=-1)      # [F, D, n, n, 6]
        sums.append(t.sum(axis=(2, 3)))
        mass.append(np.abs(t).sum(axis=(2, 3)))
    return np.concatenate(sums, axis=0), np.concatenate(mass, axis=0)


def rate_param_chain(plane_sums, r_max, r_min, q, m_th, thickness, r0, delta):
    """plane sums [G, D, 6] -> [G, 7] = d/d(kappa, rMax, rMin, q, mTh, surfaceRate, surfaceDepth), the planes in ascending order."""
    t = np.asarray(plane_sums, dtype=np.float64)
    D = t.shape[1]
    a = DO.mack_a(q, m_th)
    da_dq = a * (1.0 / (q + 1.0) - 1.0 / (q - 1.0) + math.log(1.0 - m_th))
    da_dm = -q * a / (1.0 - m_th)
    z = DO.depths(thickness, D)
    ez = np.exp(-z / delta)
    tot = t.sum(axis=1)
    return np.stack([tot[:, 0], tot[:, 1] * (a + 1.0), tot[:, 2], tot[:, 3] + tot[:, 4] * da_dq, tot[:, 4] * da_dm,
                     (t[:, :, 5] * ez).sum(axis=1), (t[:, :, 5] * (-(1.0 - r0) * ez * z / (delta * delta))).sum(axis=1)], axis=-1)


def expose_param_sums(image, gains, C, grad_acid):
    """image [F, D, n, n], grad_acid [len(gains) F, D, n, n] -> (dl/dC per gained volume [len(gains) F], the sums of the absolute
    terms): grad_acid (g I) exp(-(C g) I), a cell whose acid is NaN contributing 0."""
    I = np.asarray(image, dtype=np.float64)
    g = np.asarray(grad_acid, dtype=np.float64).reshape((len(gains),) + I.shape)
    sums, mass = [], []
    for i, gain in enumerate(gains):
        gf = float(np.float32(gain))
        with np.errstate(invalid="ignore", over="ignore"):
            ex = np.exp(-((C * gf) * I))
            ok = 1.0 - ex >= 0.0
            t = np.where(ok, np.where(ok, g[i], 0.0) * ((gf * I) * ex), 0.0)
        sums.append(t.sum(axis=(1, 2, 3)))
        mass.append(np.abs(t).sum(axis=(1, 2, 3)))
    return np.concatenate(sums), np.concatenate(mass)
