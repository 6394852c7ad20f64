"""CPU restatement (numpy, float64) of the forward mode (tangents) of the resist chain, written from the definitions in
include/litho_abbe.h ("Forward mode (tangents) of the resist chain") on peb_oracle, develop_oracle and develop_grad_oracle -- not
from the kernels.  Nothing in the reference computes any of this; this file is the parity target of
tests/test_gpu_resist_tangent.py, and tests/test_resist_tangent_cpu.py pins it to central differences of the forward oracles and,
by <g, J v> = <J^T g, v>, to the adjoint oracles.

  expose_jvp            dh0 = exp(-(C g) I) ((g I) dC + (C g) dI), 0 where the acid is NaN
  bake_jvp              the S bake steps with one tangent, the header's step formulas
  param_tangent         d(step parameters)[6] from d(physical parameters)[5], the transpose of resist_param_oracle.param_chain
  rate_jvp              the rate law's tangent from dx and the six slot directions dphi [D, 6]
  rate_param_tangent    dphi [D, 6] from d(kappa, rMax, rMin, q, mTh, surfaceRate, surfaceDepth)[7]
  ordered_tangent       the front's tangent by one pass over the cells in ascending stored T on develop_grad_oracle.links
  gather_fp32_tangent   the device's iteration restated op for op in fp32"""
import math

import numpy as np

import develop_grad_oracle as DGO
import develop_oracle as DO
import peb_oracle as PO
from resist_param_oracle import laplacians


def expose_jvp(image, gains, C, dC, dI=None):
    """image [F, D, n, n], dI alike or None -> float64 [len(gains) F, D, n, n], gain-major; the gains as the fp32 values the
    device gets.  Exactly 0 where 1 - exp(-(C g) I) is negative or NaN, whatever dI holds."""
    I = np.asarray(image, dtype=np.float64)
    dI = np.zeros(I.shape) if dI is None else np.asarray(dI, dtype=np.float64)
    out = []
    for g in gains:
        gf = float(np.float32(g))
        Cg = C * gf
        with np.errstate(invalid="ignore", over="ignore"):
            ex = np.exp(-(Cg * I))
            ok = 1.0 - ex >= 0.0
            t = ex * ((gf * I) * dC + Cg * np.where(ok, dI, 0.0))
        out.append(np.where(ok, t, 0.0))
    return np.concatenate(out, axis=0)


def _tangent_diffuse(x, dx, lam, dlxy, dlz):
    if lam is None:
        return dx
    lxy, lz = lam
    Lxy_d, Lz_d = laplacians(dx)
    Lxy, Lz = laplacians(x)
    return dx + lxy * Lxy_d + lz * Lz_d + dlxy * Lxy + dlz * Lz


def bake_tangent_step(h, q, dh, dq, da, lam_h, lam_q, beta, fl, half_dt, dstep):
    """One tangent step: (dh', dq', da') from the state (h, q) at the start of the step and its tangent; dstep = d(lxy_h, lz_h,
    lxy_q, lz_q, beta, fl)."""
    hd, qd = PO.diffuse_step(h, lam_h), PO.diffuse_step(q, lam_q)
    dhd = _tangent_diffuse(h, dh, lam_h, dstep[0], dstep[1])
    dqd = _tangent_diffuse(q, dq, lam_q, dstep[2], dstep[3])
    if math.isinf(beta):
        first = hd < qd
        R = np.where(first, hd, qd)
        dR = np.where(first, dhd, dqd)
    else:
        Dn = 1.0 + beta * (hd + qd)
        Rh = beta * qd * (1.0 + beta * qd) / (Dn * Dn)
        Rq = beta * hd * (1.0 + beta * hd) / (Dn * Dn)
        R = beta * hd * qd / Dn
        dR = Rh * dhd + Rq * dqd + (hd * qd / (Dn * Dn)) * dstep[4]
    dh_new = (dhd - dR) * fl + (hd - R) * dstep[5]
    return dh_new, dqd - dR, da + half_dt * (dh + dh_new)


def bake_jvp(h0, q0, S, lam_h, lam_q, beta, fl, half_dt, dh0=None, dq0=0.0, dstep=(0.0,) * 6):
    """((h, q, a), (dh, dq, da)) after S steps from (h0, uniform q0) with the tangent (dh0 or zero, uniform dq0, dstep)."""
    h = np.asarray(h0, dtype=np.float64).copy()
    q = np.full(h.shape, float(q0))
    a = np.zeros(h.shape)
    dh = np.zeros(h.shape) if dh0 is None else np.asarray(dh0, dtype=np.float64).copy()
    dq = np.full(h.shape, float(dq0))
    da = np.zeros(h.shape)
    for _ in range(S):
        dh, dq, da = bake_tangent_step(h, q, dh, dq, da, lam_h, lam_q, beta, fl, half_dt, dstep)
        h, q, a = PO.bake_step(h, q, a, lam_h, lam_q, beta, fl, half_dt)
    return (h, q, a), (dh, dq, da)


def param_tangent(thickness, pixel, k_quench, k_loss, sigma_h, sigma_q, vertical_scale, bake_time, D, S, dparam):
    """dparam [5] = d(kQuench, kLoss, acidDiffusionLength, quencherDiffusionLength, verticalScale) -> dstep [6]: the derivative
    of the step parameters' formulas at a fixed step count S; 0 for a zero length or scale and for kQuench = inf."""
    dp = np.asarray(dparam, dtype=np.float64)
    hz, dt = thickness / D, bake_time / S
    dxy = lambda s: s / (S * pixel * pixel)                                      # noqa: E731
    dz = lambda s: vertical_scale * vertical_scale * s / (S * hz * hz)           # noqa: E731
    dv = lambda s: vertical_scale * s * s / (S * hz * hz)                        # noqa: E731
    return np.array([dxy(sigma_h) * dp[2], dz(sigma_h) * dp[2] + dv(sigma_h) * dp[4], dxy(sigma_q) * dp[3],
                     dz(sigma_q) * dp[3] + dv(sigma_q) * dp[4], 0.0 if math.isinf(k_quench) else dt * dp[0],
                     -dt * math.exp(-k_loss * dt) * dp[1]])


def rate_slots(x, gain, kappa, r_max, r_min, q, m_th, thickness, r0, delta):
    """For x [F, D, n, n] and one gain: (ok, ds/dx, d [6, F, D, n, n]) -- the wall mask, the derivative with respect to x and the
    header's six slot derivatives (kappa, R, rmin, q, a, f)."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[-3]
    f = DO.surface_factor(thickness, D, r0, delta)[:, None, None]
    a = DO.mack_a(q, m_th)
    R = r_max * (a + 1.0)
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
        core = -ssf * (R * a / (a + X) ** 2) * (q * bs ** (q - 1.0))
        d = np.stack([core * ((g * x) * m), -ssf * X / (a + X), -ssf * np.ones_like(X),
                      np.where(bs > 0.0, -ssf * (R * a / (a + X) ** 2) * X * np.log(np.where(bs > 0.0, bs, 1.0)), 0.0),
                      -ssf * (R / (a + 1.0)) * X * (X - 1.0) / (a + X) ** 2, -s / f * np.ones_like(X)])
        return ok, core * ((kappa * g) * m), d


def rate_jvp(x, gains, kappa, r_max, r_min, q, m_th, thickness, r0, delta, dx=None, dphi=None):
    """x [F, D, n, n], dx alike or None, dphi [D, 6] or None -> ds float64 [len(gains) F, D, n, n], gain-major; exactly 0 at a wall."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[-3]
    dx = np.zeros(x.shape) if dx is None else np.asarray(dx, dtype=np.float64)
    dphi = np.zeros((D, 6)) if dphi is None else np.asarray(dphi, dtype=np.float64)
    out = []
    for gain in gains:
        ok, dsdx, d = rate_slots(x, gain, kappa, r_max, r_min, q, m_th, thickness, r0, delta)
        with np.errstate(invalid="ignore", over="ignore"):
            t = dsdx * np.where(ok, dx, 0.0)
            for j in range(6):
                t = t + d[j] * dphi[:, j][:, None, None]
        out.append(np.where(ok, t, 0.0))
    return np.concatenate(out, axis=0)


def rate_param_tangent(r_max, r_min, q, m_th, thickness, r0, delta, D, dparam):
    """dparam [7] = d(kappa, rMax, rMin, q, mTh, surfaceRate, surfaceDepth) -> dphi [D, 6], the directions of the slots (kappa, R at
    fixed a, rmin, q at fixed a, a, f of the plane)."""
    dp = np.asarray(dparam, dtype=np.float64)
    a = DO.mack_a(q, m_th)
    da_dq = a * (1.0 / (q + 1.0) - 1.0 / (q - 1.0) + math.log(1.0 - m_th))
    da_dm = -q * a / (1.0 - m_th)
    z = DO.depths(thickness, D)
    ez = np.exp(-z / delta)
    out = np.zeros((D, 6))
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = dp[0], (a + 1.0) * dp[1], dp[2], dp[3]
    out[:, 4] = da_dq * dp[3] + da_dm * dp[4]
    out[:, 5] = ez * dp[5] + (-(1.0 - r0) * ez * z / (delta * delta)) * dp[6]
    return out


def ordered_tangent(T, L, sigma, ds):
    """dT for one volume [D, n, n]: the cells in ascending stored T, each taking sigma ds and alpha dT of its upwind cells.  Exact
    because every link points strictly down in T.  ds is ignored where sigma = 0."""
    T = np.asarray(T, dtype=np.float64)
    tau = np.zeros(T.shape)
    src = np.where(sigma > 0, sigma * np.where(sigma > 0, np.asarray(ds, dtype=np.float64), 0.0), 0.0)
    idx = np.argwhere(sigma > 0)
    idx = idx[np.argsort(T[sigma > 0], kind="stable")]
    for d, y, x in idx:
        lx, ly, lz = L[d, y, x]
        v = src[d, y, x]
        if lx > 0:
            v += lx * tau[d, y, x - 1]
        elif lx < 0:
            v -= lx * tau[d, y, x + 1]
        if ly > 0:
            v += ly * tau[d, y - 1, x]
        elif ly < 0:
            v -= ly * tau[d, y + 1, x]
        if lz > 0:
            v += lz * tau[d - 1, y, x]
        elif lz < 0:
            v -= lz * tau[d + 1, y, x]
        tau[d, y, x] = v
    return tau


def time_jvp(T, s, ds, thickness, h, hz=None):
    """dT [..., D, n, n] in float64 from the stored T and s and the direction ds; exactly 0 at walls and unreached cells."""
    T, s, ds = (np.asarray(v, dtype=np.float64) for v in (T, s, ds))
    hz = float(thickness) / T.shape[-3] if hz is None else float(hz)
    L, sigma = DGO.links(T, s, h, hz)
    shape = T.shape
    Tb, Lb, sb, db = T.reshape((-1,) + shape[-3:]), L.reshape((-1,) + shape[-3:] + (3,)), sigma.reshape((-1,) + shape[-3:]), \
        ds.reshape((-1,) + shape[-3:])
    return np.stack([ordered_tangent(Tb[b], Lb[b], sb[b], db[b]) for b in range(Tb.shape[0])]).reshape(shape)


def gather_fp32_tangent(L, sigma, ds, max_sweeps=100000):
    """(dT, sweeps): the device's iteration in fp32 on one volume or a batch.  tau starts at 0; a sweep is tau_i <- sigma_i ds_i
    (one fp32 product; 0 where sigma = 0) + the terms of x, y, z in this order, each along the cell's own link from the neighbour
    its sign names, one fp32 multiplication and one addition; it stops at the first sweep that changes no bit."""
    L32, s32, d32 = np.asarray(L, dtype=np.float32), np.asarray(sigma, dtype=np.float32), np.asarray(ds, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        src = np.where(s32 > 0, (s32 * np.where(s32 > 0, d32, np.float32(0))).astype(np.float32), np.float32(0)).astype(np.float32)
    tau = np.zeros_like(src)
    for sweep in range(1, max_sweeps + 1):
        with np.errstate(invalid="ignore", over="ignore"):
            acc = src.copy()
            for c, ax in enumerate((-1, -2, -3)):
                lc = L32[..., c]
                lower, upper = DGO._zshift(tau, ax, -1), DGO._zshift(tau, ax, 1)
                acc = np.where(lc > 0, (acc + lc * lower).astype(np.float32), np.where(lc < 0, (acc + (-lc) * upper).astype(np.float32), acc))
        if np.array_equal(acc.view(np.uint32), tau.view(np.uint32)):
            return tau, sweep
        tau = acc
    raise RuntimeError("resist_tangent_oracle.gather_fp32_tangent: no fixed point")
