"""CPU restatement (numpy, float64) of the gradients through the post-exposure bake, written from the definitions in
include/litho_abbe.h ("Gradients through the bake") on peb_oracle's diffuse_step -- not from the kernels: the taped forward sweep,
the backward step, the exposure's VJP and the inhibitor's.  Nothing in the reference computes any of this; this file is the parity
target of tests/test_gpu_peb_grad.py, and tests/test_peb_grad_cpu.py pins it to central differences of peb_oracle.bake and to
closed forms."""
import math

import numpy as np

import peb_oracle as PO


def tape(h0, q0, S, lam_h, lam_q, beta, fl, half_dt):
    """The S steps of PO.bake from (h0, uniform q0), keeping each step's (hd, qd): ([(hd_0, qd_0), ...], (h_S, q_S, a_S))."""
    h = np.asarray(h0, dtype=np.float64).copy()
    q = np.full(h.shape, float(q0))
    a = np.zeros(h.shape)
    steps = []
    for _ in range(S):
        steps.append((PO.diffuse_step(h, lam_h), PO.diffuse_step(q, lam_q)))
        h, q, a = PO.bake_step(h, q, a, lam_h, lam_q, beta, fl, half_dt)
    return steps, (h, q, a)


def branch_margin(steps):
    """min |hd - qd| over every cell and step: how far the trajectory stays from a tie of instantaneous neutralisation."""
    return min(float(np.abs(hd - qd).min()) for hd, qd in steps)


def step_adjoint(hb, qb, ab, hd, qd, lam_h, lam_q, beta, fl, half_dt):
    """One backward step: (hbar_k, qbar_k) from (hbar_k+1, qbar_k+1), abar and the step's (hd, qd)."""
    hp = hb + half_dt * ab
    if math.isinf(beta):
        Rh = np.where(hd < qd, 1.0, 0.0)
        Rq = 1.0 - Rh
    else:
        Dn = 1.0 + beta * (hd + qd)
        Rh = beta * qd * (1.0 + beta * qd) / (Dn * Dn)
        Rq = beta * hd * (1.0 + beta * hd) / (Dn * Dn)
    f = fl * hp
    u = f * (1.0 - Rh) - qb * Rh
    v = qb * (1.0 - Rq) - f * Rq
    return PO.diffuse_step(u, lam_h) + half_dt * ab, PO.diffuse_step(v, lam_q)


def bake_vjp(h0, q0, S, gh, gq, ga, lam_h, lam_q, beta, fl, half_dt, taped=None):
    """(hbar_0, qbar_0) for the cotangents gh, gq, ga of (h_S, q_S, a_S); None = zero.  `taped`: tape(...)[0] of the same
    arguments, when the caller has it already."""
    steps = taped if taped is not None else tape(h0, q0, S, lam_h, lam_q, beta, fl, half_dt)[0]
    shape = steps[0][0].shape
    zero = np.zeros(shape)
    hb, qb, ab = (zero if g is None else np.asarray(g, dtype=np.float64) for g in (gh, gq, ga))
    for hd, qd in reversed(steps):
        hb, qb = step_adjoint(hb, qb, ab, hd, qd, lam_h, lam_q, beta, fl, half_dt)
    return hb, qb


def expose_vjp(image, gains, C, grad_acid):
    """gradImage [F, D, n, n] = sum_g (C g) exp(-(C g) I) gradAcid[g], the gains in ascending order; gradAcid [len(gains) F, D, n, n]."""
    I = np.asarray(image, dtype=np.float64)
    if I.ndim == 3:
        I = I[None]
    g = np.asarray(grad_acid, dtype=np.float64).reshape((len(gains),) + I.shape)
    out = np.zeros(I.shape)
    for i, gain in enumerate(gains):
        Cg = C * float(np.float32(gain))
        out = out + Cg * np.exp(-(Cg * I)) * g[i]
    return out


def inhibitor_vjp(a, k_amp, grad_inhibitor):
    """abar from mbar for m = exp(-k_amp a)."""
    return -k_amp * np.exp(-(k_amp * np.asarray(a, dtype=np.float64))) * np.asarray(grad_inhibitor, dtype=np.float64)


def bound_scale(gh, gq, ga, bake_time):
    """G = max(|gh|_inf, |gq|_inf) + bakeTime |ga|_inf, the scale of (hbar_0, qbar_0)."""
    top = lambda g: 0.0 if g is None else float(np.abs(g).max())               # noqa: E731
    return max(top(gh), top(gq)) + bake_time * top(ga)
