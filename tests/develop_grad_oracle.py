"""CPU restatement (numpy, float64) of the gradients through development, written from the definitions in include/litho_abbe.h
("Gradients through development") on top of develop_oracle.py -- not from the kernels.  tests/test_develop_grad_cpu.py pins it to
central differences of develop_oracle.arrival_time and develop_oracle.slowness; tests/test_gpu_develop_grad.py compares the
device with it.

  links             per cell: the signed upwind weights alpha of the three axes and sigma, by the header's rules (branch recomputed
                    from the stored T, ties to the lower index, strict upwind, nothing at walls and unreached cells)
  ordered_adjoint   lambda by one pass over the cells in descending T: exact for an acyclic graph
  time_vjp          lambda sigma
  gather_fp32       the device's iteration restated: fp32 links, fp32 Jacobi sweeps of the gather in the kernel's neighbour order
                    until no bit changes
  rate_vjp          the rate law backwards, the gains summed"""
import numpy as np

import develop_oracle as DO


def _neighbours(T):
    """[(minus, plus)] per axis x, y, z; +inf where there is none."""
    return [(DO._shift(T, ax, -1), DO._shift(T, ax, 1)) for ax in (-1, -2, -3)]


def links(T, s, h, hz):
    """(L, sigma): L [..., D, n, n, 3] the signed weights on x, y, z -- positive: the upwind cell is the lower-index neighbour --
    and sigma [..., D, n, n]; both 0 where the cell has no gradient.  T, s float64 arrays holding the stored values."""
    T, s = np.asarray(T, dtype=np.float64), np.asarray(s, dtype=np.float64)
    nb = _neighbours(T)
    lo = [m <= p for m, p in nb]                                           # a tie goes to the lower-index neighbour
    up = [np.where(l, m, p) for l, (m, p) in zip(lo, nb)]
    a = np.stack(up, axis=-1)
    hh = np.stack([np.full(T.shape, float(h)), np.full(T.shape, float(h)), np.full(T.shape, float(hz))], axis=-1)
    a[..., 0, :, :, 2] = 0.0                                               # the resist top, half a step above plane 0
    hh[..., 0, :, :, 2] = 0.5 * hz
    order = np.argsort(a, axis=-1, kind="stable")
    a = np.take_along_axis(a, order, axis=-1)
    hh = np.take_along_axis(hh, order, axis=-1)
    w = 1.0 / (hh * hh)
    active = np.isfinite(s) & (s > 0) & (T < np.inf) & (a[..., 0] < np.inf)
    sv = np.where(active, s, 1.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a0 = np.where(active, a[..., 0], 0.0)
        d1 = np.where(np.isfinite(a[..., 1]), a[..., 1] - a0, np.inf)
        d2 = np.where(np.isfinite(a[..., 2]), a[..., 2] - a0, np.inf)
        f1, f2 = np.where(np.isfinite(d1), d1, 0.0), np.where(np.isfinite(d2), d2, 0.0)
        ss = sv * sv
        w0, w1, w2 = w[..., 0], w[..., 1], w[..., 2]
        u1 = hh[..., 0] * sv
        A = w0 + w1
        u2 = (w1 * f1 + np.sqrt(np.maximum(A * ss - (w0 * w1) * (f1 * f1), 0.0))) / A
        A3 = A + w2
        f21 = f2 - f1
        cross = ((w0 * w1) * (f1 * f1) + (w0 * w2) * (f2 * f2)) + (w1 * w2) * (f21 * f21)
        u3 = ((w1 * f1 + w2 * f2) + np.sqrt(np.maximum(A3 * ss - cross, 0.0))) / A3
        k = np.where(u1 <= d1, 1, np.where(u2 <= d2, 2, 3))
        u = np.where(k == 1, u1, np.where(k == 2, u2, u3))
        p = np.stack([w0 * u, np.where(k >= 2, w1 * (u - f1), 0.0), np.where(k >= 3, w2 * (u - f2), 0.0)], axis=-1)
        P = (p[..., 0] + p[..., 1]) + p[..., 2]
        alpha_sorted = p / P[..., None]
        sigma = np.where(active, sv / P, 0.0)
    alpha = np.zeros_like(alpha_sorted)
    np.put_along_axis(alpha, order, alpha_sorted, axis=-1)                 # back to x, y, z
    L = np.zeros_like(alpha)
    for ax in range(3):
        strict = active & (up[ax] < T)                                     # strict upwind, on the stored values
        if ax == 2:
            strict[..., 0, :, :] = False                                   # plane 0's z axis has no upstream cell
        L[..., ax] = np.where(strict, np.where(lo[ax], alpha[..., ax], -alpha[..., ax]), 0.0)
    return L, sigma


def ordered_adjoint(T, L, sigma, g):
    """lambda for one volume [D, n, n]: the cells in descending stored T, each handing alpha lambda to its upwind cells.  Exact
    because every link points strictly down in T.  g is ignored where sigma = 0."""
    T = np.asarray(T, dtype=np.float64)
    lam = np.where(sigma > 0, np.asarray(g, dtype=np.float64), 0.0)
    idx = np.argwhere(sigma > 0)
    idx = idx[np.argsort(-T[sigma > 0], kind="stable")]
    for d, y, x in idx:
        v = lam[d, y, x]
        lx, ly, lz = L[d, y, x]
        if lx > 0:
            lam[d, y, x - 1] += lx * v
        elif lx < 0:
            lam[d, y, x + 1] -= lx * v
        if ly > 0:
            lam[d, y - 1, x] += ly * v
        elif ly < 0:
            lam[d, y + 1, x] -= ly * v
        if lz > 0:
            lam[d - 1, y, x] += lz * v
        elif lz < 0:
            lam[d + 1, y, x] -= lz * v
    return lam


def time_vjp(T, s, g, thickness, h, hz=None):
    """dl/ds [..., D, n, n] in float64 from the stored T and s and the cotangent g; exactly 0 at walls and unreached cells."""
    T, s, g = (np.asarray(v, dtype=np.float64) for v in (T, s, g))
    hz = float(thickness) / T.shape[-3] if hz is None else float(hz)
    L, sigma = links(T, s, h, hz)
    shape = T.shape
    Tb, Lb, sb, gb = T.reshape((-1,) + shape[-3:]), L.reshape((-1,) + shape[-3:] + (3,)), sigma.reshape((-1,) + shape[-3:]), \
        g.reshape((-1,) + shape[-3:])
    out = np.stack([ordered_adjoint(Tb[b], Lb[b], sb[b], gb[b]) * sb[b] for b in range(Tb.shape[0])])
    return out.reshape(shape)


def _zshift(a, ax, step):
    """The neighbour at `step` along `ax`, 0 where there is none."""
    out = np.zeros_like(a)
    src, dst = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    if step > 0:
        src[ax], dst[ax] = slice(step, None), slice(None, -step)
    else:
        src[ax], dst[ax] = slice(None, step), slice(-step, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def gather_fp32(L, sigma, g, max_sweeps=100000):
    """(grad, sweeps): the device's iteration in fp32 on one volume or a batch.  lambda starts at 0; a sweep is
    lambda_i <- g_i + the terms of x-, x+, y-, y+, z-, z+ in this order, a term only where that neighbour's link points at i, each
    one fp32 multiplication and one addition; it stops at the first sweep that changes no bit.  grad = lambda sigma, 0 where
    sigma = 0."""
    L32, s32, g32 = np.asarray(L, dtype=np.float32), np.asarray(sigma, dtype=np.float32), np.asarray(g, dtype=np.float32)
    lam = np.zeros_like(g32)
    terms = []                                                             # (weight towards i of that neighbour, axis, step)
    for c, ax in enumerate((-1, -2, -3)):
        lc = L32[..., c]
        terms.append((np.maximum(-_zshift(lc, ax, -1), np.float32(0)), ax, -1))   # the lower neighbour, if its link is negative
        terms.append((np.maximum(_zshift(lc, ax, 1), np.float32(0)), ax, 1))      # the higher neighbour, if positive
    for sweep in range(1, max_sweeps + 1):
        with np.errstate(invalid="ignore", over="ignore"):
            acc = g32.copy()
            for wgt, ax, step in terms:
                nb = _zshift(lam, ax, step)
                acc = np.where(wgt > 0, (acc + wgt * nb).astype(np.float32), acc)
        if np.array_equal(acc.view(np.uint32), lam.view(np.uint32)):
            with np.errstate(invalid="ignore", over="ignore"):
                return np.where(s32 > 0, lam * s32, np.float32(0)).astype(np.float32), sweep
        lam = acc
    raise RuntimeError("develop_grad_oracle.gather_fp32: no fixed point")


def rate_vjp(x, gains, kappa, r_max, r_min, q, m_th, thickness, r0, delta, grad_s):
    """x [F, D, n, n] (or [D, n, n]), grad_s [len(gains) F, D, n, n] gain-major -> dl/dx shaped like x, float64; the gains as the
    fp32 values the device gets.  A wall (1 - m negative or NaN) contributes 0 whatever grad_s holds there."""
    x = np.asarray(x, dtype=np.float64)
    single = x.ndim == 3
    X4 = x[None] if single else x
    F, D = X4.shape[0], X4.shape[1]
    gs = np.asarray(grad_s, dtype=np.float64).reshape((len(gains), F) + X4.shape[1:])
    f = DO.surface_factor(thickness, D, r0, delta)[None, :, None, None]
    a = DO.mack_a(q, m_th)
    R = r_max * (a + 1.0)
    out = np.zeros_like(X4)
    for i, gain in enumerate(gains):
        kg = kappa * float(np.float32(gain))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            m = np.exp(-(kg * X4))
            b = 1.0 - m
            ok = b >= 0.0
            bs = np.where(ok, b, 0.5)
            Xq = bs ** q
            r = (R * Xq / (a + Xq) + r_min) * f
            s = 1.0 / r
            ds = -(s * s) * f * (R * a / ((a + Xq) * (a + Xq))) * (q * bs ** (q - 1.0) * (kg * m))
            out += np.where(ok, np.where(ok, gs[i], 0.0) * ds, 0.0)
    return out[0] if single else out
