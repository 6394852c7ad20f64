"""CPU restatement (numpy, float64) of resist development, written from the definitions in include/litho_abbe.h -- not from
the kernels: the latent-image diffusion, Mack's rate, the Godunov update G of |grad T| = s iterated as a vectorised Jacobi
sweep from +inf until no cell decreases, and the developed depth.  Nothing in the reference computes any of this, so this file
is the parity target of tests/test_gpu_develop.py; tests/test_develop_cpu.py pins it by closed forms."""
import math

import numpy as np

import resist_oracle as RO

D_MAX = 32


def depths(thickness, D):
    """z_d = (d + 1/2) hz: FilmStack.depths(D)."""
    return np.array([thickness * (d + 0.5) / D for d in range(D)])


def mirror_index(i, D):
    """index -1 - k <-> k, D + k <-> D - 1 - k, repeated as needed."""
    m = i % (2 * D)
    return m if m < D else 2 * D - 1 - m


def diffuse(volume, sigma_xy_px, sigma_z_px):
    """volume [..., D, n, n]: the taps of the lateral resist diffusion (resist_oracle.taps) along x, then y (zero outside the
    grid), then z (mirrored faces), float64."""
    V = RO.diffuse(volume, sigma_xy_px)                                   # rows, then columns; the identity at sigma 0
    g = RO.taps(sigma_z_px)
    R = (len(g) - 1) // 2
    if R == 0:
        return V
    D = V.shape[-3]
    out = np.zeros_like(V)
    for d in range(D):
        for k in range(-R, R + 1):
            out[..., d, :, :] += g[k + R] * V[..., mirror_index(d + k, D), :, :]
    return out


def mack_a(q, m_th):
    return (q + 1.0) / (q - 1.0) * (1.0 - m_th) ** q


def rate_of_m(m, r_max, r_min, q, m_th):
    """Mack's rate as a function of the inhibitor concentration m."""
    a = mack_a(q, m_th)
    x = (1.0 - np.asarray(m, dtype=np.float64)) ** q
    return (r_max * (a + 1.0)) * x / (a + x) + r_min


def surface_factor(thickness, D, r0, delta):
    return 1.0 - (1.0 - r0) * np.exp(-depths(thickness, D) / delta)


def slowness(image, gains, C, r_max, r_min, q, m_th, thickness, r0=1.0, delta=1.0):
    """image [F, D, n, n] -> 1 / r, float64 [len(gains) F, D, n, n], gain-major; gains as the fp32 values the device gets."""
    I = np.asarray(image, dtype=np.float64)
    if I.ndim == 3:
        I = I[None]
    f = surface_factor(thickness, I.shape[1], r0, delta)[None, :, None, None]
    out = []
    for g in gains:
        m = np.exp(-((C * float(np.float32(g))) * I))
        with np.errstate(invalid="ignore"):
            s = 1.0 / (rate_of_m(m, r_max, r_min, q, m_th) * f)
        out.append(np.where(1.0 - m >= 0.0, s, np.nan))              # 1 - m negative or NaN: NaN whatever q (the header)
    return np.concatenate(out, axis=0)


def _shift(T, axis, step):
    """The neighbour at `step` along `axis`, +inf where there is none."""
    out = np.full_like(T, np.inf)
    src = [slice(None)] * T.ndim
    dst = [slice(None)] * T.ndim
    if step > 0:
        src[axis], dst[axis] = slice(step, None), slice(None, -step)
    else:
        src[axis], dst[axis] = slice(None, step), slice(-step, None)
    out[tuple(dst)] = T[tuple(src)]
    return out


def godunov(T, s, h, hz):
    """G(T) for every cell of T [..., D, n, n]; walls (s not finite and positive) give +inf."""
    D = T.shape[-3]
    wall = ~(np.isfinite(s) & (s > 0))
    sv = np.where(wall, 1.0, s)
    ax = np.minimum(_shift(T, -1, 1), _shift(T, -1, -1))
    ay = np.minimum(_shift(T, -2, 1), _shift(T, -2, -1))
    az = np.minimum(_shift(T, -3, 1), _shift(T, -3, -1))
    hzz = np.full(T.shape, float(hz))
    az[..., 0, :, :] = 0.0                                               # the resist top, half a step above plane 0
    hzz[..., 0, :, :] = 0.5 * hz
    a = np.stack([ax, ay, az], axis=-1)
    hh = np.stack([np.full(T.shape, float(h)), np.full(T.shape, float(h)), hzz], axis=-1)
    order = np.argsort(a, axis=-1, kind="stable")
    a = np.take_along_axis(a, order, axis=-1)
    hh = np.take_along_axis(hh, order, axis=-1)
    w = 1.0 / (hh * hh)
    a1 = a[..., 0]
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = np.where(np.isfinite(a[..., 1]), a[..., 1] - a1, np.inf)
        d3 = np.where(np.isfinite(a[..., 2]), a[..., 2] - a1, np.inf)
        u1 = hh[..., 0] * sv
        f2 = np.where(np.isfinite(d2), d2, 0.0)
        f3 = np.where(np.isfinite(d3), d3, 0.0)
        A = w[..., 0] + w[..., 1]
        Bq = w[..., 1] * f2
        Cq = w[..., 1] * f2 * f2 - sv * sv
        u2 = (Bq + np.sqrt(np.maximum(Bq * Bq - A * Cq, 0.0))) / A
        A3 = A + w[..., 2]
        B3 = Bq + w[..., 2] * f3
        C3 = (w[..., 1] * f2 * f2 + w[..., 2] * f3 * f3) - sv * sv
        u3 = (B3 + np.sqrt(np.maximum(B3 * B3 - A3 * C3, 0.0))) / A3
        u = np.where(u1 <= d2, u1, np.where(u2 <= d3, u2, u3))
        G = np.where(np.isfinite(a1), a1 + u, np.inf)
    return np.where(wall, np.inf, G)


def arrival_time(s, thickness, h, max_iterations=100000):
    """(T, iterations): the fixed point of T <- min(T, G(T)) from +inf, Jacobi; s [..., D, n, n]."""
    s = np.asarray(s, dtype=np.float64)
    hz = float(thickness) / s.shape[-3]
    T = np.full(s.shape, np.inf)
    for it in range(1, max_iterations + 1):
        new = np.minimum(T, godunov(T, s, h, hz))
        if not (new < T).any():
            return T, it
        T = new
    raise RuntimeError("develop_oracle.arrival_time: no fixed point")


def developed_depth(T, thickness, t):
    """z* [..., n, n] from T [..., D, n, n]: the first crossing of T = t going down each column."""
    T = np.asarray(T, dtype=np.float64)
    D = T.shape[-3]
    hz = float(thickness) / D
    z = np.full(T.shape[:-3] + T.shape[-2:], float(thickness))
    done = np.zeros(z.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for d in range(D):
            cur = T[..., d, :, :]
            hit = ~done & ~(cur <= t)
            if d == 0:
                val = (0.5 * hz) * (t / cur)
            else:
                prev = T[..., d - 1, :, :]
                frac = np.where(np.isinf(cur), 0.0, (t - prev) / (cur - prev))
                val = (d - 0.5) * hz + hz * frac
            z = np.where(hit, val, z)
            done |= hit
    return z


def serpentine(n, fast, slow):
    """One plane [n, n] of slowness: a channel one cell wide, `fast`, running along the even rows and joined at alternating ends,
    in `slow` surroundings; it is entered at (0, 0)."""
    s = np.full((n, n), float(slow))
    for r in range(0, n, 2):
        s[r, :] = fast
        if r + 1 < n:
            s[r + 1, n - 1 if (r // 2) % 2 == 0 else 0] = fast
    return s
