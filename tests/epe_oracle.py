"""CPU restatement of the edge-placement-error kernel (litho_measure_epe), written from the definition in
include/litho_abbe.h -- not from the kernel.  Nothing in the reference computes it, so this file is the parity target of
tests/test_gpu_epe.py; tests/test_epe_cpu.py pins it by closed-form cases.

Samples and classification are NumPy float32, operation for operation (every array below that carries a sample is float32,
so each * and + rounds once, as the kernel's do without contraction); the crossing's position is float64."""
import math

import numpy as np

F = np.float32
H = 0.5


def samples(image_f32, sites, range_px):
    """(v, valid, t): v float32 [planes, S, 2K + 1] the bilinear samples (0 where invalid), valid bool [S, 2K + 1],
    t float32 [2K + 1] = k / 2 for k = -K .. K."""
    img = np.asarray(image_f32, dtype=F)
    if img.ndim == 2:
        img = img[None]
    n = img.shape[-1]
    s = np.asarray(sites, dtype=F).reshape(-1, 4)
    K = int(math.ceil(float(F(range_px)) / H))
    assert 1 <= K <= 64
    t = np.arange(-K, K + 1).astype(F) * F(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        px = s[:, 0:1] + t[None, :] * s[:, 2:3]                  # one multiply, one add, float32
        py = s[:, 1:2] + t[None, :] * s[:, 3:4]
        top = F(n - 1)
        valid = np.isfinite(px) & np.isfinite(py) & (px >= 0) & (px <= top) & (py >= 0) & (py <= top) & (n >= 2)
    pxs, pys = np.where(valid, px, F(0)), np.where(valid, py, F(0))
    ix = np.minimum(np.floor(pxs).astype(np.int64), max(n - 2, 0))
    iy = np.minimum(np.floor(pys).astype(np.int64), max(n - 2, 0))
    fx, fy = pxs - ix.astype(F), pys - iy.astype(F)
    if n < 2:
        return np.zeros((img.shape[0],) + px.shape, dtype=F), valid, t
    one = F(1)
    a, b, c, d = img[:, iy, ix], img[:, iy, ix + 1], img[:, iy + 1, ix], img[:, iy + 1, ix + 1]
    v = (one - fy) * ((one - fx) * a + fx * b) + fy * ((one - fx) * c + fx * d)
    assert v.dtype == F
    return np.where(valid[None], v, F(0)), valid, t


def measure_epe(image_f32, sites, gains, threshold, exposed, range_px, pixel_size):
    """image [planes, n, n] or [n, n] fp32; sites [S, 4] = (x, y, nx, ny).  Returns (table, cond): table float64
    [n_gains, planes, S, 3] = (epe_nm, ils_per_nm, t_k), three NaN where no crossing lies in range; cond float64
    [n_gains, planes, S] = the condition term (|T| + |u_a| + |u_b|) / |u_b - u_a| of the crossing's division (0 at NaN)."""
    v, valid, t = samples(image_f32, sites, range_px)
    planes, S, M = v.shape
    T32, ps = F(threshold), float(F(pixel_size))
    k = np.arange(M - 1) - (M - 1) // 2                             # interval k = -K .. K - 1
    key = 2 * np.abs(2 * k + 1) - (k >= 0)                          # smallest |2k + 1|, a tie goes to k >= 0
    table = np.full((len(gains), planes, S, 3), np.nan)
    cond = np.zeros((len(gains), planes, S))
    for gi, gain in enumerate(gains):
        u32 = v * F(gain)
        inside = (u32 >= T32) == bool(exposed)
        cross = valid[None, :, :-1] & valid[None, :, 1:] & inside[..., :-1] & ~inside[..., 1:]
        pick = np.where(cross, key[None, None, :], np.iinfo(np.int64).max).argmin(axis=-1)
        found = cross.any(axis=-1)
        u = u32.astype(np.float64)
        ua = np.take_along_axis(u, pick[..., None], axis=-1)[..., 0]
        ub = np.take_along_axis(u, pick[..., None] + 1, axis=-1)[..., 0]
        tk = t.astype(np.float64)[pick]
        T = float(T32)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = ub - ua
            ts = tk + H * ((T - ua) / den)
            ils = np.abs(den) / ((H * ps) * T)
            cn = (abs(T) + np.abs(ua) + np.abs(ub)) / np.abs(den)
        table[gi, ..., 0] = np.where(found, ts * ps, np.nan)
        table[gi, ..., 1] = np.where(found, ils, np.nan)
        table[gi, ..., 2] = np.where(found, tk, np.nan)
        cond[gi] = np.where(found, cn, 0.0)
    return table, cond
