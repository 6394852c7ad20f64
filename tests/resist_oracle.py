"""CPU restatement (numpy, float64) of the diffused aerial image and the sub-pixel edge finder, written from the
definitions in include/litho_abbe.h -- not from the kernels.  Nothing in the reference computes either, so this file is
the parity target of tests/test_gpu_resist.py; tests/test_resist_cpu.py pins it by closed-form cases."""
import math

import numpy as np

R_MAX = 32


def taps(sigma_px):
    """g[k], k = -R..R, R = ceil(4 sigma): exp(-k^2 / (2 sigma^2)) normalised to sum 1 in double, rounded to fp32
    (returned as float64 holding the fp32 values).  sigma 0 -> [1]."""
    sigma_px = float(sigma_px)
    if not (sigma_px >= 0.0) or math.isinf(sigma_px):
        raise ValueError("sigma_px must be finite and >= 0")
    if sigma_px == 0.0:
        return np.ones(1)
    R = int(math.ceil(4.0 * sigma_px))
    if R > R_MAX:
        raise ValueError("4 sigma spans more than 32 pixels")
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma_px * sigma_px))
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def radius(sigma_px):
    return (len(taps(sigma_px)) - 1) // 2


def diffuse(image, sigma_px):
    """image [..., n, n] (zero outside the grid) convolved with the taps along the rows and along the columns, float64."""
    I = np.asarray(image, dtype=np.float64)
    g = taps(sigma_px)
    R = (len(g) - 1) // 2
    if R == 0:
        return I.copy()
    n_y, n_x = I.shape[-2], I.shape[-1]
    pad = [(0, 0)] * (I.ndim - 2)
    P = np.pad(I, pad + [(0, 0), (R, R)])
    rows = np.zeros_like(I)
    for k in range(-R, R + 1):                       # D[x] = sum_k g[k] I[x + k]  (g is symmetric)
        rows += g[k + R] * P[..., :, R + k: R + k + n_x]
    P = np.pad(rows, pad + [(R, R), (0, 0)])
    out = np.zeros_like(I)
    for k in range(-R, R + 1):
        out += g[k + R] * P[..., R + k: R + k + n_y, :]
    return out


def contour(image_f32, gain, threshold):
    """uint8 mask: fp32(image * gain) >= fp32(threshold)."""
    u = np.asarray(image_f32, dtype=np.float32) * np.float32(gain)
    return (u >= np.float32(threshold)).astype(np.uint8)


def measure_line(v_f32, c, gain, threshold, exposed, pixel_size):
    """One gauge on one line.  Returns (cd_nm, x_lo, x_hi, ils_lo, ils_hi, lo, hi, tol_lo, tol_hi); classification in
    fp32 (so lo, hi are what any fp32 implementation finds), positions in float64.  tol_* = the condition term
    (|T| + |u_a| + |u_b|) / |u_b - u_a| of the crossing's division (0 at a border); lo = hi = -1 when cd = 0."""
    v = np.asarray(v_f32, dtype=np.float32)
    n = v.shape[0]
    T32 = np.float32(threshold)
    u32 = v * np.float32(gain)
    inside = (u32 >= T32) == bool(exposed)
    nan = float("nan")
    if not inside[c]:
        return (0.0, nan, nan, nan, nan, -1, -1, 0.0, 0.0)
    lo = c
    while lo > 0 and inside[lo - 1]:
        lo -= 1
    hi = c
    while hi < n - 1 and inside[hi + 1]:
        hi += 1
    u, T, ps = u32.astype(np.float64), float(T32), float(pixel_size)

    def crossing(a, b):
        den = u[b] - u[a]
        with np.errstate(divide="ignore", invalid="ignore"):
            ils = float(np.float64(abs(den)) / np.float64(T * ps))
        return a + (T - u[a]) / den, ils, (abs(T) + abs(u[a]) + abs(u[b])) / abs(den)

    x_lo, ils_lo, tol_lo = (-0.5, nan, 0.0) if lo == 0 else crossing(lo - 1, lo)
    x_hi, ils_hi, tol_hi = (n - 0.5, nan, 0.0) if hi == n - 1 else crossing(hi, hi + 1)
    return ((x_hi - x_lo) * ps, x_lo, x_hi, ils_lo, ils_hi, lo, hi, tol_lo, tol_hi)


def measure_cd(image_f32, gauges, gains, threshold, exposed, pixel_size):
    """image [planes, n, n] or [n, n] fp32; gauges (row, col, axis) triples.  Returns (table, runs, tols):
    table float64 [n_gains, planes, G, 5] = (cd_nm, x_lo, x_hi, ils_lo, ils_hi), runs int [.., 2] = (lo, hi),
    tols float64 [.., 2]; five NaN for a gauge outside the grid."""
    img = np.asarray(image_f32, dtype=np.float32)
    if img.ndim == 2:
        img = img[None]
    planes, n = img.shape[0], img.shape[-1]
    gauges = [tuple(int(t) for t in g) for g in gauges]
    table = np.full((len(gains), planes, len(gauges), 5), np.nan)
    runs = np.full((len(gains), planes, len(gauges), 2), -1, dtype=np.int64)
    tols = np.zeros((len(gains), planes, len(gauges), 2))
    for gi, gain in enumerate(gains):
        for p in range(planes):
            for k, (row, col, axis) in enumerate(gauges):
                if not (0 <= row < n and 0 <= col < n and axis in (0, 1)):
                    continue
                line, c = (img[p, row, :], col) if axis == 0 else (img[p, :, col], row)
                res = measure_line(line, c, gain, threshold, exposed, pixel_size)
                table[gi, p, k] = res[:5]
                runs[gi, p, k] = res[5:7]
                tols[gi, p, k] = res[7:9]
    return table, runs, tols
