"""CPU restatement of the area-coverage rasteriser (litho_rasterize_coverage) -- TEST INFRASTRUCTURE ONLY.

No new rasteriser: the definition in include/litho_abbe.h IS an identity with the binary one -- sub-centre (R, C) of the
s x s supersampled pixel grid is inside exactly when oracle.layout_oracle.rasterize_edges at (pn * s, pixel / s) on the
same origin sets pixel (R, C) -- so the restatement is that raster plus an s x s block sum.  tests/test_coverage_cpu.py
pins it with closed-form areas."""
import numpy as np

from oracle import layout_oracle as LO


def coverage_counts(edges: np.ndarray, pn: int, x0: float, y0: float, pixel: float, s: int) -> np.ndarray:
    """int64 [pn, pn]: the number of inside sub-centres of every pixel (coverage * s^2)."""
    fine = LO.rasterize_edges(edges, pn * s, x0, y0, pixel / s)           # pixel / s: the one fp64 division of the definition
    return fine.astype(np.int64).reshape(pn, s, pn, s).sum(axis=(1, 3))


def coverage(edges: np.ndarray, pn: int, x0: float, y0: float, pixel: float, s: int) -> np.ndarray:
    """float32 [pn, pn] in [0, 1]; exact for the power-of-two s the rasteriser takes."""
    return (coverage_counts(edges, pn, x0, y0, pixel, s) / float(s * s)).astype(np.float32)


def random_layout(seed: int, pn: int, pixel: float, s: int, n: int = 12):
    """A dozen rectangles, triangles and concave (star-shaped) polygons in either orientation, overlapping and partly outside
    the window [0, pn pixel]^2, plus polygons with vertices exactly ON sub-centres and ON sub-grid lines of the origin (0, 0)."""
    rng = np.random.default_rng(seed)
    span, q = pn * pixel, pixel / s
    polys = []
    for i in range(n):
        cx, cy = rng.uniform(-0.1 * span, 1.0 * span, 2)
        kind = i % 3
        if kind == 0:
            w, h = rng.uniform(0.05 * span, 0.4 * span, 2)
            p = np.array([[cx, cy], [cx + w, cy], [cx + w, cy + h], [cx, cy + h]])
        elif kind == 1:
            p = np.array([cx, cy]) + rng.uniform(-0.3 * span, 0.3 * span, (3, 2))
        else:
            k = int(rng.integers(5, 11))
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            rad = rng.uniform(0.03 * span, 0.25 * span, k)
            p = np.array([cx, cy]) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
        polys.append(p[::-1] if rng.integers(2) else p)
    m = pn * s                                                             # sub-grid units below
    a, b = max(2, m // 5), max(4, (3 * m) // 5)
    polys.append(np.array([[a + 0.5, a + 0.5], [b + 0.5, a + 0.5], [b + 0.5, b - 1 + 0.5], [a + 0.5, b - 1 + 0.5]]) * q)   # on sub-centres
    polys.append(np.array([[a + 1.0, b], [m - 2.0, b], [(a + m) // 2 * 1.0, m - 1.0]]) * q)                              # on sub-grid lines
    return polys
