"""CPU restatement of the contour tracer (litho_contour_count / litho_contour_emit, litho_contour_link's order and the host
polygon rules), written from the definition in include/litho_abbe.h -- not from the kernel.  Nothing in the reference computes
it, so this file is the parity target of tests/test_gpu_contour.py; tests/test_contour_cpu.py pins it by closed forms and by
the raster round trip.

The kernel works edge by edge (which cell does the contour enter, which way does it turn); this file works CELL by cell: the
four sides of a cell taken counter-clockwise, a side that runs from an inside corner to an outside one is where a contour
ENTERS (the feature on its left), one that runs from outside to inside is where it LEAVES.  Products, the saddle's centre value
and the vertex positions are NumPy float32, operation for operation; alongside, the fraction is evaluated in float64 from the
same fp32 a, b with its condition number, for the tolerance of the GPU comparison."""
import numpy as np

F = np.float32


def products(u, gain):
    """fl32(u * gain): one fp32 multiply."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.asarray(u, dtype=F) * F(gain)
    assert a.dtype == F
    return a


def inside_of(a, T, exposed):
    with np.errstate(invalid="ignore"):
        return (a >= F(T)) == bool(exposed)                          # NaN compares false


def trace(u, gain, T, exposed):
    """One image u [n, n] fp32 at one gain.  Returns a dict:
    xy float32 [V, 2], next int32 [V]; horizontal bool [V] (an H edge: x is interpolated; else y); whole int64 [V, 2] the integer
    (c, r) the fraction is added to; frac64 float64 [V] the
    fraction in float64 from the fp32 a, b (0 on an edge with a virtual end); cond float64 [V] = (|T| + |a| + |b|) / |b - a|
    (0 where nothing is interpolated or t is forced to 0.5); saddles = (joined, cut) counts."""
    a = products(u, gain)
    n = a.shape[0]
    T32 = F(T)
    ins = np.zeros((n + 2, n + 2), dtype=bool)                        # [r + 1, c + 1]; the virtual ring is never inside
    ins[1:-1, 1:-1] = inside_of(a, T, exposed)
    hx = ins[1:-1, :-1] != ins[1:-1, 1:]                              # H(r, c): [r, c + 1], r = 0 .. n - 1, c = -1 .. n - 1
    vx = ins[:-1, 1:-1] != ins[1:, 1:-1]                              # V(r, c): [r + 1, c], r = -1 .. n - 1, c = 0 .. n - 1
    idh = np.full(hx.shape, -1, dtype=np.int64)
    idv = np.full(vx.shape, -1, dtype=np.int64)
    xy, whole, frac64, cond, horizontal = [], [], [], [], []
    T64 = float(T32)

    def cut(lo, hi):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = (T32 - lo) / (hi - lo)
            forced = not (t >= 0 and t <= 1)
            if forced:
                return F(0.5), 0.5, 0.0
            lo64, hi64 = float(lo), float(hi)
            if not (np.isfinite(lo64) and np.isfinite(hi64)):                     # finite / infinite = 0 exactly: nothing rounds
                return t, float(t), 0.0
            return t, (T64 - lo64) / (hi64 - lo64), (abs(T64) + abs(lo64) + abs(hi64)) / abs(hi64 - lo64)

    k = 0
    for r in range(-1, n):
        if r >= 0:
            for e in np.nonzero(hx[r])[0]:
                c = int(e) - 1
                idh[r, e] = k
                k += 1
                horizontal.append(True)
                if c < 0 or c + 1 >= n:
                    xr = 0 if c < 0 else n - 1
                    xy.append((F(xr), F(r))); whole.append((xr, r)); frac64.append(0.0); cond.append(0.0)
                else:
                    t, t64, cn = cut(a[r, c], a[r, c + 1])
                    xy.append((F(c) + t, F(r))); whole.append((c, r)); frac64.append(t64); cond.append(cn)
        for c in np.nonzero(vx[r + 1])[0]:
            c = int(c)
            idv[r + 1, c] = k
            k += 1
            horizontal.append(False)
            if r < 0 or r + 1 >= n:
                yr = 0 if r < 0 else n - 1
                xy.append((F(c), F(yr))); whole.append((c, yr)); frac64.append(0.0); cond.append(0.0)
            else:
                t, t64, cn = cut(a[r, c], a[r + 1, c])
                xy.append((F(c), F(r) + t)); whole.append((c, r)); frac64.append(t64); cond.append(cn)
    V = k
    nxt = np.full(V, -1, dtype=np.int64)
    joined = cutoff = 0
    # cell (i, j) between extended rows i - 1, i and columns j - 1, j; only cells whose corners differ carry a contour
    blk = ins[:-1, :-1].astype(np.int8) + ins[:-1, 1:] + ins[1:, :-1] + ins[1:, 1:]
    for i, j in zip(*np.nonzero((blk > 0) & (blk < 4))):
        i, j = int(i), int(j)
        # corners in (x, y = row upwards) axes, counter-clockwise: low-row/low-col, low-row/high-col, high-row/high-col, high-row/low-col
        corner = [ins[i, j], ins[i, j + 1], ins[i + 1, j + 1], ins[i + 1, j]]
        # sides counter-clockwise, side s runs from corner s to corner s + 1: H(i - 1, j - 1), V(i - 1, j), H(i, j - 1), V(i - 1, j - 1)
        side = [idh[i - 1, j] if i >= 1 else -1, idv[i, j] if j < n else -1, idh[i, j] if i < n else -1, idv[i, j - 1] if j >= 1 else -1]
        enter = [s for s in range(4) if corner[s] and not corner[(s + 1) % 4]]
        leave = [s for s in range(4) if not corner[s] and corner[(s + 1) % 4]]
        assert len(enter) == len(leave) and all(side[s] >= 0 for s in enter + leave)
        if len(enter) == 1:
            nxt[side[enter[0]]] = side[leave[0]]
            continue
        # saddle: two diagonal corners inside, all four real
        assert 1 <= i <= n - 1 and 1 <= j <= n - 1
        m = ((a[i, j - 1] + a[i, j]) + (a[i - 1, j - 1] + a[i - 1, j])) * F(0.25)
        join = bool(inside_of(m, T, exposed))
        joined += join
        cutoff += not join
        for s in enter:
            # joined: the OUTSIDE corner s + 1 is cut off, the contour leaves through the side after it; otherwise the inside
            # corner s is cut off and the contour leaves through the side before it
            nxt[side[s]] = side[(s + 1) % 4] if join else side[(s - 1) % 4]
    assert (nxt >= 0).all()
    return dict(xy=np.array(xy, dtype=F).reshape(V, 2), next=nxt.astype(np.int32), whole=np.array(whole, dtype=np.int64).reshape(V, 2),
                frac64=np.array(frac64), cond=np.array(cond), horizontal=np.array(horizontal, dtype=bool), saddles=(joined, cutoff), inside=ins[1:-1, 1:-1].copy())


def cycles(nxt):
    """The cycles of the permutation, each from its lowest index, ordered by it: a list of index lists."""
    nxt = np.asarray(nxt)
    seen = np.zeros(len(nxt), dtype=bool)
    out = []
    for v0 in range(len(nxt)):
        if seen[v0]:
            continue
        cyc, v = [], v0
        while not seen[v]:
            seen[v] = True
            cyc.append(v)
            v = int(nxt[v])
        assert v == v0, "not a permutation"
        out.append(cyc)
    return out


def area(q):
    q = np.asarray(q, dtype=np.float64)
    return 0.5 * float(np.sum(q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1]))


def polygons(xy, nxt):
    """The host rule: cycles as float64 polygons, consecutive duplicates collapsed (cyclically), fewer than three left: dropped."""
    pts = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    out = []
    for cyc in cycles(nxt):
        q = pts[cyc]
        keep = [k for k in range(len(q)) if not np.array_equal(q[k], q[k - 1])]
        if len(keep) >= 3:
            out.append(q[keep])
    return out


def edges_of(polys):
    """[n_edges, 4] (x0, y0, x1, y1) with every polygon's orientation KEPT."""
    rows = [np.concatenate([q, np.roll(q, -1, axis=0)], axis=1) for q in polys]
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, 4))
