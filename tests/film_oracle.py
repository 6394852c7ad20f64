"""CPU restatement of the resist film stack definition (include/litho_abbe.h) in numpy float64, written from
the definition and not from csrc/film.hip or lithographysimulator_amd/film.py: the parity target of litho_film_pupils,
filmPupils, film._host_film_pupils and vectorSocsKernels(film=).  Two formulations of the same boundary-value problem:

  `matrix`  products of 2 x 2 characteristic matrices acting on (u, v), from the substrate up -- the textbook form, fine where
            cos / sin of a complex phase do not overflow;
  `stable`  Fresnel coefficients r, t per interface, the reflection ratio swept upward and the transmitted amplitude downward,
            the upward wave of a layer referenced to that layer's bottom -- finite for any thickness and absorption.

They are pinned to closed forms and to each other in tests/test_film_cpu.py.  TEST INFRASTRUCTURE ONLY.

Conventions: a wave advancing by z into the wafer carries exp(-i kappa z); an absorbing medium (n, k), k >= 0, is n - i k;
w = sqrt(nn^2 - s) with Im w <= 0 (Re w > 0 when Im w = 0), kappa = 2 pi w / lambda.  A stack is given as plain data:
`layers` [(n, k, d_nm), ...] from the top down, `substrate` (n, k), `resist` the 0-based index of the sampled layer."""
import numpy as np

import vector_oracle as VO


def indices(n0, layers, substrate):
    """Complex indices of the media: incident, the layers, substrate."""
    return [complex(n0)] + [complex(n, -k) for n, k, _ in layers] + [complex(substrate[0], -substrate[1])]


def root(nn, s):
    """w = sqrt(nn^2 - s) on the branch Im w <= 0, Re w > 0 when Im w = 0; s a real array."""
    w = np.sqrt(nn * nn - np.asarray(s, dtype=np.float64).astype(np.complex128))
    w = np.where(w.imag > 0, -w, w)
    return np.where((w.imag == 0) & (w.real < 0), -w, w)


def _etas(pol, nn, s):
    ws = [root(m, s) for m in nn]
    return ws, [w if pol == "s" else w / (m * m) for w, m in zip(ws, nn)]


def solve_matrix(pol, n0, layers, substrate, resist, s, wavelength, depths):
    """(u [D,...], v [D,...], u_sub, v_sub) of one scalar problem by characteristic matrices.  With delta = kappa h the state at
    the top of a slab of thickness h follows from the state at its bottom by [[cos, i sin / eta], [i eta sin, cos]]."""
    nn = indices(n0, layers, substrate)
    ws, etas = _etas(pol, nn, s)
    a0 = 1.0 if pol == "s" else n0
    k0 = 2.0 * np.pi / wavelength

    def lift(u, v, m, h):
        delta = k0 * ws[m] * h
        c, sn = np.cos(delta), np.sin(delta)
        return c * u + 1j * sn / etas[m] * v, 1j * etas[m] * sn * u + c * v

    u, v = np.ones_like(ws[-1]), etas[-1] * np.ones_like(ws[-1])                  # substrate: one downward wave of amplitude 1
    R = resist + 1
    for m in range(len(layers), R, -1):
        u, v = lift(u, v, m, layers[m - 1][2])
    bottom = (u, v)                                                               # state at the bottom of the resist
    for m in range(R, 0, -1):
        u, v = lift(u, v, m, layers[m - 1][2])
    # at the top: u = a0 (1 + r), v = eta0 a0 (1 - r)  =>  2 a0 eta0 = eta0 u + v per unit substrate amplitude
    t_sub = 2.0 * a0 * etas[0] / (etas[0] * u + v)
    d_res = layers[resist][2]
    us, vs = zip(*[lift(bottom[0], bottom[1], R, d_res - float(z)) for z in np.atleast_1d(depths)])
    return np.stack(us) * t_sub, np.stack(vs) * t_sub, t_sub, etas[-1] * t_sub


def solve_stable(pol, n0, layers, substrate, resist, s, wavelength, depths):
    """The same four quantities by Fresnel coefficients, bottom-referenced: nothing grows."""
    nn = indices(n0, layers, substrate)
    ws, etas = _etas(pol, nn, s)
    a0 = 1.0 if pol == "s" else n0
    k0 = 2.0 * np.pi / wavelength
    L = len(layers)
    r = [(etas[m] - etas[m + 1]) / (etas[m] + etas[m + 1]) for m in range(L + 1)]
    t = [2.0 * etas[m] / (etas[m] + etas[m + 1]) for m in range(L + 1)]
    e = [None] + [np.exp(-1j * k0 * ws[m] * layers[m - 1][2]) for m in range(1, L + 1)]
    gamma = [None] * (L + 2)                                                      # upward / downward at the TOP of medium m
    rho = [None] * (L + 1)                                                        # the same at the BOTTOM of medium m
    gamma[L + 1] = np.zeros_like(ws[0])
    for m in range(L, -1, -1):
        rho[m] = (r[m] + gamma[m + 1]) / (1.0 + r[m] * gamma[m + 1])
        if m > 0:
            gamma[m] = rho[m] * e[m] * e[m]
    a = [None] * (L + 2)                                                          # downward amplitude at the top of medium m
    at_bottom = a0 * np.ones_like(ws[0])
    for m in range(L + 1):
        a[m + 1] = at_bottom * t[m] / (1.0 + r[m] * gamma[m + 1])
        if m + 1 <= L:
            at_bottom = a[m + 1] * e[m + 1]
    R = resist + 1
    d_res = layers[resist][2]
    us, vs = [], []
    for z in np.atleast_1d(depths):
        down = a[R] * np.exp(-1j * k0 * ws[R] * float(z))
        up = rho[R] * a[R] * e[R] * np.exp(-1j * k0 * ws[R] * (d_res - float(z)))
        us.append(down + up)
        vs.append(etas[R] * (down - up))
    return np.stack(us), np.stack(vs), a[L + 1], etas[L + 1] * a[L + 1]


SOLVERS = {"matrix": solve_matrix, "stable": solve_stable}


def film_fields(n0, layers, substrate, resist, s, wavelength, depths, method="stable"):
    """(E_s, E_rad, E_z), each complex128 [D, ...] over the array s: E_s = u_s, E_rad = v_p, E_z = -(sqrt(s) / nn^2) u_p."""
    solve = SOLVERS[method]
    us, _, _, _ = solve("s", n0, layers, substrate, resist, s, wavelength, depths)
    up, vp, _, _ = solve("p", n0, layers, substrate, resist, s, wavelength, depths)
    nn = indices(n0, layers, substrate)[resist + 1]
    return us, vp, -(np.sqrt(np.asarray(s, dtype=np.float64)) / (nn * nn)) * up


def film_pupils(P, NA, n0, layers, substrate, resist, depths, wavelength, radiometric=False, defocus=None, method="stable"):
    """complex128 [D,6,pn,pn] of one pupil plane and one defocus value (None: no phase), plane t = 2 c + j."""
    P = np.asarray(P, dtype=np.complex128)
    pn = P.shape[0]
    a, b, g, inside = VO.cosines(pn, NA, n0)
    s0 = np.where(inside, a * a + b * b, 0.0)
    Es, Erad, Ez = film_fields(n0, layers, substrate, resist, n0 * n0 * s0, wavelength, depths, method)
    centre = s0 == 0.0
    norm = np.where(centre, 1.0, np.sqrt(np.where(centre, 1.0, s0)))
    rx, ry = np.where(centre, 0.0, a / norm), np.where(centre, 0.0, b / norm)
    tx, ty = -ry, rx
    Erad = np.where(centre, Es, Erad)
    diag = np.where(centre, 1.0, 0.0)                                             # at s = 0: E_s on the diagonal, 0 elsewhere
    Q = np.stack([tx * Es * tx + rx * Erad * rx + diag * Es, tx * Es * ty + rx * Erad * ry,
                  ty * Es * tx + ry * Erad * rx, ty * Es * ty + ry * Erad * ry + diag * Es,
                  Ez * rx, Ez * ry], axis=1)                                      # [D,6,pn,pn]
    f = (1.0 / np.sqrt(g) if radiometric else 1.0) * inside
    Q = Q * (P * f)[None, None]
    return Q * VO.defocus_phase(pn, NA, n0, float(defocus), float(wavelength))[None, None] if defocus is not None else Q


# ---- the stacks the CPU and the GPU tests share --------------------------------------------------------------------------------
WL = 193.0
WATER = 1.44
SILICON = (0.88, 2.78)                          # n, k at 193 nm
STACKS = {
    # water / resist / silicon
    "L1": ([(1.70, 0.02, 120.0)], SILICON, 0),
    # water / top coat / resist / BARC / silicon, the resist in the middle
    "L3": ([(1.55, 0.0, 35.0), (1.70, 0.02, 100.0), (1.82, 0.34, 40.0)], SILICON, 1),
}


def stack16(resist):
    """Sixteen layers with indices, absorptions and thicknesses that are all different; layer 6 is frustrated at NA 1.35."""
    layers = [(1.45 + 0.05 * ((5 * i) % 7), 0.03 * ((3 * i) % 4), 12.0 + 7.0 * ((7 * i) % 5)) for i in range(16)]
    layers[6] = (1.30, 0.0, 15.0)
    return layers, SILICON, resist
