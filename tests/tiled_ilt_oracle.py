"""CPU restatement of tiled inverse lithography (lithographysimulator_amd/tiling.py optimizeMaskTiled) in
float64, composed from the existing oracles and changing none: the window cut, its adjoint (overlap-add) and the stitch's
adjoint as numpy slicing, the batched gradient as socs_grad_oracle.gradient tile by tile, and the whole tiled loss with its
gradient with respect to the one global theta, built from socs_grad_oracle.model's bookends window by window.
TEST INFRASTRUCTURE ONLY.

Tolerances of the one-iterate comparison (tests/test_gpu_tiled_ilt.py), by the rule at the head of socs_grad_oracle.py: the same
chain evaluated in torch's CPU complex64 / float32 against float64 on exactly the device test's cases (ILT_TILED_CASES: pn 32 /
halo 8 and pn 64 / halo 16, 3 x 2 tiles, 25 nm and 193 / 8 nm, binary and attenuated background, one plane and two;
test_tiled_ilt_cpu.py::test_fp32_floor_of_the_tiled_loop prints and re-checks it).  Measured:
    losses[0], losses[1]  relative 5.2e-8;   (theta0 - theta1) / step, peak 1  absolute 5.6e-6
(step 1 / 16, as there).  Both are under a quarter of socs_grad_oracle's bounds (TOL_ILT_LOSS 7.6e-7 / 4 = 1.9e-7, TOL_ILT_UPDATE
2.3e-5 / 4 = 5.8e-6), so those bounds hold here unchanged: losses 7.6e-7 relative, update 2.3e-5 absolute.  Were a floor above the
quarter, the bound would be four times the floor (the expressions below)."""
import numpy as np
import torch

import socs_grad_oracle as GO
import tiling_oracle as TO

C128 = GO.C128
WL = 193.0
PS_EPS1 = 193.0 / 8.0
# the measured complex64 floors of the tiled one-iterate loop over ILT_TILED_CASES, and the bounds they give
TILED_FLOOR_LOSS, TILED_FLOOR_UPDATE = 5.2e-8, 5.6e-6
TOL_TILED_LOSS = GO.TOL_ILT_LOSS if TILED_FLOOR_LOSS < GO.TOL_ILT_LOSS / 4 else 4 * TILED_FLOOR_LOSS
TOL_TILED_UPDATE = GO.TOL_ILT_UPDATE if TILED_FLOOR_UPDATE < GO.TOL_ILT_UPDATE / 4 else 4 * TILED_FLOOR_UPDATE


# ---- the three copies --------------------------------------------------------------------------------------------------------------
def cut(plane, place, pn, halo, fill):
    """[count,pn,pn] of plane's dtype: windows[t][r][c] = plane[place[t].row - halo + r][place[t].col - halo + c], `fill` outside."""
    plane = np.asarray(plane)
    rows, cols = plane.shape
    out = np.full((len(place), pn, pn), fill, dtype=plane.dtype)
    for t, (r0, c0) in enumerate(np.asarray(place).tolist()):
        for r in range(pn):
            gr = r0 - halo + r
            if not 0 <= gr < rows:
                continue
            c_lo, c_hi = max(0, halo - c0), min(pn, cols - c0 + halo)
            if c_hi > c_lo:
                out[t, r, c_lo:c_hi] = plane[gr, c0 - halo + c_lo:c0 - halo + c_hi]
    return out


def overlap_add(windows, place, halo, rows, cols):
    """[rows,cols] of the windows' dtype: the adjoint of `cut`, the windows added in ascending tile order into a sum of their own
    precision that starts from zero (complex64 windows: one fp32 sum per component, the kernel's definition bit for bit)."""
    windows = np.asarray(windows)
    pn = windows.shape[-1]
    out = np.zeros((rows, cols), dtype=windows.dtype)
    for t, (r0, c0) in enumerate(np.asarray(place).tolist()):
        r_lo, r_hi = max(0, halo - r0), min(pn, rows - r0 + halo)
        c_lo, c_hi = max(0, halo - c0), min(pn, cols - c0 + halo)
        if r_hi > r_lo and c_hi > c_lo:
            out[r0 - halo + r_lo:r0 - halo + r_hi, c0 - halo + c_lo:c0 - halo + c_hi] += windows[t, r_lo:r_hi, c_lo:c_hi]
    return out


def unstitch(image, place, nt, j0, core):
    """[count,planes,nt,nt] of the image's dtype: the adjoint of tiling_oracle.stitch -- the cores read back, zero around them and
    where a core leaves the image."""
    image = np.asarray(image)
    planes, n = image.shape[0], image.shape[-1]
    out = np.zeros((len(place), planes, nt, nt), dtype=image.dtype)
    for t, (r0, c0) in enumerate(np.asarray(place).tolist()):
        i0, i1 = max(0, -r0), min(core, n - r0)
        k0, k1 = max(0, -c0), min(core, n - c0)
        if i1 > i0 and k1 > k0:
            out[t][:, j0 + i0:j0 + i1, j0 + k0:j0 + k1] = image[:, r0 + i0:r0 + i1, c0 + k0:c0 + k1]
    return out


def plan_place(nx, ny, core):
    """int32 [ny nx, 2]: (row, col) of the cores of an nx x ny plan, tile t = iy nx + ix, as planTiles lays them."""
    return np.array([(iy * core, ix * core) for iy in range(ny) for ix in range(nx)], dtype=np.int32)


# ---- the batched gradient ----------------------------------------------------------------------------------------------------------
def gradient_batch(kernels, Ms, N, Gs, dtype=C128):
    """[B,pn,pn]: socs_grad_oracle.gradient tile by tile; Gs [B,pn,pn] or [B,planes,pn,pn]."""
    return torch.stack([GO.gradient(kernels, Ms[b], N, Gs[b], dtype=dtype) for b in range(len(Ms))])


# ---- the tiled loss as a function of one global theta ------------------------------------------------------------------------------
class TiledModel:
    """loss(theta) and its gradient for a TilePlan on socs_grad_oracle's chain: t = bg + span sigmoid(a theta), the windows cut
    from it (background outside), per window model(...)'s imager, the cores stitched, socs_grad_oracle.ilt_loss on
    image[:, :rows, :cols]; backwards ilt_grad_image, the stitch's adjoint, per window model(...)'s adjoint, overlap-add,
    ilt_grad_theta.  `kernels` [planes,K,pn,pn]; `target` [n,n] or [planes,n,n]."""

    def __init__(self, plan, kernels, target, threshold, dose, a_r, a_m, background, gain, dtype=C128):
        self.plan, self.kernels, self.dtype = plan, torch.as_tensor(kernels), dtype
        assert self.kernels.dim() == 4
        self.rows, self.cols = plan.ny * plan.core, plan.nx * plan.core
        self.target = torch.as_tensor(target).double()[..., :self.rows, :self.cols]
        self.threshold, self.dose, self.a_r, self.a_m, self.background = threshold, dose, a_r, a_m, background
        from oracle import abbe_oracle as O
        self.eps, self.N = O.calculate_epsilon_n(4 / plan.pixelNumber, plan.pixelSize, plan.wavelength)
        self.models = [GO.model(self.kernels, plan.pixelNumber, self.eps, self.N, gain, dtype=dtype) for _ in range(plan.count)]

    def image(self, theta):
        """float64 [planes,n,n]: the stitched image of theta (every window's adjoint then belongs to this theta)."""
        p = self.plan
        t = GO.ilt_transmission(theta, self.background, 1, self.a_m).numpy()
        windows = cut(t, p.place, p.pixelNumber, p.halo, complex(self.background))
        tiles = np.stack([self.models[i][0](torch.from_numpy(windows[i])).double().numpy() for i in range(p.count)])
        assert tiles.shape[-1] == p.n_tile
        return torch.from_numpy(TO.stitch(tiles, p.place, p.j0, p.core, p.n))

    def loss(self, theta):
        return GO.ilt_loss(self.image(theta)[:, :self.rows, :self.cols], self.target, self.threshold, self.dose, self.a_r)

    def loss_and_gradient(self, theta):
        """(loss, dl/dtheta float64 [rows,cols])."""
        p = self.plan
        covered = self.image(theta)[:, :self.rows, :self.cols]
        loss = GO.ilt_loss(covered, self.target, self.threshold, self.dose, self.a_r)
        g_cov = GO.ilt_grad_image(covered, self.target, self.threshold, self.dose, self.a_r)
        g_image = np.zeros((covered.shape[0], p.n, p.n))
        g_image[:, :self.rows, :self.cols] = g_cov.numpy()
        g_tiles = unstitch(g_image, p.place, p.n_tile, p.j0, p.core)
        g_windows = np.stack([self.models[i][1](torch.from_numpy(g_tiles[i])).to(C128).numpy() for i in range(p.count)])
        g_t = overlap_add(g_windows, p.place, p.halo, self.rows, self.cols)
        return loss, GO.ilt_grad_theta(theta, torch.from_numpy(g_t), self.background, 1, self.a_m)

    def one_iterate(self, theta0, step):
        """(losses[0], losses[1], (theta0 - theta1) / step) of optimizeMaskTiled's first update, the peak-normalised step."""
        l0, g = self.loss_and_gradient(theta0)
        update = g / g.abs().max()
        return l0, self.loss(torch.as_tensor(theta0).double() - step * update), update


# ---- the cases the CPU floor measurement and the GPU test share --------------------------------------------------------------------
ILT_TILED_CASES = [(pn, halo, ps, kind, planes) for pn, halo in ((32, 8), (64, 16)) for ps in (25.0, PS_EPS1)
                   for kind in ("binary", "attenuated") for planes in (1, 2)]
_cases = {}


class TiledCase:
    """One setting: a 3 x 2 plan, K = 3 kernels of socs_grad_oracle.sized_case per plane, theta0 seeded normal of 0.5 sigma, a
    seeded Bernoulli target on the stitched grid ([n,n] for one plane, [planes,n,n] for a stack), the threshold at the median of
    dose . image(theta0) over the covered region, resistSteepness 25 / threshold, gain 1 / ILT_WEIGHT_SUM, step 1 / 16 -- as
    socs_grad_oracle.IltCase.  The planes of a stack are scaled to one median."""

    def __init__(self, pn, halo, ps, kind, planes, nx=3, ny=2):
        from lithographysimulator_amd.tiling import planTiles
        core = pn - 2 * halo
        self.plan = planTiles((0.0, 0.0, nx * core * ps, ny * core * ps), pn, ps, WL, halo)
        assert (self.plan.nx, self.plan.ny) == (nx, ny)
        self.planes, self.background = planes, GO.ILT_BACKGROUNDS[kind]
        self.gain = 1.0 / GO.ILT_WEIGHT_SUM
        self.rows, self.cols, n = ny * core, nx * core, self.plan.n
        from oracle import abbe_oracle as O
        N = O.calculate_epsilon_n(4 / pn, ps, WL)[1]
        k = GO.sized_case(pn, N, 3, planes)[0]
        self.kernels = (k if planes > 1 else k[None]).contiguous()
        g = torch.Generator().manual_seed(9000 + 10 * pn + planes + int(ps))
        self.theta0 = (0.5 * torch.randn((self.rows, self.cols), generator=g, dtype=torch.float64)).to(torch.float32)
        shape = (planes, n, n) if planes > 1 else (n, n)
        self.target = (torch.rand(shape, generator=g, dtype=torch.float64) > 0.5).to(torch.float32)
        if planes > 1:
            med = self.model(0.0, 1.0).image(self.theta0)[:, :self.rows, :self.cols].flatten(1).median(dim=1).values
            self.kernels = (self.kernels * torch.sqrt(med[0] / med).to(torch.float32)[:, None, None, None]).contiguous()
        image0 = self.model(0.0, 1.0).image(self.theta0)[:, :self.rows, :self.cols]
        self.threshold = GO.ILT_DOSE * float(image0.median())
        self.a_r = 25.0 / self.threshold
        self._reference = None

    def model(self, threshold=None, a_r=None, dtype=C128):
        return TiledModel(self.plan, self.kernels, self.target, self.threshold if threshold is None else threshold, GO.ILT_DOSE,
                          self.a_r if a_r is None else a_r, GO.ILT_MASK_STEEPNESS, self.background, self.gain, dtype=dtype)

    def reference(self):
        """The float64 one-iterate result, computed once."""
        if self._reference is None:
            self._reference = self.model().one_iterate(self.theta0, GO.ILT_STEP)
        return self._reference


def tiled_case(pn, halo, ps, kind, planes):
    key = (pn, halo, ps, kind, planes)
    if key not in _cases:
        _cases[key] = TiledCase(pn, halo, ps, kind, planes)
    return _cases[key]
