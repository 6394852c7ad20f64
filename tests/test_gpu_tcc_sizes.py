"""litho_tcc_apply (csrc/socs.hip) at every size class: n = 16 ... 2048 with batch 3, batch 1 at 1024 and 2048 (4096 stays with
test_gpu_fft2.py: the line transforms are shared, and the float64 truth of the operator there costs more than a few seconds).

The kernel reads the pupil spectrum TRANSPOSED and the weight map in natural orientation, so the inputs are asymmetric on
purpose: P random complex inside an ellipse centred off the grid centre (P != P^T), W >= 0 with random weights inside an
off-centre disc, X random complex; all seeded on the CPU.  A pupil or weight map that is symmetric under transposition could not
tell a missing or an extra transpose; the test asserts, on the CPU, that its truth moves by more than 100 x the bound when P^T
or W^T takes the place of P or W.

Truth: socs_oracle.dense_apply in complex128 (pinned against the explicit operator in test_socs_cpu.py).  Error = max |got -
truth| / max |truth|; bound = 4 x the error of the same formula in torch CPU complex64 on the same input -- the project's rule,
the floor taken from the reference arithmetic.  In place equals out of place bit for bit, and out of place leaves X alone.

Hermitian form: T is Hermitian, so h = <X2, T X1> - conj <X1, T X2> vanishes.  With Y_i = T X_i + E_i the device gives
h = <X2, E1> - conj <X1, E2>, and a relative error `bound` of each Y_i, taken in the 2-norm, allows
|h| <= bound (||X2|| ||T X1|| + ||X1|| ||T X2||) -- the issue's 2 bound ||X1|| ||X2||, scaled by ||T X|| / ||X|| of the truth.
The inner products are accumulated in float64.  This sees what breaks the symmetry between the correlation and the convolution
-- a missing conjugate (3,500 x the allowance on the CPU at n 64), a transpose in one of the two pupil factors only; a transpose
in both gives another, equally Hermitian, operator and is left to the comparison with the truth.

The complex64 floor takes torch's inverse transforms unscaled (norm="forward") and puts n^-4 on the weight map: torch's scaled
complex64 ifft2 on the CPU was seen to apply its 1 / n^2 twice at n = 2048 on one machine (complex128 and every other size were
right), which made the floor 1.0 there.

Measured on an MI355X: error / complex64 floor 0.95 ... 1.40 at batch 3 except 2.27 at n 512 (bound 4), 1.29 and 1.05 at batch 1
(n 1024, 2048); absolute errors 2.7e-7 ... 5.9e-7; in place equal to out of place bit for bit everywhere; the truth moves by
0.82 ... 1.27 of its maximum under P^T or W^T (4e5 ... 1.6e6 x the bound); Hermitian form 1.4e-5 ... 6.0e-3 of its allowance."""
import numpy as np
import pytest
import torch

import socs_oracle as SO

pytestmark = pytest.mark.gpu
CASES = [(n, 3) for n in (16, 32, 64, 128, 256, 512, 1024, 2048)] + [(1024, 1), (2048, 1)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    assert _native.lib().litho_target_arch() == b"gfx950"
    return _native


def _inputs(n, batch):
    """(P complex64 [n,n], W float32 [n,n], X complex64 [batch,n,n]): ellipse and disc off the centre, neither symmetric under
    transposition."""
    g = torch.Generator().manual_seed(100 * n + batch)
    r, c = torch.meshgrid(torch.arange(n, dtype=torch.float64), torch.arange(n, dtype=torch.float64), indexing="ij")
    ellipse = ((r - 0.44 * n) / (0.30 * n)) ** 2 + ((c - 0.57 * n) / (0.17 * n)) ** 2 <= 1.0
    disc = (r - 0.58 * n) ** 2 + (c - 0.39 * n) ** 2 <= (0.21 * n) ** 2
    P = torch.view_as_complex(torch.randn((n, n, 2), generator=g, dtype=torch.float32)) * ellipse
    W = (torch.rand((n, n), generator=g, dtype=torch.float32) * disc).contiguous()
    X = torch.view_as_complex(torch.randn((batch, n, n, 2), generator=g, dtype=torch.float32))
    return P.contiguous(), W, X


def _formula64(P, W, X):
    """dense_apply's formula in torch CPU complex64: the floor of the bound.  The inverse transforms are taken unscaled, as
    test_gpu_fft2.py takes them, and their n^-4 -- a power of two, exact -- goes onto the weight map, where the kernel puts it."""
    n = P.shape[-1]
    ph, wsh = torch.fft.fft2(P), torch.fft.ifftshift(W) * (1.0 / float(n) ** 4)
    inner = torch.fft.ifft2(ph.conj() * torch.fft.fft2(X), norm="forward")
    return torch.fft.ifft2(ph * torch.fft.fft2(wsh * inner), norm="forward").numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _apply(nat, dev, ph, wsh, X, Y):
    nat.check(nat.lib().litho_tcc_apply(nat.ptr(ph), nat.ptr(wsh), nat.ptr(X), nat.ptr(Y), X.shape[0], X.shape[-1],
                                        nat.stream_ptr(dev)), "litho_tcc_apply")
    torch.cuda.synchronize()
    return Y


@pytest.mark.parametrize("n,batch", CASES)
def test_tcc_apply_at_every_size(nat, dev, n, batch):
    P, W, X = _inputs(n, batch)
    p, w, x = P.numpy(), W.numpy(), X.numpy()
    want = SO.dense_apply(p, w, x)
    floor = _rel(_formula64(P, W, X), want)
    bound = 4 * floor
    # the inputs can tell a transpose: the truth with P^T, or with W^T, is far from the truth (first vector; CPU only)
    moved_p = _rel(SO.dense_apply(p.T, w, x[0]), want[0])
    moved_w = _rel(SO.dense_apply(p, w.T, x[0]), want[0])
    assert moved_p > 100 * bound and moved_w > 100 * bound, (n, moved_p, moved_w, bound)

    ph = P.to(dev).clone()
    nat.check(nat.lib().litho_fft2_c2c(nat.ptr(ph), 1, n, 0, nat.stream_ptr(dev)), "litho_fft2_c2c")
    wsh = torch.fft.ifftshift(W).contiguous().to(dev)
    Xd = X.to(dev)
    out = _apply(nat, dev, ph, wsh, Xd, torch.empty_like(Xd))
    assert torch.equal(Xd.cpu(), X)                                            # out of place leaves X alone
    got = out.cpu().numpy()
    e_out = _rel(got, want)
    inplace = _apply(nat, dev, ph, wsh, Xd, Xd)
    same = torch.equal(inplace, out)
    print(f"n {n} batch {batch}: error {e_out:.3e}, complex64 floor {floor:.3e}, quotient {e_out / floor:.2f} (bound 4); in place "
          f"{'==' if same else '!='} out of place; truth moves by {moved_p:.2e} under P^T, {moved_w:.2e} under W^T "
          f"({moved_p / bound:.0f} x, {moved_w / bound:.0f} x the bound)")
    assert e_out <= bound
    assert same

    # Hermitian form, from the device's own output; batch 1 pairs the vector with itself (<X, T X> is real)
    i, j = (0, 1) if batch > 1 else (0, 0)
    x1, x2 = x[i].astype(np.complex128).ravel(), x[j].astype(np.complex128).ravel()
    y1, y2 = got[i].astype(np.complex128).ravel(), got[j].astype(np.complex128).ravel()
    h = abs(np.vdot(x2, y1) - np.conj(np.vdot(x1, y2)))
    allowed = bound * (np.linalg.norm(x2) * np.linalg.norm(want[i]) + np.linalg.norm(x1) * np.linalg.norm(want[j]))
    print(f"n {n} batch {batch}: |<X2, T X1> - conj <X1, T X2>| = {h:.3e}, allowed {allowed:.3e} ({h / allowed:.2e} of it)")
    assert h <= allowed


def test_refusals(nat, dev):
    n = 16
    ph = torch.zeros((n, n), dtype=torch.complex64, device=dev)
    w = torch.zeros((n, n), dtype=torch.float32, device=dev)
    X = torch.ones((1, n, n), dtype=torch.complex64, device=dev)
    Y = torch.full((1, n, n), 2.0, dtype=torch.complex64, device=dev)
    f, st = nat.lib().litho_tcc_apply, nat.stream_ptr(dev)
    for bad_n in (8, 8192):
        assert f(nat.ptr(ph), nat.ptr(w), nat.ptr(X), nat.ptr(Y), 1, bad_n, st) == nat.E_ARG
    assert f(nat.ptr(ph), nat.ptr(w), nat.ptr(X), nat.ptr(Y), 0, n, st) == nat.E_ARG
    assert f(None, nat.ptr(w), nat.ptr(X), nat.ptr(Y), 1, n, st) == nat.E_ARG
    assert f(nat.ptr(ph), None, nat.ptr(X), nat.ptr(Y), 1, n, st) == nat.E_ARG
    assert f(nat.ptr(ph), nat.ptr(w), None, nat.ptr(Y), 1, n, st) == nat.E_ARG
    assert f(nat.ptr(ph), nat.ptr(w), nat.ptr(X), None, 1, n, st) == nat.E_ARG
    torch.cuda.synchronize()
    assert bool((X == 1).all()) and bool((Y == 2).all())                        # a refused call writes nothing
