"""litho_tcc_apply_vector (csrc/socs.hip) at every size class, with batches that make its pointwise kernels walk: modelled on
test_gpu_tcc_sizes.py, which holds the scalar operator the same way (n = 4096 stays with test_gpu_fft2.py for the reason given
there: the line transforms are shared, and the float64 truth of the operator at that size costs more than a few seconds).

k_vec_fan_out, k_vec_mix and k_vec_fan_in walk the vectors b = blockIdx.y, blockIdx.y + gridDim.y, ... with
gridDim.y = min(max(2048 / ceil(n^2 / 512), 1), batch).  Every case but the first has batch > gridDim.y and, where gridDim.y > 1,
batch no multiple of it, so the walk takes a second step and its last step is partial:

    n      batch   gridDim.y   walk steps   transpose launches of U (6 batch matrices, 65,535 per launch)
    16         3        3          1          1      smallest size, half-empty workgroup (128 of 256 threads)
    16     10923     2048          6          2      the second launch carries 3 matrices
    32      1030     1024          2          1      second step for 6 values of blockIdx.y
    64       300      256          2          1
    128       70       64          2          1
    256       20       16          2          1
    512        6        4          2          1      second step for blockIdx.y 0 and 1
    1024       3        1          3          1
    2048       2        1          2          1      the `by < 1` clamp (2048 / 4096 = 0)

Inputs: vector_oracle.random_setting, shared with test_gpu_vector.py -- six planes inside an off-centre ellipse, three weight
maps inside an off-centre disc with W_xx != W_yy and W_xy of both signs, seeded on the CPU.  Before any launch the test asserts,
on the CPU and on the first vector, that the truth moves by more than 100 x the bound when Q^T takes the place of Q and when the
polarisation index is exchanged.

Truth: vector_oracle.fft_apply in complex128.  Error per vector e_b = max |got_b - want_b| / max |want_b|; bound = 4 x the
largest such error of the same 14-transform formula in torch CPU complex64 (vector_oracle.formula64) over the batch -- the
project's rule, the floor taken from reference arithmetic and never from the device.

Independent of the batch, bit for bit: vector 0, vector gridDim.y (the first of the second walk step) and vector batch - 1 of
the large call each equal a call with that vector alone; at (16, 10923) also vectors 10921 and 10922, which lie in the second
transpose launch of U.  In place equals out of place; out of place leaves X alone and a second call repeats the first (the
last two not at (16, 10923) and (2048, 2)).  Hermitian form from the device's own outputs, as test_gpu_tcc_sizes.py derives it.
Alignment: every buffer 8 bytes into its allocation (the weight maps 4), bit-equal to the aligned call, canaries intact.

Measured on an MI355X (error / complex64 floor, bound 4; Hermitian form as a share of its allowance):

    n      batch   quotient   Hermitian share
    16         3     1.44        7.6e-3
    16     10923     1.04        3.5e-3
    32      1030     1.07        4.2e-3
    64       300     1.20        7.9e-4
    128       70     1.56        7.6e-4
    256       20     1.21        6.9e-5
    512        6     2.17        5.0e-5      (the scalar operator has 2.27 at this size)
    1024       3     1.35        5.1e-5
    2048       2     0.99        1.3e-5

Absolute errors 3.1e-7 ... 6.0e-7, floors 2.1e-7 ... 5.6e-7; the truth moves by 0.66 ... 0.90 of its maximum under Q^T and by 0.19 ...
0.26 under an exchange of the polarisation index (1e5 ... 1e6 x the bound).  Every single-vector call equals its vector in the
batch bit for bit, in place equals out of place equals a second call, the misaligned call equals the aligned one and no canary
moves.  With `b += gridDim.y + 1` in k_vec_mix (a scratch build, once) the eight cases with batch > gridDim.y fail and the
operator tests of test_gpu_vector.py pass.  The whole file takes ten seconds, five of them the CPU side of (2048, 2)."""
import time

import numpy as np
import pytest
import torch

import vector_oracle as VO

pytestmark = pytest.mark.gpu
CASES = [(16, 3), (16, 10923), (32, 1030), (64, 300), (128, 70), (256, 20), (512, 6), (1024, 3), (2048, 2)]
IN_PLACE_ONLY = {(16, 10923), (2048, 2)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    assert _native.lib().litho_target_arch() == b"gfx950"
    return _native


def grid_y(n, batch):
    """gridDim.y of the three pointwise kernels, from the rule in litho_tcc_apply_vector."""
    bx = (n * n // 2 + 255) // 256
    return min(max(2048 // bx, 1), batch)


def _per_vector(got, want):
    """max over the batch of max |got_b - want_b| / max |want_b|."""
    d = np.abs(got - want).reshape(got.shape[0], -1).max(axis=1)
    return float((d / np.abs(want).reshape(want.shape[0], -1).max(axis=1)).max())


def _apply(nat, dev, qh, wsh, X, Y, work=None):
    batch, n = X.shape[0], X.shape[-1]
    need = int(nat.lib().litho_tcc_apply_vector_work_bytes(batch, n))
    assert need == 48 * (batch + 1) * n * n
    if work is None:
        work = torch.empty(need, dtype=torch.uint8, device=dev)
    nat.check(nat.lib().litho_tcc_apply_vector(nat.ptr(qh), nat.ptr(wsh), nat.ptr(X), nat.ptr(Y), batch, n, nat.ptr(work), need,
                                               nat.stream_ptr(dev)), "litho_tcc_apply_vector")
    torch.cuda.synchronize()
    return Y


def _spectra(nat, dev, Q):
    qh = Q.to(dev).clone()
    nat.check(nat.lib().litho_fft2_c2c(nat.ptr(qh), 6, Q.shape[-1], 0, nat.stream_ptr(dev)), "litho_fft2_c2c")
    return qh


def test_the_cases_walk():
    """The table in the head, from the launch rule: a change of the geometry shows here which cases have to move with it."""
    for n, batch in CASES:
        by = grid_y(n, batch)
        steps, launches = -(-batch // by), -(-6 * batch // 65535)
        print(f"n {n} batch {batch}: gridDim.y {by}, walk steps {steps}, transpose launches of U {launches}")
        if (n, batch) != (16, 3):
            assert batch > by and steps >= 2 and (batch % by != 0 or by == 1)       # the last step is partial where it can be
    assert grid_y(16, 10923) == 2048 and -(-10923 // 2048) == 6 and 6 * 10923 - 65535 == 3
    assert grid_y(2048, 2) == 1 and 2048 // ((2048 * 2048 // 2 + 255) // 256) == 0


@pytest.mark.parametrize("n,batch", CASES)
def test_tcc_apply_vector_at_every_size(nat, dev, n, batch):
    t0 = time.perf_counter()
    Q, maps, X = VO.random_setting(n, batch)
    q, m, x = Q.numpy(), maps.numpy(), X.numpy()
    want = VO.fft_apply(q, m, x)
    floor = _per_vector(VO.formula64(Q, maps, X), want)
    bound = 4 * floor
    # the inputs can tell a transpose and an exchange of the polarisation index (first vector; CPU only, before any launch)
    moved = _per_vector(VO.fft_apply(q.transpose(0, 2, 1), m, x[:1]), want[:1])
    swapped = _per_vector(VO.fft_apply(q[[1, 0, 3, 2, 5, 4]], m, x[:1]), want[:1])
    assert moved > 100 * bound and swapped > 100 * bound, (n, moved, swapped, bound)
    t_cpu = time.perf_counter() - t0

    by = grid_y(n, batch)
    qh, wsh = _spectra(nat, dev, Q), torch.fft.ifftshift(maps, dim=(-2, -1)).contiguous().to(dev)
    Xd = X.to(dev)
    if (n, batch) in IN_PLACE_ONLY:
        out = Xd.clone()
        _apply(nat, dev, qh, wsh, out, out)
    else:
        out = _apply(nat, dev, qh, wsh, Xd, torch.empty_like(Xd))
        assert torch.equal(Xd.cpu(), X)                                        # out of place leaves X alone
        again = _apply(nat, dev, qh, wsh, Xd, torch.empty_like(Xd))
        inplace = Xd.clone()
        _apply(nat, dev, qh, wsh, inplace, inplace)
        print(f"n {n} batch {batch}: in place {'==' if torch.equal(inplace, out) else '!='} out of place, second call "
              f"{'==' if torch.equal(again, out) else '!='} first")
        assert torch.equal(inplace, out) and torch.equal(again, out)
        del again, inplace
    got = out.cpu().numpy()
    e = _per_vector(got, want)
    print(f"n {n} batch {batch} gridDim.y {by}: error {e:.3e}, complex64 floor {floor:.3e}, quotient {e / floor:.2f} (bound 4); truth "
          f"moves by {moved:.2e} under Q^T and {swapped:.2e} under an exchange of the polarisation index "
          f"({moved / bound:.0f} x, {swapped / bound:.0f} x the bound); CPU side {t_cpu:.1f} s")
    assert e <= bound

    # a vector's result does not depend on its batch: bit for bit against a call with that vector alone
    if batch > by:
        alone = [0, by, batch - 1] + ([10921, 10922] if (n, batch) == (16, 10923) else [])
        for b in sorted(set(alone)):
            one = Xd[b:b + 1].clone()
            _apply(nat, dev, qh, wsh, one, one)
            same = torch.equal(one[0], out[b])
            print(f"n {n} batch {batch}: vector {b}{' (= gridDim.y)' if b == by else ''} alone {'==' if same else '!='} in the batch")
            assert same, (n, batch, b)

    # Hermitian form, from the device's own output
    x1, x2 = x[0].astype(np.complex128).ravel(), x[1].astype(np.complex128).ravel()
    y1, y2 = got[0].astype(np.complex128).ravel(), got[1].astype(np.complex128).ravel()
    h = abs(np.vdot(x2, y1) - np.conj(np.vdot(x1, y2)))
    allowed = bound * (np.linalg.norm(x2) * np.linalg.norm(want[0]) + np.linalg.norm(x1) * np.linalg.norm(want[1]))
    print(f"n {n} batch {batch}: |<X2, T X1> - conj <X1, T X2>| = {h:.3e}, allowed {allowed:.3e} ({h / allowed:.2e} of it)")
    assert h <= allowed


def _offset_view(like, offset, fill, dev):
    """A tensor shaped like `like` that starts `offset` elements into a fresh allocation filled with `fill`, one spare element
    behind it; (allocation, view)."""
    alloc = torch.full((like.numel() + offset + 1,), fill, dtype=like.dtype, device=dev)
    view = alloc[offset:offset + like.numel()].view(like.shape)
    return alloc, view


@pytest.mark.parametrize("n", [16, 64])
def test_buffers_that_are_not_16_byte_aligned(nat, dev, n):
    """The kernels read and write 16 bytes at a time from buffers promised 8-byte aligned only (the weight maps 4): X, Y, q_hat
    and work start 8 bytes into their allocations, w_shifted 4.  Same bits as the aligned call; the samples before and after
    Y and work keep their values."""
    batch = 3
    Q, maps, X = VO.random_setting(n, batch)
    qh, wsh = _spectra(nat, dev, Q), torch.fft.ifftshift(maps, dim=(-2, -1)).contiguous().to(dev)
    Xd = X.to(dev)
    ref = _apply(nat, dev, qh, wsh, Xd, torch.empty_like(Xd))
    need = int(nat.lib().litho_tcc_apply_vector_work_bytes(batch, n))
    canary = 7.0 - 3.0j
    _, x_v = _offset_view(Xd, 1, 0.0, dev)
    y_all, y_v = _offset_view(Xd, 1, canary, dev)
    _, q_v = _offset_view(qh, 1, 0.0, dev)
    _, w_v = _offset_view(wsh, 1, 0.0, dev)
    work_all = torch.full((need + 16,), 0xA5, dtype=torch.uint8, device=dev)
    work_v = work_all[8:8 + need]
    x_v.copy_(Xd), q_v.copy_(qh), w_v.copy_(wsh)
    for name, t, mod in (("X", x_v, 16), ("Y", y_v, 16), ("q_hat", q_v, 16), ("work", work_v, 16), ("w_shifted", w_v, 8)):
        assert t.data_ptr() % mod == mod // 2 and t.is_contiguous(), name
    _apply(nat, dev, q_v, w_v, x_v, y_v, work=work_v)
    same = torch.equal(y_v, ref)
    intact = (bool(y_all[0] == canary) and bool(y_all[-1] == canary) and bool((work_all[:8] == 0xA5).all())
              and bool((work_all[8 + need:] == 0xA5).all()))
    print(f"n {n} batch {batch}: buffers at 8 (mod 16) bytes, weights at 4 (mod 8): {'==' if same else '!='} the aligned call; "
          f"canaries {'intact' if intact else 'OVERWRITTEN'}")
    assert same and intact and torch.equal(x_v, Xd)
    inplace = x_v
    _apply(nat, dev, q_v, w_v, inplace, inplace, work=work_v)
    assert torch.equal(inplace, ref)
