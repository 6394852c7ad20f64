"""litho_fft2_c2c -- the plain 2-D DFT of the SOCS set-up (csrc/socs.hip: line transforms of fft_core.hpp, tiled transposes) --
against numpy complex128, at n = 16, 32, 64, 128, 512, 2048 and at 256, 1024, 4096 as well: every size is its own instantiation
of the line transform (another leading radix, another number of radix-16 passes, 1 to 256 threads per line, 64 to 1 lines per
workgroup).  Batch 1 and 3 (4096: 1 and 2, to keep the float64 truth quick), both directions.

Error = max |got - truth| / max |truth|.  Bound = 4 x the error of torch's CPU complex64 fft2 on the same input, computed here --
the project's "4 x the fp32 floor" rule of test_gpu_spectrum.py, with the floor taken from the reference arithmetic and never from
the code under test.  Forward then inverse returns n^2 x under the same bound (4 x the forward floor of that input).

n = 16 with a batch of 65,537 runs the transposes' second launch (grid.z holds 65,535 matrices), and the matrices of that launch
are held to the bound on their own as well.

Measured on an MI355X: error / floor 0.76 ... 1.29 over the 36 one-way cases, 1.18 ... 1.96 over the 18 round trips; batch 65,537:
1.07 both ways, matrices 65,535 and 65,536 at 6.4e-8 and 5.2e-8 of the batch's maximum, 0.97 of their own complex64 floor."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
CASES = [(n, b) for n in SIZES for b in ((1, 2) if n == 4096 else (1, 3))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    assert _native.lib().litho_target_arch() == b"gfx950"
    return _native


_inputs = {}


def _make_input(n, batch):
    g = torch.Generator().manual_seed(1000 * n + batch)
    x = torch.view_as_complex(torch.randn((batch, n, n, 2), generator=g, dtype=torch.float32))
    x128 = x.numpy().astype(np.complex128)
    fwd = np.fft.fft2(x128)
    inv = np.fft.ifft2(x128) * float(n * n)
    floor_f = np.abs(torch.fft.fft2(x).numpy() - fwd).max() / np.abs(fwd).max()
    floor_i = np.abs(torch.fft.ifft2(x, norm="forward").numpy() - inv).max() / np.abs(inv).max()
    return x, fwd, inv, floor_f, floor_i


def _input(n, batch):
    """(x complex64, forward truth, inverse truth, forward floor, inverse floor), computed once per shape."""
    if (n, batch) not in _inputs:
        _inputs[(n, batch)] = _make_input(n, batch)
    return _inputs[(n, batch)]


def _fft2(nat, dev, t, inverse):
    rc = nat.lib().litho_fft2_c2c(nat.ptr(t), t.shape[0], t.shape[-1], 1 if inverse else 0, nat.stream_ptr(dev))
    nat.check(rc, "litho_fft2_c2c")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("n,batch", CASES)
@pytest.mark.parametrize("inverse", [False, True])
def test_fft2_against_float64(nat, dev, n, batch, inverse):
    x, fwd, inv, floor_f, floor_i = _input(n, batch)
    want, floor = (inv, floor_i) if inverse else (fwd, floor_f)
    got = _fft2(nat, dev, x.to(dev), inverse).cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"n {n} batch {batch} {'inverse' if inverse else 'forward'}: error {err:.3e}, floor {floor:.3e}, quotient {err / floor:.2f} (bound 4)")
    assert err <= 4 * floor


@pytest.mark.parametrize("n,batch", CASES)
def test_forward_then_inverse_returns_n2_x(nat, dev, n, batch):
    x, fwd, inv, floor_f, floor_i = _input(n, batch)
    t = x.to(dev)
    _fft2(nat, dev, t, False)
    got = _fft2(nat, dev, t, True).cpu().numpy()
    want = x.numpy().astype(np.complex128) * float(n * n)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"n {n} batch {batch} round trip: error {err:.3e}, forward floor {floor_f:.3e}, quotient {err / floor_f:.2f} (bound 4)")
    assert err <= 4 * floor_f


@pytest.fixture(scope="module")
def many():
    """n 16, batch 65,537: transpose() launches grid.z = 65,535 matrices and then the other two.  (x, forward truth, inverse
    truth, floors) as _input gives them, kept for this module's two directions only."""
    return _make_input(16, 65537)


@pytest.mark.parametrize("inverse", [False, True])
def test_fft2_batch_beyond_one_transpose_launch(nat, dev, many, inverse):
    x, fwd, inv, floor_f, floor_i = many
    want, floor = (inv, floor_i) if inverse else (fwd, floor_f)
    got = _fft2(nat, dev, x.to(dev), inverse).cpu().numpy()
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    # the matrices of the second transpose launch, on their own: against the whole batch's scale under the whole batch's bound,
    # and each against its own maximum under 4 x the complex64 floor of these matrices
    tail = slice(65535, None)
    ref = (torch.fft.ifft2(x[tail], norm="forward") if inverse else torch.fft.fft2(x[tail])).numpy()
    own = np.abs(want[tail]).max(axis=(1, 2))
    tail_err = np.abs(got[tail] - want[tail]).max(axis=(1, 2))
    tail_floor = (np.abs(ref - want[tail]).max(axis=(1, 2)) / own).max()
    print(f"n 16 batch 65537 {'inverse' if inverse else 'forward'}: error {err:.3e}, floor {floor:.3e}, quotient {err / floor:.2f} "
          f"(bound 4); matrices 65535, 65536: {tail_err / scale} of the batch's maximum, {tail_err / own} of their own (floor "
          f"{tail_floor:.3e}, quotient {(tail_err / own).max() / tail_floor:.2f}, bound 4)")
    assert err <= 4 * floor
    assert (tail_err / scale <= 4 * floor).all()
    assert (tail_err / own <= 4 * tail_floor).all()
    assert np.abs(want[tail]).min() > 0 and not np.array_equal(got[65535], got[65536])


def test_refusals(nat, dev):
    t = torch.zeros((1, 64, 64), dtype=torch.complex64, device=dev)
    f = nat.lib().litho_fft2_c2c
    for n in (8, 48, 30, 8192):
        assert f(nat.ptr(t), 1, n, 0, nat.stream_ptr(dev)) == nat.E_ARG
    assert f(nat.ptr(t), 0, 64, 0, nat.stream_ptr(dev)) == nat.E_ARG
    assert f(None, 1, 64, 0, nat.stream_ptr(dev)) == nat.E_ARG
    torch.cuda.synchronize()
    assert int((t != 0).sum()) == 0
