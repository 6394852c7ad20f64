"""Weighted (grey-level) sources, I = sum_s w_s |E_s|^2, without a GPU: the argument errors of the two new C entries, the
float64 identity behind the weighted coarse-grid path (why k_nyquist_edges must carry w_s), and the host logic of
abbeImage(group=, weighted=True) on two gloo ranks with oracle stand-ins for the device entry points."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT


@pytest.fixture(scope="module")
def nat():
    from lithographysimulator_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", ROOT, "-j", "8", "all"])
    return _native


def test_argument_errors_before_any_gpu_work(nat):
    lib = nat.lib()
    # NULL image / spectrum / pupil: an argument error, as for litho_abbe_accumulate_opts
    assert lib.litho_abbe_accumulate_weighted(None, None, 1, None, None, 0, 256, 512, None, None, 0, None, None, None, None,
                                              None) == nat.E_ARG
    # odd pn, and NULL pointers
    eight = nat.c_void_p(8)
    assert lib.litho_source_compact_weighted(eight, 63, eight, eight, 63 * 63, eight, None, None) == nat.E_ARG
    assert lib.litho_source_compact_weighted(None, 64, eight, eight, 64 * 64, eight, None, None) == nat.E_ARG
    assert lib.litho_source_compact_weighted(eight, 64, eight, None, 64 * 64, eight, None, None) == nat.E_ARG


def _cross(u, w):
    n = len(u)
    return {kk: sum(u[i] * np.conj(w[i - kk]) for i in range(n) if 0 <= i - kk < n) for kk in range(-(n - 1), n)}


def _weighted_coarse_reconstruction(weight_the_edges):
    """tests/test_coarse_grid_math_cpu.py with a weighted source, built the way the engine builds it: A_s = P M[. + d_s] from a
    random complex P on the natural box, a random M and random shifts; the coarse samples come from sqrt(w_s) A_s (the x-pass
    amplitude), the Nyquist edge products carry w_s (or, to show that they must, do not).  Returns the relative error against
    the fine-grid sum_s w_s |E_s|^2."""
    rng = np.random.default_rng(7)
    pn = 64; N = 2 * pn; c = pn // 2; h = pn // 4; S = 6
    k = np.arange(-h, h + 1)
    KY, KX = np.meshgrid(k, k, indexing="ij")
    support = (KX ** 2 + KY ** 2) <= h * h + 9             # a disk whose rim touches the box edges over several pixels
    support[0, 0] = support[0, -1] = support[-1, 0] = support[-1, -1] = False      # the engine requires empty corners
    P = (rng.standard_normal((2 * h + 1, 2 * h + 1)) + 1j * rng.standard_normal((2 * h + 1, 2 * h + 1))) * support
    M = rng.standard_normal((pn, pn)) + 1j * rng.standard_normal((pn, pn))
    shifts = rng.integers(-(c - h) + 1, c - h - 1, size=(S, 2))                    # the window never leaves the grid
    w = rng.uniform(0.0, 2.0, size=S)
    w[w == 0] = 2.0                                                                # (0, 2]
    A = np.stack([P * M[c - h + dy:c + h + 1 + dy, c - h + dx:c + h + 1 + dx] for dy, dx in shifts])
    q = np.arange(-c, c)
    Wf = np.exp(2j * np.pi * np.outer(k, q) / N)
    I_true = sum(w[s] * np.abs(Wf.T @ A[s] @ Wf) ** 2 for s in range(S))           # fine grid, weighted
    v = np.arange(-pn // 2, pn // 2)
    Wc = np.exp(2j * np.pi * np.outer(k, v) / pn)
    I_c = sum(np.abs(Wc.T @ (np.sqrt(w[s]) * A[s]) @ Wc) ** 2 for s in range(S))    # coarse grid from sqrt(w_s) A_s
    kap = np.arange(-pn // 2, pn // 2)
    Fc = np.exp(-2j * np.pi * np.outer(kap, v) / pn)
    Chat = Fc @ I_c @ Fc.T / pn ** 2
    Wr = np.exp(2j * np.pi * np.outer(kap, q) / N)
    I_rec = (Wr.T @ Chat @ Wr).real
    Gx, Gy = {}, {}
    for s in range(S):
        ws = w[s] if weight_the_edges else 1.0
        for dst, u, ww in ((Gx, A[s][:, -1], A[s][:, 0]), (Gy, A[s][-1, :], A[s][0, :])):
            for kk, val in _cross(u, ww).items():
                dst[kk] = dst.get(kk, 0) + ws * val
    G = np.array([sum(g * np.exp(2j * np.pi * kk * qq / N) for kk, g in Gx.items()) for qq in q])
    H = np.array([sum(g * np.exp(2j * np.pi * kk * qq / N) for kk, g in Gy.items()) for qq in q])
    iq = 1j ** (q % 4)
    odd = (q % 2 != 0)
    dI = np.real(2 * G[:, None] * (iq * odd)[None, :]) + np.real(2 * H[None, :] * (iq * odd)[:, None])
    err = np.abs(I_rec + dI - I_true) / I_true.max()
    even_px = (~odd)[:, None] & (~odd)[None, :]
    return err.max(), err[even_px].max()


def test_weighted_coarse_grid_reconstruction_is_exact():
    err, _ = _weighted_coarse_reconstruction(weight_the_edges=True)
    assert err < 1e-12                                     # the bound of tests/test_coarse_grid_math_cpu.py


def test_unweighted_edge_products_are_wrong_on_odd_pixels_only():
    """Leaving w_s out of the Nyquist edge products breaks the weighted image -- on pixels with an odd coordinate only, which
    is why the GPU suite looks at those separately."""
    err, err_even = _weighted_coarse_reconstruction(weight_the_edges=False)
    assert err > 1e-6
    assert err_even < 1e-12


# ---- host logic: abbeImage(group=, weighted=True) on two gloo ranks ----------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _weighted_map(O, pn):
    """A Gaussian-apodised quasar: weights in (0, 1] on the lit pixels, exact zeros elsewhere."""
    bm = O.source_quasar(0.4, 0.8, pn, 4, -math.pi / 8)
    ax = (torch.arange(pn, dtype=torch.float32) - pn // 2) * (4.0 / pn)
    r2 = ax[:, None] ** 2 + ax[None, :] ** 2
    return torch.exp(-r2 / 0.5) * bm.to(torch.float32)


def _weighted_raw(O, mft, pf, shifts, weights, N):
    out = torch.zeros(mft.shape, dtype=torch.float32)
    for s in range(shifts.shape[0]):
        out += float(weights[s]) * O.abbe_raw(mft, pf, shifts[s:s + 1], N)
    return out


def _product_worker(rank, world, port, out_path):
    """The PRODUCT's abbeImage(group=..., weighted=True) with world_size 2: only the device entry points it calls
    (sourceWeights, abbeIntensity, postProcess) and the device check are replaced by oracle stand-ins that take weights."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lithographysimulator_amd.imageformation as IF
        from lithographysimulator_amd import _native as nat
        from oracle import abbe_oracle as O
        from lithographysimulator_amd.synthetic import lines_mask
        torch.set_num_threads(2)
        calls = []
        nat.require_gpu = lambda d: d if isinstance(d, torch.device) else torch.device(d)

        def fake_source_weights(wm, pn):
            pts = torch.argwhere(wm > 0)
            return (pts - pn // 2).int(), wm[pts[:, 0], pts[:, 1]].to(torch.float32)
        IF.sourceWeights = fake_source_weights

        def fake_intensity(mft, pf, shifts, N, out=None, options=None, weights=None):
            assert weights is not None and weights.shape[0] == shifts.shape[0]
            calls.append((int(shifts.shape[0]), weights.clone()))
            return _weighted_raw(O, mft, pf, shifts, weights, N)
        IF.abbeIntensity = fake_intensity
        IF.postProcess = lambda raw, eps: O.post_process(raw, eps)
        mask = IF.Mask(lines_mask(64), 25, torch.device("cpu"))
        mft = O.mask_spectrum(lines_mask(64), 25, 193.0)
        ab = torch.tensor([0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01], dtype=torch.float16)
        pf = O.pupil_function(ab.clone(), 64, 0.7, 193.0)
        wm = _weighted_map(O, 64)
        cpu = torch.device("cpu")
        res = {}
        res["sharded"] = IF.abbeImage(mask, mft, pf, wm, 25, mask.deltaK, 193.0, True, cpu, group=dist.group.WORLD, weighted=True)
        res["points"], res["weights"] = calls[-1]
        res["normalized"] = IF.abbeImage(mask, mft, pf, wm, 25, mask.deltaK, 193.0, True, cpu, group=dist.group.WORLD,
                                         normalize=True, weighted=True)
        eps, N = O.calculate_epsilon_n(4 / 64, 25, 193.0)
        sh, wt = fake_source_weights(wm, 64)
        res["whole"] = O.post_process(_weighted_raw(O, mft, pf, sh, wt, N), eps)
        res["all_weights"] = wt
        res["S"] = int(sh.shape[0])
        torch.save(res, out_path + f".{rank}")
    finally:
        dist.destroy_process_group()


def test_product_weighted_abbe_image_with_world_size_two(tmp_path):
    from lithographysimulator_amd.distributed import shard_bounds
    out = str(tmp_path / "result.pt")
    mp.spawn(_product_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0"), torch.load(out + ".1")
    S = r0["S"]
    wt = r0["all_weights"]
    assert S == 184 and float(wt.min()) > 0 and float(wt.max()) < 1 and len(set(wt.tolist())) > 10      # a real grey-level map
    assert (r0["points"], r1["points"]) == (S - S // 2, S // 2)                # contiguous balanced shards
    for rank, r in enumerate((r0, r1)):                                        # each rank got ITS slice of the weights
        lo, hi = shard_bounds(S, rank, 2)
        assert torch.equal(r["weights"], wt[lo:hi])
    rel = lambda a, b: float((a - b).abs().max() / b.max())
    wsum = float(wt.double().sum())
    for r in (r0, r1):                                                         # every rank holds the full image
        assert rel(r["sharded"], r["whole"]) < 2e-6                            # (the bound of tests/test_distributed_cpu.py)
        assert rel(r["normalized"] * wsum, r["whole"]) < 2e-6                  # normalised by the GLOBAL sum of weights
    assert torch.equal(r0["sharded"], r1["sharded"])
