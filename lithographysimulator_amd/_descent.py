"""The arithmetic that optimizeMask (ilt.py), optimizeSource (smo.py) and fitAberrations (aberrations.py) must keep identical.
The loops themselves stay where they are: their bookkeeping differs on purpose."""
import torch

from . import _native as nat
from . import socs as _socs


def default_resist_steepness(threshold):
    """25 per threshold: the image is in the engine's raw units (a clear field is ~1e7 at pn 64), so a fixed slope would saturate
    the sigmoid; with this one the resist goes from 8 % to 92 % between 0.9 and 1.1 thresholds.  25 at threshold 0."""
    return 25.0 / abs(float(threshold)) if float(threshold) != 0 else 25.0


def resist_loss(image, target, resistSteepness, dose, threshold, gradient=True):
    """(loss, dl/d image) of the sigmoid resist: resist = sigmoid(a_r (dose image - threshold)), loss = mean((resist - target)^2)
    over pixels and planes, a 0-dim tensor in the image's precision -- nothing is read on the host here -- and its gradient on
    the image in closed form, 2 a_r dose / count . (resist - target) resist (1 - resist).  gradient=False: (loss, None)."""
    a_r, dose = float(resistSteepness), float(dose)
    resist = torch.sigmoid(a_r * (dose * image - float(threshold)))
    diff = resist - target.to(image.dtype)
    loss = (diff * diff).mean()
    if not gradient:
        return loss, None
    return loss, (2.0 * a_r * dose / diff.numel()) * diff * resist * (1.0 - resist)


def peak(grad, dtype=None):
    """max|grad| as a 0-dim tensor, kept off zero by the smallest normal number of grad's precision (or `dtype`'s): what the
    three loops divide a gradient by to get a direction whose largest entry is 1, so that a step is a length and not a rate."""
    return torch.clamp(grad.abs().max(), min=torch.finfo(dtype or grad.dtype).tiny)


def pow2_size(who, what, n, entry):
    """The sizes the transforms of the gradient entries exist for (`entry` names the one that will refuse it otherwise)."""
    if n < _socs.MIN_PN or n > _socs.MAX_PN or n & (n - 1):
        raise ValueError(f"{who}: {what} must be a power of two, {_socs.MIN_PN} ... {_socs.MAX_PN} ({entry}); got {n}")


def check_image_grid(who, what, t, pn, epsilon, per_plane=False):
    """`t` (square on its last two axes) must live on the post-processed grid of a pn x pn raw image; ValueError otherwise."""
    n_out = nat.postprocess_size(pn, epsilon)
    if t.shape[-1] != n_out:
        raise ValueError(f"{who}: {what} must be [{n_out},{n_out}]{' per plane' if per_plane else ''}, the post-processed grid of "
                         f"pn {pn} at epsilon {epsilon:.6g}; got {tuple(t.shape)}")
