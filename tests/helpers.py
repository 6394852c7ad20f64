"""Shared constants/helpers for the parity tests (mirror tests/golden/make_golden.py)."""
import ctypes
import hashlib
import math
import os
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL, NA, PS = 193.0, 0.7, 25
DEMO_AB = [0, 0, 0.01, 0, 100, 0.01, 0, 0.01, 0.01, 0.01]

SOURCE_CASES = {
    "circ": dict(kind="annular", sin=0.0, sout=0.5),
    "annular": dict(kind="annular", sin=0.4, sout=0.8),
    "quasar": dict(kind="quasar", sin=0.4, sout=0.8),
    "annular_shift": dict(kind="annular", sin=0.4, sout=0.8, sx=0.25, sy=-0.5),
    "quasar3_oddshift": dict(kind="quasar", sin=0.3, sout=0.9, sx=0.2, sy=-0.1, count=3, rot=0.3),
}
PUPIL_CASES = {
    "ideal": None,
    "defocus_p100": [0, 0, 0, 0, 100],
    "defocus_m200": [0, 0, 0, 0, -200],
    "defocus_p30": [0, 0, 0, 0, 30],
    "demo": DEMO_AB,
    "short3": [0.1, 0.2, 0.05],
    "terms15": [0, 0, 0, 1, 3, 0, 0, 1, 0, 0, 0.02, 0.03, 0.01, 0.5, 0.2],
}
# Tolerances (measured noise floor of the reference itself: fp32 vs complex128
# of the same algorithm = 4e-7 rel-to-max at 64^2/S=184, 2.8e-6 at 256^2/S=3233).
TOL_FIELD = 5e-6          # max|dE| / max|E|          single-point field
TOL_IMAGE_MAX = 2e-5      # max|dI| / max I           image, S <= 4096
TOL_IMAGE_L2 = 5e-6       # ||dI||_2 / ||I||_2
TOL_PHI = 5e-7            # abs, pupil function


def f16(v):
    return torch.tensor(v, dtype=torch.float16)


def rel_max(a, b):
    a = torch.as_tensor(a).double() if not torch.is_complex(torch.as_tensor(a)) else torch.as_tensor(a).to(torch.complex128)
    b = torch.as_tensor(b).double() if not torch.is_complex(torch.as_tensor(b)) else torch.as_tensor(b).to(torch.complex128)
    return float((a - b).abs().max() / b.abs().max())


def rel_l2(a, b):
    a = torch.as_tensor(a).double(); b = torch.as_tensor(b).double()
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def sha256_packed(bitmap: np.ndarray) -> np.ndarray:
    packed = np.packbits(bitmap.astype(np.uint8))
    return np.frombuffer(hashlib.sha256(packed.tobytes()).digest(), dtype=np.uint8)


def unpack_bitmap(blob: np.ndarray, pn: int) -> np.ndarray:
    bits = np.unpackbits(np.frombuffer(zlib.decompress(blob.tobytes()), dtype=np.uint8))
    return bits[:pn * pn].reshape(pn, pn)


def unpack_bits(blob: np.ndarray, shape) -> np.ndarray:
    """zlib-packed bits (make_golden.pack_bits) -> uint8 0/1 array of `shape`."""
    bits = np.unpackbits(np.frombuffer(zlib.decompress(blob.tobytes()), dtype=np.uint8))
    return bits[:int(np.prod(shape))].reshape(shape)


def f16_from_bits(bits: np.ndarray) -> torch.Tensor:
    """raw uint16 -> fp16 tensor of the same shape."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.float16)


def g18_source_cases(g, pn):
    """Every small-size source case of golden g18 at `pn`: (label, sin, sout, sx, sy, count, rot, bitmap), count None for
    the annular source.  The order is the fixture's: sigma pair, shift, kind."""
    sig, sh, qs = g["src_sigma"], g["src_shift"], g["src_quasar"]
    bms = unpack_bits(g[f"src_packed_{pn}"], (len(sig), len(sh), 1 + len(qs), pn, pn))
    for a, (sin, sout) in enumerate(sig):
        for b, (sx, sy) in enumerate(sh):
            yield f"annular {sin}-{sout} shift ({sx},{sy})", float(sin), float(sout), float(sx), float(sy), None, 0.0, bms[a, b, 0]
            for q, (count, rot) in enumerate(qs):
                yield (f"quasar({int(count)},{rot:.4g}) {sin}-{sout} shift ({sx},{sy})", float(sin), float(sout), float(sx),
                       float(sy), int(count), float(rot), bms[a, b, 1 + q])


def g18_large_source_cases(g):
    """The large-size source cases of golden g18: (key, pn, kind, sx, sy); annular and quasar(4, -pi/8), 0.4-0.8."""
    for pn in g["srcL_pn"]:
        for b, (sx, sy) in enumerate(g["srcL_shift"]):
            for kind in ("annular", "quasar"):
                yield f"srcL_{kind}_{b}_{int(pn)}", int(pn), kind, float(sx), float(sy)


def g18_pupil_cases(g):
    """Every single-pupil case of golden g18: (label, pn, NA, wavelength, fp16 vector, fp16 W)."""
    nalam = g["pupil_nalam"]
    for pn in list(g["pupil_pn"]) + list(g["pupil_pn_few"]):
        few = pn in g["pupil_pn_few"]
        W = g[f"pupil_W_{int(pn)}"]
        for a, (na, lam) in enumerate(nalam[:1] if few else nalam):
            for v, name in enumerate(g["pupil_names_few"] if few else g["pupil_names"]):
                yield (f"pn {int(pn)} NA {na} lambda {lam} {name}", int(pn), float(na), float(lam),
                       f16_from_bits(g[f"vec_{name}"]), f16_from_bits(W[a, v]))


def g18_focus_cases(g):
    """The through-focus cases of golden g18: (label, pn, NA, wavelength, fp16 vector, fp16 W [planes, pn, pn])."""
    for pn in g["tf_pn"]:
        W = g[f"tf_W_{int(pn)}"]
        for a, k in enumerate(g["tf_nalam_index"]):
            na, lam = g["pupil_nalam"][int(k)]
            for v, name in enumerate(g["tf_names"]):
                yield (f"pn {int(pn)} NA {na} lambda {lam} {name}", int(pn), float(na), float(lam),
                       f16_from_bits(g[f"vec_{name}"]), f16_from_bits(W[a, v]))


def g18_support(g, pn):
    return unpack_bits(g[f"pupil_support_{pn}"], (pn, pn)).astype(bool)


def subsample_bitmap(bitmap: torch.Tensor, K: int) -> torch.Tensor:
    pts = torch.argwhere(bitmap)
    S = pts.shape[0]
    idx = (torch.arange(K) * S) // K
    out = torch.zeros_like(bitmap)
    out[pts[idx, 0], pts[idx, 1]] = 1
    return out


def crop_center(img, crop=128):
    pn = img.shape[0]
    c0 = pn // 2 - crop // 2
    return img[c0:c0 + crop, c0:c0 + crop]


def load_c_oracle():
    path = os.path.join(ROOT, "oracle", "libabbe_ref.so")
    if not os.path.exists(path):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    lib = ctypes.CDLL(path)
    lib.oracle_field.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.oracle_abbe_accumulate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def c_oracle_field(lib, pupil, maskFT, N, dy, dx):
    pn = maskFT.shape[0]
    p = np.ascontiguousarray(pupil.numpy()); m = np.ascontiguousarray(maskFT.numpy())
    out = np.zeros((pn, pn), dtype=np.complex128)
    rc = lib.oracle_field(p.ctypes.data, m.ctypes.data, pn, N, int(dy), int(dx), out.ctypes.data)
    assert rc == 0
    return torch.from_numpy(out)
