"""Restatement of adaptive discriminator augmentation (Karras et al., NeurIPS 2020) as include/sgx.h defines it (sgx_ada_gates,
sgx_ada_update, sgx_diffaug_gated): the test-side truth for the HIP kernels.  The product never imports this.

``gates`` and ``controller`` are NumPy float32 with every operation rounded to fp32 on its own, in the header's order, so the kernels must
reproduce them bit for bit; ``controller64`` is the same rule in fp64 (what the float32 one approximates).  The per-image image
reference is tests/diffaug_ref.py, called image by image with that image's bits (``apply_gated``)."""
import numpy as np
import torch

import diffaug_ref as R

f32 = np.float32
STATE = 8                        # [p, sum of signs, images counted, calls since the last update, last r_t, updates made, 0, 0]


def gates(gu, p, policy_bits):
    """gu [B,3] -> int32 [B]: policy_bits & (1 [gu0 < p] | 2 [gu1 < p] | 4 [gu2 < p]), strict < in fp32."""
    gu = np.asarray(gu, dtype=f32).reshape(-1, 3)
    on = (gu < f32(p)).astype(np.int32)
    return (int(policy_bits) & (on[:, 0] | 2 * on[:, 1] | 4 * on[:, 2])).astype(np.int32)


def signs(logits):
    """+1 / -1; 0 for +-0 and NaN."""
    v = np.asarray(logits, dtype=f32).reshape(-1)
    return (v > 0).astype(np.int64) - (v < 0).astype(np.int64)


def new_state(p=0.0, dtype=f32):
    s = np.zeros(STATE, dtype)
    s[0] = p
    return s


def controller(state, logits, target, adjust_per_image, interval):
    """One sgx_ada_update call: -> the new float32 state (the argument is left alone)."""
    s = np.array(state, dtype=f32)
    B = np.asarray(logits).size
    total = f32(int(signs(logits).sum()))                        # the signs are summed as an integer: exact
    sg, seen, calls = f32(s[1] + total), f32(s[2] + f32(B)), f32(s[3] + f32(1))
    if calls >= f32(interval):
        rt = f32(sg / seen)
        t = f32(target)
        d = f32(1) if rt > t else (f32(-1) if rt < t else f32(0))
        p = f32(s[0] + f32(d * f32(f32(adjust_per_image) * seen)))
        s[0] = min(max(p, f32(0)), f32(1))
        s[1] = s[2] = s[3] = 0
        s[4] = rt
        s[5] = f32(s[5] + f32(1))
    else:
        s[1], s[2], s[3] = sg, seen, calls
    return s


def controller64(state, logits, target, adjust_per_image, interval):
    """The same rule in fp64 (target and adjust_per_image as the fp32 numbers the kernel is given)."""
    s = np.array(state, dtype=np.float64)
    B = np.asarray(logits).size
    sg, seen, calls = s[1] + float(signs(logits).sum()), s[2] + B, s[3] + 1
    if calls >= interval:
        rt, t = sg / seen, float(f32(target))
        d = 1.0 if rt > t else (-1.0 if rt < t else 0.0)
        s[0] = min(max(s[0] + d * float(f32(adjust_per_image)) * seen, 0.0), 1.0)
        s[1] = s[2] = s[3] = 0
        s[4] = rt
        s[5] += 1
    else:
        s[1], s[2], s[3] = sg, seen, calls
    return s


def adjust_per_image(ada_kimg):
    """What the module passes: 1 / (ada_kimg * 1000) computed in Python, then fp32."""
    return f32(1.0 / (float(ada_kimg) * 1000.0))


def apply_gated(x, u, img_bits, adjoint=False, with_bias=True):
    """A batch [B,3,H,W] with draws u [B,7] and per-image bits [B]: diffaug_ref.apply_one, image by image."""
    u = np.asarray(u.detach().cpu() if isinstance(u, torch.Tensor) else u, dtype=f32)
    bits = [int(b) for b in (img_bits.detach().cpu().tolist() if isinstance(img_bits, torch.Tensor) else img_bits)]
    H, W = x.shape[2], x.shape[3]
    return torch.stack([R.apply_one(x[i], R.params(u[i], H, W, bits[i]), bits[i], adjoint, with_bias) for i in range(x.shape[0])])
