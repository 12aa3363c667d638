"""fp64 restatement of the augmentation with pixel blitting (include/sgx.h, sgx_diffaug_blit and sgx_ada_gates_n): the policy of
tests/diffaug_ref.py plus ``xflip`` and ``rot90`` -- G = Rot^k o Flip between the colour and the shift -- built from that file's
``params``, ``color``, ``shift`` and ``cut`` with ``torch.flip`` and ``torch.rot90``.  The product never imports this.

Images are logical NCHW torch tensors; ``u`` holds nine uniform draws per image: u0..u6 as in diffaug_ref, u7 the flip, u8 the turn."""
import numpy as np
import torch

import diffaug_ref as R

OPS = ("color", "xflip", "rot90", "translation", "cutout")          # the canonical order
COLOR, TRANSLATION, CUTOUT, XFLIP, ROT90 = 1, 2, 4, 8, 16
ALL = 31
EDGE = R.EDGE
f32 = np.float32


def params9(u_row, H, W, bits):
    """diffaug_ref.params plus f (0 / 1) and k (0 .. 3); an op that is not in ``bits`` gives f = 0 / k = 0 whatever its uniform is."""
    p = R.params(u_row[:7], H, W, bits & 7)
    p["f"] = R._draw(u_row[7], 2, 1) if bits & XFLIP else 0
    p["k"] = R._draw(u_row[8], 4, 3) if bits & ROT90 else 0
    if p["k"] & 1 and H != W:
        raise ValueError(f"rot90 needs square images, got {H}x{W}")
    return p


def orient(x, f, k):
    """G(x) = Rot^k(Flip^f(x)) on [3,H,W]."""
    return torch.rot90(torch.flip(x, [2]) if f else x, k, [1, 2])


def orient_t(x, f, k):
    """G^T = G^-1 = Flip^f o Rot^-k."""
    x = torch.rot90(x, -k, [1, 2])
    return torch.flip(x, [2]) if f else x


def apply_one(x, p, bits, adjoint=False, with_bias=True):
    """One image [3,H,W].  Forward: Mask(Shift(G(color(x)))) (minus the brightness bias unless with_bias); adjoint:
    L(G^T(Shift^T(Mask x)))."""
    if adjoint:
        x = orient_t(R.shift(R.cut(x, p), -p["tx"], -p["ty"]), p["f"], p["k"])
        return R.color(x, 0.0, p["s"], p["c"]) if bits & COLOR else x
    if bits & COLOR:
        x = R.color(x, p["b"] if with_bias else 0.0, p["s"], p["c"])
    return R.cut(R.shift(orient(x, p["f"], p["k"]), p["tx"], p["ty"]), p)


def _np(u):
    return np.asarray(u.detach().cpu() if isinstance(u, torch.Tensor) else u, dtype=f32)


def apply(x, u, bits, adjoint=False, with_bias=True):
    """A batch [B,3,H,W] with draws u [B,9] (any array-like) under one policy."""
    return apply_gated(x, u, [bits] * x.shape[0], adjoint, with_bias)


def apply_gated(x, u, img_bits, adjoint=False, with_bias=True):
    """A batch [B,3,H,W] with draws u [B,9] and per-image bits [B]."""
    u = _np(u)
    bits = [int(b) for b in (img_bits.detach().cpu().tolist() if isinstance(img_bits, torch.Tensor) else img_bits)]
    H, W = x.shape[2], x.shape[3]
    return torch.stack([apply_one(x[i], params9(u[i], H, W, bits[i]), bits[i], adjoint, with_bias) for i in range(x.shape[0])])


def gates_n(gu, p, policy_bits):
    """gu [B,n] (n <= 5) -> int32 [B]: policy_bits & (sum over g of (1 << g) [gu[b][g] < p]), strict < in fp32."""
    gu = np.asarray(gu, dtype=f32)
    on = (gu < f32(p)).astype(np.int32)
    word = np.zeros(gu.shape[0], np.int32)
    for g in range(gu.shape[1]):
        word |= on[:, g] << g
    return (int(policy_bits) & word).astype(np.int32)


def literal(x, p, adjoint=False):
    """The index rules of include/sgx.h transcribed pixel by pixel for one image [3,H,W] without the colour: the forward gather
    (cutout test at the output, shifted position tested against the image, source G^-1 of it) and the adjoint gather ((a, b) =
    G(i, j), source (a - tx, b - ty) tested against the image and the cutout)."""
    _, H, W = x.shape
    N = H
    f, k = p["f"], p["k"]

    def g_inv(a, b):                       # G(x)[a][b] = x[g_inv(a, b)]: the rotation's rule, then the flip's
        if k == 1:
            a, b = b, N - 1 - a
        elif k == 2:
            a, b = N - 1 - a, N - 1 - b
        elif k == 3:
            a, b = N - 1 - b, a
        return (a, W - 1 - b) if f else (a, b)

    where = {g_inv(a, b): (a, b) for a in range(H) for b in range(W)}          # G(i, j): where input pixel (i, j) lands
    cut = lambda i, j: p["r0"] <= i < p["r1"] and p["c0"] <= j < p["c1"]
    y = torch.zeros_like(x)
    for i in range(H):
        for j in range(W):
            if adjoint:
                a, b = where[(i, j)]
                si, sj = a - p["tx"], b - p["ty"]
                if 0 <= si < H and 0 <= sj < W and not cut(si, sj):
                    y[:, i, j] = x[:, si, sj]
            else:
                a, b = i + p["tx"], j + p["ty"]
                if not cut(i, j) and 0 <= a < H and 0 <= b < W:
                    si, sj = g_inv(a, b)
                    y[:, i, j] = x[:, si, sj]
    return y


def edge_draws9(B, seed=0):
    """[B,9] fp32 draws: diffaug_ref.edge_draws (its rows 0..3 are the edges of u0..u6) with u7, u8 such that rows 0..7 run through
    all eight (f, k) -- row b has f = b & 1, k = b >> 1, with u7 and u8 at 0 and at 1 - 2^-24 where those give the value -- and
    random beyond."""
    g = np.random.default_rng(seed + 977)
    u = np.concatenate([R.edge_draws(B, seed), g.random((B, 2), dtype=f32)], axis=1)
    u7 = [f32(0), EDGE, f32(0.25), f32(0.75)]                               # f = 0, 1, 0, 1
    u8 = [f32(0), f32(0.3), f32(0.6), EDGE]                                 # k = 0, 1, 2, 3
    for b in range(min(B, 8)):
        u[b, 7] = u7[(b & 1) + 2 * ((b >> 2) & 1)]
        u[b, 8] = u8[b >> 1]
    return u.astype(f32)
