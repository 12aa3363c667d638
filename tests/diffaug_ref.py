"""fp64 restatement of DiffAugment (Zhao et al., NeurIPS 2020, policy ``color,translation,cutout``) as the discriminator's input
augmentation defines it (include/sgx.h, sgx_diffaug): the test-side truth for the HIP kernels.  The product never imports this.

Images here are logical NCHW torch tensors (any float dtype; the ops are differentiable, twice, so the oracle's R1 penalty runs
through them).  ``u`` holds seven uniform draws per image: u0..u2 colour, u3/u4 translation, u5/u6 cutout."""
import numpy as np
import torch
import torch.nn.functional as TF

OPS = ("color", "translation", "cutout")
COLOR, TRANSLATION, CUTOUT = 1, 2, 4
EDGE = float(np.float32(1.0) - np.float32(2.0 ** -24))          # the largest fp32 below 1


def _draw(u, n, hi):
    """min(floor(u * n), hi) with the product rounded to fp32, as the kernels compute it."""
    return min(int(np.floor(np.float32(u) * np.float32(n))), hi)


def params(u_row, H, W, bits):
    """The integer and colour parameters of one image: dict(b, s, c, tx, ty, r0, r1, c0, c1) (cutout rows [r0, r1) x cols [c0, c1))."""
    u = [float(np.float32(v)) for v in u_row]
    p = dict(b=0.0, s=1.0, c=1.0, tx=0, ty=0, r0=0, r1=0, c0=0, c1=0)
    if bits & COLOR:
        p.update(b=u[0] - 0.5, s=u[1] * 2, c=u[2] + 0.5)
    if bits & TRANSLATION:
        sh, sw = int(H * 0.125 + 0.5), int(W * 0.125 + 0.5)
        p.update(tx=_draw(u[3], 2 * sh + 1, 2 * sh) - sh, ty=_draw(u[4], 2 * sw + 1, 2 * sw) - sw)
    if bits & CUTOUT:
        ch, cw = int(H * 0.5 + 0.5), int(W * 0.5 + 0.5)
        ox = _draw(u[5], H + 1 - ch % 2, H - ch % 2)
        oy = _draw(u[6], W + 1 - cw % 2, W - cw % 2)
        p.update(r0=max(ox - ch // 2, 0), r1=min(ox - ch // 2 + ch, H), c0=max(oy - cw // 2, 0), c1=min(oy - cw // 2 + cw, W))
    return p


def color(x, b, s, c):
    """DiffAugment's rand_brightness, rand_saturation, rand_contrast in its op order, one image [3,H,W]."""
    x = x + b
    m = x.mean(dim=0, keepdim=True)
    x = (x - m) * s + m
    M = x.mean()
    return (x - M) * c + M


def shift(x, tx, ty):
    """y[:, i, j] = x[:, i + tx, j + ty] inside the image, 0 outside (F.pad crops with negative amounts)."""
    return TF.pad(x, (-ty, ty, -tx, tx))


def cut(x, p):
    if p["r1"] <= p["r0"] or p["c1"] <= p["c0"]:
        return x
    mask = torch.ones(x.shape[1:], dtype=x.dtype, device=x.device)
    mask[p["r0"]:p["r1"], p["c0"]:p["c1"]] = 0
    return x * mask


def apply_one(x, p, bits, adjoint=False, with_bias=True):
    """One image [3,H,W].  Forward: Mask(Shift(color(x))) (minus the brightness bias unless with_bias); adjoint: L(Shift^T(Mask x))."""
    if adjoint:
        x = shift(cut(x, p), -p["tx"], -p["ty"])
        return color(x, 0.0, p["s"], p["c"]) if bits & COLOR else x     # L: the colour chain without its bias (symmetric)
    if bits & COLOR:
        x = color(x, p["b"] if with_bias else 0.0, p["s"], p["c"])
    return cut(shift(x, p["tx"], p["ty"]), p)


def apply(x, u, bits, adjoint=False, with_bias=True):
    """A batch [B,3,H,W] with draws u [B,7] (any array-like)."""
    u = np.asarray(u.detach().cpu() if isinstance(u, torch.Tensor) else u, dtype=np.float32)
    H, W = x.shape[2], x.shape[3]
    return torch.stack([apply_one(x[i], params(u[i], H, W, bits), bits, adjoint, with_bias) for i in range(x.shape[0])])


def literal(x, p, bits):
    """DiffAugment's published indexing transcribed for given parameters, one batch [B,3,H,W] with one parameter dict for every image:
    translation pads by one pixel and gathers at clamp(i + tx + 1, 0, H + 1); cutout zeroes a mask at clamp(grid + offset - size // 2)."""
    B, _, H, W = x.shape
    if bits & COLOR:
        x = x + p["b"]
        xm = x.mean(dim=1, keepdim=True)
        x = (x - xm) * p["s"] + xm
        xm = x.mean(dim=[1, 2, 3], keepdim=True)
        x = (x - xm) * p["c"] + xm
    if bits & TRANSLATION:
        gb, gx, gy = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
        gx = torch.clamp(gx + p["tx"] + 1, 0, H + 1)
        gy = torch.clamp(gy + p["ty"] + 1, 0, W + 1)
        xp = TF.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
        x = xp.permute(0, 2, 3, 1).contiguous()[gb, gx, gy].permute(0, 3, 1, 2)
    if bits & CUTOUT:
        ch, cw = int(H * 0.5 + 0.5), int(W * 0.5 + 0.5)
        gb, gx, gy = torch.meshgrid(torch.arange(B), torch.arange(ch), torch.arange(cw), indexing="ij")
        gx = torch.clamp(gx + p["ox"] - ch // 2, min=0, max=H - 1)
        gy = torch.clamp(gy + p["oy"] - cw // 2, min=0, max=W - 1)
        mask = torch.ones(B, H, W, dtype=x.dtype)
        mask[gb, gx, gy] = 0
        x = x * mask.unsqueeze(1)
    return x


def edge_draws(B, seed=0):
    """[B,7] fp32 draws: random rows plus the edges -- u = 0, u = 1 - 2^-24 (the clamps), saturation 0, cutout at both corners."""
    g = np.random.default_rng(seed)
    u = g.random((max(B, 1), 7), dtype=np.float32)
    edges = [np.zeros(7, np.float32), np.full(7, EDGE, np.float32)]
    s0 = g.random(7, dtype=np.float32); s0[1] = 0.0                    # s = 0
    corner = g.random(7, dtype=np.float32); corner[5] = corner[6] = EDGE
    for k, row in enumerate(edges + [s0, corner]):
        if k < B:
            u[k] = row
    return u[:B]
