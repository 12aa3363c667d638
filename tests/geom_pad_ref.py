"""Restatement of the geometric resample with reflection padding (include/sgx.h, sgx_ada_geom_reflect), built on geom_ref's positions
and weight: the same table, the same float32 position and weight expressions, and per axis of length N >= 2 the rule

    a tap index t is valid iff -(N-1) <= t <= 2 (N-1);  a valid tap reads pixel r(t) = -t (t < 0), 2 (N-1) - t (t > N-1), t (else);
    the weight is taken at the unreflected t;  a tap beyond one period contributes zero.

  ``tap_info``    the four taps of every output pixel in the device's order: unreflected (tx, ty), validity, float32 weight (0 where
                  the tap is not valid)
  ``taps``        the same as (flat index of the pixel read, weight), the form of geom_ref.taps: the device's weights bit for bit
  ``apply``       the resample (or its transpose) of a torch batch in the batch's own dtype, from indexing and products with those
                  weights, so autograd yields its adjoint and double backward and it composes with the oracle's discriminator
  ``tap_counts``  how many non-zero coefficients each output element sums (the n of the per-element bound)

The product never imports this."""
import numpy as np
import torch

import geom_ref as G

f32 = np.float32


def reflect(t, N):
    """r(t) of the rule, for valid t (int64 arrays)."""
    return np.where(t < 0, -t, np.where(t > N - 1, 2 * (N - 1) - t, t))


def valid(t, N):
    return (t >= -(N - 1)) & (t <= 2 * (N - 1))


def tap_info(row, H, W):
    """A list of four (tx, ty, ok, w): the unreflected tap indices [H,W] int64, whether the tap is within one period on both axes, and
    the float32 weight at the unreflected index (0 where not ok)."""
    assert H >= 2 and W >= 2
    sx, sy = G.positions(row, H, W)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = x0 + dx, y0 + dy
            ok = valid(tx, W) & valid(ty, H)
            out.append((tx, ty, ok, np.where(ok, G.weight(sx, sy, tx, ty), f32(0)).astype(f32)))
    return out


def taps(row, H, W):
    """(flat index of the pixel a tap reads [H,W] int64 (clipped where the tap is not valid), weight [H,W] float32), four of them."""
    out = []
    for tx, ty, ok, w in tap_info(row, H, W):
        rx, ry = np.clip(reflect(tx, W), 0, W - 1), np.clip(reflect(ty, H), 0, H - 1)
        out.append((ry * W + rx, w))
    return out


def apply_one(x, row, adjoint=False):
    """One image [3,H,W] (any float dtype) under one table row: R x, or R^T x by scattering with the same coefficients."""
    if G.is_identity(row):
        return x.clone()
    C, H, W = x.shape
    flat = x.reshape(C, H * W)
    out = torch.zeros_like(flat)
    for idx, w in taps(row, H, W):
        idx_t = torch.from_numpy(idx.reshape(-1))
        w_t = torch.from_numpy(w.reshape(-1)).to(x.dtype)
        if adjoint:
            out = out.index_add(1, idx_t, flat * w_t)
        else:
            out = out + flat[:, idx_t] * w_t
    return out.reshape(C, H, W)


def apply(x, mat, adjoint=False):
    """A batch [B,3,H,W] under the table ``mat`` [B,8] (any array-like; the weights are computed from its float32 rounding)."""
    mat = np.asarray(mat.detach().cpu() if isinstance(mat, torch.Tensor) else mat)
    return torch.stack([apply_one(x[b], mat[b], adjoint) for b in range(x.shape[0])])


def tap_counts(row, H, W, adjoint=False):
    """int64 [H,W]: the number of non-zero coefficients of every output element (identity: 1)."""
    if G.is_identity(row):
        return np.ones((H, W), np.int64)
    n = np.zeros(H * W, np.int64)
    for idx, w in taps(row, H, W):
        if adjoint:
            np.add.at(n, idx.reshape(-1), (w.reshape(-1) > 0).astype(np.int64))
        else:
            n += (w.reshape(-1) > 0)
    return n.reshape(H, W)


def census(row, H, W):
    """What a row reaches at H x W: non-zero taps, those of them reflected on each side, taps beyond one period whose weight would
    have been non-zero, and output pixels without a non-zero coefficient."""
    sx, sy = G.positions(row, H, W)
    c = dict(nonzero=0, left=0, right=0, top=0, bottom=0, reflected=0, beyond=0)
    for tx, ty, ok, w in tap_info(row, H, W):
        nz = w > 0
        c["nonzero"] += int(nz.sum())
        c["left"] += int((nz & (tx < 0)).sum()); c["right"] += int((nz & (tx > W - 1)).sum())
        c["top"] += int((nz & (ty < 0)).sum()); c["bottom"] += int((nz & (ty > H - 1)).sum())
        c["reflected"] += int((nz & ((tx < 0) | (tx > W - 1) | (ty < 0) | (ty > H - 1))).sum())
        c["beyond"] += int((~ok & (G.weight(sx, sy, tx, ty) > 0)).sum())
    c["empty"] = int((tap_counts(row, H, W) == 0).sum())
    return c
