"""Restatement of ADA's general geometric group (include/sgx.h, sgx_ada_geom_matrix and sgx_ada_geom): scale, rotate and aniso composed
per image into one affine map T about the image centre and applied by one bilinear resample.  The product never imports this.

  ``matrices``        draws -> the [B,8] table {T^-1, T} in fp64, from the same fp32 uniforms (what the device's fp32 table approximates)
  ``taps``            positions and weights in NumPy float32, every product and sum rounded to fp32 on its own in the header's order:
                      the device's weights bit for bit
  ``apply``           the resample (or its transpose) of a torch batch in the batch's own dtype, built from indexing and products with
                      those weights, so autograd yields its adjoint and double backward and it composes with the oracle's discriminator
  ``tap_counts``      how many non-zero coefficients each output element sums (the n of the per-element bound)

Images are logical NCHW torch tensors; ``u`` holds five uniform draws per image (u0, u1: scale; u2: rotate; u3, u4: aniso)."""
import numpy as np
import torch

OPS = ("scale", "rotate", "aniso")
SCALE, ROTATE, ANISO = 32, 64, 128
ALL = SCALE | ROTATE | ANISO
f32 = np.float32
EDGE = f32(1.0 - 2.0 ** -24)                       # the largest float32 below 1
IDENTITY = (1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0)


def gates(gu, p, policy_bits):
    """gu [B,3] -> int [B]: policy_bits & (32 [gu0 < p] | 64 [gu1 < p] | 128 [gu2 < p]), strict < in fp32 (the rule of tests/ada_ref.py)."""
    gu = np.asarray(gu, dtype=f32).reshape(-1, 3)
    on = (gu < f32(p)).astype(np.int64)
    return (int(policy_bits) & ALL) & (SCALE * on[:, 0] | ROTATE * on[:, 1] | ANISO * on[:, 2])


def params(u_row, bits):
    """One image's z_s, s, theta, z_a, a in fp64 from its fp32 uniforms; an op that is not in ``bits`` gives s = 1 / theta = 0 / a = 1."""
    u = [float(f32(v)) for v in u_row]

    def z(ua, ub):
        return min(max(np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(2.0 * np.pi * ub), -3.0), 3.0)
    z_s, z_a = z(u[0], u[1]), z(u[3], u[4])
    return dict(z_s=z_s, z_a=z_a, s=2.0 ** (0.2 * z_s) if bits & SCALE else 1.0, theta=2.0 * np.pi * (u[2] - 0.5) if bits & ROTATE else 0.0,
                a=2.0 ** (0.2 * z_a) if bits & ANISO else 1.0)


def matrix(s, theta, a):
    """(T^-1, T) row major as eight numbers: T = Rot(theta) diag(s a, s / a) on (column, row), Rot = [cos -sin; sin cos]."""
    sx, sy, c, sn = s * a, s / a, np.cos(theta), np.sin(theta)
    return (c / sx, sn / sx, -sn / sy, c / sy, c * sx, -sn * sy, sn * sx, c * sy)


def matrices(u, img_bits):
    """u [B,5], per-image bits [B] (or one int) -> fp64 [B,8]; an image with no geometric bit gets the exact identity row."""
    u = np.asarray(u, dtype=f32)
    bits = [int(img_bits)] * u.shape[0] if np.isscalar(img_bits) else [int(b) for b in img_bits]
    out = np.zeros((u.shape[0], 8), np.float64)
    for b in range(u.shape[0]):
        if not bits[b] & ALL:
            out[b] = IDENTITY
        else:
            p = params(u[b], bits[b])
            out[b] = matrix(p["s"], p["theta"], p["a"])
    return out


def table(tinv):
    """A test-supplied table row from T^-1 (four numbers): T is its fp64 inverse rounded to fp32."""
    m = np.asarray(tinv, np.float64).reshape(2, 2)
    return np.concatenate([m.reshape(-1), np.linalg.inv(m).reshape(-1)]).astype(f32)


def positions(row, H, W):
    """float32 source positions (sx, sy) [H,W] of every output pixel under the table row: s = c + (m0 dx + m1 dy), ... in fp32."""
    m = np.asarray(row, dtype=f32)
    cx, cy = f32((W - 1) * 0.5), f32((H - 1) * 0.5)
    dx = (np.arange(W, dtype=f32) - cx)[None, :].repeat(H, 0)
    dy = (np.arange(H, dtype=f32) - cy)[:, None].repeat(W, 1)
    sx = cx + (m[0] * dx + m[1] * dy)
    sy = cy + (m[2] * dx + m[3] * dy)
    assert sx.dtype == f32 and sy.dtype == f32
    return sx, sy


def weight(sx, sy, tx, ty):
    """float32 w(s, t) = max(0, 1 - |sx - tx|) max(0, 1 - |sy - ty|), every operation rounded on its own."""
    wx = np.maximum(f32(0), f32(1) - np.abs(sx - tx.astype(f32)))
    wy = np.maximum(f32(0), f32(1) - np.abs(sy - ty.astype(f32)))
    w = wx * wy
    assert w.dtype == f32
    return w


def taps(row, H, W):
    """The four taps of every output pixel, in the device's order: a list of (flat source index [H,W] int64 (clipped), weight [H,W]
    float32 with 0 where the tap is outside the image)."""
    sx, sy = positions(row, H, W)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    out = []
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = x0 + dx, y0 + dy
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            w = np.where(inside, weight(sx, sy, tx, ty), f32(0)).astype(f32)
            out.append((np.clip(ty, 0, H - 1) * W + np.clip(tx, 0, W - 1), w))
    return out


def is_identity(row):
    return tuple(float(v) for v in np.asarray(row).reshape(-1)) == IDENTITY


def apply_one(x, row, adjoint=False):
    """One image [3,H,W] (any float dtype) under one table row: R x, or R^T x by scattering with the same coefficients."""
    if is_identity(row):
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
    if is_identity(row):
        return np.ones((H, W), np.int64)
    n = np.zeros(H * W, np.int64)
    for idx, w in taps(row, H, W):
        if adjoint:
            np.add.at(n, idx.reshape(-1), (w.reshape(-1) > 0).astype(np.int64))
        else:
            n += (w.reshape(-1) > 0)
    return n.reshape(H, W)


def edge_draws5(B, seed=0):
    """[B,5] fp32 draws whose first eight rows pin the edges:
       row 0: z_s and z_a at the upper clamp (u0 = u3 = 1 - 2^-24, u1 = u4 = 0), theta at its lower end (u2 = 0: -pi)
       row 1: z_s and z_a at the lower clamp (u1 = u4 = 0.5), theta at its upper end (u2 = 1 - 2^-24)
       row 2: theta = 0 (u2 = 0.5);  row 3: theta = +pi/2 (u2 = 0.75);  row 4: theta = -pi/2 (u2 = 0.25)
       row 5: z_s up, z_a down;  row 6: z_s down, z_a up;  row 7 and beyond: random."""
    g = np.random.default_rng(seed + 4099)
    u = g.random((B, 5), dtype=f32)
    up, down = (EDGE, f32(0)), (EDGE, f32(0.5))
    pins = [(up, f32(0), up), (down, EDGE, down), (None, f32(0.5), None), (None, f32(0.75), None), (None, f32(0.25), None),
            (up, None, down), (down, None, up)]
    for b, (zs, th, za) in enumerate(pins[:B]):
        if zs is not None:
            u[b, 0], u[b, 1] = zs
        if th is not None:
            u[b, 2] = th
        if za is not None:
            u[b, 3], u[b, 4] = za
    return u.astype(f32)
