"""Restatement of ADA's colour group (include/sgx.h, sgx_ada_color_matrix and sgx_ada_color): brightness, contrast, lumaflip, hue and
saturation composed per image into one affine map y = M x + t of the RGB vector.  The product never imports this.

  ``matrices``        draws -> the [B,12] table {M row major, t} in fp64, from the same fp32 uniforms (what the device's fp32 table
                      approximates); ``homogeneous`` the five 4x4 matrices of the paper, whose product the table must equal
  ``apply32``         the three passes (forward, linear part, adjoint) in NumPy float32, every product and sum rounded to fp32 on its
                      own in the header's order: the device's output bit for bit, given the device's table
  ``apply``           the same maps on a torch batch in the batch's own dtype, so autograd yields the adjoint and the double backward
                      and it composes with the oracle's discriminator

``u`` holds eight uniform draws per image (u0, u1: brightness; u2, u3: contrast; u4: lumaflip; u5: hue; u6, u7: saturation)."""
import numpy as np
import torch

OPS = ("brightness", "contrast", "lumaflip", "hue", "saturation")
BRIGHTNESS, CONTRAST, LUMAFLIP, HUE, SATURATION = 256, 512, 1024, 2048, 4096
OP_BITS = (BRIGHTNESS, CONTRAST, LUMAFLIP, HUE, SATURATION)
ALL = sum(OP_BITS)
f32 = np.float32
EDGE = f32(1.0 - 2.0 ** -24)                       # the largest float32 below 1
BELOW_HALF = f32(0.5 - 2.0 ** -25)                 # the largest float32 below 0.5
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
V = np.ones(3) / np.sqrt(3.0)
P = np.outer(V, V)
K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]]) / np.sqrt(3.0)


def gates(gu, p, policy_bits):
    """gu [B,5] -> int [B]: policy_bits & (256 [gu0 < p] | 512 [gu1 < p] | ... | 4096 [gu4 < p]), strict < in fp32 (the rule of
    tests/ada_ref.py)."""
    gu = np.asarray(gu, dtype=f32).reshape(-1, 5)
    on = (gu < f32(p)).astype(np.int64)
    return (int(policy_bits) & ALL) & sum(bit * on[:, k] for k, bit in enumerate(OP_BITS))


def params(u_row, bits):
    """One image's z_b, z_c, z_s and b, c, sigma, theta, s in fp64 from its fp32 uniforms; an op that is not in ``bits`` gives its off
    value (b = 0, c = 1, sigma = 1, theta = 0, s = 1)."""
    u = [float(f32(v)) for v in u_row]

    def z(ua, ub):
        return min(max(np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(2.0 * np.pi * ub), -3.0), 3.0)
    z_b, z_c, z_s = z(u[0], u[1]), z(u[2], u[3]), z(u[6], u[7])
    return dict(z_b=z_b, z_c=z_c, z_s=z_s,
                b=0.2 * z_b if bits & BRIGHTNESS else 0.0,
                c=2.0 ** (0.5 * z_c) if bits & CONTRAST else 1.0,
                sigma=1.0 - 2.0 * min(np.floor(2.0 * u[4]), 1.0) if bits & LUMAFLIP else 1.0,
                theta=2.0 * np.pi * (u[5] - 0.5) if bits & HUE else 0.0,
                s=2.0 ** z_s if bits & SATURATION else 1.0)


def matrix(b, c, sigma, theta, s):
    """{M row major, t} as twelve numbers: M = c [sigma P + s (cos(theta) (I - P) + sin(theta) K)], t = c sigma b (1,1,1)."""
    M = c * (sigma * P + s * (np.cos(theta) * (np.eye(3) - P) + np.sin(theta) * K))
    return np.concatenate([M.reshape(-1), np.full(3, c * sigma * b)])


def homogeneous(b, c, sigma, theta, s):
    """The five 4x4 matrices of the paper in the order they are applied: brightness, contrast, luma flip, hue rotation, saturation."""
    def h(A=np.eye(3), t=np.zeros(3)):
        out = np.eye(4)
        out[:3, :3], out[:3, 3] = A, t
        return out
    rot = P + np.cos(theta) * (np.eye(3) - P) + np.sin(theta) * K            # Rodrigues' rotation about v
    return [h(t=np.full(3, b)), h(c * np.eye(3)), h(np.eye(3) - (1.0 - sigma) * P), h(rot), h(P + (np.eye(3) - P) * s)]


def matrices(u, img_bits):
    """u [B,8], per-image bits [B] (or one int) -> fp64 [B,12]; an image with no colour bit gets the exact identity row."""
    u = np.asarray(u, dtype=f32)
    bits = [int(img_bits)] * u.shape[0] if np.isscalar(img_bits) else [int(b) for b in img_bits]
    out = np.zeros((u.shape[0], 12), np.float64)
    for k in range(u.shape[0]):
        if not bits[k] & ALL:
            out[k] = IDENTITY
        else:
            p = params(u[k], bits[k])
            out[k] = matrix(p["b"], p["c"], p["sigma"], p["theta"], p["s"])
    return out


def is_identity(row):
    return tuple(float(v) for v in np.asarray(row).reshape(-1)) == IDENTITY


def is_diagonal_case(u_row, bits):
    """No flip (lumaflip off, or on with sigma = 1), hue and saturation off: the row the header promises exactly diagonal."""
    return not bits & (HUE | SATURATION) and params(u_row, bits)["sigma"] == 1.0


def coefficients(row, adjoint):
    """(c [3,3], t [3]) of one table row as the pass applies them: out_k = ((c[k,0] in_0 + c[k,1] in_1) + c[k,2] in_2) (+ t[k])."""
    row = np.asarray(row)
    M = row[:9].reshape(3, 3)
    return (M.T if adjoint else M), row[9:]


def apply32(x, mat, adjoint=False, with_bias=True):
    """float32 [B,H,W,3] under the float32 table ``mat`` [B,12] in the kernel's operation order; an identity row is a copy."""
    x, mat = np.asarray(x), np.asarray(mat)
    assert x.dtype == f32 and mat.dtype == f32 and not (adjoint and with_bias)
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        if is_identity(mat[b]):
            out[b] = x[b]
            continue
        c, t = coefficients(mat[b], adjoint)
        for k in range(3):
            o = (c[k, 0] * x[b, ..., 0] + c[k, 1] * x[b, ..., 1]) + c[k, 2] * x[b, ..., 2]
            out[b, ..., k] = o + t[k] if with_bias else o
    assert out.dtype == f32
    return out


def apply(x, mat, adjoint=False, with_bias=True):
    """A torch batch [B,3,H,W] (any float dtype) under the table ``mat`` [B,12] (any array-like): M x + t, M x, or M^T x."""
    mat = np.asarray(mat.detach().cpu() if isinstance(mat, torch.Tensor) else mat, dtype=np.float64)
    M = torch.from_numpy(mat[:, :9].reshape(-1, 3, 3).copy()).to(x.dtype)
    if adjoint:
        assert not with_bias
        M = M.transpose(1, 2)
    y = torch.einsum("bkj,bjhw->bkhw", M, x)
    if with_bias:
        y = y + torch.from_numpy(mat[:, 9:].copy()).to(x.dtype)[:, :, None, None]
    return y


def edge_draws8(B, seed=0):
    """[B,8] fp32 draws whose first eight rows pin the edges (up: u_a = 1 - 2^-24, u_b = 0 gives z = +3; down: u_b = 0.5 gives z = -3):
       row 0: z_b, z_c, z_s at the upper clamp, a flip with u4 = 0.5 exactly, theta at its lower end (u5 = 0: -pi)
       row 1: z_b, z_c, z_s at the lower clamp, no flip with u4 the largest float below 0.5, theta at its upper end (u5 = 1 - 2^-24)
       row 2: theta = 0 (u5 = 0.5), u4 = 0;  row 3: theta = +pi/2 (u5 = 0.75), u4 = 1 - 2^-24;  row 4: theta = -pi/2 (u5 = 0.25)
       row 5: z_c up, z_s down;  row 6: z_c down, z_s up, z_b up
       row 7: the all-off row: draws whose parameters are the off values (u_a = 0 gives z = 0: b = 0, c = 1, s = 1; no flip; theta = 0)
       row 8 and beyond: random."""
    g = np.random.default_rng(seed + 8191)
    u = g.random((B, 8), dtype=f32)
    up, down, zero = (EDGE, f32(0)), (EDGE, f32(0.5)), (f32(0), f32(0))
    pins = [(up, up, f32(0.5), f32(0), up), (down, down, BELOW_HALF, EDGE, down), (None, None, f32(0), f32(0.5), None),
            (None, None, EDGE, f32(0.75), None), (None, None, None, f32(0.25), None), (None, up, None, None, down),
            (up, down, None, None, up), (zero, zero, f32(0), f32(0.5), zero)]
    for b, (zb, zc, flip, hue, zs) in enumerate(pins[:B]):
        for col, pair in ((0, zb), (2, zc), (6, zs)):
            if pair is not None:
                u[b, col], u[b, col + 1] = pair
        if flip is not None:
            u[b, 4] = flip
        if hue is not None:
            u[b, 5] = hue
    return u.astype(f32)
