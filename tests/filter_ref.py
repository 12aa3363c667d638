"""The image-space filtering group of the ADA paper (``imgfilter``, policy bit 8192; include/sgx.h) restated in
fp64 NumPy: the constant 4 x 43 filter bank, the variate, the per-image band gains and the [22] half-rows, the whole-sample
reflection, and the operator y = A_v A_h x with its adjoint A_h^T A_v^T g -- once by explicit ``np.pad(mode="reflect")`` and
convolution, once (independently) through the dense per-axis matrix A -- and a torch-double version for autograd.  Images here are
[B, H, W, 3] (the kernels' layout) unless a function says otherwise."""
import numpy as np
import torch

f32 = np.float32
BIT = 8192
TAPS, HALF = 43, 21
EDGE = np.nextafter(f32(1), f32(0))                       # the largest fp32 below 1


# ------------------------------------------------------------------------------------------------------------------- the bank
def bank():
    """fp64 [4][43]: band i of the sym2 filter bank, as the header builds it."""
    s3 = np.sqrt(3.0)
    lo = np.array([1 - s3, 3 - s3, 3 + s3, 1 + s3]) / (4 * np.sqrt(2.0))
    hi = lo * (-1.0) ** np.arange(4)
    lo2 = np.convolve(lo, lo[::-1]) / 2
    hi2 = np.convolve(hi, hi[::-1]) / 2
    fb = np.array([[1.0], [0.0], [0.0], [0.0]])
    for i in range(1, 4):
        n = fb.shape[1]
        z = np.zeros((4, 2 * n - 1))
        z[:, ::2] = fb
        fb = np.stack([np.convolve(r, lo2) for r in z])
        c = fb.shape[1] // 2
        fb[i, c - 3:c + 4] += hi2
    assert fb.shape == (4, TAPS)
    fb[np.abs(fb) < 1e-12] = 0.0
    return fb


FB = bank()
FBH = FB[:, HALF:].astype(f32)                            # the half-rows the kernels hold, fbh[i][j] = fb[i][21 + j] rounded to fp32


# ------------------------------------------------------------------------------------------------------- draws, gains, rows
def z(ua, ub):
    ua, ub = np.asarray(ua, f32).astype(np.float64), np.asarray(ub, f32).astype(np.float64)
    return np.clip(np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(2.0 * np.pi * ub), -3.0, 3.0)


def gates(gu, p, policy=BIT):
    """[B,4] gate uniforms against p (strict fp32 <) -> bool [B,4]: band i is on."""
    gu = np.asarray(gu, f32)
    on = gu < f32(p)
    return on if policy & BIT else np.zeros_like(on)


def gains(u, on=None):
    """u [B,8] -> fp64 [B,4] band gains; on: bool [B,4] (None: every band on)."""
    u = np.asarray(u, f32)
    B = u.shape[0]
    on = np.ones((B, 4), bool) if on is None else np.asarray(on, bool)
    g = np.ones((B, 4))
    for i in range(4):
        t = np.ones((B, 4))
        t[:, i] = np.where(on[:, i], 2.0 ** z(u[:, 2 * i], u[:, 2 * i + 1]), 1.0)
        t /= np.sqrt((t * t).mean(axis=1, keepdims=True))
        g *= t
    return g


IDENTITY = (1.0,) + (0.0,) * HALF


def rows(u, on=None):
    """-> fp64 [B,22] half-rows c[j] = sum_i g_i fbh[i][j]; an image with every band off gets (1, 0, ..., 0)."""
    g = gains(u, on)
    c = g @ FBH.astype(np.float64)
    if on is not None:
        c[~np.asarray(on, bool).any(axis=1)] = IDENTITY
    return c


def is_identity(row):
    return tuple(float(v) for v in row) == IDENTITY


def full(c):
    """half-row(s) [..., 22] -> the 43 taps h[k] = c[|k - 21|]."""
    c = np.asarray(c)
    return c[..., np.abs(np.arange(TAPS) - HALF)]


def edge_draws8(B, seed=0):
    """[B,8] fp32 draws: rows 0..4 pin every band's z at a clamp end (ua just under 1; ub = 0 gives +3, ub = 0.5 gives -3) in patterns
    that differ between the bands -- equal gains would give a scaled impulse, the bank's rows sum to one -- row 5 has every u at 0
    (z = 0: gains of exactly 1), row 6 every ub just under 1; the rest are random."""
    g = np.random.default_rng(seed + 43)
    u = g.random((B, 8)).astype(f32)
    signs = [(1, -1, 1, -1), (-1, 1, -1, 1), (1, 1, -1, -1), (-1, -1, -1, 1), (1, -1, -1, -1)]
    for r, sg in enumerate(signs[:B]):
        u[r, 0::2] = EDGE
        u[r, 1::2] = [0.0 if v > 0 else 0.5 for v in sg]
    if B > 5:
        u[5] = 0.0
    if B > 6:
        u[6, 1::2] = EDGE
    return u


def gate_patterns():
    """[16,4] gate uniforms: against p = 0.5 row k switches exactly the bands of the bits of k on."""
    k = np.arange(16)[:, None]
    return np.where((k >> np.arange(4)) & 1, 0.25, 0.75).astype(f32)


# ------------------------------------------------------------------------------------------------------------- the operator
def refl(q, N):
    """Whole-sample reflection continued periodically: np.pad(mode='reflect') for any pad width; N >= 2."""
    P = 2 * (N - 1)
    m = np.mod(q, P)
    return np.where(m < N, m, P - m)


def dense(c, N, shift=0, edge=False):
    """The fp64 [N][N] matrix A of one axis: (A x)[i] = sum_k h[k] x[refl(i + k - 21)].  shift / edge plant errors (a row shifted by one
    tap; reflection that repeats the edge sample) for the tests that show the bounds bite."""
    h = full(np.asarray(c, np.float64))
    A = np.zeros((N, N))
    for i in range(N):
        for k in range(TAPS):
            q = i + k - HALF + shift
            A[i, int(np.clip(q, 0, N - 1)) if edge else int(refl(q, N))] += h[k]
    return A


def folds(N):
    """The largest number of positions q in [-21, N + 20] that reflect onto one sample of an axis of length N."""
    return int(np.bincount(refl(np.arange(-HALF, N + HALF), N), minlength=N).max())


def axis_pad(x, c, axis):
    """One axis by explicit padding: np.pad(mode='reflect') by 21 each side, then the 43-tap correlation."""
    h = full(np.asarray(c, np.float64))
    pad = [(0, 0)] * x.ndim
    pad[axis] = (HALF, HALF)
    xp = np.pad(x, pad, mode="reflect")
    N = x.shape[axis]
    out = np.zeros_like(x)
    for k in range(TAPS):
        out += h[k] * np.take(xp, np.arange(k, k + N), axis=axis)
    return out


def axis_pad_adjoint(g, c, axis):
    """The adjoint of axis_pad as the header states it: the zero-extended g correlated with h over q in [-21, N + 20], then every q
    folded onto refl(q)."""
    h = full(np.asarray(c, np.float64))
    N = g.shape[axis]
    pad = [(0, 0)] * g.ndim
    pad[axis] = (2 * HALF, 2 * HALF)
    gp = np.pad(g, pad)                                       # zeros: gp index = i + 42
    zq = np.zeros_like(np.take(gp, np.arange(N + 2 * HALF), axis=axis))
    for i_off in range(TAPS):                                 # z[q] = sum_i h[q - i + 21] g[i],  q = -21 .. N + 20
        zq += h[TAPS - 1 - i_off] * np.take(gp, np.arange(i_off, i_off + N + 2 * HALF), axis=axis)
    out = np.zeros_like(g)
    tgt = refl(np.arange(-HALF, N + HALF), N)
    zq = np.moveaxis(zq, axis, 0)
    o = np.moveaxis(out, axis, 0)
    for n, j in enumerate(tgt):
        o[j] += zq[n]
    return out


def apply_pad(x, c, adjoint=False):
    """x fp64 [B,H,W,3], c [B,22] -> A_v A_h x (or A_h^T A_v^T x) by padding and convolution."""
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        if adjoint:
            out[b] = axis_pad_adjoint(axis_pad_adjoint(x[b], c[b], 0), c[b], 1)
        else:
            out[b] = axis_pad(axis_pad(x[b], c[b], 1), c[b], 0)
    return out


def apply_dense(x, c, adjoint=False, absolute=False, **plant):
    """The same through the dense matrices: y[b] = A_H x[b] A_W^T per channel (adjoint: A_H^T x[b] A_W).  absolute: A built from |h| -- the taps' magnitudes
    folded, what a sum over the 43 taps accumulates its rounding errors against (the magnitudes of the error bounds)."""
    x = np.asarray(x, np.float64)
    B, H, W, _ = x.shape
    out = np.empty_like(x)
    for b in range(B):
        cb = np.abs(c[b]) if absolute else c[b]
        AH, AW = dense(cb, H, **plant), dense(cb, W, **plant)
        if adjoint:
            AH, AW = AH.T, AW.T
        out[b] = np.einsum("ikc,lk->ilc", np.einsum("ij,jkc->ikc", AH, x[b]), AW)
    return out


def apply_torch(x, c, adjoint=False):
    """torch-double, differentiable in x: x [B,H,W,3] double, c [B,22] (NumPy)."""
    B, H, W, _ = x.shape
    outs = []
    for b in range(B):
        AH, AW = torch.from_numpy(dense(c[b], H)), torch.from_numpy(dense(c[b], W))
        if adjoint:
            AH, AW = AH.T, AW.T
        outs.append(torch.einsum("ikc,lk->ilc", torch.einsum("ij,jkc->ikc", AH.to(x.device), x[b]), AW.to(x.device)))
    return torch.stack(outs)


def gamma(n):
    e = n * 2.0 ** -24
    return e / (1 - e)
