"""The image-space corruptions of the ADA paper (``noise`` 16384, ``imgcutout`` 32768; include/sgx.h) restated in
NumPy: Philox4x32-10 in integer arithmetic, the per-image table (sigma, k0, k1, x0, x1, y0, y1, 0) in float32 (its integer entries
exactly the kernel's), the normals in fp64 from the same generator outputs, the forward y = M (x + sigma n) and the linear part M g
with the cut mask from the table's bounds, and the per-element criterion the GPU tests hold the kernels to.  Images are [B, H, W, 3]."""
import numpy as np

f32 = np.float32
NOISE, CUTOUT = 16384, 32768
ALL = NOISE | CUTOUT
EDGE = np.nextafter(f32(1), f32(0))                       # the largest fp32 below 1
ZERO_ROW = (0.0,) * 8
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------------------------ the generator
def philox(counter, key, rounds=10):
    """Philox4x32 on uint32 words held in uint64 arrays: counter (c0, c1, c2, c3) and key (k0, k1), each word a scalar or an array of
    one shape -> uint32 [..., 4]."""
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) & _MASK for v in np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in counter]))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                              # 32 x 32 -> 64 bits: no overflow
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def normals(q, k0, k1, rounds=10):
    """The four normals of the counters q (an integer array) under the key -> fp64 [len(q), 4]: two Box-Muller pairs, no clamp."""
    q = np.asarray(q, np.uint64)
    o = philox((q, 0, 0, 0), (int(k0), int(k1)), rounds).astype(np.uint64)
    u = (o >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    out = np.empty(q.shape + (4,))
    for m in range(2):
        rad = np.sqrt(-2.0 * np.log(1.0 - u[..., 2 * m]))
        out[..., 2 * m] = rad * np.cos(2.0 * np.pi * u[..., 2 * m + 1])
        out[..., 2 * m + 1] = rad * np.sin(2.0 * np.pi * u[..., 2 * m + 1])
    return out


def field(k0, k1, n, rounds=10, q_offset=0, order=(0, 1, 2, 3)):
    """The first n elements of an image's field, fp64 [n]: element e takes normal e & 3 of counter e >> 2.  rounds / q_offset / order
    plant errors (nine rounds, the counter q + 1, the normals of a counter taken in another order)."""
    e = np.arange(n, dtype=np.int64)
    nq = normals(np.arange((n + 3) // 4, dtype=np.int64) + q_offset, k0, k1, rounds)
    return nq[e >> 2, np.asarray(order)[e & 3]]


# ---------------------------------------------------------------------------------------------------------------------- the table
def z(ua, ub):
    ua, ub = np.asarray(ua, f32).astype(np.float64), np.asarray(ub, f32).astype(np.float64)
    return np.clip(np.sqrt(-2.0 * np.log(1.0 - ua)) * np.cos(2.0 * np.pi * ub), -3.0, 3.0)


def gates(gu, p, policy=ALL):
    """[B,2] gate uniforms against p (strict fp32 <) -> bool [B,2]: (noise, cutout) on."""
    on = np.asarray(gu, f32) < f32(p)
    return on & np.array([bool(policy & NOISE), bool(policy & CUTOUT)])


def sigma64(u):
    """fp64 [B]: 0.1 |z(u0, u1)|."""
    u = np.asarray(u, f32)
    return 0.1 * np.abs(z(u[:, 0], u[:, 1]))


def key(u):
    """min((uint32)(u * 2^24), 2^24 - 1): exact in any arithmetic, u is an fp32 in [0, 1]."""
    return np.minimum(np.floor(np.asarray(u, f32).astype(np.float64) * 16777216.0), 16777215.0)


def interval(c, N):
    """The cut interval [lo, hi) of an axis of N samples around the centres c (fp32), in float32 arithmetic, every operation rounded
    on its own, as the header orders them."""
    c, n = np.asarray(c, f32), f32(N)
    a, q = c * n, f32(0.25) * n
    lo = np.maximum(0, np.floor((a - q) - f32(0.5)).astype(np.int64) + 1)
    hi = np.minimum(N, np.ceil((a + q) - f32(0.5)).astype(np.int64))
    return lo, hi


def interval64(c, N):
    """The paper's predicate in fp64: bool [len(c), N], sample j is cut iff |(j + 0.5) / N - c| < 0.25."""
    c = np.asarray(c, f32).astype(np.float64)[:, None]
    return np.abs((np.arange(N) + 0.5) / N - c) < 0.25


def table(u, H, W, on=None):
    """u [B,6] -> float32 [B,8] rows; on: bool [B,2] (None: both ops on).  sigma is the fp64 value rounded (the kernel's differs by its
    libm: compare it with a tolerance); every other entry is exact."""
    u = np.asarray(u, f32)
    B = u.shape[0]
    on = np.ones((B, 2), bool) if on is None else np.asarray(on, bool)
    t = np.zeros((B, 8), f32)
    t[:, 0] = np.where(on[:, 0], sigma64(u), 0.0)
    t[:, 1] = np.where(on[:, 0], key(u[:, 2]), 0.0)
    t[:, 2] = np.where(on[:, 0], key(u[:, 3]), 0.0)
    x0, x1 = interval(u[:, 4], W)
    y0, y1 = interval(u[:, 5], H)
    for k, v in zip((3, 4, 5, 6), (x0, x1, y0, y1)):
        t[:, k] = np.where(on[:, 1], v, 0)
    return t


def edge_draws6(B, seed=0):
    """[B,6] fp32 draws: rows 0..4 put the centre at 0, just under 1, 0.25, 0.75 and 0.5 (cx and cy in different patterns), rows 0 and 1
    pin z at the clamp ends (ua just under 1; ub = 0 gives +3, ub = 0.5 gives -3), row 2 has u0 = 0 (sigma = 0 with the op on), row 3
    every u just under 1, row 4 key draws of 0; the rest are random."""
    g = np.random.default_rng(seed + 6)
    u = g.random((B, 6)).astype(f32)
    cs = [(0.0, EDGE), (EDGE, 0.25), (0.25, 0.75), (0.75, 0.5), (0.5, 0.0)]
    for r, (cx, cy) in enumerate(cs[:B]):
        u[r, 4], u[r, 5] = cx, cy
    if B > 0:
        u[0, 0], u[0, 1] = EDGE, 0.0
    if B > 1:
        u[1, 0], u[1, 1] = EDGE, 0.5
    if B > 2:
        u[2, 0] = 0.0
    if B > 3:
        u[3, :4] = EDGE
    if B > 4:
        u[4, 2:4] = 0.0
    return u


def gate_patterns():
    """[4,2] gate uniforms: against p = 0.5 row k switches exactly the ops of the bits of k on (bit 0 noise, bit 1 cutout)."""
    k = np.arange(4)[:, None]
    return np.where((k >> np.arange(2)) & 1, 0.25, 0.75).astype(f32)


# -------------------------------------------------------------------------------------------------------------------- the passes
def cut_mask(tab, H, W):
    """bool [B,H,W]: the cut pixels of every row of the table."""
    tab = np.asarray(tab)
    i, j = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    x0, x1, y0, y1 = (tab[:, k].astype(np.int64)[:, None, None] for k in (3, 4, 5, 6))
    return (i >= y0) & (i < y1) & (j >= x0) & (j < x1)


def noise_term(tab, H, W, **plant):
    """fp64 [B,H,W,3]: sigma n of every image under its (fp32) row."""
    tab = np.asarray(tab, f32)
    out = np.zeros((tab.shape[0], H, W, 3))
    for b, r in enumerate(tab):
        if r[0] != 0:
            out[b] = (float(r[0]) * field(int(r[1]), int(r[2]), 3 * H * W, **plant)).reshape(H, W, 3)
    return out


def linear(x, tab):
    """M x in x's dtype: a cut pixel is +0, every other element keeps its bits."""
    x = np.asarray(x)
    out = x.copy()
    out[cut_mask(tab, x.shape[1], x.shape[2])] = 0
    return out


def forward(x, tab, **plant):
    """fp64 [B,H,W,3]: M (x + sigma n)."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        y = x.astype(np.float64)
    noisy = np.asarray(tab)[:, 0] != 0                       # (an image with sigma == 0 keeps its x: -0 + 0 would lose the sign)
    y[noisy] += noise_term(tab, x.shape[1], x.shape[2], **plant)[noisy]
    y[cut_mask(tab, x.shape[1], x.shape[2])] = 0.0
    return y


def bits(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


def violations(y, x, tab, mode, n_tol):
    """The per-element criterion: bool [B,H,W,3], True where y (fp32, what a pass under the fp32 table gave for the fp32 x) breaks it.
    Mode 1, cut pixels and the images with sigma == 0 are held bit for bit to ``linear``; a noisy element to
    |y - y64| <= 2^-24 (|sigma n64| + |y64|) + sigma n_tol: the two roundings of the product and the sum, and the normal's own error."""
    y, x, tab = np.asarray(y, f32), np.asarray(x, f32), np.asarray(tab, f32)
    B, H, W, _ = x.shape
    bad = bits(y) != bits(linear(x, tab))
    if mode == 1:
        return bad
    noisy = (tab[:, 0] != 0)[:, None, None] & ~cut_mask(tab, H, W)
    sn = noise_term(tab, H, W)
    with np.errstate(invalid="ignore"):                       # (signalling NaNs among the inputs)
        y64 = x.astype(np.float64) + sn
        yd = y.astype(np.float64)
        ok = np.abs(yd - y64) <= 2.0 ** -24 * (np.abs(sn) + np.abs(y64)) + tab[:, 0].astype(np.float64)[:, None, None, None] * n_tol
        ok = np.where(np.isfinite(y64), ok, (yd == y64) | (np.isnan(yd) & np.isnan(y64)))      # an infinite or NaN x stays what it is
    return np.where(noisy[..., None], ~ok, bad)
