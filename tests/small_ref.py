"""fp64 restatements of the entry points of csrc/small.hip that are not streaming kernels -- the fp32 MFMA GEMM with its EqualizedLinear fusions,
the grouped style affines, minibatch stddev and the logistic loss head -- written from their definitions in include/sgx.h; the launcher rules
of that file restated in Python (which kernel, which grid, how many splits, how long a wave's K slice); the per-element criteria; and the table of
cases that walks every launch path.  Test-side only: the product never imports this, and nothing here calls the library under test.  The
criterion, the guard bands and the kernel names are streaming_ref's (assert_elementwise, Guarded, kernel_id, f32); epilogue_ref lends
assert_within and kink_cap.

Operands are drawn on the CPU from seeded generators (tests/test_small_coverage.py checks the references' own properties -- the kink counts, the
exactness of the integer rows -- without a GPU); the GPU tests move them to the device."""
from collections import namedtuple

import numpy as np
import torch

import epilogue_ref as ER
import streaming_ref as SR
from streaming_ref import LRELU, U32, Case, f32

F, H = torch.float32, torch.bfloat16
ULP32 = 2.0 ** -23                  # one fp32 ulp relative to the value, at most
TINY32 = 2.0 ** -126                # the smallest normal fp32: what a flushed or gradually underflowing result may be off by
# expf / log1pf: the HIP math documentation is not part of the ROCm tree these tests run against, so the allowance is an assumption, the
# OpenCL full-profile limits that the device library (OCML) is written to: exp <= 3 ulp, log1p <= 2 ulp.
ULP_EXP, ULP_LOG1P = 3, 2


def cdiv(a, b):
    return -(-a // b)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    return scale * torch.randn(tuple(shape), generator=_gen(seed), dtype=torch.float32)


def ints(shape, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).to(torch.float32)


def slope(mask):
    """lrelu_slope of the kernels: 1 where the stored activation is > 0, else 0.2f."""
    return torch.where(mask > 0, 1.0, LRELU).to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------- launcher rules: GEMM
K1, K8, OUTER, REDUCE = "gemm_f32_kernel<1>", "gemm_f32_kernel<8>", "gemm_outer_kernel", "gemm_splitk_reduce"
GemmPlan = namedtuple("GemmPlan", "kernels launches splits kper body tail")


def gemm_splits(M, N, K):
    tiles = cdiv(M, 16) * cdiv(N, 16)
    if tiles >= 256 or K < 1024:
        return 1
    return max(1, min(K // 256, cdiv(512, tiles)))


def gemm_ws_bytes(M, N, K):
    s = gemm_splits(M, N, K)
    return s * M * N * 4 if s > 1 else 0


def gemm_slices(K, splits):
    """[z][wave] -> (kb, ke) as gemm_f32_kernel derives them: kb >= ke is an empty slice."""
    kz = cdiv(cdiv(K, splits), 16) * 16
    out = []
    for z in range(splits):
        kz0 = z * kz
        kz1 = kz0 + kz if kz0 + kz < K else K
        kper = cdiv(cdiv(max(kz1 - kz0, 0), 4), 16) * 16
        out.append([(kz0 + w * kper, min(kz0 + w * kper + kper, kz1) if kz0 + w * kper + kper < kz1 else kz1) for w in range(4)])
    return out


def gemm_plan(M, N, K, ta, tb, mask=False, epi=False, ws_bytes=0, aligned=True):
    """gemm_launch.  mask: amask given; epi: bias, activation or colsum fused (those keep one split); ws_bytes: 0 for a NULL workspace;
    aligned: B and C on 16 bytes (the outer-product kernel's own check)."""
    splits = gemm_splits(M, N, K)
    if splits > 1 and (ws_bytes < splits * M * N * 4 or epi):
        splits = 1
    if K <= 4 and not tb and N % 4 == 0 and not (mask or epi) and aligned:
        return GemmPlan((OUTER,), [((cdiv(M * (N // 4), 256), 1, 1), (256, 1, 1), 0)], 1, K, None, False)
    kern = K8 if cdiv(K, splits) >= 512 else K1
    sl = [s for z in gemm_slices(K, splits) for s in z]
    kper = max(max(ke - kb, 0) for kb, ke in sl)
    body = (not ta and K % 4 == 0, bool(tb) and K % 4 == 0, bool(mask))
    tail = any(ke > kb and (ke - kb) % 16 for kb, ke in sl)
    launches = [((cdiv(N, 16), cdiv(M, 16), splits), (256, 1, 1), 0)]
    if splits == 1:
        return GemmPlan((kern,), launches, 1, kper, body, tail)
    return GemmPlan((kern, REDUCE), launches + [((cdiv(M * N, 256), 1, 1), (256, 1, 1), 0)], splits, kper, body, tail)


def gemm_plan_ints(pl, align):
    """A GemmPlan as the seven ints of sgx_gemm_plan (include/sgx.h): kernel 0 / 1 / 2, splits, that kernel's grid, the reduce's grid (0 when
    unsplit) and vec.  align: the query's own argument, whose bits 0 and 1 (A and its mask, B on 16 bytes) are the tile kernel's vec."""
    (gx, gy, gz), _, _ = pl.launches[0]
    kind = {OUTER: 0, K1: 1, K8: 2}[pl.kernels[0]]
    return [kind, pl.splits, gx, gy, gz, pl.launches[1][0][0] if len(pl.launches) > 1 else 0, align & 3 if kind else 0]


def gemm_chain(pl, mask=False, bias=False, act=False):
    """The fp32 operations on an output's longest chain.  Every product that enters an MFMA accumulator counts as one (the order inside the
    instruction is not specified): a wave's slice of kper values of k is kper of them (the outer-product kernel: K fused multiply-adds).  Then
    the 3 adds across the waves' partials in LDS, `splits` adds in gemm_splitk_reduce when the launch is split, the multiply by alpha; a masked
    operand was rounded once when it was multiplied by its slope; the bias costs its product and the add, LeakyReLU one multiply."""
    return pl.kper + 3 + (pl.splits if pl.splits > 1 else 0) + 1 + (1 if mask else 0) + (2 if bias else 0) + (1 if act else 0)


# ---------------------------------------------------------------------------------------------------------------- launcher rules: the rest
def style_mb(B):
    return 4 if B <= 4 else 8 if B <= 8 else 16 if B <= 16 else 32


def style_layout(Ns, B):
    """-> (y offsets in elements, first tiles, row offsets of dw / db, total tiles), one entry per group."""
    yoff, tile, noff, yo, ti, no = 0, 0, 0, [], [], []
    for n in Ns:
        yo.append(yoff); ti.append(tile); no.append(noff)
        yoff += B * n; tile += cdiv(n, 16); noff += n
    return yo, ti, no, tile


def style_plan(entry, B, D, Ns):
    mb, G = style_mb(B), len(Ns)
    tiles = style_layout(Ns, B)[3]
    if entry == "sgx_style_fwd":
        return (f"style_fwd_kernel<{mb}>",), [((tiles, 1, 1), (256, 1, 1), B * D * 4)]
    if entry == "sgx_style_bwd_data":                        # LDS: the transposed gy image [max_n][MB], reused for the wave partials [4][B][64]
        return (f"style_bwd_data_kernel<{mb}>",), [((D // 64, G, 1), (256, 1, 1), max(mb * max(Ns), 4 * B * 64) * 4)]
    return (f"style_bwd_param_kernel<{mb}>",), [((tiles, 1, 1), (256, 1, 1), 0)]


def style_full_chunks(N, wave=0):
    """16-row chunks a wave of style_bwd_data_kernel owns entirely (the pipelined part of its loop)."""
    return (N - wave + 3) // 4 // 16 if N > wave else 0


MBSTD_NB, MBSTD_BATCH = 8, 8 * 1024                          # blocks per slot; MBSTD_U * blockDim elements per trip of the unrolled loops


def mbstd_plan(entry, B, dtype):
    G = min(B, 4)
    return (f"{entry[4:]}_kernel<{SR.tname(dtype)}>",), [((B // G, MBSTD_NB, 1), (1024, 1, 1), 0)]


def plan(c):
    """A row's expected (kernel list, launch geometry) from its arguments and the rules above."""
    a = c.args
    if c.entry == "sgx_gemm_f32":
        ws = {"full": gemm_ws_bytes(a["M"], a["N"], a["K"]), "null": 0, "short": gemm_ws_bytes(a["M"], a["N"], a["K"]) - 4}[a["ws"]]
        p = gemm_plan(a["M"], a["N"], a["K"], a["ta"], a["tb"], ws_bytes=ws, aligned="B" not in a["shift"])
    elif c.entry == "sgx_linear_fwd":
        p = gemm_plan(a["B"], a["N"], a["K"], 0, 1, epi=bool(a["bias"] or a["act"]))
    elif c.entry == "sgx_linear_bwd_data":
        p = gemm_plan(a["B"], a["K"], a["N"], 0, 0, mask=a["mask"])
    elif c.entry == "sgx_linear_bwd_param":
        p = gemm_plan(a["N"], a["K"], a["B"], 1, 0, mask=a["mask"], epi=a["db"])
    elif c.entry.startswith("sgx_style"):
        return style_plan(c.entry, a["B"], a["D"], a["Ns"])
    elif c.entry.startswith("sgx_mbstd"):
        return mbstd_plan(c.entry, a["B"], c.dtype)
    else:
        return ("logistic_loss_kernel",), [((1, 1, 1), (64, 1, 1), 0)]
    return p.kernels, p.launches


def gemm_plan_of(c):
    a = c.args
    if c.entry == "sgx_gemm_f32":
        ws = {"full": gemm_ws_bytes(a["M"], a["N"], a["K"]), "null": 0, "short": gemm_ws_bytes(a["M"], a["N"], a["K"]) - 4}[a["ws"]]
        return gemm_plan(a["M"], a["N"], a["K"], a["ta"], a["tb"], ws_bytes=ws, aligned="B" not in a["shift"])
    if c.entry == "sgx_linear_fwd":
        return gemm_plan(a["B"], a["N"], a["K"], 0, 1, epi=bool(a["bias"] or a["act"]))
    if c.entry == "sgx_linear_bwd_data":
        return gemm_plan(a["B"], a["K"], a["N"], 0, 0, mask=a["mask"])
    return gemm_plan(a["N"], a["K"], a["B"], 1, 0, mask=a["mask"], epi=a["db"])


# ---------------------------------------------------------------------------------------------------------------- references: GEMM family
def gemm(A, Bm, ta, tb, alpha, amask=None):
    """C = alpha op(A') op(B), A' = A * slope(amask) element by element (amask in A's layout).  fp64 in, -> (C, S)."""
    if amask is not None:
        A = A * slope(amask)
    a, b = (A.t() if ta else A), (Bm.t() if tb else Bm)
    return alpha * (a @ b), abs(alpha) * (a.abs() @ b.abs())


def linear_fwd(x, w, bias, w_mul, b_mul):
    """The pre-activation w_mul x W^T + b_mul bias and its S; the activation is applied by check_act (the kink rule)."""
    pre, S = gemm(x, w, 0, 1, w_mul)
    if bias is not None:
        pre, S = pre + b_mul * bias, S + abs(b_mul) * bias.abs()
    return pre, S


def linear_bwd_data(gy, y_act, w, w_mul):
    """gx = w_mul gz W, gz = gy slope(y_act)."""
    return gemm(gy, w, 0, 0, w_mul, y_act)


def linear_bwd_param(gy, y_act, x, w_mul, b_mul):
    """dW = w_mul gz^T x, db = b_mul sum_b gz."""
    gz = gy if y_act is None else gy * slope(y_act)
    dw, Sdw = gemm(gz, x, 1, 0, w_mul)
    return dw, Sdw, b_mul * gz.sum(0), abs(b_mul) * gz.abs().sum(0)


def check_act(got, pre, S, n, act, what):
    """assert_elementwise of act(pre).  With LeakyReLU an output whose reference pre-activation lies within the bound of zero may meet either
    slope (the kernel's fp32 pre-activation may have the other sign): the nearer of the two references is taken for those elements only, and
    their number -- a property of the reference alone -- stays under kink_cap."""
    if not act:
        return SR.assert_elementwise(got, pre, S, n, F, what)
    ref = SR.act(pre, 1)
    kink = pre.abs() <= (n + 2) * U32 * S
    assert int(kink.sum()) <= ER.kink_cap(pre.numel()), f"{what}: {int(kink.sum())} reference pre-activations inside the kink window"
    alt = torch.where(pre > 0, LRELU * pre, pre)
    g = got.detach().to(torch.float64).to(pre.device)
    ref = torch.where(kink & ((g - alt).abs() < (g - ref).abs()), alt, ref)
    return SR.assert_elementwise(got, ref, S, n, F, what)


def kink_count(pre, S, n):
    return int((pre.abs() <= (n + 2) * U32 * S).sum())


def assert_bits(got, exact, what, rounded=False):
    """An integer row: every partial sum is exact in fp32 in any order, so the result is the exact value's fp32, bit for bit.  rounded: the
    exact value is a product of two fp32 numbers (LeakyReLU's 0.2f * v) that the kernel rounds once, as the conversion from fp64 does."""
    want = exact.to(torch.float32)
    assert rounded or torch.equal(want.to(torch.float64), exact), f"{what}: the exact value is no fp32 number -- the row is not an integer row"
    want = want.to(got.device)
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = (got.view(torch.int32) != want.view(torch.int32)).flatten().nonzero().flatten()
        i = int(bad[0])
        at = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ from the exact value; first at flat index {i} {at}: got "
                             f"{float(got.flatten()[i])!r}, exact {float(want.flatten()[i])!r}")
    return 0.0


# ---------------------------------------------------------------------------------------------------------------- references: style affines
def style_fwd(x, W, bias, w_mul, b_mul):
    """y_g[B][N] = w_mul x_g W_g^T + b_mul bias_g."""
    ref, S = w_mul * (x @ W.t()), abs(w_mul) * (x.abs() @ W.abs().t())
    if bias is not None:
        ref, S = ref + b_mul * bias, S + abs(b_mul) * bias.abs()
    return ref, S


def style_bwd_data(gy, W, w_mul):
    """glm[layer_g][B][D] = w_mul gy_g W_g."""
    return w_mul * (gy @ W), abs(w_mul) * (gy.abs() @ W.abs())


def style_bwd_param(gy, x, w_mul, b_mul):
    """dW_g[N][D] = w_mul gy_g^T x_g, db_g[N] = b_mul sum_b gy_g."""
    return w_mul * (gy.t() @ x), abs(w_mul) * (gy.abs().t() @ x.abs()), b_mul * gy.sum(0), abs(b_mul) * gy.abs().sum(0)


def style_chain(entry, B, D, N):
    """style_fwd: a lane sums D / 64 pieces, each (p + p) + (p + p) of four products -- 3 roundings inside a piece, D / 64 adds of pieces --
    then 4 shuffle adds over the 16 k-lanes, w_mul, and b_mul * bias with its add: D / 64 + 10.  style_bwd_data: a wave adds its ceil(N / 4)
    rows, each a product and an add (ceil(N / 4) + 1 on the chain), two levels of adds across the waves, w_mul: ceil(N / 4) + 4.
    style_bwd_param: B products added in order, w_mul: B + 2 (db: B adds and b_mul)."""
    return D // 64 + 10 if entry == "sgx_style_fwd" else cdiv(N, 4) + 4 if entry == "sgx_style_bwd_data" else B + 2


# ---------------------------------------------------------------------------------------------------------------- references: minibatch stddev
Mbstd = namedtuple("Mbstd", "G M v mu d s dd ds stat dstat")


def mbstd_stats(x):
    """x fp64 [B][HW][C] -> the group statistics of include/sgx.h (group g, slot m: sample g M + m) and the error of their fp32 evaluation
    by mbstd_std, to first order plus the one second-order term that matters when the true variance is 0:
      mu   : G - 1 adds and the division, each relative to at most sum|v|        |dmu| <= u sum|v|        (G u sum|v| / G)
      d_g  : one subtraction of two values of which mu carries dmu               |dd|  <= dmu + u (max|v| + |mu|)
      var  : squares, G - 1 adds, / G, + 1e-8                                    |dvar| <= mean(2 |d| dd + dd^2) + (G + 2) u (var + 1e-8)
      s    : sqrt, concave: a generous 1 / s in place of 1 / (2 s)               |ds|  <= dvar / s + u s
    stat[m] is the mean of s over HW x C accumulated in fp64 and rounded to fp32 once: |dstat| <= mean(ds) + 2 u stat."""
    B = x.shape[0]
    G = min(B, 4)
    M = B // G
    v = x.reshape(G, M, *x.shape[1:])
    mu = v.mean(0)
    d = v - mu
    var = (d * d).mean(0)
    s = torch.sqrt(var + 1e-8)
    A = v.abs().sum(0)
    dd = U32 * (A + v.abs().amax(0) + A / G)
    dvar = (2 * d.abs() * dd + dd * dd).mean(0) + (G + 2) * U32 * (var + 1e-8)
    ds = dvar / s + U32 * s
    stat = s.mean((1, 2))
    return Mbstd(G, M, v, mu, d, s, dd, ds, stat, ds.mean((1, 2)) + 2 * U32 * stat)


def mbstd_bwd(dy, x, C):
    """dx = dy[..., :C] + k d / s, k[m] = sum_{g,hw} dy[g M + m][hw][C] / (C HW G) -> (dx, bound): the kernel forms k as (float)(sum / n) / G
    from an fp64 sum (2 roundings), then k * (v - mu) / s (2) and the add (1): 6 u (|dy| + kabs |d| / s) with one of slack, plus what the
    errors of d and s (mbstd_stats) do to the term: kabs (dd + |d| ds / s) / s."""
    st = mbstd_stats(x)
    n = x.shape[1] * x.shape[2]
    g = dy.reshape(st.G, st.M, *dy.shape[1:])
    k = (g[..., C].sum((0, 2)) / (n * st.G)).view(1, -1, 1, 1)
    kabs = (g[..., C].abs().sum((0, 2)) / (n * st.G)).view(1, -1, 1, 1)
    ref = g[..., :C] + k * st.d / st.s
    bound = kabs * (st.dd + st.d.abs() * st.ds / st.s) / st.s + 6 * U32 * (g[..., :C].abs() + kabs * st.d.abs() / st.s)
    return ref.reshape(x.shape), bound.reshape(x.shape)


def mbstd_bwd2(ggx, dy, x, C):
    """The second-order backward: with dot = sum_g d_g gg_g,
      dstat[m] = mean_{hw,c}(dot / s) / G                                         (the statistic column of ddy; its first C channels are ggx)
      gx_g     = k (u_g - mean_g u),  u_g = gg_g / s - dot d_g / (G s^3)
    -> (dstat, its bound, gx, its bound).  Errors, term by term, from the kernel's arithmetic:
      dot      : |ddot| <= sum_g dd |gg_g| + (G + 1) u dotabs,   dotabs = sum_g |d_g| |gg_g|
      dot / s  : ddot / s + dotabs / s (ds / s + u); dstat accumulates it in fp64, then (float), / G: 3 u more
      u_g      : |gg_g| / s (ds / s + u) + (ddot |d_g| + dotabs dd + dotabs |d_g| (3 ds / s + 5 u)) / (G s^3)      (product, G s s s, /, -)
      mean_g u : mean_g du + G u mean_g uabs;   u_g - mean: + u (uabs_g + mean uabs);   k: 2 roundings, the product 1: 3 u."""
    st = mbstd_stats(x)
    G, n = st.G, x.shape[1] * x.shape[2]
    gg = ggx.reshape(G, st.M, *x.shape[1:])
    g = dy.reshape(G, st.M, *dy.shape[1:])
    k = (g[..., C].sum((0, 2)) / (n * G)).view(1, -1, 1, 1)
    kabs = (g[..., C].abs().sum((0, 2)) / (n * G)).view(1, -1, 1, 1)
    d, s, dd, ds = st.d, st.s, st.dd, st.ds
    dot, dotabs = (d * gg).sum(0), (d.abs() * gg.abs()).sum(0)
    ddot = (dd * gg.abs()).sum(0) + (G + 1) * U32 * dotabs
    e = ddot / s + dotabs / s * (ds / s + U32)
    dstat = (dot / s).mean((1, 2)) / G
    dstat_b = e.mean((1, 2)) / G + 3 * U32 * (dotabs / s).mean((1, 2)) / G
    u = gg / s - dot * d / (G * s ** 3)
    uabs = gg.abs() / s + dotabs * d.abs() / (G * s ** 3)
    du = gg.abs() / s * (ds / s + U32) + (ddot * d.abs() + dotabs * dd + dotabs * d.abs() * (3 * ds / s + 5 * U32)) / (G * s ** 3)
    dum = du.mean(0) + G * U32 * uabs.mean(0)
    gx = k * (u - u.mean(0))
    gx_b = kabs * (du + dum + U32 * (uabs + uabs.mean(0))) + 3 * U32 * kabs * (uabs + uabs.mean(0))
    return dstat, dstat_b, gx.reshape(x.shape), gx_b.reshape(x.shape)


def with_store(ref, bound, dtype):
    """The bound after the store: half a bf16 ulp of the value for bf16 (r = 2^-8), one fp32 rounding otherwise."""
    return bound + ref.abs() * (SR.R_BF16 if dtype == H else U32)


def check_padded(y, src, col, colref, colbound, B, C, what):
    """The padded layout mbstd_fwd and mbstd_bwd2 write: channels < C are a copy of src (bit for bit), channel C holds one value per slot --
    identical bits at every position and in all G images of the slot, within colbound of colref[m] -- and the channels beyond it are +0."""
    G = min(B, 4)
    M = B // G
    iv = lambda t: t.view(torch.int16 if t.dtype == H else torch.int32)
    assert torch.equal(iv(y[..., :C].contiguous()), iv(src.contiguous())), f"{what}: the first C channels are no copy of the input"
    pad = iv(y[..., C + 1:].contiguous())
    assert bool((pad == 0).all()), f"{what}: {int((pad != 0).sum())} padding elements are not +0, first at {tuple(int(i) for i in (pad != 0).nonzero()[0])}"
    colv = y[..., C].reshape(G, M, -1)
    first = colv[0, :, 0]
    assert torch.equal(iv(colv.contiguous()), iv(first.view(1, M, 1).expand_as(colv).contiguous())), f"{what}: the statistic column is not one value per slot"
    return ER.assert_within(first, colref, with_store(colref, colbound, y.dtype), what + " statistic")


# ---------------------------------------------------------------------------------------------------------------- references: logistic head
def _softplus(x):
    return torch.nn.functional.softplus(x, beta=1.0, threshold=1e9)


def logistic(fake, real, scale, gen):
    """-> (loss, bound, g_fake, bound, g_real, bound) in fp64.  softplus as log1pf(expf(x)) (the identity above 20): the argument of log1p
    carries expf's ULP_EXP ulps, which the logarithm turns into e / (1 + e) of that relative to e <= softplus; its own ULP_LOG1P ulps
    follow.  A lane adds ceil(n / 64) terms, wave_sum 6 more, then / n, the sum of the two means and scale: ceil(n / 64) + 9 roundings on
    sum softplus.  sigmoid = 1 / (1 + expf(-x)): ULP_EXP ulps on e / (1 + e) <= 1 of the value, the add and the division; sgn scale (.) / n:
    3 more.  TINY32 is what a result below the normal range may lose (expf(-100) = 3.7e-44)."""
    sgn = -1.0 if gen else 1.0
    fx = ULP32 * (ULP_EXP + ULP_LOG1P)
    xf = sgn * fake
    nf, nr = fake.numel(), (0 if real is None else real.numel())
    sf = _softplus(xf)
    loss = sf.mean()
    lb = (fx + (cdiv(nf, 64) + 9) * U32) * sf.mean() + TINY32
    gf = sgn * scale * torch.sigmoid(xf) / nf
    gfb = gf.abs() * (ULP_EXP * ULP32 + 6 * U32) + TINY32
    gr = grb = None
    if nr:
        sr = _softplus(-real)
        loss = loss + sr.mean()
        lb = lb + (fx + (cdiv(nr, 64) + 9) * U32) * sr.mean() + U32 * loss.abs()
        gr = -scale * torch.sigmoid(-real) / nr
        grb = gr.abs() * (ULP_EXP * ULP32 + 6 * U32) + TINY32
    return (scale * loss).reshape(1), (abs(scale) * lb).reshape(1), gf, gfb, gr, grb


SPECIAL_LOGITS = [20.0, float(np.nextafter(np.float32(20), np.float32(21))), float(np.nextafter(np.float32(20), np.float32(19))), 100.0, -100.0,
                  0.0, -20.0, 88.0, -88.0]


# ---------------------------------------------------------------------------------------------------------------- operands
def gemm_operands(c):
    """CPU fp32 operands of a GEMM-family row.  Integer rows: |v| <= 3 (9 * 8200 < 2^24: every partial sum exact), alpha, w_mul, b_mul powers of
    two, an integer bias, a mask that is positive everywhere."""
    a = c.args
    it = a["data"] == "int"
    op = (lambda shape, seed: ints(shape, seed)) if it else (lambda shape, seed: rnd(shape, seed))
    if c.entry == "sgx_gemm_f32":
        M, N, K = a["M"], a["N"], a["K"]
        return dict(A=op((K, M) if a["ta"] else (M, K), 11), B=op((N, K) if a["tb"] else (K, N), 12), alpha=f32(0.5 if it else 0.37))
    B, N, K = a["B"], a["N"], a["K"]
    o = dict(w_mul=f32(0.25 if it else 0.37), b_mul=f32(2.0 if it else 1.3))
    if c.entry == "sgx_linear_fwd":
        o.update(x=op((B, K), 21), w=op((N, K), 22), bias=op((N,), 23) if a["bias"] else None)
    else:
        o.update(gy=op((B, N), 24), y_act=(ints((B, N), 25, 1, 3) if it else rnd((B, N), 25)) if a["mask"] else None)
        if c.entry == "sgx_linear_bwd_data":
            o.update(w=op((N, K), 22))
        else:
            o.update(x=op((B, K), 21))
    return o


def style_operands(c):
    a = c.args
    it = a["data"] == "int"
    op = ints if it else rnd
    B, D, Ns, L = a["B"], a["D"], a["Ns"], a["L"]
    G = len(Ns)
    return dict(lm=op((L, B, D), 31), Ws=[op((n, D), 40 + g) for g, n in enumerate(Ns)],
                biases=[op((n,), 140 + g) for g, n in enumerate(Ns)] if a["bias"] else [None] * G,
                gys=[op((B, n), 240 + g) for g, n in enumerate(Ns)],
                w_muls=[f32(0.5 if it else 0.37 + 0.01 * (g % 7)) for g in range(G)], b_muls=[f32(2.0 if it else 1.3) for g in range(G)])


def mbstd_operands(c):
    a = c.args
    B, HW, C, Cpad = a["B"], a["HW"], a["C"], a["Cpad"]
    if a["data"] == "const":                                 # one value per (slot, position, channel), quarters: the true variance is 0
        G = min(B, 4)
        x = ((rnd((1, B // G, HW, C), 51, 4.0)).round() / 4.0).expand(G, B // G, HW, C).reshape(B, HW, C).contiguous()
    else:
        x = rnd((B, HW, C), 51) + torch.tensor([0.0, 0.5, -1.5, 3.0])[torch.arange(C) % 4]
    return dict(x=x.to(c.dtype), dy=rnd((B, HW, Cpad), 52).to(c.dtype), ggx=rnd((B, HW, C), 53).to(c.dtype))


def logistic_operands(c):
    a = c.args
    if a.get("special"):
        fake = torch.tensor(SPECIAL_LOGITS, dtype=torch.float32)
        real = None if a["nr"] == 0 else -torch.tensor(SPECIAL_LOGITS[:a["nr"]], dtype=torch.float32)
        return dict(fake=fake, real=real)
    return dict(fake=rnd((a["nf"],), 61, 3.0), real=rnd((a["nr"],), 62, 3.0) if a["nr"] else None)


# ---------------------------------------------------------------------------------------------------------------- the case table
# id, entry point, dtype, args (what the runner of that entry in tests/test_gpu_small_paths.py reads), the kernels the profiler must report in
# order, and the launcher rule or kernel branch the row is there for.
CASES = []


def _case(id, entry, dtype, kernels, why, **args):
    CASES.append(Case(id, entry, dtype, args, tuple(kernels), why))


_KERN = {"O": (OUTER,), "1": (K1,), "8": (K8,), "1R": (K1, REDUCE), "8R": (K8, REDUCE)}

# ---- sgx_gemm_f32: M, N, K, ta, tb, data, kernels, workspace, shifted operands, why
for _M, _N, _K, _ta, _tb, _data, _k, _ws, _sh, _why in [
    (5, 20, 1, 0, 0, "int", "O", "full", "", "K = 1, tb = 0, N % 4 == 0, aligned: the outer-product kernel with three clamped k"),
    (16, 20, 2, 0, 0, "int", "O", "full", "", "outer product, K = 2"),
    (33, 4, 3, 1, 0, "int", "O", "full", "", "outer product with ta = 1, one vector per row"),
    (17, 16, 4, 1, 0, "int", "O", "full", "", "outer product, K = 4: no clamped k"),
    (1, 16, 4, 0, 0, "rnd", "O", "full", "", "outer product, M = 1, a partial block"),
    (512, 8192, 4, 1, 0, "int", "O", "full", "", "the dense layer's batch-4 weight gradient: 4096 blocks of the outer-product kernel"),
    (5, 20, 4, 0, 0, "rnd", "1", "full", "B", "outer-product shape with B 4 bytes off: the tile kernel, the aligned (outer) call's bits"),
    (5, 30, 3, 1, 0, "int", "1", "full", "", "K <= 4 but N % 4 != 0: the tile kernel, nothing but a TAIL step"),
    (5, 16, 4, 0, 1, "int", "1", "full", "", "K <= 4 but tb: the tile kernel"),
    (17, 15, 7, 0, 0, "int", "1", "full", "", "K % 4 != 0, t00: body !VA !VB, TAIL"),
    (1, 30, 7, 0, 1, "int", "1", "full", "", "K % 4 != 0, t01: body !VA !VB, TAIL"),
    (33, 4, 7, 1, 0, "int", "1", "full", "", "K % 4 != 0, t10: body !VA !VB, TAIL"),
    (16, 20, 7, 1, 1, "int", "1", "full", "", "K % 4 != 0, t11: body !VA !VB, TAIL"),
    (17, 15, 16, 0, 0, "int", "1", "full", "", "K % 4 == 0, t00: body VA !VB, one full step in wave 0, three empty slices"),
    (5, 30, 16, 0, 1, "int", "1", "full", "", "K % 4 == 0, t01: body VA VB"),
    (33, 16, 16, 1, 0, "int", "1", "full", "", "K % 4 == 0, t10: body !VA !VB"),
    (16, 20, 16, 1, 1, "int", "1", "full", "", "K % 4 == 0, t11: body !VA VB"),
    (17, 20, 16, 0, 1, "rnd", "1", "full", "A", "A 4 bytes off: the scalar A body, the aligned call's bits"),
    (17, 20, 16, 0, 1, "rnd", "1", "full", "B", "B 4 bytes off (tb): the scalar B body, the aligned call's bits"),
    (33, 30, 8, 1, 0, "int", "1", "full", "", "K = 8: a TAIL step of two whole lane groups, two zeroed"),
    (5, 20, 15, 0, 1, "int", "1", "full", "", "K = 15: the TAIL step's last lane group holds one zeroed k"),
    (16, 15, 17, 1, 1, "int", "1", "full", "", "K = 17: wave 0 a full step, wave 1 a TAIL of one k, waves 2 and 3 empty"),
    (17, 30, 77, 0, 0, "int", "1", "full", "", "K = 77: slices of 32, 32, 13"),
    (17, 30, 77, 0, 0, "rnd", "1", "full", "", "the same on randn: the chain bound"),
    (33, 20, 100, 0, 1, "int", "1", "full", "", "K = 100, VA VB: vector steps, then a TAIL of 4 in wave 3 through the scalar loads"),
    (33, 20, 100, 0, 1, "rnd", "1", "full", "", "the same on randn"),
    (5, 4, 127, 1, 0, "int", "1", "full", "", "K = 127: last slice 31 = a full step and a TAIL of 15"),
    (16, 16, 128, 0, 0, "int", "1", "full", "", "K = 128: four slices of 32, no TAIL"),
    (17, 20, 511, 0, 1, "int", "1", "full", "", "K = 511: the last K of <1>; slices of 128 never enter an 8-step loop there"),
    (5, 30, 512, 0, 0, "int", "8", "full", "", "K = 512: the first K of <8>; each slice is one 8-step trip"),
    (5, 30, 512, 0, 0, "rnd", "8", "full", "", "the same on randn"),
    (33, 16, 520, 1, 1, "int", "8", "full", "", "K = 520: slices of 144 = an 8-step trip and a single step; the last 88 = single steps and a TAIL"),
    (1, 15, 1024, 0, 1, "int", "1R", "full", "", "K = 1024, one tile: 4 even splits of 256"),
    (16, 20, 1025, 0, 0, "int", "1R", "full", "", "K = 1025, 2 tiles: 4 splits of 272, the last owns 209"),
    (16, 20, 1025, 0, 0, "rnd", "1R", "full", "", "the same on randn"),
    (16, 20, 1025, 0, 0, "int", "8", "null", "", "NULL workspace at a K that would split: one split, K = 1025 in <8>"),
    (5, 16, 1030, 1, 0, "int", "1R", "full", "", "K = 1030, ta: 4 splits of 272"),
    (5, 16, 1030, 1, 0, "int", "8", "short", "", "workspace 4 bytes short: one split"),
    (16, 30, 4112, 0, 1, "int", "1R", "full", "", "K = 4112, 2 tiles: 16 splits of 272, the last owns 32"),
    (5, 15, 8200, 0, 0, "int", "1R", "full", "", "K = 8200, one tile: 32 splits of 272; split 31 starts beyond K and writes a zero partial, wave 3 of split 30 is empty"),
    (4, 512, 8192, 0, 1, "rnd", "8R", "full", "", "the dense layer forward at batch 4: 32 tiles, 16 splits of 512 in <8>"),
    (4, 512, 8192, 0, 1, "int", "8R", "full", "", "the same on integers"),
    (4, 8192, 512, 0, 0, "rnd", "8", "full", "", "the dense layer's data gradient at batch 4: 512 tiles, unsplit"),
    (1, 4096, 1024, 0, 1, "int", "8", "full", "", "K = 1024 at exactly 256 tiles: no split"),
]:
    _case(f"gemm-{_M}x{_N}x{_K}-t{_ta}{_tb}-{_data}" + (f"-ws{_ws}" if _ws != "full" else "") + (f"-shift{_sh}" if _sh else ""), "sgx_gemm_f32", F, _KERN[_k], _why,
          M=_M, N=_N, K=_K, ta=_ta, tb=_tb, data=_data, ws=_ws, shift=_sh)

# ---- sgx_linear_fwd: gemm(B, N, K) t01 with bias / activation in the store
for _B, _N, _K, _act, _bias, _data, _k, _why in [
    (1, 6, 10, 0, True, "int", "1", "K % 4 != 0: scalar bodies, bias without activation"),
    (3, 36, 100, 1, True, "rnd", "1", "VA VB with bias and LeakyReLU"),
    (4, 512, 512, 1, True, "rnd", "8", "the mapping network's layer at batch 4: <8>"),
    (9, 6, 512, 0, False, "int", "8", "no bias, no activation: unfused through the linear entry point"),
    (15, 36, 10, 1, False, "rnd", "1", "activation without bias"),
    (17, 512, 100, 0, True, "int", "1", "two row tiles"),
    (32, 36, 512, 1, True, "int", "8", "LeakyReLU on integers: 0.2f * v is one rounding of an exact product"),
]:
    _case(f"linear_fwd-B{_B}-N{_N}-K{_K}-act{_act}-{'bias' if _bias else 'nobias'}-{_data}", "sgx_linear_fwd", F, _KERN[_k], _why, B=_B, N=_N, K=_K, act=_act, bias=_bias,
          data=_data, shift="")
_case("linear_fwd-B3-N36-K100-shiftx", "sgx_linear_fwd", F, (K1,), "x 4 bytes off: the scalar A body, the aligned call's bits", B=3, N=36, K=100, act=1, bias=True, data="rnd", shift="A")

# ---- sgx_linear_bwd_data: gemm(B, K, N) t00 with the mask on A
for _B, _N, _K, _mask, _data, _k, _why in [
    (1, 6, 10, True, "int", "1", "N % 4 != 0: body !VA MASK"),
    (3, 36, 100, True, "rnd", "1", "body VA MASK"),
    (4, 512, 512, True, "rnd", "8", "the mapping network's layer at batch 4"),
    (9, 6, 512, True, "rnd", "1", "body !VA MASK on randn: a rounding per masked operand"),
    (15, 36, 10, False, "int", "1", "y_act NULL: the plain GEMM"),
    (17, 512, 100, True, "int", "8", "two row tiles, K of the GEMM = N = 512"),
    (32, 6, 100, False, "rnd", "1", "y_act NULL, batch 32"),
    (4, 3, 100, False, "int", "O", "y_act NULL and N <= 4: the GEMM's K <= 4, an outer product"),
]:
    _case(f"linear_bwd_data-B{_B}-N{_N}-K{_K}-{'mask' if _mask else 'nomask'}-{_data}", "sgx_linear_bwd_data", F, _KERN[_k], _why, B=_B, N=_N, K=_K, mask=_mask, data=_data, shift="")
_case("linear_bwd_data-B3-N36-K100-shiftmask", "sgx_linear_bwd_data", F, (K1,), "y_act 4 bytes off: the scalar A body, the aligned call's bits", B=3, N=36, K=100, mask=True, data="rnd", shift="M")

# ---- sgx_linear_bwd_param: gemm(N, K, B) t10 with the mask on A and db as the column sum
for _B, _N, _K, _mask, _db, _data, _k, _why in [
    (1, 6, 10, True, True, "int", "1", "B = 1: colsum's remainder loop only"),
    (3, 36, 100, True, False, "rnd", "1", "B = 3, db NULL: no colsum"),
    (4, 512, 512, True, True, "rnd", "1", "the mapping network's layer at batch 4"),
    (9, 6, 512, True, True, "int", "1", "B = 9: colsum's 8-at-a-time loop and a remainder of 1"),
    (15, 36, 10, False, True, "rnd", "1", "B = 15: a remainder of 7, no mask"),
    (17, 512, 100, True, True, "int", "1", "B = 17: two 8-trips and a remainder of 1; 32 row tiles write db"),
    (32, 36, 512, True, True, "rnd", "1", "B = 32: colsum in four 8-trips, no remainder"),
    (4, 36, 100, False, False, "int", "O", "no mask, db NULL, B <= 4: an outer product"),
]:
    _case(f"linear_bwd_param-B{_B}-N{_N}-K{_K}-{'mask' if _mask else 'nomask'}-{'db' if _db else 'nodb'}-{_data}", "sgx_linear_bwd_param", F, _KERN[_k], _why, B=_B, N=_N, K=_K,
          mask=_mask, db=_db, data=_data, shift="")

# ---- the grouped style affines: one set of groups, the three entry points
for _tag, _B, _D, _Ns, _layers, _L, _bias, _db, _data, _why in [
    ("G65", 1, 64, [2] * 65, list(range(65)), 66, True, True, "int", "G = 65: style_group's walk; B = 1; N = 2: waves 2, 3 of bwd_data own no row; layer 65 untouched"),
    ("G6", 3, 128, [2, 15, 16, 17, 40, 70], [7, 0, 2, 3, 5, 6], 8, True, True, "rnd", "G = 6 by ballot, ragged and whole tiles, D = 128: the clamped k; full = 0 and 1; layers 1, 4 untouched"),
    ("G6i", 3, 128, [2, 15, 16, 17, 40, 70], [7, 0, 2, 3, 5, 6], 8, True, True, "int", "the same on integers"),
    ("B4", 4, 512, [260, 17], [0, 1], 2, False, False, "rnd", "MB = 4 with full = 4: the two-chunk pipeline; bias NULL, db NULL"),
    ("B5", 5, 64, [70], [0], 1, True, True, "int", "MB = 8 with B = 5, D = 64: one 16-byte piece per lane, the rest clamped"),
    ("B8", 8, 128, [260, 200, 2], [2, 0, 1], 3, True, True, "rnd", "MB = 8 full: full = 4 (even) and 3 (odd tail of the pipeline)"),
    ("B9", 9, 512, [40, 15], [1, 0], 3, True, False, "int", "MB = 16 with B = 9: one chunk at a time, full = 0; db NULL"),
    ("B16", 16, 64, [70, 260], [0, 1], 2, False, True, "rnd", "MB = 16 full; bias NULL"),
    ("B17", 17, 128, [16], [0], 1, True, True, "int", "MB = 32 with B = 17, a single whole tile"),
    ("B32", 32, 512, [1024, 17], [1, 0], 2, True, True, "rnd", "MB = 32 at max N = 1024: 128 KB of dynamic LDS, the batch-32 benchmark's launch"),
    ("B32i", 32, 512, [1024, 17], [1, 0], 2, True, True, "int", "the same on integers"),
]:
    for _e in ("fwd", "bwd_data", "bwd_param"):
        _case(f"style_{_e}-{_tag}", f"sgx_style_{_e}", F, (f"style_{_e}_kernel<{style_mb(_B)}>",), _why, B=_B, D=_D, Ns=_Ns, layers=_layers, L=_L, bias=_bias, db=_db, data=_data)

# ---- minibatch stddev: HW * C before, at, inside and after a trip of MBSTD_U * 1024 = 8192 elements
for _B, _HW, _C, _Cpad, _data, _why in [
    (1, 4, 24, 25, "rnd", "B = 1: G = 1, every variance 0, members 1 .. 3 clamped to image 0"),
    (2, 4, 72, 80, "rnd", "B = 2: G = 2, the second-order term cancels; Cpad - C = 8"),
    (3, 16, 40, 41, "rnd", "B = 3: G = 3, one clamped member"),
    (4, 16, 512, 520, "rnd", "the 1024^2 discriminator at batch 4: exactly one trip of 8192; Cpad - C = 8"),
    (8, 16, 24, 25, "rnd", "B = 8: M = 2 slots; the loops end inside the first trip"),
    (12, 9, 1000, 1008, "rnd", "B = 12: M = 3; 9000 elements: a trip and 808"),
    (4, 16, 2600, 2601, "rnd", "41600 elements: five trips and 640"),
    (4, 4, 24, 32, "const", "constant groups: the true variance is 0, s = sqrt(1e-8)"),
]:
    for _e in ("fwd", "bwd", "bwd2"):
        for _dt in (F, H):
            _case(f"mbstd_{_e}-{SR.tname(_dt).replace('bf16_t', 'bf16').replace('float', 'f32')}-B{_B}-HW{_HW}-C{_C}-pad{_Cpad - _C}-{_data}", f"sgx_mbstd_{_e}", _dt,
                  (f"mbstd_{_e}_kernel<{SR.tname(_dt)}>",), _why, B=_B, HW=_HW, C=_C, Cpad=_Cpad, data=_data)

# ---- the logistic loss head
for _nf, _nr in ((1, 3), (63, 64), (64, 65), (65, 1), (200, 63)):
    _case(f"logistic-d-nf{_nf}-nr{_nr}", "sgx_logistic_loss", F, ("logistic_loss_kernel",), "discriminator head: lanes with 0 .. 4 logits each, n_real != n_fake", nf=_nf, nr=_nr, gen=0)
_case("logistic-d-special", "sgx_logistic_loss", F, ("logistic_loss_kernel",), "logits at softplus' threshold 20 and its two fp32 neighbours, +-100, +-88: no NaN or Inf", nf=len(SPECIAL_LOGITS), nr=7, gen=0, special=True)
for _nf in (1, 65):
    _case(f"logistic-g-nf{_nf}", "sgx_logistic_loss", F, ("logistic_loss_kernel",), "generator head: n_real = 0, real and g_real NULL", nf=_nf, nr=0, gen=1)
_case("logistic-g-special", "sgx_logistic_loss", F, ("logistic_loss_kernel",), "generator head on the special logits", nf=len(SPECIAL_LOGITS), nr=0, gen=1, special=True)

assert len({c.id for c in CASES}) == len(CASES), "duplicate case id"
BY_ID = {c.id: c for c in CASES}

# Contract rejections: (id, entry, expected code, the words sgx_last_error must contain, why).  Each returns before any launch, so they run
# without a GPU (tests/test_small_coverage.py) on pointers that are never followed.
EINVAL, EUNSUPPORTED = -1, -2
REJECTIONS = [
    ("gemm-M0", "sgx_gemm_f32", EINVAL, "gemm: bad shape", "M = 0"),
    ("gemm-K-negative", "sgx_gemm_f32", EINVAL, "gemm: bad shape", "K < 0"),
    ("linear_fwd-N0", "sgx_linear_fwd", EINVAL, "gemm: bad shape", "N = 0 through the linear entry point"),
    ("linear_bwd_data-B0", "sgx_linear_bwd_data", EINVAL, "gemm: bad shape", "B = 0"),
    ("linear_bwd_param-K0", "sgx_linear_bwd_param", EINVAL, "gemm: bad shape", "K = 0"),
    ("mbstd_fwd-B6", "sgx_mbstd_fwd", EINVAL, "not divisible by group size", "B = 6: above 4 and no multiple of it"),
    ("mbstd_bwd-B6", "sgx_mbstd_bwd", EINVAL, "not divisible by group size", "B = 6"),
    ("mbstd_bwd2-B6", "sgx_mbstd_bwd2", EINVAL, "not divisible by group size", "B = 6"),
    ("mbstd_fwd-Cpad-eq-C", "sgx_mbstd_fwd", EINVAL, "Cpad must exceed C", "Cpad = C: no room for the statistic"),
    ("mbstd_bwd-Cpad-lt-C", "sgx_mbstd_bwd", EINVAL, "Cpad must exceed C", "Cpad < C"),
    ("mbstd_bwd2-Cpad-eq-C", "sgx_mbstd_bwd2", EINVAL, "Cpad must exceed C", "Cpad = C"),
    ("mbstd_fwd-dtype2", "sgx_mbstd_fwd", EINVAL, "mbstd_fwd: dtype 2", "dtype 2: neither SGX_F32 nor SGX_BF16"),
    ("mbstd_bwd-dtype2", "sgx_mbstd_bwd", EINVAL, "mbstd_bwd: dtype 2", "dtype 2"),
    ("mbstd_bwd2-dtype2", "sgx_mbstd_bwd2", EINVAL, "mbstd_bwd2: dtype 2", "dtype 2"),
    ("style_fwd-B33", "sgx_style_fwd", EUNSUPPORTED, "style affines", "B above STYLE_MAXB = 32"),
    ("style_bwd_data-B33", "sgx_style_bwd_data", EUNSUPPORTED, "style affines", "B = 33"),
    ("style_bwd_param-B33", "sgx_style_bwd_param", EUNSUPPORTED, "style affines", "B = 33"),
    ("style_fwd-D96", "sgx_style_fwd", EUNSUPPORTED, "style affines", "D % 64 != 0"),
    ("style_bwd_data-D96", "sgx_style_bwd_data", EUNSUPPORTED, "style affines", "D = 96"),
    ("style_bwd_param-D96", "sgx_style_bwd_param", EUNSUPPORTED, "style affines", "D = 96"),
    ("style_fwd-lm-misaligned", "sgx_style_fwd", EINVAL, "16-byte aligned", "lm 4 bytes off: style_fwd_kernel stages it with 16-byte loads"),
    ("logistic-fake-null", "sgx_logistic_loss", EINVAL, "logistic_loss", "fake NULL"),
    ("logistic-nf0", "sgx_logistic_loss", EINVAL, "logistic_loss", "n_fake = 0"),
    ("logistic-g-with-real", "sgx_logistic_loss", EINVAL, "not part of the generator loss", "generator head with n_real = 1"),
    ("logistic-d-real-null", "sgx_logistic_loss", EINVAL, "are required", "discriminator head with real NULL"),
    ("logistic-d-g_real-null", "sgx_logistic_loss", EINVAL, "are required", "discriminator head with g_real NULL"),
    ("logistic-d-nr0", "sgx_logistic_loss", EINVAL, "are required", "discriminator head with n_real = 0"),
]

# Rows per entry point: dropping one has to be a decision made here too (tests/test_small_coverage.py).
ROWS = {"sgx_gemm_f32": 44, "sgx_linear_fwd": 8, "sgx_linear_bwd_data": 9, "sgx_linear_bwd_param": 8, "sgx_style_fwd": 11, "sgx_style_bwd_data": 11, "sgx_style_bwd_param": 11,
        "sgx_mbstd_fwd": 16, "sgx_mbstd_bwd": 16, "sgx_mbstd_bwd2": 16, "sgx_logistic_loss": 9}
# The kernels of small.hip this table answers for (the R1 head and PixelNorm belong to streaming_ref.SMALL_HIP_COVERED)
KERNELS = ("mbstd_fwd_kernel", "mbstd_bwd_kernel", "mbstd_bwd2_kernel", "gemm_outer_kernel", "gemm_f32_kernel", "gemm_splitk_reduce", "style_fwd_kernel", "style_bwd_data_kernel",
           "style_bwd_param_kernel", "logistic_loss_kernel")
