"""-m gpu: every launch path of the streaming kernels (csrc/pointwise.hip, the R1 head and PixelNorm of csrc/small.hip) at the C ABI.

Each row of streaming_ref.CASES is one call through native.lib(): the library's own profiler brackets it, the kernels that ran must be exactly
the row's, every output element must meet streaming_ref.assert_elementwise against an fp64 restatement of the op, and the sentinel bands
around every output must be untouched.  The bit-for-bit promises of include/sgx.h ride along as torch.equal on the raw bits."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import streaming_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


def _native():
    from stylegan.pytorch_amd import native
    return native


def rnd(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, device=DEV, dtype=torch.float32).to(dtype)


@functools.lru_cache(maxsize=3)
def big(n, seed):
    """The 2^29-element bf16 operands of the headline cases, drawn once and shared (read only)."""
    return rnd((n,), BF16, seed)


@pytest.fixture(scope="module", autouse=True)
def _release_big_operands():
    yield
    big.cache_clear()
    torch.cuda.empty_cache()


def operand(shape, dtype, seed):
    n = int(np.prod(shape, dtype=np.int64))
    if n >= 1 << 28 and dtype == BF16:
        return big(n, seed).view(tuple(shape))
    return rnd(shape, dtype, seed)


def shifted(t, shift):
    """A contiguous copy of t that starts ``shift`` bytes into its storage."""
    if not shift:
        return t
    buf = torch.empty(t.numel() * t.element_size() + 256, dtype=torch.uint8, device=t.device)
    v = buf[shift:shift + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == shift % 16 and v.is_contiguous()
    return v


def p(t):
    return None if t is None else t.data_ptr()


def d(t):
    return None if t is None else t.double()


def dev_scalars(*v):
    return torch.tensor(list(v), dtype=torch.float32, device=DEV)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def G(shape, dtype, shift=0):
    return SR.Guarded(shape, dtype, DEV, shift)


_FAULT = None


def launch(c, call, kernels=None):
    """Run one C ABI call under the library's profiler: it succeeds and launches exactly the expected kernels, in order, each with the grid,
    block and dynamic LDS size of tests/golden/streaming_launch.json."""
    global _FAULT
    N = _native()
    assert _FAULT is None, f"not run: the GPU reported an error in an earlier case ({_FAULT})"
    N.prof_start(1)
    try:
        rc = call()
        torch.cuda.synchronize()
    except RuntimeError as e:                               # a HIP error is sticky: nothing more is started on the device from this process
        _FAULT = f"{c.id}: {e}"
        raise
    finally:
        N.prof_start(0)
    N.check(rc, c.entry)
    ran = [SR.kernel_id(r[0]) for r in N.prof_records()]
    want = list(c.kernels if kernels is None else kernels)
    assert ran == want, f"{c.id}: launched {ran}, expected {want} ({c.why})"
    SR.check_geometry(c.id, ran, N.prof_launches())


def check(c, g, ref, S, nterms, what=""):
    r = SR.assert_elementwise(g.t, ref.reshape(g.t.shape), S.reshape(g.t.shape), nterms, g.t.dtype, f"{c.id}{what}")
    g.assert_intact(f"{c.id}{what}")
    return r


def dtc(c):
    return 0 if c.dtype == F32 else 1


def layout(a):
    """(sj, sc) of the parameter: from_rgb [C][3] is (1, 3), to_rgb [3][C] is (C, 1)."""
    return (1, 3) if a["layout"] == "in" else (a["C"], 1)


# ---------------------------------------------------------------------------------------------------------------- runners
def run_bias_act(L, N, c):
    a = c.args; npix, C = a["npix"], a["C"]
    x = operand((npix, C), c.dtype, 1)
    bias = rnd((C,), F32, 2) if a.get("bias", True) else None
    bscale = SR.f32(0.37)
    out = G((npix, C), c.dtype)
    launch(c, lambda: L.sgx_bias_act(p(x), p(bias), bscale, p(out.t), npix, C, a["act"], dtc(c), N.stream()))
    ref, S = SR.bias_act(x.double(), d(bias), bscale, a["act"])
    check(c, out, ref, S, 3)                                # bscale * bias, the sum, the slope


def run_lrelu_bwd(L, N, c):
    a = c.args; n = a["n"]; bits = c.entry.endswith("_bits")
    dy, y = operand((n,), c.dtype, 3), operand((n,), c.dtype, 4)
    mask = y > 0
    m = SR.pack_bits(mask.view(-1, 8)).flatten() if bits else y
    fn = L.sgx_lrelu_bwd_bits if bits else L.sgx_lrelu_bwd
    slope, scale = SR.f32(a["slope"]), SR.f32(a["scale"])
    sd = dev_scalars(scale) if a.get("dev") else None
    out = G((n,), c.dtype)
    launch(c, lambda: fn(p(dy), p(m), p(out.t), n, slope, 0.0 if sd is not None else scale, p(sd), dtc(c), N.stream()))
    ref, S = SR.lrelu_bwd(dy.double(), mask, slope, scale)
    check(c, out, ref, S, 2)                                # scale * dy, times the slope
    if sd is not None:
        host = G((n,), c.dtype)
        N.check(fn(p(dy), p(m), p(host.t), n, slope, scale, None, dtc(c), N.stream()), c.entry)
        assert bits_equal(out.t, host.t), f"{c.id}: scale_dev differs from the host-argument call"


def run_axpby(L, N, c):
    a = c.args; n = a["n"]; dev = c.entry.endswith("_dev")
    x = operand((n,), c.dtype, 5)
    b = operand((n,), c.dtype, 6) if a.get("b", True) else None
    alpha, beta = SR.f32(a["alpha"]), SR.f32(a["beta"])
    out = G((n,), c.dtype)
    host = lambda o: L.sgx_axpby(p(x), p(b), p(o.t), alpha, beta, n, dtc(c), N.stream())
    if dev:
        ad, bd = dev_scalars(alpha), (dev_scalars(beta) if b is not None else None)
        launch(c, lambda: L.sgx_axpby_dev(p(x), p(b), p(out.t), p(ad), p(bd), n, dtc(c), N.stream()))
    else:
        launch(c, lambda: host(out))
    ref, S = SR.axpby(x.double(), d(b), alpha, beta)
    check(c, out, ref, S, 2)                                # two products and a sum: a term passes 2 roundings (the library is built with -ffp-contract=off)
    if dev:
        h = G((n,), c.dtype)
        N.check(host(h), "sgx_axpby")
        assert bits_equal(out.t, h.t), f"{c.id}: device coefficients differ from the host-argument call"


def run_blur(L, N, c):
    a = c.args; B, H, W, C, mode = a["B"], a["H"], a["W"], a["C"], a["mode"]
    bits = c.entry == "sgx_blur3x3_bits"
    x = operand((B, H, W, C), c.dtype, 7)
    z = operand((B, H, W, C), c.dtype, 8) if mode >= 2 else None
    out = G((B, H, W, C), c.dtype)
    if bits:
        mask = z > 0
        zb = SR.pack_bits(mask)
        launch(c, lambda: L.sgx_blur3x3_bits(p(x), p(zb), p(out.t), B, H, W, C, mode, dtc(c), N.stream()))
        ref, S = SR.blur3x3(x.double(), mask, mode)
    else:
        launch(c, lambda: L.sgx_blur3x3_act(p(x), p(z), p(out.t), B, H, W, C, mode, dtc(c), N.stream()))
        ref, S = SR.blur3x3(x.double(), d(z), mode)
    # one term per tap: a tap's value passes two sums of three (4 additions; the weights 2 and 1/16 are exact), 9 bounds it; + the slope
    check(c, out, ref, S, 9 + (1 if mode else 0))


def taps_for(K):
    return np.float32(np.sin(1.0 + 1.7 * np.arange(K * K)))          # non-symmetric, both signs


def call_blur_kxk(L, N, x, y, taps, K, pad, B, IH, IW, OH, OW, C, dtype):
    arr = (ctypes.c_float * (K * K))(*[float(t) for t in taps])
    return L.sgx_blur_kxk(p(x), p(y), ctypes.cast(arr, ctypes.c_void_p), K, pad, B, IH, IW, OH, OW, C, 0 if dtype == F32 else 1, N.stream())


def run_blur_kxk(L, N, c):
    a = c.args; K, pad, B, IH, IW, C = a["K"], a["pad"], a["B"], a["IH"], a["IW"], a["C"]
    OH, OW = IH + 2 * pad - K + 1 - a["dOH"], IW + 2 * pad - K + 1 - a["dOW"]
    taps = taps_for(K)
    x = rnd((B, IH, IW, C), c.dtype, 9)
    out = G((B, OH, OW, C), c.dtype)
    launch(c, lambda: call_blur_kxk(L, N, x, out.t, taps, K, pad, B, IH, IW, OH, OW, C, c.dtype))
    ref, S = SR.blur_kxk(x.double(), taps, K, pad, OH, OW)
    check(c, out, ref, S, K * K)                            # a chain of K * K sums (each product rounds once more, relative to its own term: inside the + 2)


def run_pool2(L, N, c):
    a = c.args; B, H, W, C, sh = a["B"], a["H"], a["W"], a["C"], a.get("shift", 0)
    scale = SR.f32(a["scale"])
    x0 = operand((B, H, W, C), c.dtype, 10)
    x = shifted(x0, sh)
    out = G((B, H // 2, W // 2, C), c.dtype, sh)
    launch(c, lambda: L.sgx_pool2(p(x), p(out.t), B, H, W, C, scale, dtc(c), N.stream()))
    ref, S = SR.pool2(x.double(), scale)
    check(c, out, ref, S, 4)                                # three additions and the scale
    xf = x0.float()                                         # every variant sums (a + b) + (c + d) and rounds once: the bits of the same sum in fp32
    want = (scale * ((xf[:, 0::2, 0::2] + xf[:, 0::2, 1::2]) + (xf[:, 1::2, 0::2] + xf[:, 1::2, 1::2]))).to(c.dtype)
    assert bits_equal(out.t, want), f"{c.id}: summation order"
    if sh:
        al = G((B, H // 2, W // 2, C), c.dtype)
        N.check(L.sgx_pool2(p(x0), p(al.t), B, H, W, C, scale, dtc(c), N.stream()), c.entry)
        assert bits_equal(out.t, al.t), f"{c.id}: differs from the aligned call"


def run_up2(L, N, c):
    a = c.args; B, H, W, C, sh = a["B"], a["H"], a["W"], a["C"], a.get("shift", 0)
    scale = SR.f32(a["scale"])
    x0 = operand((B, H, W, C), c.dtype, 11)
    x = shifted(x0, sh)
    out = G((B, 2 * H, 2 * W, C), c.dtype, sh)
    launch(c, lambda: L.sgx_up2(p(x), p(out.t), B, H, W, C, scale, dtc(c), N.stream()))
    ref, S = SR.up2(x.double(), scale)
    check(c, out, ref, S, 1)
    want = SR.nearest_up2(x0 if scale == 1.0 else (scale * x0.float()).to(c.dtype))     # a copy (one product, one rounding, with a scale)
    assert bits_equal(out.t, want), f"{c.id}: up-sampling is a copy"
    if sh:
        al = G((B, 2 * H, 2 * W, C), c.dtype)
        N.check(L.sgx_up2(p(x0), p(al.t), B, H, W, C, scale, dtc(c), N.stream()), c.entry)
        assert bits_equal(out.t, al.t), f"{c.id}: differs from the aligned call"


def run_up2_add(L, N, c):
    a = c.args; B, H, W, C, sh = a["B"], a["H"], a["W"], a["C"], a.get("shift", 0)
    scale = SR.f32(a["scale"])
    x = operand((B, H, W, C), c.dtype, 12)
    add = shifted(operand((B, 2 * H, 2 * W, C), c.dtype, 13), sh)
    out = G((B, 2 * H, 2 * W, C), c.dtype, sh)
    launch(c, lambda: L.sgx_up2_add(p(x), p(add), p(out.t), B, H, W, C, scale, dtc(c), N.stream()))
    ref, S = SR.up2_add(x.double(), add.double(), scale)
    check(c, out, ref, S, 2)                                # the product and the sum


def run_downsample_fade(L, N, c):
    a = c.args; B, H, W = a["B"], a["H"], a["W"]
    alpha, beta = SR.f32(a["alpha"]), SR.f32(a["beta"])
    x = rnd((B, H, W, 3), F32, 14)
    ab = dev_scalars(alpha, beta) if a.get("dev") else None
    out = G((B, H, W, 3), F32)
    launch(c, lambda: L.sgx_downsample_fade_rgb(p(x), p(out.t), B, H, W, 0.0 if ab is not None else alpha, 0.0 if ab is not None else beta, p(ab), N.stream()))
    ref, S = SR.downsample_fade_rgb(x.double(), alpha, beta)
    check(c, out, ref, S, 6)                                # three additions (x 0.25 exact), beta, alpha, the sum
    if ab is not None:
        h = G((B, H, W, 3), F32)
        N.check(L.sgx_downsample_fade_rgb(p(x), p(h.t), B, H, W, alpha, beta, None, N.stream()), c.entry)
        assert bits_equal(out.t, h.t), f"{c.id}: ab_dev differs from the host-argument call"


def run_images_u8(L, N, c):
    a = c.args; B, H, W, chw = a["B"], a["H"], a["W"], a["chw"]
    n = B * H * W * 3
    src = ((torch.arange(n, dtype=torch.int64) * 89 + 3) % 256).to(torch.uint8).view((B, 3, H, W) if chw else (B, H, W, 3)).to(DEV)
    assert src.unique().numel() == 256
    flip = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    out = G((B, H, W, 3), c.dtype)
    launch(c, lambda: L.sgx_images_u8_to_nhwc(p(src), p(out.t), p(flip), B, H, W, chw, dtc(c), N.stream()))
    ref, S = SR.images_u8(src, flip, chw)
    check(c, out, ref, S, 2)                                # the division and the subtraction (x 2 exact)
    nf = G((B, H, W, 3), c.dtype)
    N.check(L.sgx_images_u8_to_nhwc(p(src), p(nf.t), None, B, H, W, chw, dtc(c), N.stream()), c.entry)
    ref, S = SR.images_u8(src, None, chw)
    check(c, nf, ref, S, 2, " (flip NULL)")


def run_colsum(L, N, c):
    a = c.args; npix, C = a["npix"], a["C"]
    scale = SR.f32(0.37)
    x = operand((npix, C), c.dtype, 15)
    wsb = L.sgx_colsum_ws_bytes(npix, C)
    ws = N.workspace(wsb, DEV)
    out = G((C,), F32)
    launch(c, lambda: L.sgx_colsum(p(x), p(out.t), scale, p(ws), wsb, npix, C, dtc(c), N.stream()))
    ref, S = SR.colsum(x.double(), scale)
    check(c, out, ref, S, SR.colsum_chain(npix, C, c.dtype, c.kernels[0].startswith("colsum_stage1")))


def rgb_params(a, seed):
    C = a["C"]
    sj, sc = layout(a)
    return rnd((3 * C,), F32, seed), sj, sc, SR.f32(0.37)


def run_rgb_in(L, N, c):
    a = c.args; npix, C = a["npix"], a["C"]; with_add = c.entry == "sgx_rgb_in_add"
    w, sj, sc, wscale = rgb_params(a, 16)
    img = rnd((npix, 3), F32, 17)
    bias = rnd((C,), F32, 18) if (a.get("bias", True) and not with_add) else None
    add = operand((npix, C), c.dtype, 19) if with_add else None

    def call(im, ad, y, n):
        if with_add:
            return L.sgx_rgb_in_add(p(im), p(w), sj, sc, wscale, p(ad), p(y), n, C, dtc(c), N.stream())
        return L.sgx_rgb_in(p(im), p(w), sj, sc, wscale, p(bias), p(y), n, C, dtc(c), N.stream())
    out = G((npix, C), c.dtype)
    launch(c, lambda: call(img, add, out.t, npix))
    ref, S = SR.rgb_in(img.double(), w.double(), sj, sc, wscale, d(bias), C, d(add))
    check(c, out, ref, S, 5 + (1 if with_add else 0))       # wscale * w, the product, two sums, the bias (, the joined gradient)
    if a.get("slices"):                                     # rgb_in1_kernel == rgb_in_kernel bit for bit: the same pixels through a small launch
        for lo, hi in ((0, 1000), (npix - 999, npix)):
            y = G((hi - lo, C), c.dtype)
            launch(c, lambda: call(img[lo:hi], None, y.t, hi - lo), [f"rgb_in_kernel<{SR.tname(c.dtype)}>"])
            assert bits_equal(out.t[lo:hi], y.t), f"{c.id}: pixels [{lo}, {hi}) differ from the loop kernel"


def run_rgb_out(L, N, c):
    a = c.args; C = a["C"]; fade = c.entry == "sgx_rgb_out_fade"
    if fade:
        B, H, W = a["B"], a["H"], a["W"]; npix = B * H * W
        alpha, beta = SR.f32(a["alpha"]), SR.f32(a["beta"])
        low = rnd((B, H // 2, W // 2, 3), F32, 20)
    else:
        npix = a["npix"]
    w, sj, sc, wscale = rgb_params(a, 21)
    x = operand((npix, C), c.dtype, 22)
    bias = rnd((3,), F32, 23) if a.get("bias", True) else None
    out = G((npix, 3), F32)
    if fade:
        ab = dev_scalars(alpha, beta) if a.get("dev") else None
        host = lambda o: L.sgx_rgb_out_fade(p(x), p(w), sj, sc, wscale, p(bias), p(low), alpha, beta, None, p(o.t), B, H, W, C, dtc(c), N.stream())
        if ab is not None:
            launch(c, lambda: L.sgx_rgb_out_fade(p(x), p(w), sj, sc, wscale, p(bias), p(low), 0.0, 0.0, p(ab), p(out.t), B, H, W, C, dtc(c), N.stream()))
        else:
            launch(c, lambda: host(out))
        ref, S = SR.rgb_out(x.double(), w.double(), sj, sc, wscale, d(bias), C, low.double(), alpha, beta, (B, H, W))
    else:
        call = lambda xs, o, n: L.sgx_rgb_out(p(xs), p(w), sj, sc, wscale, p(bias), p(o), n, C, dtc(c), N.stream())
        launch(c, lambda: call(x, out.t, npix))
        ref, S = SR.rgb_out(x.double(), w.double(), sj, sc, wscale, d(bias), C)
    ve = 4 if c.dtype == F32 else 8
    cv = C // ve; lpp = min(cv, 16)
    # (alpha wscale) w: 2; the product: 1; a lane's chain of VE * ceil(cv / lpp) sums, log2(lpp) exchange steps, the bias and the low image: + 2
    check(c, out, ref, S, 3 + ve * math.ceil(cv / lpp) + int(math.log2(lpp)) + 2)
    if fade and a.get("dev"):
        h = G((npix, 3), F32)
        N.check(host(h), c.entry)
        assert bits_equal(out.t, h.t), f"{c.id}: ab_dev differs from the host-argument call"
    if a.get("slices"):                                     # rgb_out1_kernel == rgb_out_kernel bit for bit
        for lo, hi in ((0, 1000), (npix - 999, npix)):
            y = G((hi - lo, 3), F32)
            launch(c, lambda: call(x[lo:hi], y.t, hi - lo), [f"rgb_out_kernel<{SR.tname(c.dtype)}>"])
            assert bits_equal(out.t[lo:hi], y.t), f"{c.id}: pixels [{lo}, {hi}) differ from the loop kernel"


def run_rgb_wgrad(L, N, c):
    a = c.args; npix, C = a["npix"], a["C"]
    sj, sc = layout(a)
    wscale = SR.f32(0.37)
    img = rnd((npix, 3), F32, 24)
    f = operand((npix, C), c.dtype, 25)
    wsb = L.sgx_rgb_wgrad_ws_bytes(npix, C)
    ws = N.workspace(wsb, DEV)
    out = G((3 * C,), F32)
    launch(c, lambda: L.sgx_rgb_wgrad(p(img), p(f), p(out.t), sj, sc, wscale, p(ws), wsb, npix, C, dtc(c), N.stream()))
    ref, S = SR.rgb_wgrad(img.double(), f.double(), sj, sc, wscale, C)
    check(c, out, ref, S, 1 + SR.colsum_chain(npix, C, c.dtype, c.kernels[0].startswith("rgb_wgrad_stage1")))     # the product, then the fp32 chain


def run_fade_rgb_bwd2(L, N, c):
    a = c.args; npix, C = a["npix"], a["C"]
    alpha, ws = SR.f32(a["alpha"]), SR.f32(0.37)
    ggy, ggp = rnd((npix, C), BF16, 26), rnd((npix, 3), F32, 27)
    mask = rnd((npix, C), F32, 28) > 0
    bits = SR.pack_bits(mask)
    wr = rnd((C, 3), F32, 29)
    out = G((npix, C), BF16)
    launch(c, lambda: L.sgx_fade_rgb_bwd2(p(ggy), p(ggp), p(bits), p(wr), ws, alpha, 1.0, None, p(out.t), npix, C, 1, N.stream()))
    t1, s1 = SR.lrelu_bwd(ggy.double(), mask, SR.LRELU, alpha)
    t2 = ggp.double() @ (ws * wr.double()).t()
    ref, S = SR.fade_rgb_bwd2(ggy.double(), ggp.double(), mask, wr.double(), ws, alpha, None)
    # sgx.h keeps the roundings of the three passes: t1 and t2 are each rounded to bf16 before the sum is (r |t1| + r |t2|, on top of the one
    # final rounding assert_elementwise grants); expressed in units of the criterion's fp32 term.  fp32 chain: ws * wr, product, two sums: 4.
    nterms = 4
    extra = (t1.abs() + t2.abs()) * (SR.R_BF16 * (1 + SR.R_BF16) / ((nterms + 2) * SR.U32))
    check(c, out, ref, S + extra, nterms)
    # ... and equals the three passes bit for bit
    y1, y2 = G((npix, C), BF16), G((npix, C), BF16)
    N.check(L.sgx_lrelu_bwd_bits(p(ggy), p(bits), p(y1.t), npix * C, SR.LRELU, alpha, None, 1, N.stream()), "sgx_lrelu_bwd_bits")
    N.check(L.sgx_rgb_in(p(ggp), p(wr), 1, 3, ws, None, p(y2.t), npix, C, 1, N.stream()), "sgx_rgb_in")
    assert bits_equal(out.t, y1.t + y2.t), f"{c.id}: differs from lrelu_bwd_bits + rgb_in + add"


def run_fade_rgb_bwd(L, N, c):
    a = c.args; npix, C = a["npix"], a["C"]
    alpha = SR.f32(a["alpha"]); beta = SR.f32(1.0 - alpha); ws, bs = SR.f32(0.37), SR.f32(0.01)
    g, pimg = rnd((npix, C), BF16, 30), rnd((npix, 3), F32, 31)
    mask = rnd((npix, C), F32, 32) > 0
    bits = SR.pack_bits(mask)
    wr = rnd((C, 3), F32, 33)
    wsb = L.sgx_fade_rgb_bwd_ws_bytes(npix, C)
    wsp = N.workspace(wsb, DEV)
    gy, dw, db, gp = G((npix, C), BF16), G((C, 3), F32), G((C,), F32), G((npix, 3), F32)
    st = N.stream()
    if a.get("split"):
        def call():
            rc = L.sgx_fade_rgb_bwd(p(g), p(bits), p(pimg), p(wr), ws, bs, alpha, beta, None, p(gy.t), None, None, 0, p(gp.t), p(wsp), wsb, npix, C, 1, st)
            return rc or L.sgx_fade_rgb_bwd_finish(p(wsp), wsb, npix, C, ws, bs, beta, None, p(dw.t), p(db.t), 0, st)
    else:
        call = lambda: L.sgx_fade_rgb_bwd(p(g), p(bits), p(pimg), p(wr), ws, bs, alpha, beta, None, p(gy.t), p(dw.t), p(db.t), 0, p(gp.t), p(wsp), wsb, npix, C, 1, st)
    launch(c, call)
    g64, p64, w64 = g.double(), pimg.double(), wr.double()
    ref, S = SR.lrelu_bwd(g64, mask, SR.LRELU, alpha)
    check(c, gy, ref, S, 2, " gy")
    # gpimg[p][j] = beta ws sum_c g[p][c] wr[c][j]: (beta ws) wr: 2, product 1, 8 sums per lane, log2(C / 8) exchange steps
    check(c, gp, g64 @ ((beta * ws) * w64), g64.abs() @ ((beta * ws) * w64.abs()), 3 + 8 + int(math.log2(C // 8)), " gpimg")
    # parameter gradients: fp32 partials flushed to fp64 every 64 pixels (+ the product), the rest fp64
    check(c, dw, (beta * ws) * (g64.t() @ p64), (beta * ws) * (g64.abs().t() @ p64.abs()), 65, " dwr")
    check(c, db, (beta * bs) * g64.sum(0), (beta * bs) * g64.abs().sum(0), 64, " drb")


def epi_operands(c):
    a = c.args; B, HW, C = a["B"], a["H"] * a["W"], a["C"]
    y = rnd((B, HW, C), c.dtype, 60)
    ebias = rnd((C,), F32, 61) if c.dtype == BF16 else None
    noise, nw, style = rnd((B, HW), F32, 62), rnd((C,), F32, 63), 0.5 * rnd((B, 2 * C), F32, 64)
    mean, rstd = 0.3 * rnd((B, C), F32, 65), rnd((B, C), F32, 66).abs() + 0.5
    x2, x2a = SR.epilogue_x2(y.double(), d(ebias), noise.double(), nw.double(), style.double(), mean.double(), rstd.double())
    return y, ebias, noise, nw, style, mean, rstd, x2, x2a


def run_rgb_out_epi(L, N, c):
    a = c.args; B, H, W, C = a["B"], a["H"], a["W"], a["C"]
    y, ebias, noise, nw, style, mean, rstd, x2, x2a = epi_operands(c)
    w, sj, sc, wscale = rgb_params(a, 67)
    rbias = rnd((3,), F32, 68)
    low = rnd((B, H // 2, W // 2, 3), F32, 69) if a["low"] else None
    alpha, beta = SR.f32(0.3), SR.f32(0.7)
    out = G((B * H * W, 3), F32)
    launch(c, lambda: L.sgx_rgb_out_epi(p(y), p(ebias), p(noise), p(nw), p(style), p(mean), p(rstd), p(w), sj, sc, wscale, p(rbias), p(low), alpha, beta, None,
                                        p(out.t), B, H, W, C, dtc(c), N.stream()))
    ref, S = SR.rgb_out_epi(x2, x2a, w.double(), sj, sc, wscale, rbias.double(), d(low), alpha, beta, (B, H, W))
    ve = 4 if c.dtype == F32 else 8
    cv = C // ve; lpp = min(cv, 16)
    # the kernel folds the epilogue into the weights: A = rstd (s0 + 1) (2), S = s1 - mean A (2), (alpha wscale) w A (3); the activation
    # t (4: two sums, nw noise, the slope); the product (1); the pixel's chain of VE ceil(cv / lpp) sums and log2(lpp) exchange steps; the
    # constant sum_c w S: a thread's ceil(C / 256) terms, then 256 partials summed in sequence, the bias and the low image (+ 2)
    check(c, out, ref, S, 7 + 4 + 1 + max(ve * math.ceil(cv / lpp) + int(math.log2(lpp)), math.ceil(C / 256) + 256) + 2)


def run_rgb_wgrad_epi(L, N, c):
    a = c.args; B, HW, C = a["B"], a["H"] * a["W"], a["C"]
    y, ebias, noise, nw, style, mean, rstd, x2, x2a = epi_operands(c)
    sj, sc = layout(a)
    scale, bscale = SR.f32(0.37), SR.f32(0.3)
    g = rnd((B, HW, 3), F32, 70)
    wsb = L.sgx_rgb_wgrad_epi_ws_bytes(B, HW, C)
    ws = N.workspace(wsb, DEV)
    dw, db = G((3 * C,), F32), G((3,), F32)
    launch(c, lambda: L.sgx_rgb_wgrad_epi(p(y), p(g), p(ebias), p(noise), p(nw), p(style), p(mean), p(rstd), p(dw.t), p(db.t), sj, sc, scale, bscale, p(ws), wsb,
                                          B, HW, C, dtc(c), N.stream()))
    rw, Sw, rb, Sb = SR.rgb_wgrad_epi(x2, x2a, g.double(), sj, sc, scale, bscale)
    # fp32: A and S of the epilogue (4), the activation (4), the product (1), a lane's partial over ceil(per / rows) pixels of its block
    # (blocks = min(ceil(HW / 256), 1024 / B) per image, rows = 256 / (C / VE)); fp64 from there
    nblk = max(1, min((HW + 255) // 256, max(1, 1024 // B)))
    chain = math.ceil(math.ceil(HW / nblk) / (256 // (C // (4 if c.dtype == F32 else 8))))
    check(c, dw, rw, Sw, 9 + chain, " dw")
    check(c, db, rb, Sb, chain, " db")


def run_sumsq(L, N, c):
    n = c.args["n"]
    x = rnd((n,), F32, 34)
    wsb = L.sgx_sumsq_ws_bytes()
    ws = N.workspace(wsb, DEV)
    out = G((1,), F32)
    launch(c, lambda: L.sgx_sumsq_f32(p(x), n, p(ws), wsb, p(out.t), N.stream()))
    ref, S = SR.sumsq(x.double())
    # fp32 before the fp64 flush: the square (1), the sum of eight squares (3), then at most 6 partial sums left unflushed by the four-in-flight
    # loop (it flushes every 4th trip of 2), 3 trips of the single loop and 3 tail elements
    check(c, out, ref, S, 1 + 3 + 6 + 3 + 3)


def run_scale_dev(L, N, c):
    a = c.args; n = a["n"]
    alpha = SR.f32(a["alpha"])
    x = rnd((n,), F32, 35)
    s = dev_scalars(0.77)
    out = G((n,), F32)
    launch(c, lambda: L.sgx_scale_dev_f32(p(x), p(s), alpha, p(out.t), n, N.stream()))
    ref, S = SR.scale_dev(x.double(), float(s.double().item()), alpha)
    check(c, out, ref, S, 2)                                # alpha * s, times x


def pixelnorm_terms(C):
    """fp32 chain of r = rsqrt(mean(x^2) + eps): a lane's ceil(C / 64) multiply-adds, 6 exchange steps, the division and the sum with eps
    move the radicand by e_ss units; the square root halves that; rsqrtf is good to 1 ulp (2 units), taken as 2 ulps."""
    e_ss = math.ceil(C / 64) + 6 + 2
    return e_ss, math.ceil(e_ss / 2) + 4


def run_pixelnorm(L, N, c):
    a = c.args; B, C = a["B"], a["C"]
    x = rnd((B, C), F32, 36)
    out = G((B, C), F32)
    e_ss, e_r = pixelnorm_terms(C)
    if c.entry == "sgx_pixelnorm_fwd":
        launch(c, lambda: L.sgx_pixelnorm_fwd(p(x), p(out.t), B, C, N.stream()))
        ref, S = SR.pixelnorm_fwd(x.double())
        check(c, out, ref, S, e_r + 1)                      # r, times x
    else:
        dy = rnd((B, C), F32, 37)
        launch(c, lambda: L.sgx_pixelnorm_bwd(p(dy), p(x), p(out.t), B, C, N.stream()))
        ref, S = SR.pixelnorm_bwd(dy.double(), x.double())
        # k = r r r dot / C: three factors r, three products / the division, the dot product's chain (as e_ss less the two scalar steps + its
        # products); dx = dy r - x k: the larger of the two terms' chains + its product + the difference
        check(c, out, ref, S, 3 * e_r + 4 + e_ss + 2)


RUNNERS = {
    "sgx_bias_act": run_bias_act, "sgx_lrelu_bwd": run_lrelu_bwd, "sgx_lrelu_bwd_bits": run_lrelu_bwd, "sgx_axpby": run_axpby, "sgx_axpby_dev": run_axpby,
    "sgx_blur3x3_act": run_blur, "sgx_blur3x3_bits": run_blur, "sgx_blur_kxk": run_blur_kxk, "sgx_pool2": run_pool2, "sgx_up2": run_up2,
    "sgx_up2_add": run_up2_add, "sgx_downsample_fade_rgb": run_downsample_fade, "sgx_images_u8_to_nhwc": run_images_u8, "sgx_colsum": run_colsum,
    "sgx_rgb_in": run_rgb_in, "sgx_rgb_in_add": run_rgb_in, "sgx_rgb_out": run_rgb_out, "sgx_rgb_out_fade": run_rgb_out, "sgx_rgb_wgrad": run_rgb_wgrad,
    "sgx_rgb_out_epi": run_rgb_out_epi, "sgx_rgb_wgrad_epi": run_rgb_wgrad_epi, "sgx_fade_rgb_bwd2": run_fade_rgb_bwd2, "sgx_fade_rgb_bwd": run_fade_rgb_bwd, "sgx_sumsq_f32": run_sumsq, "sgx_scale_dev_f32": run_scale_dev,
    "sgx_pixelnorm_fwd": run_pixelnorm, "sgx_pixelnorm_bwd": run_pixelnorm,
}


@pytest.mark.parametrize("case", SR.CASES, ids=[c.id for c in SR.CASES])
def test_streaming_case(case):
    N = _native()
    RUNNERS[case.entry](N.lib(), N, case)


@pytest.mark.parametrize("K,pad,dt", [(2, 0, F32), (4, 1, F32), (5, 2, F32), (5, 4, F32), (7, 3, F32), (7, 1, F32)])
def test_blur_kxk_adjoint_identity(K, pad, dt):
    """include/sgx.h: the adjoint of sgx_blur_kxk is the same call with the taps flipped, pad' = K-1-pad and the sizes swapped.
    <A x, y> = <x, A^T y> in fp64 on fp32 runs; each side is an elementwise-bounded fp32 result, so the two inner products differ by at most
    (K K + 2) 2^-24 (<S_A, |y|> + <|x|, S_AT>) with S the references' absolute-value expressions."""
    N = _native(); L = N.lib()
    B, IH, IW, C = 2, 11, 9, 12
    OH, OW = IH + 2 * pad - K + 1, IW + 2 * pad - K + 1
    taps = taps_for(K)
    x, y = rnd((B, IH, IW, C), dt, 40), rnd((B, OH, OW, C), dt, 41)
    ax, aty = G((B, OH, OW, C), dt), G((B, IH, IW, C), dt)
    N.check(call_blur_kxk(L, N, x, ax.t, taps, K, pad, B, IH, IW, OH, OW, C, dt), "sgx_blur_kxk")
    N.check(call_blur_kxk(L, N, y, aty.t, taps[::-1].copy(), K, K - 1 - pad, B, OH, OW, IH, IW, C, dt), "sgx_blur_kxk")
    torch.cuda.synchronize()
    ax.assert_intact("A x"); aty.assert_intact("A^T y")
    _, s1 = SR.blur_kxk(x.double(), taps, K, pad, OH, OW)
    _, s2 = SR.blur_kxk(y.double(), taps[::-1].copy(), K, K - 1 - pad, IH, IW)
    lhs, rhs = (ax.t.double() * y.double()).sum().item(), (x.double() * aty.t.double()).sum().item()
    bound = (K * K + 2) * SR.U32 * ((s1 * y.double().abs()).sum().item() + (x.double().abs() * s2).sum().item())
    print(f"adjoint K={K} pad={pad}: <Ax,y>={lhs!r} <x,ATy>={rhs!r} bound={bound:.3e}")
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


@pytest.mark.parametrize("rej", SR.REJECTIONS, ids=[r[0] for r in SR.REJECTIONS])
def test_contract_rejections_launch_nothing(rej):
    """Arguments an SGX_REQUIRE refuses: the documented code comes back, sgx_last_error names the entry point, no kernel is launched."""
    N = _native(); L = N.lib()
    rid, entry, code, why = rej
    x = rnd((64, 48), F32, 50); xb = x.bfloat16(); img = rnd((64, 3), F32, 51)
    out = G((64 * 4104,), F32)
    ws = N.workspace(L.sgx_rgb_wgrad_ws_bytes(64, 48), DEV)
    st = N.stream()
    N.prof_start(1)
    try:
        if rid == "bias_act-bf16-C12":
            rc = L.sgx_bias_act(p(xb), None, 1.0, p(out.t), 64, 12, 1, 1, st)
        elif rid == "blur_kxk-K8":
            rc = call_blur_kxk(L, N, x, out.t, np.ones(64, np.float32), 8, 3, 1, 8, 8, 7, 7, 48, F32)
        elif rid == "colsum-short-workspace":
            rc = L.sgx_colsum(p(x), p(out.t), 1.0, p(ws), L.sgx_colsum_ws_bytes(64, 48) - 1, 64, 48, 0, st)
        elif rid == "rgb_wgrad-C48":
            rc = L.sgx_rgb_wgrad(p(img), p(x), p(out.t), 48, 1, 1.0, p(ws), L.sgx_rgb_wgrad_ws_bytes(64, 48), 64, 48, 0, st)
        elif rid.endswith("-dtype7"):                       # valid buffers and shapes (64 pixels x 48 channels, 8 x 8 images), dtype 7
            rc = {"sgx_bias_act": lambda: L.sgx_bias_act(p(x), None, 1.0, p(out.t), 64, 48, 1, 7, st),
                  "sgx_pool2": lambda: L.sgx_pool2(p(x), p(out.t), 1, 8, 8, 48, 1.0, 7, st),
                  "sgx_up2": lambda: L.sgx_up2(p(x), p(out.t), 1, 8, 8, 48, 1.0, 7, st),
                  "sgx_up2_add": lambda: L.sgx_up2_add(p(x[:16]), p(x), p(out.t), 1, 4, 4, 48, 1.0, 7, st),
                  "sgx_colsum": lambda: L.sgx_colsum(p(x), p(out.t), 1.0, p(ws), L.sgx_colsum_ws_bytes(64, 48), 64, 48, 7, st),
                  "sgx_rgb_in": lambda: L.sgx_rgb_in(p(img), p(x), 1, 3, 1.0, None, p(out.t), 64, 48, 7, st),
                  "sgx_rgb_out": lambda: L.sgx_rgb_out(p(x), p(x), 48, 1, 1.0, None, p(out.t), 64, 48, 7, st),
                  "sgx_lrelu_bwd_bits": lambda: L.sgx_lrelu_bwd_bits(p(xb), p(xb), p(out.t), 64 * 48, 0.2, 1.0, None, 7, st),
                  "sgx_img_in": lambda: L.sgx_img_in(p(x), p(x), 4, 1, 4, 1.0, None, p(out.t), 64, 48, 7, st)}[entry]()
        else:
            w = rnd((3 * 4104,), F32, 52); xw = rnd((4, 4104), F32, 53)
            rc = L.sgx_rgb_out(p(xw), p(w), 4104, 1, 1.0, None, p(out.t), 4, 4104, 0, st)
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    assert rc == code, f"{rid} ({why}): returned {rc}, documented {code}"
    assert N.prof_records() == [], f"{rid}: a kernel was launched"
    assert L.sgx_last_error(), rid
    L.sgx_clear_error()
    assert bool((out.buf == SR.SENTINEL).all()), f"{rid}: the output was written"
