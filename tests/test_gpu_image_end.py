"""-m gpu: the image end of the discriminator (csrc/rgbconv.hip and its callers).

Kernel tests: integer-valued inputs (the gradient gz and the image in [-3, 3], W0, Wr, br in [-2, 2], scales 1), so every bf16 pack
value, every product and every fp32 partial sum is an integer below 2^24 -- exact in ANY summation order -- and the kernels are
compared with plain fp64 torch by exact equality: there is no tolerance to choose.  Each reference's magnitude is asserted to stay
below 2^24 (and that of the intermediate dW', whose entries bound the partial sums of the chain rule).  Outputs live in
``streaming_ref.Guarded`` buffers: sentinel fill, guard bands intact.  tests/test_gpu_rgbconv_paths.py runs the same shapes and more (rows of
tests/rgbconv_ref.py, which restates these references at the C ABI's layouts and with non-unit scales; tests/test_rgbconv_coverage.py checks
the two restatements against each other): single ``acc`` bits, NULL outputs, wfinish's second trip, the tile loop, the workspace itself.

The D step: its final backward is asked for the parameters' gradients only (SGX_D_REAL_IMAGE_GRAD=0, the default), so the adjoint chain
down to the real batch is not launched; the parameter gradients are those of the plain backward (=1) bit for bit."""
import collections
import random

import pytest
import torch

import golden_util as gu
import streaming_ref as SR
from gpu_util import DEV, load_into, pin_noise
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

EXACT = float(2 ** 24)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from stylegan.pytorch_amd import native
    assert torch.cuda.is_available()
    native.lib()


def ints(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def int_params(C, seed=0):
    return {"w0": ints((C, C, 3, 3), 11 + seed, -2, 2), "b0": ints((C,), 12 + seed, -2, 2),
            "wr": ints((C, 3, 1, 1), 13 + seed, -2, 2), "br": ints((C,), 14 + seed, -2, 2)}


def composed(p):
    """W'[o][j][ky][kx] = sum_i W0[o][i][ky][kx] Wr[i][j] (scales 1): the 3 -> C 3x3 convolution from_rgb o conv0 is, bias channel aside."""
    return torch.einsum("oiyx,ij->ojyx", p["w0"], p["wr"][:, :, 0, 0])


def chain64(img, p, bias):
    """fp64: from_rgb (1x1) -> conv0 (3x3, zero padding of from_rgb's OUTPUT, so the bias br stops at the image border)."""
    f = torch.nn.functional.conv2d(img, p["wr"], p["br"] if bias else None)
    return torch.nn.functional.conv2d(f, p["w0"], p["b0"] if bias else None, padding=1)


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. image gradient
@pytest.fixture(scope="module")
def dgrad_refs():
    """(B, H, W, C) -> (gz NCHW fp64, parameters, fp64 image gradient NCHW): computed once, shared, never written."""
    out = {}
    for B, H, W, C in DGRAD_SHAPES:
        p = int_params(C)
        gz = ints((B, C, H, W), 32, -3, 3)
        img = torch.zeros((B, 3, H, W), dtype=torch.float64, requires_grad=True)
        (gi,) = torch.autograd.grad((chain64(img, p, False) * gz).sum(), img)
        assert composed(p).abs().max() <= 256 and gi.abs().max() < EXACT          # bf16-exact pack, fp32-exact sums
        out[(B, H, W, C)] = (gz, p, gi)
    return out


# the smallest shapes sgx_rgbconv_ok admits (H % 16 == 0, W % 64 == 0): one row block with every 14-column strip at a border of a
# 64-wide image; interior strips, several row blocks and a ragged last one; the 32-channel instantiation over odd and even strips
DGRAD_SHAPES = [(2, 16, 64, 16), (1, 48, 128, 16), (1, 32, 192, 32)]


@pytest.mark.parametrize("B,H,W,C", DGRAD_SHAPES)
def test_rgbconv_dgrad_is_the_fp64_adjoint_of_the_composed_convolution(B, H, W, C, dgrad_refs):
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    gz, p, want = dgrad_refs[(B, H, W, C)]
    assert L.sgx_rgbconv_ok(B, H, W, C, N.BF16)
    w0, wr = p["w0"].float().to(DEV), p["wr"].float().to(DEV)
    wf = torch.empty((3, C, 16), dtype=torch.bfloat16, device=DEV)
    wd = torch.empty((3, 16, C), dtype=torch.bfloat16, device=DEV)
    N.check(L.sgx_rgbconv_pack(N.ptr(w0), 1.0, N.ptr(wr), 1.0, None, 1.0, N.ptr(wf), N.ptr(wd), C, N.stream()), "sgx_rgbconv_pack")
    gzd = nhwc(gz, torch.bfloat16)
    out = SR.Guarded((B, H, W, 3), torch.float32, DEV)
    N.check(L.sgx_rgbconv_dgrad(N.ptr(gzd), N.ptr(wd), N.ptr(out.t), B, H, W, C, N.BF16, N.stream()), "sgx_rgbconv_dgrad")
    torch.cuda.synchronize()
    out.assert_intact(f"rgbconv_dgrad B{B} {H}x{W} C{C}")
    got = out.t.permute(0, 3, 1, 2).double().cpu()
    bad = (got != want).nonzero()
    assert torch.equal(got, want), f"{bad.shape[0]} elements differ, first at (b, j, y, x) = {bad[0].tolist()}"


# ---------------------------------------------------------------------------------------------------------------- 2. parameter gradients
WGRAD_SHAPES = [(2, 16, 64, 16), (1, 32, 128, 32)]
NAMES = ["w0", "b0", "wr", "br"]


@pytest.fixture(scope="module")
def wgrad_refs():
    out = {}
    for B, H, W, C in WGRAD_SHAPES:
        p = {k: v.requires_grad_(True) for k, v in int_params(C).items()}
        img, gz = ints((B, 3, H, W), 41, -3, 3), ints((B, C, H, W), 42, -3, 3)
        want = dict(zip(NAMES, torch.autograd.grad((chain64(img, p, True) * gz).sum(), [p[k] for k in NAMES])))
        # dW' (what the partial sums add up to, bias channel included): gradient of the plain 4 -> C convolution of (image, 1)
        wp = torch.zeros((C, 4, 3, 3), dtype=torch.float64, requires_grad=True)
        x4 = torch.cat([img, torch.ones_like(img[:, :1])], 1)
        (dwp,) = torch.autograd.grad((torch.nn.functional.conv2d(x4, wp, padding=1) * gz).sum(), wp)
        # every partial sum of the chain rule is a sum of at most 9 C (or 4) terms |dW'| * 2: bounded by the figures below
        assert dwp.abs().max() * 2 * 9 * C < EXACT and all(v.abs().max() < EXACT for v in want.values())
        out[(B, H, W, C)] = (img, gz, {k: v.detach() for k, v in p.items()}, want)
    return out


@pytest.mark.parametrize("acc", [0, 15])
@pytest.mark.parametrize("B,H,W,C", WGRAD_SHAPES)
def test_rgbconv_wgrad_gives_the_four_fp64_parameter_gradients(B, H, W, C, acc, wgrad_refs):
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    img, gz, p, want = wgrad_refs[(B, H, W, C)]
    d = {k: v.float().to(DEV) for k, v in p.items()}
    outs = {k: SR.Guarded(tuple(p[k].shape), torch.float32, DEV) for k in NAMES}
    pre = {k: ints(tuple(p[k].shape), 50 + i, -5, 5) for i, k in enumerate(NAMES)}
    if acc:
        for k in NAMES:
            outs[k].t.copy_(pre[k].float())
    wsb = L.sgx_rgbconv_wgrad_ws_bytes(B, H, W, C)
    ws = N.workspace(wsb, torch.device(DEV))
    imgd, gzd = nhwc(img, torch.float32), nhwc(gz, torch.bfloat16)
    N.check(L.sgx_rgbconv_wgrad(N.ptr(imgd), N.ptr(gzd), 1, N.ptr(d["w0"]), 1.0, N.ptr(d["wr"]), 1.0,
                                N.ptr(d["br"]), 1.0, N.ptr(outs["w0"].t), N.ptr(outs["b0"].t), N.ptr(outs["wr"].t), N.ptr(outs["br"].t), acc,
                                N.ptr(ws), wsb, B, H, W, C, N.BF16, N.stream()), "sgx_rgbconv_wgrad")
    torch.cuda.synchronize()
    for k in NAMES:
        outs[k].assert_intact(f"rgbconv_wgrad {k} B{B} {H}x{W} C{C} acc {acc}")
        ref = want[k] + pre[k] if acc else want[k]
        assert ref.abs().max() < EXACT
        got = outs[k].t.double().cpu()
        assert torch.equal(got, ref), (k, acc, int((got != ref).sum()), float((got - ref).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- 3. the D step
# FFHQ's settings (linear structure, logistic loss with R1, 8 mapping layers, no truncation) at resolution 64 with fmap_base 512: the
# widths 16, 32, 64, 128, 256 of the 1024-model's five newest blocks, so that the image end runs the composed kernels as it does there
R64 = dict(resolution=64, mapping_layers=8, fmap_base=512, fmap_max=512, total_depth=5)
IMAGE_ONLY = ("rgbconv_dgrad", "up2+add", "up2 ", "rgb_out")      # launches (by layer description) whose only output is an image gradient


def make_r64():
    from stylegan.pytorch_amd.GAN import StyleGAN
    opt = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
    c = R64
    sg = StyleGAN(structure="linear", resolution=c["resolution"], num_channels=3, latent_size=512,
                  g_args=dict(latent_size=512, mapping_layers=c["mapping_layers"], blur_filter=[1, 2, 1], truncation_psi=-1.0, truncation_cutoff=8,
                              fmap_base=c["fmap_base"], fmap_max=c["fmap_max"]),
                  d_args=dict(use_wscale=True, blur_filter=[1, 2, 1], fmap_base=c["fmap_base"], fmap_max=c["fmap_max"]),
                  g_opt_args=opt, d_opt_args=opt, loss="logistic", d_repeats=1, use_ema=True, ema_decay=0.999,
                  device=torch.device(DEV), act_dtype=torch.bfloat16, use_graphs=False)
    gp = O.make_generator_params(c["resolution"], c["mapping_layers"], 512, c["fmap_base"], c["fmap_max"], dtype=torch.float64)
    dp = O.make_discriminator_params(c["resolution"], c["fmap_base"], c["fmap_max"], dtype=torch.float64)
    for p in (gp, dp):
        for k in list(p):
            rg = p[k].requires_grad
            p[k] = gu.fill_value(k, p[k].shape, torch.float64).requires_grad_(rg)
    gp.pop("truncation.avg_latent", None)
    load_into(sg.gen, gp); load_into(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, [gu.seeded((4, 1, 4 * 2 ** (i // 2), 4 * 2 ** (i // 2)), 100 + i, torch.float64) for i in range(2 * c["total_depth"])])
    return sg


def test_d_step_backward_stops_above_the_real_batch(monkeypatch):
    from stylegan.pytorch_amd import native as N
    sg = make_r64()
    B, depth, alpha = 4, R64["total_depth"] - 1, 0.5
    z = gu.seeded((B, 512), 300).to(DEV); real = gu.seeded((B, 3, 64, 64), 301).to(DEV)
    zero_grads = sg._zero_grads

    def zero_grads_then_profile(kind, d):           # _d_grads zeroes the gradients between R1's first-order pass and the final backward
        zero_grads(kind, d)
        torch.cuda.synchronize()
        N.prof_start(1)
    monkeypatch.setattr(sg, "_zero_grads", zero_grads_then_profile)

    def step(switch):
        if switch is None:
            monkeypatch.delenv("SGX_D_REAL_IMAGE_GRAD", raising=False)
        else:
            monkeypatch.setenv("SGX_D_REAL_IMAGE_GRAD", switch)
        torch.manual_seed(7); random.seed(7)
        try:
            loss = sg._d_grads(z, real, depth, alpha)           # optimize_discriminator's loss and backward, without the update
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        launches = [(SR.kernel_id(r[0]), r[4]) for r in N.prof_records()]
        grads = {k: p.grad.detach().clone() for k, p in sg.dis.named_parameters() if p.grad is not None}
        return float(loss), grads, launches

    loss_old, g_old, l_old = step("1")
    loss_new, g_new, l_new = step(None)
    for name, launches in (("SGX_D_REAL_IMAGE_GRAD=1", l_old), ("default", l_new)):
        print(f"[{name}] {len(launches)} launches in the backward; image-only: {[d for _, d in launches if d.startswith(IMAGE_ONLY)]}")
    assert loss_old == loss_new
    assert sorted(g_old) == sorted(g_new) and len(g_new) > 0
    for k in g_old:
        assert torch.equal(g_old[k], g_new[k]), k

    def n_dgrad(launches):
        return sum(k.startswith("rgbconv_dgrad_kernel") for k, _ in launches)
    assert n_dgrad(l_old) >= 1 and n_dgrad(l_new) == n_dgrad(l_old) - 1
    assert not [(k, d) for k, d in l_new if d.startswith(IMAGE_ONLY)], "a launch whose only output is an image gradient"
    # nothing is launched that the plain backward does not launch, and what is left out is image gradients only
    c_old, c_new = collections.Counter(l_old), collections.Counter(l_new)
    assert not (c_new - c_old), c_new - c_old
    assert all(d.startswith(IMAGE_ONLY) for _, d in (c_old - c_new)), c_old - c_new
