"""-m gpu: models that are not RGB (num_channels 1, 2, 4) on the kernels of csrc/imgconv.hip.

1. the kernels at the C ABI: every element against the fp64 restatement of tests/imgconv_ref.py (streaming_ref.assert_elementwise, guard
   bands), the launched kernel asserted by name through the library's profiler, both sides of the launchers' size threshold;
2. the autograd Functions against CPU fp64 autograd on conv2d, first order and the R1-shaped second order;
3. the networks against the reference's run (tests/golden/channels.npz) and the fp64 oracle: forward, gradients, one full step;
4. bf16 activations against the 3-channel network of the same size; 5. StyleGAN.train from a yaml with dataset.channels: 1."""
import math
import random

import numpy as np
import pytest
import torch

import channels_util as CU
import golden_util as gu
import imgconv_ref as IR
import streaming_ref as SR
from gpu_util import DEV, assert_close, load_into, pin_noise, rel_err
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
IMG1_MIN = 65536                    # csrc/imgconv.hip: launches of at least this many y vectors (img_in) / pixels (img_out) run as short-lived blocks
TIGHT = 2e-5                        # tests/test_gpu_kernels.py: the fp32 bar of the Rgb functions' values and data gradients (1e-4: parameter gradients)


def _native():
    from stylegan.pytorch_amd import native
    return native


def rnd(shape, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, device=DEV, dtype=torch.float32).to(dtype)


def p(t):
    return None if t is None else t.data_ptr()


def d(t):
    return None if t is None else t.double()


def launch(what, call, kernels):
    """One C ABI call under the library's profiler: it succeeds and launches exactly ``kernels``, in order, each with the grid, block and
    dynamic LDS size of tests/golden/streaming_launch.json (``what`` is the row id)."""
    N = _native()
    N.prof_start(1)
    try:
        rc = call()
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    N.check(rc, what)
    ran = [SR.kernel_id(r[0]) for r in N.prof_records()]
    assert ran == list(kernels), f"{what}: launched {ran}, expected {list(kernels)}"
    SR.check_geometry(what, ran, N.prof_launches())


def check(g, ref, S, n, what):
    SR.assert_elementwise(g.t, ref.reshape(g.t.shape), S.reshape(g.t.shape), n, g.t.dtype, what)
    g.assert_intact(what)


def in_shapes(dtype):
    """(npix, C): a tail smaller than one block; several blocks; the widest weight table; one launch on each side of the threshold."""
    cv = 16 // IR.ve(dtype)
    return [(3 * 6 * 6, 16), (2 * 64 * 64, 32), (2 * 8 * 8, 512), (IMG1_MIN // cv - 1, 16), (IMG1_MIN // cv, 16)]


# ---------------------------------------------------------------------------------------------------------------- 1. kernel rows
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("J", [1, 2, 4, 8])
def test_img_in_rows(J, dtype):
    N = _native(); L = N.lib()
    t, dtc = SR.tname(dtype), 0 if dtype == F32 else 1
    seen = set()
    for npix, C in in_shapes(dtype):
        short = npix * (C // IR.ve(dtype)) >= IMG1_MIN
        kern = f"img_in{'1' if short else ''}_kernel<{t}, {J}>"
        seen.add(short)
        img = rnd((npix, J), F32, 17)
        for kind in ("in", "out"):
            sj, sc = IR.layout(kind, J, C)
            w, wscale = rnd((J * C,), F32, 16), SR.f32(0.37)
            for bias in (rnd((C,), F32, 18), None):
                what = f"img_in J{J} {t} {npix}x{C} {kind} bias={bias is not None}"
                out = SR.Guarded((npix, C), dtype, DEV)
                launch(what, lambda: L.sgx_img_in(p(img), p(w), J, sj, sc, wscale, p(bias), p(out.t), npix, C, dtc, N.stream()), [kern])
                ref, S, n = IR.img_in(img.double(), w.double(), J, sj, sc, wscale, d(bias), C)
                check(out, ref, S, n, what)
    assert seen == {False, True}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("J", [1, 2, 4])
def test_img_out_rows(J, dtype):
    N = _native(); L = N.lib()
    t, dtc = SR.tname(dtype), 0 if dtype == F32 else 1
    seen = set()
    for npix, C in [(3 * 6 * 6, 16), (2 * 64 * 64, 32), (2 * 8 * 8, 512), (IMG1_MIN - 1, 16), (IMG1_MIN, 16)]:
        short = npix >= IMG1_MIN and C // IR.ve(dtype) <= 16
        kern = f"img_out{'1' if short else ''}_kernel<{t}, {J}>"
        seen.add(short)
        x = rnd((npix, C), dtype, 22)
        for kind in ("in", "out"):
            sj, sc = IR.layout(kind, J, C)
            w, wscale = rnd((J * C,), F32, 21), SR.f32(0.37)
            for bias in (rnd((J,), F32, 23), None):
                what = f"img_out J{J} {t} {npix}x{C} {kind} bias={bias is not None}"
                out = SR.Guarded((npix, J), F32, DEV)
                launch(what, lambda: L.sgx_img_out(p(x), p(w), J, sj, sc, wscale, p(bias), p(out.t), npix, C, dtc, N.stream()), [kern])
                ref, S, n = IR.img_out(x.double(), w.double(), J, sj, sc, wscale, d(bias), C, dtype)
                check(out, ref, S, n, what)
    assert seen == {False, True}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("J", [1, 2, 4, 8])
def test_img_wgrad_rows(J, dtype):
    """(No size threshold in this launcher: one stage-1 kernel per J.)  Run twice: the same bits."""
    N = _native(); L = N.lib()
    t, dtc = SR.tname(dtype), 0 if dtype == F32 else 1
    for npix, C in [(3 * 6 * 6, 16), (2 * 64 * 64, 32), (2 * 8 * 8, 512), (70001, 16)]:      # (the last: more pixels than 64 per block x 1024 blocks)
        img, f = rnd((npix, J), F32, 24), rnd((npix, C), dtype, 25)
        wsb = L.sgx_img_wgrad_ws_bytes(npix, J, C)
        ws = N.workspace(wsb, DEV)
        for kind in ("in", "out"):
            sj, sc = IR.layout(kind, J, C)
            wscale = SR.f32(0.37)
            what = f"img_wgrad J{J} {t} {npix}x{C} {kind}"
            outs = []
            for _ in range(2):
                out = SR.Guarded((J * C,), F32, DEV)
                launch(what, lambda: L.sgx_img_wgrad(p(img), p(f), p(out.t), J, sj, sc, wscale, p(ws), wsb, npix, C, dtc, N.stream()),
                       [f"img_wgrad_stage1<{t}, {J}>", "img_wgrad_stage2"])
                outs.append(out)
            ref, S, n = IR.img_wgrad(img.double(), f.double(), J, sj, sc, wscale, C, dtype)
            check(outs[0], ref, S, n, what)
            assert torch.equal(outs[0].t.view(torch.int32), outs[1].t.view(torch.int32)), f"{what}: two runs differ"


@pytest.mark.parametrize("W", [6, 64])
@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("J", [1, 2, 4])
def test_images_from_uint8_channels(J, layout, W):
    """The criterion of tests/test_gpu_kernels.py::test_images_from_uint8: bit-exact in fp32 against the oracle's transform chain, bf16 = that
    result rounded to nearest even; flips by per-image decision; every byte value occurs."""
    from stylegan.pytorch_amd import functional as F
    B, H = 3, 16
    hwc = torch.randint(0, 256, (B, H, W, J), dtype=torch.uint8, generator=torch.Generator().manual_seed(B * H + W + J))
    hwc.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    flip = [bool(i % 2) for i in range(B)]
    src = (hwc if layout == "hwc" else hwc.permute(0, 3, 1, 2).contiguous()).to(DEV)
    ref, ref_fl = O.images_u8_to_float(hwc).to(DEV), O.images_u8_to_float(hwc, flip).to(DEV)
    N = _native()
    N.prof_start(1)
    try:
        out = F.images_from_uint8(src, layout=layout)
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    ran = [SR.kernel_id(r[0]) for r in N.prof_records()]
    assert ran == [f"images_u8_c_{'' if W % 4 == 0 else 'px_'}kernel<float, {J}, {'true' if layout == 'chw' else 'false'}>"], ran
    assert out.shape == (B, J, H, W) and out.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(out, ref)
    assert torch.equal(F.images_from_uint8(src, flip=flip, layout=layout), ref_fl)
    assert torch.equal(F.images_from_uint8(src, flip=flip, out_dtype=BF16, layout=layout), ref_fl.to(BF16))
    assert torch.equal(F.images_from_uint8(src, out_dtype=BF16, layout=layout), ref.to(BF16))
    with pytest.raises(N.SgxError):
        F.images_from_uint8(src)                                             # no layout inference outside 3 channels


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("chw", [0, 1])
def test_images_u8_three_channels_equal_the_rgb_entry_point(chw, dtype):
    N = _native(); L = N.lib()
    B, H, W = 3, 6, 64
    n = B * H * W * 3
    src = ((torch.arange(n, dtype=torch.int64) * 89 + 3) % 256).to(torch.uint8).view((B, 3, H, W) if chw else (B, H, W, 3)).to(DEV)
    dtc = 0 if dtype == F32 else 1
    for flip in (torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV), None):
        a, b = SR.Guarded((B, H, W, 3), dtype, DEV), SR.Guarded((B, H, W, 3), dtype, DEV)
        N.check(L.sgx_images_u8_to_nhwc(p(src), p(a.t), p(flip), B, H, W, chw, dtc, N.stream()), "sgx_images_u8_to_nhwc")
        N.check(L.sgx_images_u8_to_nhwc_c(p(src), p(b.t), p(flip), B, H, W, 3, chw, dtc, N.stream()), "sgx_images_u8_to_nhwc_c")
        torch.cuda.synchronize()
        assert torch.equal(a.t.view(torch.uint8), b.t.view(torch.uint8))
        a.assert_intact("rgb entry"); b.assert_intact("J = 3")


def test_unsupported_widths_launch_nothing():
    """C = 12 in bf16 (not whole 16-byte vectors), C = 6 in fp32, J = 3 (5 for the ingest): the host check refuses, nothing is launched."""
    from stylegan.pytorch_amd import functional as F
    N = _native(); L = N.lib()
    img, x = rnd((64, 4), F32, 1), rnd((64, 12), BF16, 2)
    w, y, o = rnd((4 * 12,), F32, 3), SR.Guarded((64, 12), BF16, DEV), SR.Guarded((64, 4), F32, DEV)
    ws = N.workspace(L.sgx_img_wgrad_ws_bytes(64, 4, 12), DEV)
    st = N.stream()
    N.prof_start(1)
    try:
        rcs = [L.sgx_img_in(p(img), p(w), 4, 1, 4, 1.0, None, p(y.t), 64, 12, 1, st),
               L.sgx_img_in(p(img), p(w), 4, 1, 4, 1.0, None, p(y.t), 64, 6, 0, st),
               L.sgx_img_in(p(img), p(w), 3, 1, 3, 1.0, None, p(y.t), 64, 16, 0, st),
               L.sgx_img_out(p(x), p(w), 4, 1, 4, 1.0, None, p(o.t), 64, 12, 1, st),
               L.sgx_img_out(p(x), p(w), 3, 1, 3, 1.0, None, p(o.t), 64, 16, 0, st),
               L.sgx_img_wgrad(p(img), p(x), p(o.t), 4, 1, 4, 1.0, p(ws), ws.numel(), 64, 12, 1, st),
               L.sgx_images_u8_to_nhwc_c(p(x), p(o.t), None, 1, 4, 4, 5, 0, 0, st)]
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    assert rcs == [-2] * 7, rcs
    assert N.prof_records() == []
    y.assert_intact("rejected img_in"); o.assert_intact("rejected img_out")
    with pytest.raises(N.SgxError):
        F.call(F.ImgInFn, img.view(1, 8, 8, 4), w.view(12, 4, 1, 1), None, 1.0, BF16)
    with pytest.raises(N.SgxError):
        F.call(F.ImgOutFn, x.view(1, 8, 8, 12), w.view(4, 12, 1, 1), None, 1.0, 4)


# ---------------------------------------------------------------------------------------------------------------- 2. autograd
@pytest.mark.parametrize("J", [1, 4])
def test_img_functions_first_and_second_order(J, monkeypatch):
    """ImgInFn (from_rgb) and ImgOutFn (to_rgb) through the 1x1 layers: values and image / weight / bias gradients against CPU fp64 autograd
    on conv2d, and the R1-shaped second order -- the gradient of |d(sum(from_rgb(img) r))/d img|^2 with respect to the weight.  Bars: those
    tests/test_gpu_kernels.py holds the Rgb functions to (rel-L2 2e-5 on values and data gradients, 1e-4 on parameter gradients)."""
    import torch.nn.functional as TF
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd.CustomLayers import EqualizedConv2d
    C = 16
    fr = EqualizedConv2d(J, C, 1, gain=math.sqrt(2), use_wscale=True).to(DEV)
    to = EqualizedConv2d(C, J, 1, gain=1, use_wscale=True).to(DEV)
    with torch.no_grad():
        fr.bias.copy_(0.1 * gu.seeded((C,), 30)); to.bias.copy_(0.1 * gu.seeded((J,), 31))
    calls = []
    for fn in (F.ImgInFn, F.ImgOutFn, F.ImgWgradFn):
        monkeypatch.setattr(fn, "forward", staticmethod(lambda ctx, *a, _o=fn.forward, _n=fn.__name__: (calls.append(_n), _o(ctx, *a))[1]))
    img = gu.seeded((2, J, 8, 8), 32)
    ig = img.to(DEV).requires_grad_(True)
    out = to(fr(ig))
    i64 = img.double().requires_grad_(True)
    p64 = [t.detach().double().cpu().requires_grad_(True) for t in (fr.weight, fr.bias, to.weight, to.bias)]
    ref = TF.conv2d(TF.conv2d(i64, p64[0] * fr.w_mul, p64[1]), p64[2] * to.w_mul, p64[3])
    assert out.shape == (2, J, 8, 8)
    assert_close(out, ref, TIGHT, "roundtrip")
    g = gu.seeded(ref.shape, 33)
    out.backward(g.to(DEV)); ref.backward(g.double())
    assert_close(ig.grad, i64.grad, TIGHT, "d img")
    for ours, r, name in zip((fr.weight, fr.bias, to.weight, to.bias), p64, ("from_rgb.weight", "from_rgb.bias", "to_rgb.weight", "to_rgb.bias")):
        assert_close(ours.grad, r.grad, 1e-4, name)
    assert {"ImgInFn", "ImgOutFn", "ImgWgradFn"} <= set(calls)
    # R1 shape: inner gradient under create_graph, then the penalty's gradient with respect to the weight
    fr.weight.grad = None
    r = gu.seeded((2, C, 8, 8), 34)
    ig2 = img.to(DEV).requires_grad_(True)
    with F.data_grad_only():
        (g1,) = torch.autograd.grad((fr(ig2) * r.to(DEV)).sum(), ig2, create_graph=True)
    pen = (g1 * g1).sum()
    pen.backward()
    w64 = fr.weight.detach().double().cpu().requires_grad_(True)
    j64 = img.double().requires_grad_(True)
    (g64,) = torch.autograd.grad((TF.conv2d(j64, w64 * fr.w_mul, p64[1].detach()) * r.double()).sum(), j64, create_graph=True)
    pen64 = (g64 * g64).sum()
    pen64.backward()
    assert_close(g1, g64, TIGHT, "d out / d img")
    assert_close(pen, pen64, TIGHT, "penalty")
    assert_close(fr.weight.grad, w64.grad, 1e-4, "R1 grad from_rgb.weight")


# ---------------------------------------------------------------------------------------------------------------- 3. networks
def build(cfg, nc, cond=False, act_dtype=F32):
    from stylegan.pytorch_amd.GAN import Discriminator, Generator
    extra = dict(conditional=True, n_classes=CU.NCLS) if cond else {}
    gen = Generator(resolution=CU.RES, num_channels=nc, latent_size=512, mapping_layers=CU.MAPPING, blur_filter=[1, 2, 1], truncation_psi=0.7,
                    truncation_cutoff=8, structure="linear", act_dtype=act_dtype, **cfg, **extra).to(DEV)
    dis = Discriminator(resolution=CU.RES, num_channels=nc, use_wscale=True, blur_filter=[1, 2, 1], structure="linear", act_dtype=act_dtype,
                        **cfg, **extra).to(DEV)
    return gen, dis


def hip_forward(gen, dis, nc, depth, alpha, cond):
    z = gu.seeded((CU.B, 512), 11)
    lab = CU.labels().to(DEV) if cond else None
    with torch.no_grad():
        gen.truncation.avg_latent.copy_(gu.fill_value("truncation.avg_latent", (512,)).to(DEV))
        img = gen(z.to(DEV), depth, alpha, labels_in=lab)
        score = dis(CU.real_for(nc, depth, F32).to(DEV), depth, alpha, labels_in=lab)
    return img, score


@pytest.fixture(scope="module")
def fx():
    return CU.fixture()


# configuration a (fmap_base 64) has 8 feature maps at 16x16, which the MFMA convolutions do not take (multiples of 16): on the GPU it is
# held to the fixture at depth 0; configuration b (16 everywhere) at depth 0 and at depth 2
@pytest.mark.parametrize("ck,nc,cond,depth,alpha", [("a", 1, False, 0, 1.0), ("a", 4, False, 0, 1.0), ("a", 1, True, 0, 1.0)]
                         + [("b", nc, cond, dp_, al) for nc, cond in ((1, False), (4, False), (1, True)) for dp_, al in CU.CASES])
def test_forward_vs_reference_and_oracle(fx, ck, nc, cond, depth, alpha):
    gp, dp = CU.params(CU.CONFIGS[ck], nc, cond)
    gen, dis = build(CU.CONFIGS[ck], nc, cond)
    load_into(gen, gp); load_into(dis, dp)
    gen.train(); dis.train(); gen.style_mixing_prob = None
    pin_noise(gen, CU.noises())
    img, score = hip_forward(gen, dis, nc, depth, alpha, cond)
    assert img.shape == (CU.B, nc, 4 * 2 ** depth, 4 * 2 ** depth)
    key = f"{ck}_{'cond' if cond else 'nc'}{nc}_"
    assert_close(img, torch.from_numpy(fx[f"{key}f64_g_d{depth}_img"]), 1e-3, "G image vs reference")
    assert_close(score, torch.from_numpy(fx[f"{key}f64_d_d{depth}_score"]), 1e-3, "D score vs reference")
    oi, osc = CU.oracle_forward(gp, dp, nc, depth, alpha, cond, torch.float64)
    assert_close(img, oi, 1e-3, "G image vs oracle")
    assert_close(score, osc, 1e-3, "D score vs oracle")


def make_stylegan(nc, act_dtype=F32):
    from stylegan.pytorch_amd.GAN import StyleGAN
    cfg = CU.CONFIGS["b"]
    kw = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
    return StyleGAN(structure="linear", resolution=CU.RES, num_channels=nc, latent_size=512,
                    g_args=dict(latent_size=512, mapping_layers=CU.MAPPING, blur_filter=[1, 2, 1], truncation_psi=0.7, truncation_cutoff=8, **cfg),
                    d_args=dict(use_wscale=True, blur_filter=[1, 2, 1], **cfg), g_opt_args=kw, d_opt_args=kw, loss="logistic", d_repeats=1,
                    use_ema=True, ema_decay=0.999, device=torch.device(DEV), act_dtype=act_dtype)


@pytest.mark.parametrize("nc", [1, 4])
def test_full_step_vs_oracle_and_reference(fx, nc):
    """One optimize_discriminator (logistic loss with R1) + optimize_generator at depth 2, alpha 0.5: losses against the reference's fp64
    run and the oracle; every parameter gradient against fp64 within max(1e-3 |g64|, 4 x the reference's own fp32 error, floor); the
    updated parameters; parameters of the inactive resolutions bit-unchanged."""
    key = f"b_step{nc}_"
    depth, alpha = 2, 0.5
    sg = make_stylegan(nc)
    gp, dp = CU.params(CU.CONFIGS["b"], nc)
    load_into(sg.gen, gp); load_into(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    noises = CU.noises()
    pin_noise(sg.gen, noises)
    before = {("d", k): v.detach().clone() for k, v in sg.dis.named_parameters()}
    before.update({("g", k): v.detach().clone() for k, v in sg.gen.named_parameters()})
    z = gu.seeded((CU.B, 512), 21); real = gu.seeded((CU.B, nc, CU.RES, CU.RES), 22)
    torch.manual_seed(77); random.seed(77)
    d_loss = sg.optimize_discriminator(z.to(DEV), real.to(DEV), depth, alpha)
    d_grads = {k: q.grad.detach().clone() for k, q in sg.dis.named_parameters() if q.grad is not None}
    torch.manual_seed(78); random.seed(78)
    g_loss = sg.optimize_generator(z.to(DEV), real.to(DEV), depth, alpha)
    g_grads = {k: q.grad.detach().clone() for k, q in sg.gen.named_parameters() if q.grad is not None}

    shadow = {k: v.detach().clone() for k, v in gp.items()}
    kw = dict(total_depth=CU.TOTAL_DEPTH, mapping_layers=CU.MAPPING, noises=noises)
    torch.manual_seed(77); random.seed(77)
    l2, cut = O.draw_mixing(z.shape, depth)
    od_loss, od_grads = O.d_step(gp, dp, O.AdamState(), z.double(), real.double(), depth, alpha, latents2=l2.double(), mixing_cutoff=cut, **kw)
    torch.manual_seed(78); random.seed(78)
    l2, cut = O.draw_mixing(z.shape, depth)
    og_loss, og_grads = O.g_step(gp, dp, O.AdamState(), z.double(), depth, alpha, latents2=l2.double(), mixing_cutoff=cut, shadow=shadow, **kw)

    print(f"[channels {nc}] d_loss {d_loss:.6f} (reference {float(fx[key + 'f64_d_loss']):.6f}, oracle {od_loss:.6f}), "
          f"g_loss {g_loss:.6f} (reference {float(fx[key + 'f64_g_loss']):.6f}, oracle {og_loss:.6f})")
    assert abs(d_loss - float(fx[key + "f64_d_loss"])) <= 1e-4 * abs(float(fx[key + "f64_d_loss"]))
    assert abs(g_loss - float(fx[key + "f64_g_loss"])) <= 1e-4 * abs(float(fx[key + "f64_g_loss"]))
    assert abs(d_loss - od_loss) <= 1e-4 * abs(od_loss) and abs(g_loss - og_loss) <= 1e-4 * abs(og_loss)

    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(v.double()) for v in g_grads.values()])).item()
    coef = min(1.0, 10.0 / (total + 1e-6))                       # oracle grads are post-clip, ours pre-clip
    for net, ours, ref, scale in (("d", d_grads, od_grads, 1.0), ("g", g_grads, og_grads, coef)):
        names = [str(n) for n in fx[f"{key}{net}_grad_names"]]
        assert sorted(ours) == names == sorted(k for k, v in ref.items() if v is not None)
        norm64 = dict(zip(names, fx[f"{key}{net}_grad_norm64"])); err32 = dict(zip(names, fx[f"{key}{net}_grad_err32"]))
        net_scale = max(norm64.values())
        for k in names:
            a = ours[k].double().cpu() * scale
            err = torch.linalg.vector_norm(a - ref[k]).item()
            tol = max(1e-3 * norm64[k], 4 * err32[k], 1e-7 * net_scale)
            assert err <= tol, f"{net} grad {k}: err {err:.3e} > tol {tol:.3e} (|g|={norm64[k]:.3e}, ref fp32 err {err32[k]:.3e})"
            if f"{key}{net}_grad64::{k}" in fx.files:              # direct check against the reference's fp64 gradient
                assert torch.linalg.vector_norm(a - torch.from_numpy(fx[f"{key}{net}_grad64::{k}"])).item() <= tol, k
    # parameters after the Adam steps (lr 0.003, beta1 0: each element moves ~lr * sign(g)) and the EMA shadow: the oracle's, and the reference's
    for name, net, mod, ref in (("dis", "d", sg.dis, dp), ("gen", "g", sg.gen, gp), ("shadow", "s", sg.gen_shadow, shadow)):
        for k, q in mod.named_parameters():
            if k.endswith("init_block.bias"):
                continue      # analytically-zero gradient (InstanceNorm removes it): Adam at beta1=0 turns round-off into +-lr
            for src, want in (("oracle", ref[k].detach()), ("reference", fx.get(f"{key}{net}_param64::{k}") if f"{key}{net}_param64::{k}" in fx.files else None)):
                if want is None:
                    continue
                want = torch.as_tensor(want).double()
                dd = (q.detach().double().cpu() - want).abs()
                frac_bad = float((dd > 1e-5 * (1 + want.abs())).double().mean())
                assert frac_bad <= max(2e-2, 2.0 / q.numel()), (name, src, k, frac_bad)         # sign flips of ~zero gradients only
    assert_close(sg.gen.truncation.avg_latent, gp["truncation.avg_latent"], 1e-5, "avg_latent")
    untouched = [("d", k) for k, q in sg.dis.named_parameters() if k not in d_grads] + [("g", k) for k, q in sg.gen.named_parameters() if k not in g_grads]
    assert ("d", f"from_rgb.{CU.TOTAL_DEPTH - 1}.weight") in untouched and ("g", "g_synthesis.to_rgb.0.weight") in untouched
    mods = {"d": dict(sg.dis.named_parameters()), "g": dict(sg.gen.named_parameters())}
    for net, k in untouched:
        assert torch.equal(mods[net][k].detach(), before[net, k]), f"{net}:{k} (inactive at depth {depth}) changed"


def test_conditional_gradients_vs_oracle(monkeypatch):
    """The conditional discriminator (num_channels=1: from_rgb over [image, label embedding], one ImgInFn call of J = 2): parameter gradients
    of score + R1-shaped penalty at depth 2 against fp64 autograd through the oracle, within max(1e-3 |g64|, floor)."""
    from stylegan.pytorch_amd import functional as F
    nc, depth, alpha = 1, 2, 0.5
    gp, dp = CU.params(CU.CONFIGS["b"], nc, True)
    _, dis = build(CU.CONFIGS["b"], nc, True)
    load_into(dis, dp); dis.train()
    real, lab = CU.real_for(nc, depth), CU.labels()
    calls = []
    orig = F.ImgInFn.forward
    monkeypatch.setattr(F.ImgInFn, "forward", staticmethod(lambda ctx, img, *a: (calls.append(int(img.shape[3])), orig(ctx, img, *a))[1]))
    rg = real.float().to(DEV).requires_grad_(True)
    score = dis(rg, depth, alpha, labels_in=lab.to(DEV))
    (g1,) = torch.autograd.grad(score.sum(), rg, create_graph=True)
    ((g1 * g1).sum() + score.sum()).backward()
    assert calls and set(calls) == {2}, calls                      # J = 2 * num_channels, never a loop of slices
    r64 = real.clone().requires_grad_(True)
    s64 = O.discriminator(dp, r64, depth, alpha, CU.TOTAL_DEPTH, labels=lab)
    (g64,) = torch.autograd.grad(s64.sum(), r64, create_graph=True)
    names = [k for k, v in dp.items() if v.requires_grad]
    grads = torch.autograd.grad((g64 * g64).sum() + s64.sum(), [dp[k] for k in names], allow_unused=True)
    ref = {k: v for k, v in zip(names, grads) if v is not None}
    ours = {k: q.grad for k, q in dis.named_parameters() if q.grad is not None}
    assert_close(score, s64, 1e-3, "conditional score")
    assert_close(g1, g64, 1e-3, "conditional d score / d img")
    assert sorted(ours) == sorted(ref)
    net_scale = max(float(torch.linalg.vector_norm(v)) for v in ref.values())
    for k, v in ref.items():
        n = float(torch.linalg.vector_norm(v))
        err = float(torch.linalg.vector_norm(ours[k].double().cpu() - v))
        assert err <= max(1e-3 * n, 1e-7 * net_scale), f"{k}: err {err:.3e}, |g| {n:.3e}"


@pytest.mark.parametrize("nc", [1, 4])
def test_fixed_structure_vs_oracle(nc):
    """structure='fixed' (no fade-in, every block, the last to_rgb / first from_rgb): equals the linear structure at full depth with
    alpha = 1 (tests/test_gpu_networks.py::test_fixed_structure_equals_linear_at_full_depth), which the oracle computes."""
    from stylegan.pytorch_amd.GAN import Discriminator, Generator
    cfg, depth = CU.CONFIGS["b"], CU.TOTAL_DEPTH - 1
    gp, dp = CU.params(cfg, nc)
    gen = Generator(resolution=CU.RES, num_channels=nc, latent_size=512, mapping_layers=CU.MAPPING, blur_filter=[1, 2, 1], truncation_psi=0.7,
                    truncation_cutoff=8, structure="fixed", **cfg).to(DEV)
    dis = Discriminator(resolution=CU.RES, num_channels=nc, use_wscale=True, blur_filter=[1, 2, 1], structure="fixed", **cfg).to(DEV)
    load_into(gen, gp); load_into(dis, dp)
    gen.train(); dis.train(); gen.style_mixing_prob = None
    pin_noise(gen, CU.noises())
    img, score = hip_forward(gen, dis, nc, depth, 1.0, False)
    oi, osc = CU.oracle_forward(gp, dp, nc, depth, 1.0, False, torch.float64)
    assert img.shape == (CU.B, nc, CU.RES, CU.RES)
    assert_close(img, oi, 1e-3, "fixed G image vs oracle")
    assert_close(score, osc, 1e-3, "fixed D score vs oracle")


@pytest.mark.parametrize("nc", [1, 4])
def test_graph_replay_equals_eager(nc):
    """The captured half-iterations (alpha in device memory: FadeFn on the image, the lerp of the newest discriminator block reading
    [alpha, 1 - alpha] itself) against eager launches over three iterations that change alpha, latents and images.  Loss agreement per
    iteration as tests/test_gpu_graphs.py holds the 3-channel model to (its LOSS_TOL: ulp-level first, then the documented amplification)."""
    from stylegan.pytorch_amd.GAN import StyleGAN
    tol = [2e-6, 5e-6, 1e-4]
    kw = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
    cfg = CU.CONFIGS["b"]
    runs = []
    for graphs in (False, True):
        sg = StyleGAN(structure="linear", resolution=CU.RES, num_channels=nc, latent_size=512,
                      g_args=dict(latent_size=512, mapping_layers=CU.MAPPING, blur_filter=[1, 2, 1], truncation_psi=0.7, truncation_cutoff=8, **cfg),
                      d_args=dict(use_wscale=True, blur_filter=[1, 2, 1], **cfg), g_opt_args=kw, d_opt_args=kw, loss="logistic", d_repeats=1,
                      use_ema=True, ema_decay=0.999, device=torch.device(DEV), use_graphs=graphs)
        gp, dp = CU.params(cfg, nc)
        load_into(sg.gen, gp); load_into(sg.dis, dp); load_into(sg.gen_shadow, gp)
        sg.gen.train(); sg.dis.train()
        pin_noise(sg.gen, CU.noises())
        torch.manual_seed(5); random.seed(5)
        losses = []
        for i in range(3):
            alpha = 0.25 + 0.15 * i
            z = gu.seeded((CU.B, 512), 100 + i).to(DEV); real = gu.seeded((CU.B, nc, CU.RES, CU.RES), 200 + i).to(DEV)
            losses.append((float(sg.optimize_discriminator(z, real, 2, alpha)), float(sg.optimize_generator(z, real, 2, alpha))))
        torch.cuda.synchronize()
        runs.append(losses)
    print(f"[channels {nc}] eager {runs[0]}, replay {runs[1]}")
    for i, ((d0, g0), (d1, g1)) in enumerate(zip(*runs)):
        assert math.isfinite(d0) and math.isfinite(g0)
        assert abs(d0 - d1) <= tol[i] * abs(d0) and abs(g0 - g1) <= tol[i] * abs(g0), (i, runs)


# ---------------------------------------------------------------------------------------------------------------- 4. bf16
def bf16_errors(nc):
    """(image rel-L2, D score rel-L2) of the bf16 network with ``nc`` image channels against its own fp64 oracle run: configuration b,
    depth 2, alpha 0.5, the pinned latents and noises, 32 real images."""
    depth, alpha = 2, 0.5
    gp, dp = CU.params(CU.CONFIGS["b"], nc)
    gen, dis = build(CU.CONFIGS["b"], nc, act_dtype=BF16)
    load_into(gen, gp); load_into(dis, dp)
    gen.train(); dis.train(); gen.style_mixing_prob = None
    pin_noise(gen, CU.noises())
    z = gu.seeded((CU.B, 512), 11)
    real = gu.seeded((32, nc, CU.RES, CU.RES), 65, torch.float64)
    with torch.no_grad():
        gen.truncation.avg_latent.copy_(gu.fill_value("truncation.avg_latent", (512,)).to(DEV))
        img = gen(z.to(DEV), depth, alpha)
        score = dis(real.float().to(DEV), depth, alpha)
        g2 = dict(gp); g2["truncation.avg_latent"] = gu.fill_value("truncation.avg_latent", (512,), torch.float64)
        ri, _ = O.generator(g2, z.double(), depth, alpha, CU.noises(), mapping_layers=CU.MAPPING, num_layers=2 * CU.TOTAL_DEPTH)
        rs = O.discriminator(dp, real, depth, alpha, CU.TOTAL_DEPTH)
    assert img.dtype == F32 and img.shape == ri.shape
    return rel_err(img, ri), rel_err(score, rs)


@pytest.fixture(scope="module")
def bf16_rgb():
    return bf16_errors(3)


@pytest.mark.parametrize("nc", [1, 4])
def test_bf16_tracks_the_rgb_network(bf16_rgb, nc):
    """The 3-channel network runs the parent's kernels: at most twice its error against fp64.  Then one bf16 step: finite parameters."""
    ei, es = bf16_errors(nc)
    print(f"[channels {nc} bf16] image rel {ei:.3e} (3 channels: {bf16_rgb[0]:.3e}), D score rel {es:.3e} (3 channels: {bf16_rgb[1]:.3e})")
    assert ei <= 2 * bf16_rgb[0], (ei, bf16_rgb[0])
    assert es <= 2 * bf16_rgb[1], (es, bf16_rgb[1])
    sg = make_stylegan(nc, BF16)
    gp, dp = CU.params(CU.CONFIGS["b"], nc)
    load_into(sg.gen, gp); load_into(sg.dis, dp); load_into(sg.gen_shadow, gp)
    pin_noise(sg.gen, CU.noises())
    z = gu.seeded((CU.B, 512), 21); real = gu.seeded((CU.B, nc, CU.RES, CU.RES), 22)
    torch.manual_seed(77); random.seed(77)
    d_loss = sg.optimize_discriminator(z.to(DEV), real.to(DEV), 2, 0.5)
    torch.manual_seed(78); random.seed(78)
    g_loss = sg.optimize_generator(z.to(DEV), real.to(DEV), 2, 0.5)
    assert math.isfinite(float(d_loss)) and math.isfinite(float(g_loss))
    for q in list(sg.gen.parameters()) + list(sg.dis.parameters()) + list(sg.gen_shadow.parameters()):
        assert torch.isfinite(q).all()


# ---------------------------------------------------------------------------------------------------------------- 5. StyleGAN.train
def test_yaml_grayscale_trains(tmp_path):
    """A config with dataset.channels: 1 trains through StyleGAN.train (the tiny schedule of test_gpu_diffaug.py::test_yaml_policy_trains)."""
    import logging
    from stylegan.pytorch_amd.GAN import StyleGAN
    from stylegan.pytorch_amd.config import default_cfg
    from stylegan.pytorch_amd.data import SyntheticImages
    y = tmp_path / "gray.yaml"
    y.write_text('structure: "linear"\ndataset:\n  resolution: 32\n  channels: 1\nmodel:\n  gen:\n    mapping_layers: 2\nsched:\n'
                 '  epochs: [1, 1, 1, 1]\n  batch_sizes: [4, 4, 4, 4]\n  fade_in_percentage: [50, 50, 50, 50]\n')
    opt = default_cfg()
    opt.merge_from_file(str(y))
    assert opt.dataset.channels == 1
    g_args = dict(opt.model.gen, fmap_base=256, fmap_max=32)
    d_args = dict(opt.model.dis, fmap_base=256, fmap_max=32)
    sg = StyleGAN(structure=opt.structure, conditional=opt.conditional, n_classes=opt.n_classes, resolution=opt.dataset.resolution,
                  num_channels=opt.dataset.channels, latent_size=opt.model.gen.latent_size, g_args=g_args, d_args=d_args,
                  g_opt_args=opt.model.g_optim, d_opt_args=opt.model.d_optim, loss=opt.loss, drift=opt.drift, d_repeats=opt.d_repeats,
                  use_ema=opt.use_ema, ema_decay=opt.ema_decay, device=torch.device(DEV))
    assert sg.gen.g_synthesis.to_rgb[0].weight.shape[0] == 1 and sg.dis.from_rgb[0].weight.shape[1] == 1
    losses = []
    log = logging.getLogger("gray"); log.setLevel(logging.INFO)

    class H(logging.Handler):
        def emit(self, r):
            m = r.getMessage()
            if m.startswith("Elapsed"):
                losses.append((float(m.split("D_Loss:")[1].split()[0]), float(m.split("G_Loss:")[1].split()[0])))
    h = H(); log.addHandler(h)
    try:
        sg.train(dataset=SyntheticImages(8, 32, channels=1), num_workers=0, epochs=opt.sched.epochs, batch_sizes=opt.sched.batch_sizes,
                 fade_in_percentage=opt.sched.fade_in_percentage, logger=log, output=str(tmp_path), num_samples=4, feedback_factor=2,
                 checkpoint_factor=100)
    finally:
        log.removeHandler(h)
    assert losses and all(math.isfinite(a) and math.isfinite(b) for a, b in losses), losses
    for q in list(sg.dis.parameters()) + list(sg.gen.parameters()):
        assert torch.isfinite(q).all()
