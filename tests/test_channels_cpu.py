"""CPU: models that are not RGB (num_channels 1, 2, 4).  The oracle against the reference's own run (tests/golden/channels.npz), our
modules' state dicts against the reference's, the fp64 restatement of the image-side kernels (tests/imgconv_ref.py) against
torch.nn.functional.conv2d and CPU autograd to second order, and the surface around them (binding table, DiffAugment refusal, yaml)."""
import random

import numpy as np
import pytest
import torch

import channels_util as CU
import golden_util as gu
import imgconv_ref as IR
from oracle import stylegan_oracle as O

FORWARD = [(ck, nc, cond) for ck in ("a", "b") for nc, cond in ((1, False), (4, False), (1, True))]


def T(a, dtype):
    return torch.from_numpy(np.asarray(a)).to(dtype)


def close(a, b, rtol, atol):
    a = a.detach().double(); b = T(b, torch.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item(); ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"max err {err:.3e} vs ref max {ref:.3e}"


@pytest.fixture(scope="module")
def g():
    return CU.fixture()


# ------------------------------------------------------------------ the oracle against the reference (tolerances: tests/test_oracle_golden.py)
@pytest.mark.parametrize("dtype,tag,tol", [(torch.float32, "f32", 2e-5), (torch.float64, "f64", 2e-4)])
@pytest.mark.parametrize("ck,nc,cond", FORWARD)
def test_oracle_networks_against_the_reference(g, ck, nc, cond, dtype, tag, tol):
    """Generator image and discriminator score at depth 0 and depth 2 (alpha 0.5) against the reference's run of the same precision,
    and the fp32 oracle against the reference's fp64."""
    gp, dp = CU.params(CU.CONFIGS[ck], nc, cond, dtype)
    key = f"{ck}_{'cond' if cond else 'nc'}{nc}_"
    for depth, alpha in CU.CASES:
        img, score = CU.oracle_forward(gp, dp, nc, depth, alpha, cond, dtype)
        assert img.shape == (CU.B, nc, 4 * 2 ** depth, 4 * 2 ** depth)
        close(img, g[f"{key}{tag}_g_d{depth}_img"], tol, tol)
        close(score, g[f"{key}{tag}_d_d{depth}_score"], 10 * tol, 10 * tol)
        close(img, g[f"{key}f64_g_d{depth}_img"], 2e-4, 2e-4)
        close(score, g[f"{key}f64_d_d{depth}_score"], 2e-3, 2e-3)


@pytest.mark.parametrize("ck,nc,cond", FORWARD)
def test_state_dicts_equal_the_reference(g, ck, nc, cond):
    """Keys and shapes of our Generator / Discriminator, and of the oracle's parameter dicts, equal the reference's; the values the tests
    load are the reference run's (golden_util.fill_value of the name: checked through the recorded [sum, sum|.|, norm])."""
    from stylegan.pytorch_amd.GAN import Discriminator, Generator
    cfg = CU.CONFIGS[ck]
    extra = dict(conditional=True, n_classes=CU.NCLS) if cond else {}
    gen = Generator(resolution=CU.RES, num_channels=nc, mapping_layers=CU.MAPPING, blur_filter=[1, 2, 1], **cfg, **extra)
    dis = Discriminator(resolution=CU.RES, num_channels=nc, blur_filter=[1, 2, 1], **cfg, **extra)
    gp, dp = CU.params(cfg, nc, cond, torch.float32)
    key = f"{ck}_{'cond' if cond else 'nc'}{nc}_"
    for net, mod, p in (("g", gen, gp), ("d", dis, dp)):
        want = {str(n): tuple(int(v) for v in str(s).split(";")) for n, s in zip(g[f"{key}{net}_names"], g[f"{key}{net}_shapes"])}
        ours = {k: tuple(v.shape) for k, v in mod.state_dict().items() if not k.endswith(".kernel")}
        assert ours == want
        assert {k: tuple(v.shape) for k, v in p.items()} == want
        for n, st in zip(g[f"{key}{net}_names"], g[f"{key}{net}_stats"]):
            s = gu.tensor_stats(p[str(n)])
            assert abs(s[2] - st[2]) <= 1e-6 * st[2] + 1e-12 and abs(s[0] - st[0]) <= 1e-6 * st[1] + 1e-12, str(n)


def run_oracle_step(nc, dtype):
    gp, dp = CU.params(CU.CONFIGS["b"], nc, False, dtype)
    shadow = {k: v.detach().clone() for k, v in gp.items()}
    depth, alpha = 2, 0.5
    z = gu.seeded((CU.B, 512), 21, dtype); real = gu.seeded((CU.B, nc, CU.RES, CU.RES), 22, dtype)
    kw = dict(total_depth=CU.TOTAL_DEPTH, mapping_layers=CU.MAPPING, noises=CU.noises(dtype))
    d_opt, g_opt = O.AdamState(), O.AdamState()
    torch.manual_seed(77); random.seed(77)
    l2, cut = O.draw_mixing(z.shape, depth)
    d_loss, d_grads = O.d_step(gp, dp, d_opt, z, real, depth, alpha, latents2=l2.to(dtype), mixing_cutoff=cut, **kw)
    torch.manual_seed(78); random.seed(78)
    l2, cut = O.draw_mixing(z.shape, depth)
    g_loss, g_grads = O.g_step(gp, dp, g_opt, z, depth, alpha, latents2=l2.to(dtype), mixing_cutoff=cut, shadow=shadow, **kw)
    return d_loss, g_loss, d_grads, g_grads, gp, dp, shadow


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
@pytest.mark.parametrize("nc", [1, 4])
def test_oracle_step_against_the_reference(g, nc, tag, dtype):
    """One LogisticGAN D step and G step (R1, Adam, EMA) at depth 2: losses, gradients, updated parameters."""
    key = f"b_step{nc}_"
    d_loss, g_loss, d_grads, g_grads, gp, dp, shadow = run_oracle_step(nc, dtype)
    rel = 1e-4 if dtype == torch.float32 else 1e-9
    assert abs(d_loss - float(g[f"{key}{tag}_d_loss"])) <= rel * abs(float(g[f"{key}{tag}_d_loss"]))
    assert abs(g_loss - float(g[f"{key}{tag}_g_loss"])) <= rel * abs(float(g[f"{key}{tag}_g_loss"]))
    close(gp["truncation.avg_latent"], g[f"{key}{tag}_avg_latent"], 1e-5, 1e-6)
    for net, grads in (("d", d_grads), ("g", g_grads)):
        names = [str(n) for n in g[f"{key}{net}_grad_names"]]
        assert sorted(k for k, v in grads.items() if v is not None) == names      # same active set
        norm64, err32 = g[f"{key}{net}_grad_norm64"], g[f"{key}{net}_grad_err32"]
        floor = (1e-12 if dtype == torch.float64 else 1e-7) * float(norm64.max())
        for k, n64, e32 in zip(names, norm64, err32):
            ref64 = g.get(f"{key}{net}_grad64::{k}") if f"{key}{net}_grad64::{k}" in g.files else None
            if ref64 is not None:
                err = torch.linalg.vector_norm(grads[k].detach().double() - T(ref64, torch.float64)).item()
                tol = max(floor, 1e-9 * n64 if dtype == torch.float64 else max(1e-3 * n64, 4 * e32))
                assert err <= tol, (k, err, tol)
            else:
                n = gu.tensor_stats(grads[k])[2]
                assert abs(n - n64) <= (1e-8 if dtype == torch.float64 else 2e-2) * n64 + floor, k
    if dtype == torch.float64:
        for net, params in (("d", dp), ("g", gp), ("s", shadow)):
            names = [str(n) for n in g[f"{key}{net}_param_names"]]
            for k, st in zip(names, g[f"{key}{tag}_{net}_param_stats"]):
                s = gu.tensor_stats(params[k])
                assert abs(s[2] - st[2]) <= 1e-9 * st[2] + 1e-12, (net, k)
                assert abs(s[0] - st[0]) <= 1e-7 * st[1] + 1e-12, (net, k)


# ------------------------------------------------------------------ the fp64 restatement of the kernels
def _ops(J, C, kind, npix=37, seed=0):
    gen = torch.Generator().manual_seed(100 * J + C + seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    sj, sc = IR.layout(kind, J, C)
    return r(npix, J), r(npix, C), r(J * C), r(C), r(J), sj, sc


def _conv_weight(w, J, sj, sc, C, kind):
    """The flat parameter as the conv2d weight of its layer: from_rgb [C][J][1][1] / to_rgb [J][C][1][1]."""
    return w.view(C, J, 1, 1) if kind == "in" else w.view(J, C, 1, 1)


@pytest.mark.parametrize("kind", ["in", "out"])
@pytest.mark.parametrize("J", [1, 2, 4, 8])
def test_ref_matches_conv2d(J, kind):
    """img_in is conv2d with the from_rgb-shaped weight (or the transposed convolution with the to_rgb-shaped one), img_out the other way
    round, img_wgrad the gradient autograd gives conv2d's weight; S bounds |ref| and is ref on non-negative operands."""
    import torch.nn.functional as TF
    C, ws = 16, 0.37
    img, x, w, bc, bj, sj, sc = _ops(J, C, kind)
    img4, x4 = img.t().reshape(1, J, 37, 1), x.t().reshape(1, C, 37, 1)
    W = _conv_weight(w, J, sj, sc, C, kind).clone().requires_grad_(True)
    flat = lambda t: t.reshape(t.shape[1], 37).t()
    ref, S, n = IR.img_in(img, w, J, sj, sc, ws, bc, C)
    got = TF.conv2d(img4, ws * W, bc) if kind == "in" else TF.conv_transpose2d(img4, ws * W) + bc.view(1, -1, 1, 1)
    assert torch.allclose(ref, flat(got), rtol=1e-12, atol=1e-12) and n == J + 2 and bool((S >= ref.abs() - 1e-12).all())
    f = torch.randn(37, C, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    (gw,) = torch.autograd.grad((flat(got) * f).sum(), W)
    rw, Sw, nw = IR.img_wgrad(img, f, J, sj, sc, ws, C, torch.float32)
    assert torch.allclose(rw, gw.reshape(-1), rtol=1e-12, atol=1e-12) and bool((Sw >= rw.abs() - 1e-12).all()) and nw == 2
    ref, S, n = IR.img_out(x, w, J, sj, sc, ws, bj, C, torch.float32)
    got = TF.conv_transpose2d(x4, ws * W) + bj.view(1, -1, 1, 1) if kind == "in" else TF.conv2d(x4, ws * W, bj)
    assert torch.allclose(ref, flat(got), rtol=1e-12, atol=1e-12) and bool((S >= ref.abs() - 1e-12).all())
    assert n == 2 + 4 * 1 + 2 + 1                          # C = 16 in fp32: 4 vectors per pixel, 4 lanes, 2 exchange steps
    ra, Sa, _ = IR.img_in(img.abs(), w.abs(), J, sj, sc, ws, bc.abs(), C)
    assert torch.allclose(ra, Sa, rtol=1e-12, atol=0)


@pytest.mark.parametrize("J", [1, 4])
def test_ref_closes_under_differentiation(J):
    """First and second order: the gradients of y = img_in(img) are img_out (image), img_wgrad (weight) and the column sum (bias), and the
    R1-shaped gradient of |d(sum(y r))/d img|^2 with respect to the weight is 2 wscale * img_wgrad(gi, r) -- what the Img autograd
    Functions compose -- against CPU autograd on conv2d."""
    import torch.nn.functional as TF
    C, ws, npix = 16, 0.37, 2 * 8 * 8
    img, _, w, bc, _, sj, sc = _ops(J, C, "in", npix)
    r = torch.randn(npix, C, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    W = w.view(C, J, 1, 1).clone().requires_grad_(True)
    im = img.t().reshape(1, J, npix, 1).clone().requires_grad_(True)
    b = bc.clone().requires_grad_(True)
    y = TF.conv2d(im, ws * W, b).reshape(C, npix).t()
    gi, gw, gb = torch.autograd.grad((y * r).sum(), (im, W, b), create_graph=True)
    ri, _, _ = IR.img_out(r, w, J, sj, sc, ws, None, C, torch.float32)
    rw, _, _ = IR.img_wgrad(img, r, J, sj, sc, ws, C, torch.float32)
    assert torch.allclose(gi.reshape(J, npix).t(), ri, rtol=1e-12, atol=1e-12)
    assert torch.allclose(gw.reshape(-1), rw, rtol=1e-12, atol=1e-12)
    assert torch.allclose(gb, r.sum(0), rtol=1e-12, atol=1e-12)
    (g2,) = torch.autograd.grad((gi * gi).sum(), W)
    r2, _, _ = IR.img_wgrad(2 * ri, r, J, sj, sc, ws, C, torch.float32)
    assert torch.allclose(g2.reshape(-1), r2, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("J", [1, 2, 3, 4])
def test_ref_images_u8_is_the_oracles_transform(J, chw):
    """The ingest restatement equals the oracle's transform chain (channel-generic) to fp32 rounding, with flips."""
    hwc = torch.randint(0, 256, (3, 4, 6, J), dtype=torch.uint8, generator=torch.Generator().manual_seed(J))
    flip = [True, False, True]
    ref, S, n = IR.images_u8(hwc.permute(0, 3, 1, 2).contiguous() if chw else hwc, torch.tensor(flip), chw)
    want = O.images_u8_to_float(hwc, flip).permute(0, 2, 3, 1).double()
    assert n == 2 and ref.shape == (3, 4, 6, J) and float((ref - want).abs().max()) <= 4 * 2.0 ** -24 and bool((S >= ref.abs()).all())


# ------------------------------------------------------------------ the surface
def test_binding_table_lists_the_image_entry_points():
    from stylegan.pytorch_amd import native
    for name in ("sgx_img_in", "sgx_img_out", "sgx_img_wgrad", "sgx_img_wgrad_ws_bytes", "sgx_images_u8_to_nhwc_c"):
        assert name in native.SIGNATURES, name


def test_img_layout():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native
    assert F.img_layout(torch.zeros(16, 4, 1, 1), 4) == (1, 4, 16)
    assert F.img_layout(torch.zeros(1, 32, 1, 1), 1) == (32, 1, 32)
    assert F.img_layout(torch.zeros(8, 4, 1, 1), 4) == (1, 4, 8) and F.img_layout(torch.zeros(8, 4, 1, 1), 8) == (4, 1, 4)
    assert F.rgb_layout(torch.zeros(16, 3, 1, 1)) == (1, 3, 16)
    for w, J in ((torch.zeros(4, 4, 1, 1), 4), (torch.zeros(16, 4, 1, 1), 3), (torch.zeros(16, 2, 1, 1), 4), (torch.zeros(16, 4, 3, 3), 4)):
        with pytest.raises(native.SgxError):
            F.img_layout(w, J)


def test_diffaug_needs_rgb():
    from stylegan.pytorch_amd.GAN import Discriminator
    kw = dict(resolution=8, blur_filter=[1, 2, 1], fmap_base=64, fmap_max=16)
    with pytest.raises(ValueError, match="num_channels == 3"):
        Discriminator(num_channels=1, diffaug_policy="color", **kw)
    with pytest.raises(ValueError, match="num_channels == 3"):
        Discriminator(num_channels=4, diffaug_policy="xflip", ada_target=0.6, **kw)
    assert Discriminator(num_channels=1, **kw).from_rgb[0].weight.shape == (16, 1, 1, 1)
    assert Discriminator(num_channels=3, diffaug_policy="color", **kw)._diffaug_bits == 1


def test_one_by_one_layer_still_refuses_other_widths():
    """5 image channels (or 5 -> 16 with a 4-channel input) has no kernel: NotImplementedError before anything touches a device."""
    from stylegan.pytorch_amd.CustomLayers import EqualizedConv2d
    with pytest.raises(NotImplementedError):
        EqualizedConv2d(5, 16, 1).forward_nhwc(torch.zeros(1, 4, 4, 5))
    with pytest.raises(NotImplementedError):
        EqualizedConv2d(16, 5, 1).forward_nhwc(torch.zeros(1, 4, 4, 16))
    with pytest.raises(NotImplementedError):
        EqualizedConv2d(4, 16, 1).forward_nhwc(torch.zeros(1, 4, 4, 2))


def test_yaml_dataset_channels_merge(tmp_path):
    from stylegan.pytorch_amd.config import default_cfg
    p = tmp_path / "gray.yaml"
    p.write_text('structure: "linear"\ndataset:\n  resolution: 32\n  channels: 1\n')
    opt = default_cfg()
    assert opt.dataset.channels == 3
    opt.merge_from_file(str(p))
    assert opt.dataset.channels == 1 and opt.dataset.resolution == 32


def test_synthetic_images_channels():
    from stylegan.pytorch_amd.data import SyntheticImages
    ds = SyntheticImages(4, 8, channels=1)
    assert ds[0].shape == (1, 8, 8) and SyntheticImages(4, 8, channels=4)[1].shape == (4, 8, 8)
