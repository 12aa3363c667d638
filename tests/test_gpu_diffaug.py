"""-m gpu: DiffAugment of the discriminator's input (csrc/diffaug.hip, functional.DiffAugFn, Discriminator(diffaug_policy=...)) against
the fp64 restatement in tests/diffaug_ref.py -- the kernels alone, D with its R1 double backward, whole training steps (the oracle's
discriminator composed with the restatement under the same pinned draws), graph replay and the invariants of the default path."""
import random

import pytest
import torch

import aug_ref as AR
import diffaug_ref as R
import golden_util as gu
from aug_gpu_util import mid_dis
from gpu_util import DEV, MID, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

POLICY = "color,translation,cutout"
OPT = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)


def run_kernel(x, u, bits, adjoint, with_bias):
    """functional._diffaug (sgx_diffaug) under the library's profiler: every launch it records is what sgx_aug_plan reports for the call."""
    from stylegan.pytorch_amd import functional as F, native as N
    N.prof_start(1)
    try:
        y = F._diffaug(x, u, bits, adjoint, with_bias)
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    AR.assert_recorded_is_planned(N, AR.DIFFAUG, x, y, bits, adjoint, with_bias)
    return y


# (B, H, W, base offset in floats): the vector path (W % 4 == 0, aligned bases) and the per-pixel one (odd widths, unaligned base)
SHAPES = [(1, 4, 4, 0), (4, 8, 8, 0), (3, 64, 64, 0), (2, 128, 128, 0), (2, 1024, 1024, 0), (8, 16, 16, 0),
          (4, 5, 7, 0), (2, 6, 10, 0), (3, 9, 12, 0), (4, 16, 16, 1), (2, 33, 20, 1)]


@pytest.mark.parametrize("B,H,W,off", SHAPES)
def test_kernel_vs_restatement(B, H, W, off):
    g = torch.Generator().manual_seed(H * 1000 + W + B)
    x = torch.randn(B, H, W, 3, generator=g)
    gy = torch.randn(B, H, W, 3, generator=g)
    u = torch.from_numpy(R.edge_draws(B, seed=H + W + B))
    buf = torch.zeros(B * H * W * 3 + off, device=DEV)
    xd = buf[off:].view(B, H, W, 3)
    xd.copy_(x.to(DEV))
    ud = u.to(DEV)
    for bits in range(1, 8):
        for adjoint, with_bias in ((False, True), (False, False), (True, False)):
            y = run_kernel(xd, ud, bits, adjoint, with_bias)
            ref = R.apply(x.double().permute(0, 3, 1, 2), u, bits, adjoint, with_bias).permute(0, 2, 3, 1)
            err = float((y.double().cpu() - ref).abs().max())
            assert err <= 1e-5 * float(ref.abs().max()) + 1e-30, (bits, adjoint, with_bias, err)
            y2 = run_kernel(xd, ud, bits, adjoint, with_bias)
            assert torch.equal(y, y2), (bits, adjoint, with_bias)                        # bit-reproducible run to run
        ax = run_kernel(xd, ud, bits, False, False).double().cpu()
        aty = run_kernel(gy.to(DEV), ud, bits, True, False).double().cpu()
        lhs, rhs = float((ax * gy.double()).sum()), float((x.double() * aty).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((ax * gy.double()).abs().sum()), (bits, lhs, rhs)   # adjoint identity on the kernels


def patch_oracle(monkeypatch, u, bits):
    """Every oracle D evaluation sees the restatement with the draws ``u`` (what diffaug_override does to ours)."""
    orig = O.discriminator

    def discriminator(p, img, depth, alpha, total_depth, **kw):
        return orig(p, R.apply(img, u, bits), depth, alpha, total_depth, **kw)
    monkeypatch.setattr(O, "discriminator", discriminator)


@pytest.mark.parametrize("depth,alpha", [(5, 0.5), (3, 0.3)])
def test_network_first_and_second_order_vs_oracle(monkeypatch, depth, alpha):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss (R1 included: second order through the augmentation)."""
    from stylegan.pytorch_amd import Losses
    B, res = 4, 4 * 2 ** depth
    gp, dp = mid_params(torch.float64)
    dis = load_into(mid_dis(POLICY), dp)
    dis.train()
    u = torch.from_numpy(R.edge_draws(B, seed=depth))
    dis.diffaug_override = u.to(DEV)
    patch_oracle(monkeypatch, u, 7)
    real = gu.seeded((B, 3, res, res), 300 + depth); fake = gu.seeded((B, 3, res, res), 400 + depth)

    score = dis(real.to(DEV), depth, alpha)
    ref = O.discriminator(dp, real.double(), depth, alpha, MID_DEPTH)
    assert float((score.double().cpu() - ref).norm()) <= 2e-5 * float(ref.norm()), (score, ref)

    loss_fn = Losses.LogisticGAN(dis)
    rd = real.to(DEV).requires_grad_(True)
    r1 = loss_fn._r1_from_logit(dis(rd, depth, alpha), rd)
    r1_ref = O.r1_penalty(dp, real.double(), depth, alpha, MID_DEPTH)
    assert abs(float(r1) - float(r1_ref)) <= 1e-4 * abs(float(r1_ref)), (float(r1), float(r1_ref))

    params = [p for p in dis.parameters()]
    names = [k for k, _ in dis.named_parameters()]
    loss = loss_fn.dis_loss(real.to(DEV), fake.to(DEV), depth, alpha)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    oloss = O.logistic_d_loss(dp, real.double(), fake.double(), depth, alpha, MID_DEPTH)
    ograds = torch.autograd.grad(oloss, [dp[k] for k in names], allow_unused=True)
    assert abs(float(loss) - float(oloss)) <= 1e-4 * abs(float(oloss)), (float(loss), float(oloss))
    net_scale = max(float(g.norm()) for g in ograds if g is not None)
    checked = 0
    for k, a, b in zip(names, grads, ograds):
        if b is None or float(b.norm()) == 0.0:
            assert a is None or float(a.abs().max()) == 0.0, k
            continue
        err = float((a.double().cpu() - b).norm())
        assert err <= 1e-3 * float(b.norm()) + 1e-6 * net_scale, (k, err, float(b.norm()))
        checked += 1
    assert checked >= 6


def make_sg(loss="logistic", policy=POLICY, use_graphs=False, conditional=False):
    from stylegan.pytorch_amd.GAN import StyleGAN
    return StyleGAN(structure="linear", resolution=128, num_channels=3, latent_size=512,
                    g_args=dict(latent_size=512, mapping_layers=MID["mapping_layers"], blur_filter=[1, 2, 1], truncation_psi=0.7,
                                truncation_cutoff=8, fmap_base=MID["fmap_base"], fmap_max=MID["fmap_max"]),
                    d_args=dict(use_wscale=True, blur_filter=[1, 2, 1], fmap_base=MID["fmap_base"], fmap_max=MID["fmap_max"],
                                diffaug_policy=policy),
                    g_opt_args=OPT, d_opt_args=OPT, loss=loss, d_repeats=1, use_ema=True, ema_decay=0.999,
                    device=torch.device(DEV), use_graphs=use_graphs, conditional=conditional, n_classes=5 if conditional else 0)


def module_params(module):
    names = {k for k, _ in module.named_parameters()}
    return {k: v.detach().double().cpu().requires_grad_(k in names) for k, v in module.state_dict().items() if not k.endswith(".kernel")}


@pytest.mark.parametrize("loss,depth,alpha,conditional", [("logistic", 5, 0.5, False), ("logistic", 2, 0.3, False),
                                                          ("hinge", 4, 0.75, False), ("conditional-loss", 3, 0.5, True)])
def test_full_step_vs_oracle(monkeypatch, loss, depth, alpha, conditional):
    B = 4
    sg = make_sg(loss, conditional=conditional)
    if conditional:
        for m in (sg.gen, sg.dis):
            m.load_state_dict({k: (v if k.endswith(".kernel") else gu.fill_value(k, v.shape).to(v.device)) for k, v in m.state_dict().items()})
        sg.gen_shadow.load_state_dict(sg.gen.state_dict())
        gp, dp = module_params(sg.gen), module_params(sg.dis)
        labels = torch.tensor([0, 3, 1, 4])
        zw = 1024                                                # the mixing latents have the concatenated width
    else:
        gp, dp = mid_params(torch.float64)
        load_into(sg.gen, gp); load_into(sg.dis, dp); load_into(sg.gen_shadow, gp)
        labels, zw = None, 512
    sg.gen.train(); sg.dis.train()
    noises = mid_noises(B)
    pin_noise(sg.gen, noises)
    u = torch.from_numpy(R.edge_draws(B, seed=10 + depth))
    sg.dis.diffaug_override = u.to(DEV)
    patch_oracle(monkeypatch, u, 7)
    z = gu.seeded((B, 512), 51 + depth); real = gu.seeded((B, 3, 128, 128), 61 + depth)
    ld = None if labels is None else labels.to(DEV)
    torch.manual_seed(71); random.seed(71)
    d_loss = float(sg.optimize_discriminator(z.to(DEV), real.to(DEV), depth, alpha, ld))
    d_grads = {k: p.grad.detach().clone() for k, p in sg.dis.named_parameters() if p.grad is not None}
    torch.manual_seed(72); random.seed(72)
    g_loss = float(sg.optimize_generator(z.to(DEV), real.to(DEV), depth, alpha, ld))

    okw = dict(total_depth=MID_DEPTH, mapping_layers=MID["mapping_layers"], noises=noises, loss=loss, labels=labels)
    torch.manual_seed(71); random.seed(71)
    l2, cut = O.draw_mixing((B, zw), depth)
    od, odg = O.d_step(gp, dp, O.AdamState(), z.double(), real.double(), depth, alpha, latents2=l2.double(), mixing_cutoff=cut, **okw)
    torch.manual_seed(72); random.seed(72)
    l2, cut = O.draw_mixing((B, zw), depth)
    og, _ = O.g_step(gp, dp, O.AdamState(), z.double(), depth, alpha, latents2=l2.double(), mixing_cutoff=cut, real_full=real.double(), **okw)
    assert abs(d_loss - od) <= 1e-4 * abs(od) + 1e-6, (d_loss, od)
    assert abs(g_loss - og) <= 1e-4 * abs(og) + 1e-6, (g_loss, og)
    net_scale = max(float(v.norm()) for v in odg.values() if v is not None)
    assert sorted(d_grads) == sorted(k for k, v in odg.items() if v is not None)
    for k, a in d_grads.items():
        err = float((a.double().cpu() - odg[k]).norm())
        assert err <= 1e-3 * float(odg[k].norm()) + 1e-6 * net_scale, (k, err, float(odg[k].norm()))


def train_run(use_graphs, iters=4, override=True, seed=5):
    sg = make_sg(use_graphs=use_graphs)
    gp, dp = mid_params(torch.float64)
    load_into(sg.gen, gp); load_into(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, mid_noises(4))
    if override:
        sg.dis.diffaug_override = torch.from_numpy(R.edge_draws(4, seed=3)).to(DEV)
    torch.manual_seed(seed); random.seed(seed)
    losses = []
    for i in range(iters):
        alpha = min(1.0, 0.25 + 0.15 * i)
        z = gu.seeded((4, 512), 100 + i).to(DEV); real = gu.seeded((4, 3, 128, 128), 200 + i).to(DEV)
        losses.append((float(sg.optimize_discriminator(z, real, 5, alpha)), float(sg.optimize_generator(z, real, 5, alpha))))
    torch.cuda.synchronize()
    return losses, sg


def test_graph_replay_matches_eager_with_pinned_draws():
    from test_gpu_graphs import losses_agree
    le, _ = train_run(False)
    lg, sg = train_run(True)
    assert all(g.graph is not None for g in sg._step_graphs.values()) and len(sg._step_graphs) == 2
    losses_agree(le, lg)


def test_replayed_draws_are_fresh():
    """A captured D(x) draws new augmentation parameters at every replay (torch's graph-safe generator), nothing is baked in."""
    dis = load_into(mid_dis(POLICY), mid_params(torch.float64)[1])
    dis.train()
    x = gu.seeded((4, 3, 128, 128), 9).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(2):
            dis(x, 5, 0.5)                                            # warm up (weight packs) outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    from stylegan.pytorch_amd import native
    native.reserve_capture_staging(1 << 20)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        out = dis(x, 5, 0.5)
    g.replay(); torch.cuda.synchronize()
    a = out.clone()
    g.replay(); torch.cuda.synchronize()
    assert not torch.equal(a, out)


def test_same_seed_is_bit_identical_and_eval_does_not_augment():
    l0, sg0 = train_run(False, iters=2, override=False, seed=11)
    l1, _ = train_run(False, iters=2, override=False, seed=11)
    assert l0 == l1
    dis, plain = sg0.dis, mid_dis("")
    plain.load_state_dict(dis.state_dict())
    dis.eval(); plain.eval()
    x = gu.seeded((4, 3, 128, 128), 19).to(DEV)
    with torch.no_grad():
        assert torch.equal(dis(x, 5, 0.5), plain(x, 5, 0.5))


def test_empty_policy_is_the_default_path():
    """Policy '': the same outputs AND the same device-RNG state as a Discriminator built without the key."""
    from stylegan.pytorch_amd.GAN import Discriminator
    dp = mid_params(torch.float64)[1]
    plain = load_into(Discriminator(resolution=MID["resolution"], num_channels=3, use_wscale=True, blur_filter=[1, 2, 1],
                                    fmap_base=MID["fmap_base"], fmap_max=MID["fmap_max"], structure="linear").to(DEV), dp)
    empty = load_into(mid_dis(""), dp)
    plain.train(); empty.train()
    x = gu.seeded((4, 3, 128, 128), 29).to(DEV)
    outs, states = [], []
    for d in (plain, empty):
        torch.cuda.manual_seed(123)
        outs.append(d(x, 5, 0.5).detach())
        states.append(torch.cuda.get_rng_state())
    assert torch.equal(outs[0], outs[1]) and torch.equal(states[0], states[1])
    on = load_into(mid_dis(POLICY), dp)
    on.train()
    torch.cuda.manual_seed(123)
    on(x, 5, 0.5)
    assert not torch.equal(torch.cuda.get_rng_state(), states[0])          # (the policy-on forward does draw)


def test_diffaug_kernels_have_no_scratch():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.collect() if k["file"] == "diffaug.hip"]
    assert len(ks) >= 8, ks
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, k


def test_yaml_policy_trains(tmp_path):
    """A config with model.dis.diffaug_policy trains through StyleGAN.train (train.py's construction: d_args=opt.model.dis)."""
    from stylegan.pytorch_amd.GAN import StyleGAN
    from stylegan.pytorch_amd.config import default_cfg
    from stylegan.pytorch_amd.data import SyntheticImages
    p = tmp_path / "da.yaml"
    p.write_text('structure: "linear"\ndataset:\n  resolution: 32\nmodel:\n  gen:\n    mapping_layers: 2\n  dis:\n'
                 '    diffaug_policy: "color,translation,cutout"\nsched:\n  epochs: [1, 1, 1, 1]\n  batch_sizes: [4, 4, 4, 4]\n'
                 '  fade_in_percentage: [50, 50, 50, 50]\n')
    opt = default_cfg()
    opt.merge_from_file(str(p))
    g_args = dict(opt.model.gen, fmap_base=256, fmap_max=32)
    d_args = dict(opt.model.dis, fmap_base=256, fmap_max=32)
    sg = StyleGAN(structure=opt.structure, conditional=opt.conditional, n_classes=opt.n_classes, resolution=opt.dataset.resolution,
                  num_channels=opt.dataset.channels, latent_size=opt.model.gen.latent_size, g_args=g_args, d_args=d_args,
                  g_opt_args=opt.model.g_optim, d_opt_args=opt.model.d_optim, loss=opt.loss, drift=opt.drift, d_repeats=opt.d_repeats,
                  use_ema=opt.use_ema, ema_decay=opt.ema_decay, device=torch.device(DEV))
    assert sg.dis._diffaug_bits == 7
    import logging
    sg.train(dataset=SyntheticImages(8, 32), num_workers=0, epochs=opt.sched.epochs, batch_sizes=opt.sched.batch_sizes,
             fade_in_percentage=opt.sched.fade_in_percentage, logger=logging.getLogger("diffaug"), output=str(tmp_path),
             num_samples=4, feedback_factor=100, checkpoint_factor=100)
    for p_ in sg.dis.parameters():
        assert torch.isfinite(p_).all()
