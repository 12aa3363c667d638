"""-m gpu: adaptive discriminator augmentation (csrc/diffaug.hip: sgx_ada_gates, sgx_diffaug_gated, sgx_ada_update; the img_bits
argument of functional.DiffAug*Fn; Discriminator(ada_target=...)) against the restatement in tests/ada_ref.py -- the three kernels alone,
D with its R1 double backward under mixed per-image gates, graph replay with a moving p, and the invariants of the default path."""
import random
import types

import numpy as np
import pytest
import torch

import ada_ref as A
import aug_ref as AR
import diffaug_ref as R
import golden_util as gu
from aug_gpu_util import dev_state, dparams, make_sg, mid_dis, small_dis
from gpu_util import DEV, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

POLICY = "color,translation,cutout"
OPT = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
f32 = np.float32
EDGE = f32(R.EDGE)
BIG_KIMG = 1e9                                   # p does not move within a test: 4 images * 1e-12 is far below half an ulp of 0.5 and 1


# ------------------------------------------------------------------------------------------------------------------ 1. the gates
@pytest.mark.parametrize("B", [1, 7, 64, 1000])
def test_gates_kernel_vs_restatement(B):
    from stylegan.pytorch_amd import functional as F
    rng = np.random.default_rng(B)
    for p in (f32(0), f32(2.0 ** -24), f32(0.5), EDGE, f32(1)):
        gu_ = rng.random((B, 3), dtype=f32)
        flat = gu_.reshape(-1)
        for k, v in enumerate((f32(0), EDGE, p, p)):                     # the edges of [0,1) and values equal to p
            flat[(k * 5) % flat.size] = v
        if B == 1:
            flat[:] = (f32(0), EDGE, p)
        state = dev_state(p)
        for bits in range(1, 8):
            out = F.ada_gates(torch.from_numpy(gu_).to(DEV), state, bits)
            assert out.dtype == torch.int32 and tuple(out.shape) == (B,)
            assert np.array_equal(out.cpu().numpy(), A.gates(gu_, p, bits)), (float(p), bits)
        uniforms = torch.from_numpy(np.minimum(gu_, EDGE)).to(DEV)          # what torch.rand can give: [0, 1), without the values == 1
        if p == 0:
            assert int(F.ada_gates(uniforms, state, 7).abs().sum()) == 0     # p = 0 gates nothing, not even u = 0
        if p == 1:
            assert bool((F.ada_gates(uniforms, state, 7) == 7).all())        # p = 1 gates everything, up to the largest fp32 below 1


# ------------------------------------------------------------------------------------------------------------ 2. the gated kernel
GUARD = 64                                       # floats around y (a multiple of 4: y keeps its 16-byte alignment)
SENTINEL = 12345.5


def run_gated(xd, ud, bitsd, adjoint, with_bias, policy=7):
    """sgx_diffaug_gated into a buffer with guard floats on both sides of y; -> y (a copy), the guards checked, and every launch the
    profiler recorded what sgx_aug_plan reports for the call."""
    from stylegan.pytorch_amd import native as N
    B, H, W, _ = xd.shape
    n = xd.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    y = buf[GUARD:GUARD + n].view(B, H, W, 3)
    L = N.lib()
    nb = L.sgx_diffaug_ws_bytes(B, H, W)
    ws = N.workspace(nb, xd.device)
    N.prof_start(1)
    try:
        rc = L.sgx_diffaug_gated(N.ptr(xd), N.ptr(y), N.ptr(ud), N.ptr(bitsd), B, H, W, policy, int(adjoint), int(with_bias), N.ptr(ws), nb, N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    N.check(rc, "sgx_diffaug_gated")
    AR.assert_recorded_is_planned(N, AR.GATED, xd, y, policy, adjoint, with_bias)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), "guard floats were written"
    return y.clone()


# (B, H, W, base offset in floats): the vector path; two partials per image in the sum pass (132 * 128 > 16384 pixels); the per-pixel
# path (odd widths, an unaligned base)
GATED_SHAPES = [(8, 8, 8, 0), (8, 16, 16, 0), (8, 132, 128, 0), (8, 5, 7, 0), (8, 9, 12, 0), (8, 16, 16, 1)]


@pytest.mark.parametrize("B,H,W,off", GATED_SHAPES)
def test_gated_kernel(B, H, W, off):
    from stylegan.pytorch_amd import functional as F
    g = torch.Generator().manual_seed(H * 1000 + W + B)
    x = torch.randn(B, H, W, 3, generator=g)
    gy = torch.randn(B, H, W, 3, generator=g)
    u = torch.from_numpy(R.edge_draws(B, seed=H + W + B))
    bits = list(range(8))                                                  # every combination of ops in one batch
    bufs = []
    for t in (x, gy):
        buf = torch.zeros(B * H * W * 3 + off, device=DEV)
        v = buf[off:].view(B, H, W, 3)
        v.copy_(t.to(DEV))
        bufs.append(v)
    xd, gd = bufs
    ud, bd = u.to(DEV), torch.tensor(bits, dtype=torch.int32, device=DEV)
    for adjoint, with_bias in ((False, True), (False, False), (True, False)):
        y = run_gated(xd, ud, bd, adjoint, with_bias)
        ref = A.apply_gated(x.double().permute(0, 3, 1, 2), u, bits, adjoint, with_bias).permute(0, 2, 3, 1)
        err = float((y.double().cpu() - ref).abs().max())
        assert err <= 1e-5 * float(ref.abs().max()) + 1e-30, (adjoint, with_bias, err)                     # (a)
        assert torch.equal(y[0], xd[0]), (adjoint, with_bias)                                               # (b) bits 0: a copy
        for b in (0, 2, 4, 6):                                                                              # (c) no colour: pure gathers
            single = F._diffaug(xd[b:b + 1], ud[b:b + 1], bits[b], adjoint, with_bias)
            assert torch.equal(y[b:b + 1], single), (b, adjoint, with_bias)
        assert torch.equal(y, run_gated(xd, ud, bd, adjoint, with_bias)), (adjoint, with_bias)              # (d)
        assert torch.equal(y, F._diffaug(xd, ud, 7, adjoint, with_bias, bd))                                # the autograd functions' path
    ax = run_gated(xd, ud, bd, False, False).double().cpu()
    aty = run_gated(gd, ud, bd, True, False).double().cpu()
    lhs, rhs = float((ax * gy.double()).sum()), float((x.double() * aty).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((ax * gy.double()).abs().sum()), (lhs, rhs)                       # (e) <A x, g> = <x, A^T g>
    # the union decides only whether the sum pass runs: without the colour bit in it, every image is gathered under its other bits
    y = run_gated(xd, ud, bd, False, True, policy=6)
    for b in range(8):
        assert torch.equal(y[b:b + 1], F._diffaug(xd[b:b + 1], ud[b:b + 1], bits[b] & 6, False, True)), b


# ------------------------------------------------------------------------------------------------------------- 3. the controller
def logits_for(B, call, sign, rng):
    v = (np.abs(rng.standard_normal(B)) * 1e20 * sign).astype(f32)          # large magnitudes, mostly one sign
    v[rng.random(B) < 0.05] *= f32(-1e-30)                                  # ... a few of the other, tiny
    special = (f32(np.nan), f32(0.0), f32(-0.0))
    if B == 1:
        if call % 4 == 3:
            v[0] = special[(call // 4) % 3]
    else:
        v[call % B] = special[0]                                            # exactly one NaN
        v[(call + 1) % B] = special[1]
        v[(call + 2) % B] = special[2]
    return v


@pytest.mark.parametrize("B", [1, 4, 100, 1000])
@pytest.mark.parametrize("interval", [1, 4])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_controller_kernel_vs_restatement(B, interval, sign):
    from stylegan.pytorch_amd import functional as F
    rng = np.random.default_rng(B * 10 + interval)
    p0 = 0.7 if sign > 0 else 0.3
    adjust = f32(0.25 / (B * interval))                                     # a quarter per update: the clamp is reached by the second one
    target = 0.1 if sign > 0 else 0.6                                       # (at B = 4 three logits are NaN and +-0: r_t = +-0.25)
    ref, state = A.new_state(p0), dev_state(p0)
    hit = False
    for call in range(12):
        lg = logits_for(B, call, sign, rng)
        ref = A.controller(ref, lg, target, adjust, interval)
        F.ada_update(torch.from_numpy(lg).to(DEV), state, target, float(adjust), interval)
        got = state.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (call, got, ref)
        hit = hit or ref[0] == (1.0 if sign > 0 else 0.0)
    assert hit and ref[5] == 12 // interval                                 # the trajectory did reach its clamp


def test_controller_crosses_the_target():
    """r_t on both sides of the target and equal to it (p held), interval 1, bit-equal states."""
    from stylegan.pytorch_amd import functional as F
    ref, state = A.new_state(0.5), dev_state(0.5)
    adjust = A.adjust_per_image(0.02)                                       # 0.05 per image
    for lg in ([1, 1, 1, 1], [-1, -1, 1, -1], [1, 1, 1, -1], [3, np.nan, 0.0, -0.0], [1, 1, 1, -1]):
        lg = np.array(lg, f32)
        ref = A.controller(ref, lg, 0.5, adjust, 1)
        F.ada_update(torch.from_numpy(lg).to(DEV), state, 0.5, float(adjust), 1)
        assert np.array_equal(state.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (lg, ref)
    assert ref[5] == 5 and ref[4] == 0.5


# ----------------------------------------------------------------------------------------------------------- 4. pinned equivalences
def load_ada(module, params):
    """gpu_util.load_into for a module that may have the ``ada_state`` buffer, which the oracle's parameters do not: it keeps its own."""
    if getattr(module, "ada", False):
        params = dict(params, ada_state=module.ada_state.detach().clone())
    return load_into(module, params)


def spread_gates(B):
    """[B,3] gate uniforms spread over (0, 1): at any p in steps of 0.2 from 0.1 some are below and some above."""
    return torch.tensor([[((3 * b + k) * 5 % 12 + 0.5) / 12 for k in range(3)] for b in range(B)], dtype=torch.float32)


def test_pinned_p_equivalences(dparams):
    B, depth, alpha = 4, 5, 0.5
    x = gu.seeded((B, 3, 128, 128), 29).to(DEV)
    u = torch.from_numpy(R.edge_draws(B, seed=2)).to(DEV)
    gates_ = spread_gates(B).to(DEV)

    def out(policy, **kw):
        d = load_ada(mid_dis(policy, **kw), dparams)
        d.train()
        d.diffaug_override = u
        if kw:
            d.ada_gate_override = gates_
        with torch.no_grad():
            y = d(x, depth, alpha)
        if kw:
            assert d.ada_p == kw["ada_p_init"]
        return y
    one = dict(ada_target=0.6, ada_p_init=1.0, ada_kimg=BIG_KIMG)
    zero = dict(ada_target=0.6, ada_p_init=0.0, ada_kimg=BIG_KIMG)
    a, b = out(POLICY, **one), out(POLICY)                                  # p = 1: every image has the colour bit
    assert float((a.double() - b.double()).norm()) <= 2e-5 * float(b.double().norm()), (a, b)
    assert torch.equal(out("translation,cutout", **one), out("translation,cutout"))
    assert torch.equal(out(POLICY, **zero), out(""))                        # p = 0: nothing is augmented


# ------------------------------------------------------------------------------------------- 5. first and second order, mixed gates
def patch_oracle(monkeypatch, u, img_bits):
    """Every oracle D evaluation sees the per-image restatement with the draws ``u`` and the bits the gates must give."""
    orig = O.discriminator

    def discriminator(p, img, depth, alpha, total_depth, **kw):
        return orig(p, A.apply_gated(img, u, img_bits), depth, alpha, total_depth, **kw)
    monkeypatch.setattr(O, "discriminator", discriminator)


@pytest.mark.parametrize("depth,alpha", [(5, 0.5), (3, 0.3)])
def test_network_first_and_second_order_vs_oracle(monkeypatch, dparams, depth, alpha):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss with per-image gates (p = 0.5 against pinned uniforms)."""
    from stylegan.pytorch_amd import Losses
    B, res = 4, 4 * 2 ** depth
    dp = dparams
    dis = load_ada(mid_dis(POLICY, ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG), dp)
    dis.train()
    u = torch.from_numpy(R.edge_draws(B, seed=depth))
    gates_ = spread_gates(B)
    bits = A.gates(gates_.numpy(), 0.5, 7).tolist()
    assert len(set(bits)) >= 3 and any(b & 1 for b in bits) and any(not b & 1 for b in bits), bits       # mixed
    dis.diffaug_override, dis.ada_gate_override = u.to(DEV), gates_.to(DEV)
    patch_oracle(monkeypatch, u, bits)
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
    assert dis._ada_real is not None and dis.ada_p == 0.5                    # the loss reported D(real); nothing moved p


# ------------------------------------------------------------------------------------------------------ 6. graph replay, moving p
def train_run(use_graphs, iters=4, seed=5):
    # 1 / (0.02 * 1000) = 0.05 per image: one update (interval 1) at batch 4 moves p by 0.2
    sg = make_sg(POLICY, use_graphs, ada_target=0.6, ada_interval=1, ada_kimg=0.02, ada_p_init=0.5)
    gp, dp = mid_params(torch.float64)
    load_into(sg.gen, gp); load_ada(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, mid_noises(4))
    sg.dis.diffaug_override = torch.from_numpy(R.edge_draws(4, seed=3)).to(DEV)
    sg.dis.ada_gate_override = spread_gates(4).to(DEV)
    torch.manual_seed(seed); random.seed(seed)
    losses, states = [], []
    for i in range(iters):
        alpha = min(1.0, 0.25 + 0.15 * i)
        z = gu.seeded((4, 512), 100 + i).to(DEV); real = gu.seeded((4, 3, 128, 128), 200 + i).to(DEV)
        losses.append((float(sg.optimize_discriminator(z, real, 5, alpha)), float(sg.optimize_generator(z, real, 5, alpha))))
        states.append(sg.dis.ada_state.cpu().clone())
    torch.cuda.synchronize()
    return losses, states, sg


def test_graph_replay_matches_eager_with_a_moving_p():
    from test_gpu_graphs import losses_agree
    le, se, _ = train_run(False)
    lg, sg_, sg = train_run(True)
    assert all(g.graph is not None for g in sg._step_graphs.values()) and len(sg._step_graphs) == 2
    for i, (a, b) in enumerate(zip(se, sg_)):
        assert torch.equal(a, b), (i, a, b)                                 # p, the accumulators and the update count, step by step
    ps = [float(s[0]) for s in se]
    assert [float(s[5]) for s in se] == [1.0, 2.0, 3.0, 4.0]
    assert all(abs(abs(ps[i] - (ps[i - 1] if i else 0.5)) - 0.2) < 1e-6 or ps[i] in (0.0, 1.0) for i in range(4)), ps
    losses_agree(le, lg)


# ----------------------------------------------------------------------------------------------------------------- 7. fresh draws
def test_fresh_gates_statistics(monkeypatch):
    from stylegan.pytorch_amd import functional as F
    B, p = 4096, 0.3
    dis = small_dis(diffaug_policy=POLICY, ada_target=0.6, ada_p_init=p)
    dis.train()
    seen = []
    orig = F.ada_gates
    monkeypatch.setattr(F, "ada_gates", lambda *a: seen.append(orig(*a)) or seen[-1])
    torch.cuda.manual_seed(7)
    with torch.no_grad():
        dis(torch.randn(B, 3, 4, 4, device=DEV), 0, 1.0)
    assert len(seen) == 1
    bits = seen[0].cpu().numpy()
    sigma = (B * p * (1 - p)) ** 0.5
    cols = [(bits >> k) & 1 for k in range(3)]
    for k, c in enumerate(cols):
        assert abs(int(c.sum()) - B * p) <= 6 * sigma, (k, int(c.sum()))
    assert not np.array_equal(cols[0], cols[1]) and not np.array_equal(cols[1], cols[2]) and not np.array_equal(cols[0], cols[2])


# ------------------------------------------------------------------------------------------------------------------ 8. checkpoint
def test_checkpoint_round_trip():
    from stylegan.pytorch_amd import functional as F
    kw = dict(diffaug_policy=POLICY, ada_target=0.6, ada_interval=2, ada_kimg=0.01)
    a = small_dis(**kw)
    F.ada_update(torch.ones(8, device=DEV), a.ada_state, 0.6, a._ada_adjust, 2)
    F.ada_update(torch.ones(8, device=DEV), a.ada_state, 0.6, a._ada_adjust, 2)
    F.ada_update(-torch.ones(8, device=DEV), a.ada_state, 0.6, a._ada_adjust, 2)
    assert 0.0 < a.ada_p <= 1.0 and float(a.ada_state[5]) == 1.0 and float(a.ada_state[3]) == 1.0
    b = small_dis(**kw)
    b.load_state_dict(a.state_dict(), strict=True)
    assert torch.equal(a.ada_state, b.ada_state) and b.ada_p == a.ada_p
    off = small_dis(diffaug_policy=POLICY)
    off2 = small_dis(diffaug_policy=POLICY)
    off2.load_state_dict(off.state_dict(), strict=True)                      # an ADA-off checkpoint has exactly the keys it had
    assert "ada_state" not in off.state_dict()


# ------------------------------------------------------------------------------------------------------------------------ 9. yaml
def test_yaml_ada_trains(tmp_path):
    """A config with model.dis.ada_target trains through StyleGAN.train (train.py's construction: d_args=opt.model.dis)."""
    from stylegan.pytorch_amd.GAN import StyleGAN
    from stylegan.pytorch_amd.config import default_cfg
    from stylegan.pytorch_amd.data import SyntheticImages
    p = tmp_path / "ada.yaml"
    p.write_text('structure: "linear"\ndataset:\n  resolution: 32\nmodel:\n  gen:\n    mapping_layers: 2\n  dis:\n'
                 '    diffaug_policy: "color,translation,cutout"\n    ada_target: 0.6\n    ada_interval: 2\n    ada_kimg: 0.1\n'
                 'sched:\n  epochs: [1, 1, 1, 1]\n  batch_sizes: [4, 4, 4, 4]\n  fade_in_percentage: [50, 50, 50, 50]\n')
    opt = default_cfg()
    opt.merge_from_file(str(p))
    g_args = dict(opt.model.gen, fmap_base=256, fmap_max=32)
    d_args = dict(opt.model.dis, fmap_base=256, fmap_max=32)
    sg = StyleGAN(structure=opt.structure, conditional=opt.conditional, n_classes=opt.n_classes, resolution=opt.dataset.resolution,
                  num_channels=opt.dataset.channels, latent_size=opt.model.gen.latent_size, g_args=g_args, d_args=d_args,
                  g_opt_args=opt.model.g_optim, d_opt_args=opt.model.d_optim, loss=opt.loss, drift=opt.drift, d_repeats=opt.d_repeats,
                  use_ema=opt.use_ema, ema_decay=opt.ema_decay, device=torch.device(DEV))
    assert sg.dis.ada and sg.dis._diffaug_bits == 7
    import logging
    sg.train(dataset=SyntheticImages(8, 32), num_workers=0, epochs=opt.sched.epochs, batch_sizes=opt.sched.batch_sizes,
             fade_in_percentage=opt.sched.fade_in_percentage, logger=logging.getLogger("ada"), output=str(tmp_path),
             num_samples=4, feedback_factor=100, checkpoint_factor=100)
    state = sg.dis.ada_state.tolist()
    assert 0.0 <= state[0] <= 1.0 and state[5] > 0, state
    for p_ in sg.dis.parameters():
        assert torch.isfinite(p_).all()


# --------------------------------------------------------------------------------------------------------------- 10. data parallel
def test_data_parallel_with_ada_is_refused():
    group = types.SimpleNamespace(world_size=2)                              # (all the constructor reads of it before it refuses)
    with pytest.raises(ValueError, match="not supported"):
        make_sg(POLICY, data_parallel=group, ada_target=0.6)


# ---------------------------------------------------------------------------------------------------------------- 11. default path
def test_default_path_draws_as_before(dparams):
    """ada_target absent: a policy-on training forward is torch.rand(B, 7) and nothing else on the device generator."""
    B = 4
    on = load_into(mid_dis(POLICY), dparams)
    plain = load_into(mid_dis(""), dparams)
    on.train(); plain.train()
    x = gu.seeded((B, 3, 128, 128), 29).to(DEV)
    torch.cuda.manual_seed(123)
    with torch.no_grad():
        a = on(x, 5, 0.5)
    s_on = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(123)
    u = torch.rand(B, 7, device=DEV)                                         # the unchanged path, spelled out
    with torch.no_grad():
        plain(x, 5, 0.5)
    assert torch.equal(s_on, torch.cuda.get_rng_state())
    on.diffaug_override = u
    with torch.no_grad():
        assert torch.equal(a, on(x, 5, 0.5))
    assert not on.ada and "ada_state" not in on.state_dict()
