"""-m gpu: ADA's pixel blitting fused into the augmentation gather (csrc/diffaug.hip: sgx_diffaug_blit, sgx_ada_gates_n; the nine-draw
path of functional.DiffAug*Fn; Discriminator(diffaug_policy="...xflip,rot90...")) against the fp64 restatement in tests/blit_ref.py --
the kernels alone on every launch path, continuity with the kernels of the three-op policies, D with its R1 double backward under
mixed per-image gates, graph replay with a moving p, and what a training forward draws."""
import itertools
import random
import types

import numpy as np
import pytest
import torch

import aug_ref as AR
import blit_cases as C
import blit_ref as Bl
import golden_util as gu
from aug_gpu_util import dev_state, dparams, load_ada, make_sg, mid_dis, small_dis
from gpu_util import DEV, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

FULL = C.FULL
OPT = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
f32 = np.float32
EDGE = f32(Bl.EDGE)
BIG_KIMG = 1e9                                   # p does not move within a test
GUARD = 64                                       # floats around y (a multiple of 4: y keeps its 16-byte alignment)
SENTINEL = 12345.5
MODES = ((False, True), (False, False), (True, False))                     # (adjoint, with_bias)


def run_blit(xd, ud, bitsd, policy, adjoint, with_bias):
    """sgx_diffaug_blit into a buffer with guard floats on both sides of y; -> (y (a copy), the note names of the launches), the
    guards checked.  ``ud`` may be rows of a wider tensor."""
    from stylegan.pytorch_amd import native as N
    B, H, W, _ = xd.shape
    n = xd.numel()
    off = (xd.data_ptr() // 4) % 4                                          # y gets x's alignment
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=DEV)
    y = buf[GUARD + off:GUARD + off + n].view(B, H, W, 3)
    L = N.lib()
    nb = L.sgx_diffaug_ws_bytes(B, H, W)
    ws = N.workspace(nb, xd.device)
    N.prof_start(1)
    try:
        rc = L.sgx_diffaug_blit(N.ptr(xd), N.ptr(y), ud.data_ptr(), ud.stride(0), None if bitsd is None else N.ptr(bitsd), B, H, W, policy,
                                int(adjoint), int(with_bias), N.ptr(ws), nb, N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    notes = [r[4].split(" ")[0] for r in N.prof_records()]
    N.check(rc, "sgx_diffaug_blit")
    AR.assert_recorded_is_planned(N, AR.BLIT, xd, y, policy, adjoint, with_bias)        # kernels, template arguments, grids: sgx_aug_plan's
    assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + n:] == SENTINEL).all()), "guard floats were written"
    return y.clone(), notes


def on_device(t, off):
    buf = torch.zeros(t.numel() + off, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t.to(DEV))
    return v


def expected_notes(policy, H, W, off):
    vec = W % 4 == 0 and off == 0
    apply_ = "diffaug_blit_tile" if vec and policy & Bl.ROT90 else ("diffaug_blit_row" if vec else "diffaug_blit_px")
    return (["diffaug_blit_sum"] if policy & Bl.COLOR else []) + [apply_]


def check_against_reference(y, x, u, img_bits, adjoint, with_bias, what):
    """Per image: without the colour bit gathers and zeros, bit-exact against the fp32 reference; with it the bound of
    tests/test_gpu_diffaug.py (1e-5 of the largest reference value) against the fp64 reference."""
    x_nchw = x.permute(0, 3, 1, 2)
    ref64 = Bl.apply_gated(x_nchw.double(), u, img_bits, adjoint, with_bias).permute(0, 2, 3, 1)
    ref32 = Bl.apply_gated(x_nchw, u, img_bits, adjoint, with_bias).permute(0, 2, 3, 1)
    yc = y.cpu()
    for b, bits in enumerate(img_bits):
        if bits & Bl.COLOR:
            err = float((yc[b].double() - ref64[b]).abs().max())
            print(what, b, bits, "err", err, "bound", 1e-5 * float(ref64.abs().max()))
            assert err <= 1e-5 * float(ref64.abs().max()) + 1e-30, (what, b, bits, err)
        else:
            assert torch.equal(yc[b], ref32[b]), (what, b, bits)


# ------------------------------------------------------------------------------------------------- 1. the kernels, every launch path
# (H, W, base offset in floats, policies): the smallest; the vector paths; a multiple of 4 that overhangs the 32 x 32 tile; two sum
# partials per image (132 * 132 > 16384 pixels) with an overhang; the per-pixel path (an odd size, an unaligned base); not square
# (xflip without rot90)
SQUARE = (31, 30, 24, 25, 8, 16)
KERNEL_SHAPES = [(8, 8, 0, SQUARE), (16, 16, 0, SQUARE), (36, 36, 0, SQUARE), (132, 132, 0, (31, 30)), (7, 7, 0, SQUARE),
                 (16, 16, 1, SQUARE), (5, 7, 0, (15, 14, 8, 9)), (9, 12, 0, (15, 14, 8, 9))]
MIXED = (31, 0, 7, 24, 17, 10, 29, 22)                                      # per-image gates: every op on and off somewhere


@pytest.mark.parametrize("H,W,off,policies", KERNEL_SHAPES)
def test_kernel_vs_restatement(H, W, off, policies):
    B = 8
    g = torch.Generator().manual_seed(H * 1000 + W + off)
    x = torch.randn(B, H, W, 3, generator=g)
    gy = torch.randn(B, H, W, 3, generator=g)
    u = Bl.edge_draws9(B, seed=H + W)
    assert {(p["f"], p["k"]) for p in (Bl.params9(u[b], 8, 8, Bl.ALL) for b in range(B))} == set(itertools.product((0, 1), range(4)))
    xd, gd = on_device(x, off), on_device(gy, off)
    assert (xd.data_ptr() % 16 == 0) == (off == 0)
    ud = torch.from_numpy(u).to(DEV)
    wide = torch.rand(B, 14, device=DEV)                                    # the same draws as rows of a [B,14] tensor
    wide[:, :9] = ud
    for policy in policies:
        for adjoint, with_bias in MODES:
            src, host = (gd, gy) if adjoint else (xd, x)
            y, notes = run_blit(src, ud, None, policy, adjoint, with_bias)
            assert notes == expected_notes(policy, H, W, off), (policy, notes)
            check_against_reference(y, host, u, [policy] * B, adjoint, with_bias, ("ungated", policy, adjoint, with_bias))
            y2, _ = run_blit(src, wide[:, :9], None, policy, adjoint, with_bias)
            assert torch.equal(y, y2), (policy, adjoint, with_bias)         # the row stride; and bit-reproducible
        ax = run_blit(xd, ud, None, policy, False, False)[0].double().cpu()
        aty = run_blit(gd, ud, None, policy, True, False)[0].double().cpu()
        lhs, rhs = float((ax * gy.double()).sum()), float((x.double() * aty).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((ax * gy.double()).abs().sum()), (policy, lhs, rhs)     # <A x, g> = <x, A^T g>
    union = policies[0]
    img_bits = [union & m for m in MIXED]
    bd = torch.tensor(img_bits, dtype=torch.int32, device=DEV)
    for adjoint, with_bias in MODES:
        src, host = (gd, gy) if adjoint else (xd, x)
        y, notes = run_blit(src, ud, bd, union, adjoint, with_bias)
        assert notes == expected_notes(union, H, W, off), notes
        check_against_reference(y, host, u, img_bits, adjoint, with_bias, ("gated", adjoint, with_bias))
        assert torch.equal(y[1], src[1])                                    # bits 0: a copy
        from stylegan.pytorch_amd import functional as F
        assert torch.equal(y, F._diffaug(src, wide[:, :9], union, adjoint, with_bias, bd))               # the autograd functions' path


# ------------------------------------------------------------------------------------------ 2. continuity with the three-op kernels
@pytest.mark.parametrize("N_", [16, 132])
def test_identity_orientation_is_todays_kernels_bit_for_bit(N_):
    from stylegan.pytorch_amd import functional as F
    B = 8
    g = torch.Generator().manual_seed(N_)
    xd = torch.randn(B, N_, N_, 3, generator=g).to(DEV)
    u = Bl.edge_draws9(B, seed=N_)
    u0 = u.copy()
    u0[:, 7:] = 0
    u0d, ud = torch.from_numpy(u0).to(DEV), torch.from_numpy(u).to(DEV)
    u7 = u0d[:, :7].contiguous()
    for adjoint, with_bias in MODES:
        y, notes = run_blit(xd, u0d, None, 31, adjoint, with_bias)
        assert notes == ["diffaug_blit_sum", "diffaug_blit_tile"]
        assert torch.equal(y, F._diffaug(xd, u7, 7, adjoint, with_bias)), (adjoint, with_bias)
        y, _ = run_blit(xd, u0d, None, 15, adjoint, with_bias)              # the row path
        assert torch.equal(y, F._diffaug(xd, u7, 7, adjoint, with_bias)), (adjoint, with_bias)
        # gated: the two new bits off for every image, their uniforms anything
        bits = torch.tensor(list(range(8)), dtype=torch.int32, device=DEV)
        y, _ = run_blit(xd, ud, bits, 31, adjoint, with_bias)
        assert torch.equal(y, F._diffaug(xd, u7, 7, adjoint, with_bias, bits)), (adjoint, with_bias)


# ----------------------------------------------------------------------------------------------------------- 3. reproducibility
def test_two_runs_are_bit_identical():
    B, N_ = 8, 132
    g = torch.Generator().manual_seed(7)
    xd = torch.randn(B, N_, N_, 3, generator=g).to(DEV)
    ud = torch.from_numpy(Bl.edge_draws9(B, seed=9)).to(DEV)
    bd = torch.tensor(MIXED, dtype=torch.int32, device=DEV)
    for adjoint, with_bias in MODES:
        for bits in (None, bd):
            a, _ = run_blit(xd, ud, bits, 31, adjoint, with_bias)
            b, _ = run_blit(xd, ud, bits, 31, adjoint, with_bias)
            assert torch.equal(a, b), (adjoint, with_bias)


# ---------------------------------------------------------------------------------------------------------------- 4. rejections
def test_rejections_leave_the_output_alone():
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    B = 2

    def call(H, W, policy, stride=9, same=False, old=False):
        x = torch.randn(B, H, W, 3, device=DEV)
        y = x if same else torch.full((B, H, W, 3), SENTINEL, device=DEV)
        keep = y.clone()
        u = torch.rand(B, max(stride, 9), device=DEV)
        nb = L.sgx_diffaug_ws_bytes(B, H, W)
        ws = N.workspace(nb, x.device)
        N.prof_start(1)
        try:
            if old:
                rc = L.sgx_diffaug(N.ptr(x), N.ptr(y), N.ptr(u[:, :7].contiguous()), B, H, W, policy, 0, 1, N.ptr(ws), nb, N.stream())
            else:
                rc = L.sgx_diffaug_blit(N.ptr(x), N.ptr(y), N.ptr(u), stride, None, B, H, W, policy, 0, 1, N.ptr(ws), nb, N.stream())
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], "a kernel was launched"
        assert torch.equal(y, keep)
        return rc
    assert call(8, 12, 16) != 0                                            # rot90 with H != W
    assert call(8, 12, 31) != 0
    assert call(8, 8, 31, same=True) != 0                                   # in place
    assert call(8, 8, 31, stride=8) != 0 and call(8, 8, 8, stride=7) != 0   # rows too close
    assert call(8, 8, 32) != 0 and call(8, 8, 63) != 0 and call(8, 8, -1) != 0
    assert call(8, 8, 8, old=True) != 0 and call(8, 8, 16, old=True) != 0 and call(8, 8, 31, old=True) != 0    # the old entry: bits <= 7


def test_python_entry_rejects_wrong_widths():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    x = torch.randn(2, 8, 8, 3, device=DEV)
    with pytest.raises(N.SgxError):
        F._diffaug(x, torch.rand(2, 7, device=DEV), 8, False, True)
    with pytest.raises(N.SgxError):
        F._diffaug(x, torch.rand(2, 9, device=DEV), 7, False, True)
    with pytest.raises(N.SgxError):
        F._diffaug(torch.randn(2, 8, 12, 3, device=DEV), torch.rand(2, 9, device=DEV), 16, False, True)
    dis = small_dis(diffaug_policy=FULL, ada_target=0.6)
    dis.train()
    img = torch.randn(2, 8, 8, 3, device=DEV)
    dis.diffaug_override = torch.rand(2, 7, device=DEV)
    with pytest.raises(ValueError, match="diffaug_override"):
        dis._diffaug(img)
    dis.diffaug_override, dis.ada_gate_override = torch.rand(2, 9, device=DEV), torch.rand(2, 3, device=DEV)
    with pytest.raises(ValueError, match="ada_gate_override"):
        dis._diffaug(img)


# ----------------------------------------------------------------------------------------------------------------- 5. the gates
@pytest.mark.parametrize("B", [1, 7, 1000])
def test_gates_n_kernel_vs_restatement(B):
    from stylegan.pytorch_amd import functional as F
    rng = np.random.default_rng(B)
    for p in (f32(0), f32(0.3), f32(1)):
        g_ = rng.random((B, 5), dtype=f32)
        flat = g_.reshape(-1)
        for k, v in enumerate((f32(0), EDGE, p, p)):                        # the edges of [0,1) and values equal to p
            flat[(k * 3) % flat.size] = v
        state = dev_state(p)
        wide = torch.rand(B, 14, device=DEV)
        wide[:, 9:] = torch.from_numpy(g_).to(DEV)
        for bits in (31, 24, 8, 16, 7, 21, 1):
            out = F.ada_gates_n(torch.from_numpy(g_).to(DEV), state, bits)
            assert out.dtype == torch.int32 and tuple(out.shape) == (B,)
            assert np.array_equal(out.cpu().numpy(), Bl.gates_n(g_, p, bits)), (float(p), bits)
            assert torch.equal(out, F.ada_gates_n(wide[:, 9:], state, bits))                             # rows of the [B,14] draw
        uniforms = torch.from_numpy(np.minimum(g_, EDGE)).to(DEV)
        if p == 0:
            assert int(F.ada_gates_n(uniforms, state, 31).abs().sum()) == 0
        if p == 1:
            assert bool((F.ada_gates_n(uniforms, state, 31) == 31).all())


# ------------------------------------------------------------------------------------------------------------------ 6. autograd
def test_first_and_second_order_through_the_functions():
    """(y . w).sum() and the R1-shaped grad(...).pow(2).sum() through DiffAugFn at the full policy against torch autograd on the fp64
    restatement.  Bounds: one pass carries the kernels' 1e-5 of the largest value (tests/test_gpu_diffaug.py); the second-order
    result is two passes, the first one's error amplified by at most |L| <= c s <= 1.5 * 2 = 3 in the second: (1 + 3) * 1e-5."""
    from stylegan.pytorch_amd import functional as F
    B, N_ = 4, 16
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N_, N_, 3, generator=g)
    w = torch.randn(B, N_, N_, 3, generator=g)
    u = Bl.edge_draws9(8, seed=5)[[1, 2, 5, 7]]                             # f, k = (1,0), (0,1), (1,2), (1,3)
    ud = torch.from_numpy(u).to(DEV)

    def run(apply_, x_, w_):
        y = apply_(x_)
        loss = (y * w_).sum()
        gx, = torch.autograd.grad(loss, x_, create_graph=True)
        r1 = gx.pow(2).sum()
        gw, = torch.autograd.grad(r1, w_)
        return y.detach(), gx.detach(), gw.detach()
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y, gx, gw = run(lambda t: F.call(F.DiffAugFn, t, ud, 31), xd, wd)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ry, rgx, rgw = run(lambda t: Bl.apply(t.permute(0, 3, 1, 2), u, 31).permute(0, 2, 3, 1), x64, w64)
    for name, a, b, k in (("y", y, ry, 1), ("dx", gx, rgx, 1), ("d2w", gw, rgw, 4)):
        err = float((a.double().cpu() - b).abs().max())
        print(name, "err", err, "bound", k * 1e-5 * float(b.abs().max()))
        assert err <= k * 1e-5 * float(b.abs().max()), (name, err)
    # the D step's fakes: no input gradient is asked for, none is computed
    ctx = types.SimpleNamespace(needs_input_grad=(False, False, False, False), saved_tensors=(ud, None), bits=31)
    assert F.DiffAugFn.backward(ctx, wd.detach()) == (None, None, None, None)
    assert not F.call(F.DiffAugFn, x.to(DEV), ud, 31).requires_grad


# ------------------------------------------------------------------------------------------------------------------- 7. network
def patch_oracle(monkeypatch, u, img_bits):
    """Every oracle D evaluation sees the per-image restatement with the draws ``u`` and the bits the gates must give."""
    orig = O.discriminator

    def discriminator(p, img, depth, alpha, total_depth, **kw):
        return orig(p, Bl.apply_gated(img, u, img_bits), depth, alpha, total_depth, **kw)
    monkeypatch.setattr(O, "discriminator", discriminator)


@pytest.mark.parametrize("depth,alpha", [(5, 0.5), (3, 0.3)])
def test_network_first_and_second_order_vs_oracle(monkeypatch, dparams, depth, alpha):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss under the full policy with per-image gates (p = 0.5
    against pinned uniforms); tolerances of tests/test_gpu_ada.py."""
    from stylegan.pytorch_amd import Losses
    B, res = C.NET_B, 4 * 2 ** depth
    dp = dparams
    dis = load_ada(mid_dis(FULL, ada_target=0.6, ada_p_init=C.NET_P, ada_kimg=BIG_KIMG), dp)
    dis.train()
    u, gates_, bits = C.network_draws(depth)
    ks = [Bl.params9(u[b], res, res, bits[b])["k"] for b in range(B)]
    assert any(b & Bl.ROT90 and k & 1 for b, k in zip(bits, ks)) and any(not b & Bl.ROT90 for b in bits), (bits, ks)      # mixed
    assert len(set(bits)) >= 3 and any(b & 1 for b in bits) and any(not b & 1 for b in bits), bits
    dis.diffaug_override, dis.ada_gate_override = torch.from_numpy(u).to(DEV), gates_.to(DEV)
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
    assert dis._ada_real is not None and dis.ada_p == C.NET_P


# ------------------------------------------------------------------------------------------------------ 8. graph replay, moving p
def train_run(use_graphs, iters=4, seed=5):
    # 1 / (0.02 * 1000) = 0.05 per image: one update (interval 1) at batch 4 moves p by 0.2
    sg = make_sg(FULL, use_graphs, ada_target=0.6, ada_interval=1, ada_kimg=0.02, ada_p_init=0.5)
    gp, dp = mid_params(torch.float64)
    load_into(sg.gen, gp); load_ada(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, mid_noises(4))
    sg.dis.diffaug_override = torch.from_numpy(Bl.edge_draws9(8, seed=3)[[0, 3, 4, 7]]).to(DEV)
    sg.dis.ada_gate_override = C.spread_gates5(4).to(DEV)
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
        assert torch.equal(a, b), (i, a, b)
    assert [float(s[5]) for s in se] == [1.0, 2.0, 3.0, 4.0]
    losses_agree(le, lg)


# ------------------------------------------------------------------------------------------------------------ 9. draw consumption
@pytest.mark.parametrize("ada", [False, True])
def test_training_forward_draws_nine_or_fourteen(dparams, ada):
    B = 4
    kw = dict(ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG) if ada else {}
    on = load_ada(mid_dis(FULL, **kw), dparams)
    plain = load_into(mid_dis(""), dparams)
    on.train(); plain.train()
    x = gu.seeded((B, 3, 128, 128), 29).to(DEV)
    torch.cuda.manual_seed(123)
    with torch.no_grad():
        a = on(x, 5, 0.5)
    s_on = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(123)
    r = torch.rand(B, 14 if ada else 9, device=DEV)
    with torch.no_grad():
        plain(x, 5, 0.5)
    assert torch.equal(s_on, torch.cuda.get_rng_state())
    on.diffaug_override = r[:, :9]
    if ada:
        on.ada_gate_override = r[:, 9:]
    with torch.no_grad():
        assert torch.equal(a, on(x, 5, 0.5))
    assert ("ada_state" in on.state_dict()) == ada


# ------------------------------------------------------------------------------------------------------ 10. fresh-draw statistics
def test_fresh_orientations_are_uniform():
    B, N_ = 4096, 8
    dis = small_dis(diffaug_policy="xflip,rot90")
    dis.train()
    marker = torch.zeros(3, N_, N_)
    marker[:, 0, 0], marker[:, 0, 1], marker[1, 2, 5] = 1.0, 2.0, 3.0       # no symmetry: the eight orientations differ
    table = torch.stack([Bl.orient(marker, f, k) for f, k in itertools.product((0, 1), range(4))]).permute(0, 2, 3, 1)
    assert len({tuple(t.reshape(-1).tolist()) for t in table}) == 8
    torch.cuda.manual_seed(11)
    with torch.no_grad():
        y = dis._diffaug(marker.permute(1, 2, 0).expand(B, N_, N_, 3).contiguous().to(DEV))
    match = (y.reshape(B, 1, -1) == table.to(DEV).reshape(1, 8, -1)).all(dim=2)                           # [B, 8]
    assert bool((match.sum(dim=1) == 1).all())
    counts = match.sum(dim=0).cpu().tolist()
    sigma = (B * (1 / 8) * (7 / 8)) ** 0.5
    print("counts", counts, "sigma", sigma)
    assert all(abs(c - B / 8) <= 5 * sigma for c in counts), counts
