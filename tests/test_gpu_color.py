"""-m gpu: ADA's colour group -- brightness, contrast, lumaflip, hue, saturation composed into one affine map y = M x + t of the RGB
vector per image and applied last by one streaming pass (csrc/adacolor.hip: sgx_ada_color_matrix, sgx_ada_color;
functional.ada_color_matrix / AdaColorFn / AdaColorAdjFn / AdaColorLinFn; Discriminator(diffaug_policy="...,brightness,...")) against
the restatements in tests/color_ref.py: the table kernel, the three passes on both launch paths bit for bit, the copy branch, the
transpose property on the device, continuity with the policies of today, D with its R1 double backward under mixed per-image gates,
graph replay with a moving p, and the rejections."""
import random
import types

import numpy as np
import pytest
import torch

import aug_ref as AR
import blit_ref as Bl
import color_cases as CC
import color_ref as K
import geom_cases as GC
import geom_ref as G
import golden_util as gu
from aug_gpu_util import bits_equal, dev_state, dparams, load_ada, make_sg, mid_dis, nchw, nhwc, on_device, recorded, small_dis
from gpu_util import DEV, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

OPT = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
f32 = np.float32
BIG_KIMG = 1e9                                   # p does not move within a test
GUARD = 64                                       # floats around y (a multiple of 4: y keeps its 16-byte alignment)
SENTINEL = 12345.5
EPS = 2.0 ** -24
# Entries of the device's fp32 table against the fp64 restatement over the draws of test_matrix_kernel_vs_restatement, the
# hue,saturation rows at the clamp included (entries of up to c s = 2^4.5 = 22.6, whose ulp is 1.9e-6).  The inputs of an entry are logf /
# cosf / sinf / exp2f results of an ulp or two, theta itself is rounded to fp32, and five roundings follow; the largest error measured
# on the MI355X over these draws is MATRIX_ERR_MEASURED, the bound four times that.
MATRIX_ERR_MEASURED = 9.88e-7
MATRIX_TOL = 4 * MATRIX_ERR_MEASURED
assert MATRIX_TOL <= 1e-5
MATRIX_B = 10                                    # the eight pinned rows of edge_draws8 and two random ones


def run_color(xd, matd, adjoint, with_bias):
    """sgx_ada_color into a buffer with guard floats on both sides of y; -> (y (a copy), the note names of the launches), the guards
    checked."""
    from stylegan.pytorch_amd import native as N
    B, H, W, _ = xd.shape
    n = xd.numel()
    off = (xd.data_ptr() // 4) % 4                                          # y gets x's alignment
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=DEV)
    y = buf[GUARD + off:GUARD + off + n].view(B, H, W, 3)
    L = N.lib()
    N.prof_start(1)
    try:
        rc = L.sgx_ada_color(N.ptr(xd), N.ptr(y), N.ptr(matd), B, H, W, int(adjoint), int(with_bias), N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    notes = [r[4].split(" ")[0] for r in N.prof_records()]
    N.check(rc, "sgx_ada_color")
    AR.assert_recorded_is_planned(N, AR.COLOR, xd, y, 0, adjoint, with_bias)            # kernel, template arguments, grid: sgx_aug_plan's
    assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + n:] == SENTINEL).all()), "guard floats were written"
    return y.clone(), notes


PASSES = (("fwd", False, True), ("lin", False, False), ("adj", True, False))


def expected_note(H, W, off):
    return "ada_color_vec" if (H * W) % 4 == 0 and off == 0 else "ada_color_px"


def mixed_table(seed=0):
    """The device's own table for a batch of five: rows 1 and 3 gated off (identity rows), rows 0, 2, 4 the upper clamp with a flip at
    theta = -pi, the lower clamp, and a flip at theta = +pi/2 with random variates."""
    from stylegan.pytorch_amd import functional as F
    u = K.edge_draws8(MATRIX_B, seed)[[0, 7, 1, 8, 3]]
    gates = np.full((5, 5), 0.25, f32)
    gates[1] = gates[3] = 0.75
    mat = F.ada_color_matrix(torch.from_numpy(u).to(DEV), K.ALL, torch.from_numpy(gates).to(DEV), dev_state(0.5))
    rows = mat.cpu().numpy()
    assert [K.is_identity(r) for r in rows] == [False, True, False, True, False]
    return mat, rows


# --------------------------------------------------------------------------------------------------------- 1. the table kernel
def test_matrix_kernel_vs_restatement():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B = MATRIX_B
    u = K.edge_draws8(B, seed=3)
    ud = torch.from_numpy(u).to(DEV)
    gates = GC.C.spread_gates5(B).numpy().copy()
    gates[5], gates[6] = (0.5, 0.5, 0.5, 0.5, 0.5), (0.0, float(K.EDGE), 0.5, float(K.BELOW_HALF), 0.25)   # values equal to p = 0.5 (strict <)
    gates[9] = 0.9                                                            # one row off whatever else is drawn
    gd = torch.from_numpy(gates).to(DEV)
    wide = torch.rand(B, 13, device=DEV)                                    # the same draws and gates as rows of one [B,13] tensor
    wide[:, :8], wide[:, 8:] = ud, gd
    worst = 0.0

    def check(mat, bits, what):
        nonlocal worst
        ref = K.matrices(u, bits)
        got = mat.cpu().numpy()
        assert got.dtype == f32 and got.shape == (B, 12)
        for b in range(B):
            M = got[b, :9].reshape(3, 3)
            if not bits[b] & K.ALL:
                assert tuple(got[b].tolist()) == K.IDENTITY and not np.signbit(got[b]).any(), (what, b, got[b])      # the flag
                continue
            if K.is_diagonal_case(u[b], bits[b]):                             # c on the diagonal, +0 off it, bit for bit
                off_diag = M[~np.eye(3, dtype=bool)]
                assert (off_diag == 0).all() and not np.signbit(off_diag).any() and M[0, 0] == M[1, 1] == M[2, 2], (what, b, M)
                if not bits[b] & K.CONTRAST:
                    assert M[0, 0] == 1.0
            if not bits[b] & K.HUE:                                           # theta = 0: symmetric in its off-diagonals, bit for bit
                assert M[0, 1] == M[0, 2], (what, b, M)
            assert M[0, 0] == M[1, 1] == M[2, 2] and M[0, 1] == M[1, 2] == M[2, 0] and M[0, 2] == M[1, 0] == M[2, 1]
            assert got[b, 9] == got[b, 10] == got[b, 11]
            err = float(np.abs(got[b].astype(np.float64) - ref[b]).max())
            worst = max(worst, err)
            assert err <= MATRIX_TOL, (what, b, err, got[b], ref[b])
    policies = [K.ALL, K.HUE | K.SATURATION] + list(K.OP_BITS) + [K.BRIGHTNESS | K.CONTRAST, K.LUMAFLIP | K.CONTRAST, K.CONTRAST | K.HUE]
    for policy in policies:
        N.prof_start(1)
        try:
            mat = F.ada_color_matrix(ud, policy)
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert [r[4].split(" ")[0] for r in N.prof_records()] == ["ada_color_matrix"]
        check(mat, [policy] * B, ("ungated", policy))
        assert torch.equal(mat, F.ada_color_matrix(wide[:, :8], policy))      # the row stride; and bit-reproducible
        for p in (0.0, 0.5, 1.0):
            bits = K.gates(gates, p, policy)
            mat = F.ada_color_matrix(ud, policy, gd, dev_state(p))
            check(mat, bits, ("gated", policy, p))
            assert torch.equal(mat, F.ada_color_matrix(wide[:, :8], policy, wide[:, 8:], dev_state(p)))
            if p == 0.0:
                assert not bits.any()
            if p == 1.0:
                assert (bits == policy).all()
    only_flip = F.ada_color_matrix(ud, K.LUMAFLIP).cpu().numpy()[0, :9].reshape(3, 3)                   # row 0: lumaflip on and drawn
    assert np.array_equal(only_flip, only_flip.T) and only_flip[0, 0] > 0 > only_flip[0, 1]
    assert F.ada_color_matrix(ud, 0).cpu().numpy().tolist() == [list(K.IDENTITY)] * B                   # no colour op in the policy
    assert F.ada_color_matrix(ud, 255).cpu().numpy().tolist() == [list(K.IDENTITY)] * B                 # the other stages' bits
    print("matrix kernel: largest |entry - fp64| =", worst, "bound", MATRIX_TOL)


# -------------------------------------------------------------------------------------- 2. the three passes, on both launch paths
SHAPES = [(1, 1), (1, 4), (2, 2), (5, 7), (4, 257), (33, 31), (64, 64)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("H,W", SHAPES)
def test_passes_vs_restatement_bit_for_bit(H, W, off):
    B = 5
    g = torch.Generator().manual_seed(H * 1000 + W + off)
    x = torch.randn(B, H, W, 3, generator=g)
    xd = on_device(x, off)
    assert (xd.data_ptr() % 16 == 0) == (off == 0)
    matd, mat = mixed_table(seed=H + W)
    x64 = nchw(x).double()
    for name, adjoint, bias in PASSES:
        y, notes = run_color(xd, matd, adjoint, bias)
        assert notes == [expected_note(H, W, off)], notes
        if off == 1:
            assert notes == ["ada_color_px"]
        want = torch.from_numpy(K.apply32(x.numpy(), mat, adjoint, bias))
        assert bits_equal(y, want), (name, float((y.cpu() - want).abs().max()))
        # and against fp64 under the same table: |y - y64| <= 10 2^-24 (sum |M x| + |t|) per element
        ref = nhwc(K.apply(x64, mat, adjoint, bias))
        mag = nhwc(K.apply(x64.abs(), np.abs(mat), adjoint, bias))
        err = (y.cpu().double() - ref).abs()
        print(name, "largest err / bound", float((err / (10 * EPS * mag).clamp_min(1e-300)).max()))
        assert bool((err <= 10 * EPS * mag).all()), (name, float((err - 10 * EPS * mag).max()))
        for b in (1, 3):
            assert bits_equal(y[b], x[b])                                     # the identity rows


# ------------------------------------------------------------------------------------------------------ 3. identity rows copy
@pytest.mark.parametrize("off", [0, 1])
def test_identity_rows_copy_special_values(off):
    B, H, W = 2, 2, 4
    # -0, +inf, -inf, quiet NaNs with payloads of either sign, a signalling NaN, the smallest denormals
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001, 0x7f800123, 0x00000001, 0x80000001], np.uint32)
    words = torch.from_numpy(np.resize(special, B * H * W * 3).view(np.int32).copy())
    buf = torch.zeros(words.numel() + off, dtype=torch.int32, device=DEV)
    buf[off:] = words.to(DEV)
    xd = buf[off:].view(torch.float32).view(B, H, W, 3)
    assert torch.equal(xd.view(torch.int32).cpu().reshape(-1), words)
    matd = torch.tensor([K.IDENTITY] * B, dtype=torch.float32, device=DEV)
    for name, adjoint, bias in PASSES:
        y, notes = run_color(xd, matd, adjoint, bias)
        assert notes == ["ada_color_vec" if off == 0 else "ada_color_px"]
        assert torch.equal(y.view(torch.int32).cpu().reshape(-1), words), name


# ------------------------------------------------------------------------------------------ 4. the transpose property, on the device
@pytest.mark.parametrize("off", [0, 1])
def test_forward_column_is_adjoint_row_bit_for_bit(off):
    """One-hot RGB inputs at 2x2: pixel q of the linear pass holds column q of M, pixel q of the adjoint row q of M^T... the same fp32
    numbers, and they are the table's."""
    from stylegan.pytorch_amd import functional as F
    B = MATRIX_B
    matd = F.ada_color_matrix(torch.from_numpy(K.edge_draws8(B, seed=11)).to(DEV), K.ALL)
    mat = matd.cpu().numpy()
    onehot = torch.zeros(B, 2, 2, 3)
    for q in range(3):
        onehot[:, q // 2, q % 2, q] = 1.0
    xd = on_device(onehot, off)
    lin, notes = run_color(xd, matd, False, False)                              # lin[b, q, k] = M[k, q]
    adj, _ = run_color(xd, matd, True, False)                                   # adj[b, q, k] = M[q, k]
    assert notes == [expected_note(2, 2, off)]
    lin, adj = lin.cpu().reshape(B, 4, 3)[:, :3], adj.cpu().reshape(B, 4, 3)[:, :3]
    assert bits_equal(lin.transpose(1, 2), adj)
    assert np.array_equal(adj.numpy().reshape(B, 9), mat[:, :9])


# ------------------------------------------------------------------------------------------------------------- 5. continuity
def test_old_policies_launch_what_they_launched():
    from stylegan.pytorch_amd import functional as F
    B = 8
    img = torch.randn(B, 16, 16, 3, device=DEV)
    u9 = torch.from_numpy(Bl.edge_draws9(B, seed=2)).to(DEV)
    u5 = torch.from_numpy(G.edge_draws5(B, seed=2)).to(DEV)
    dis = small_dis(diffaug_policy=GC.FULL8)
    dis.train()
    dis.diffaug_override, dis.geom_override = u9, u5
    y, notes = recorded(lambda: dis._diffaug(img))
    assert notes[-2:] == ["ada_geom_matrix", "ada_geom_tile"] and not any(n.startswith("ada_color") for n in notes), notes
    assert torch.equal(y, F.call(F.AdaGeomFn, F.call(F.DiffAugFn, img, u9, 31), F.ada_geom_matrix(u5, 224)))
    two = small_dis(diffaug_policy="color,cutout")
    two.train()
    two.diffaug_override = u9[:, :7].contiguous()
    y, notes = recorded(lambda: two._diffaug(img))
    assert notes == ["diffaug_sum", "diffaug"], notes
    assert torch.equal(y, F.call(F.DiffAugFn, img, u9[:, :7].contiguous(), 5))


@pytest.mark.parametrize("base", [GC.FULL8, "color,cutout", ""])
def test_new_ops_at_p_zero_change_nothing(base):
    B = 8
    img = torch.randn(B, 16, 16, 3, device=DEV)
    policy13 = (base + "," if base else "") + ",".join(K.OPS)
    ada = dict(ada_target=0.6, ada_p_init=0.0, ada_kimg=BIG_KIMG)
    with13 = small_dis(diffaug_policy=policy13, **ada)
    with13.train()
    width = 9 if "xflip" in base else 7
    u = torch.from_numpy(Bl.edge_draws9(B, seed=4)).to(DEV)[:, :width].contiguous()
    gates_ = torch.rand(B, 5 if width == 9 else 3, device=DEV)
    u5, gates3 = torch.from_numpy(G.edge_draws5(B)).to(DEV), torch.rand(B, 3, device=DEV)

    def pin(dis):
        dis.diffaug_override, dis.ada_gate_override, dis.geom_override, dis.geom_gate_override = u, gates_, u5, gates3
    pin(with13)
    with13.color_override, with13.color_gate_override = torch.from_numpy(K.edge_draws8(B)).to(DEV), torch.rand(B, 5, device=DEV)
    y13, notes = recorded(lambda: with13._diffaug(img))
    assert notes[-2:] == ["ada_color_matrix", "ada_color_vec"], notes
    if base:
        without = small_dis(diffaug_policy=base, **ada)
        without.train()
        pin(without)
        y, old_notes = recorded(lambda: without._diffaug(img))
        assert torch.equal(y13, y) and notes[:-2] == old_notes
    assert torch.equal(y13, img)                                            # and p = 0 gates every op off: the image itself


def test_training_forward_draws_its_own_eight_or_thirteen():
    B = 4
    img = torch.randn(B, 16, 16, 3, device=DEV)
    for ada in (False, True):
        kw = dict(ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG) if ada else {}
        dis = small_dis(diffaug_policy=CC.FULL13, **kw)
        dis.train()
        torch.cuda.manual_seed(77)
        y = dis._diffaug(img)
        after = torch.cuda.get_rng_state()
        old = small_dis(diffaug_policy=GC.FULL8, **kw)
        old.train()
        torch.cuda.manual_seed(77)
        y8 = old._diffaug(img)                                               # what the eight-op policy draws today, then the stage's own
        r3 = torch.rand(B, 13 if ada else 8, device=DEV)
        assert torch.equal(after, torch.cuda.get_rng_state())
        dis.color_override = r3[:, :8]
        if ada:
            dis.color_gate_override = r3[:, 8:]
        torch.cuda.manual_seed(77)
        assert torch.equal(y, dis._diffaug(img))
        from stylegan.pytorch_amd import functional as F
        mat = F.ada_color_matrix(r3[:, :8], K.ALL, *((r3[:, 8:], dis.ada_state) if ada else ()))
        assert torch.equal(y, F.call(F.AdaColorFn, y8, mat))
        assert ("ada_state" in dis.state_dict()) == ada
    net = mid_dis(CC.FULL13)
    net.eval()
    x = gu.seeded((B, 3, 128, 128), 19).to(DEV)
    before = torch.cuda.get_rng_state()
    with torch.no_grad():
        _, notes = recorded(lambda: net(x, 5, 0.5))
    assert torch.equal(before, torch.cuda.get_rng_state())                   # no draw in eval(), and no augmentation launch
    assert not any(n.startswith(("ada_", "diffaug")) for n in notes)


# ---------------------------------------------------------------------------------------------------------------- 8. autograd
def test_first_and_second_order_through_the_functions():
    """(y . w).sum() and the R1-shaped grad(...).pow(2).sum() through AdaColorFn at 8x8 against torch autograd on the fp64 restatement
    under the device's table.  Bounds: each pass 10 2^-24 sum |M| |input| (+ |t|) on the input that pass was given (read back from the
    device), plus |M| applied to the bound of the pass before."""
    from stylegan.pytorch_amd import functional as F
    B, N_ = 5, 8
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N_, N_, 3, generator=g)
    w = torch.randn(B, N_, N_, 3, generator=g)
    matd, mat = mixed_table(seed=21)
    amat = np.abs(mat)

    def second_order(table):
        xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        y, notes = recorded(lambda: F.call(F.AdaColorFn, xd, table))
        assert notes == ["ada_color_vec"]
        (gx,), notes = recorded(lambda: torch.autograd.grad((y * wd).sum(), xd, create_graph=True))
        assert [n for n in notes if n.startswith("ada_")] == ["ada_color_vec"]
        (gw,), notes = recorded(lambda: torch.autograd.grad(gx.pow(2).sum(), wd))
        assert [n for n in notes if n.startswith("ada_")] == ["ada_color_vec"]
        return y.detach().cpu(), gx.detach().cpu(), gw.cpu()
    y, gx, gw = second_order(matd)

    def M(t, adjoint=False, bias=False, table=mat):
        return nhwc(K.apply(nchw(t), table, adjoint, bias))
    x64, w64 = x.double(), w.double()
    assert bool(((y.double() - M(x64, bias=True)).abs() <= 10 * EPS * M(x64.abs(), bias=True, table=amat)).all())
    e1 = 10 * EPS * M(w64.abs(), True, table=amat)
    assert bool(((gx.double() - M(w64, True)).abs() <= e1).all())
    assert bits_equal(gx, torch.from_numpy(K.apply32(w.numpy(), mat, True, False)))
    v = 2.0 * gx.double()                                                   # what the second pass was given (2 gx is exact in fp32)
    e2 = 10 * EPS * M(v.abs(), table=amat) + M(2.0 * e1, table=amat)
    err = (gw.double() - 2.0 * M(M(w64, True))).abs()
    print("d2w: largest err / bound", float((err / e2.clamp_min(1e-300)).max()))
    assert bool((err <= e2).all())
    assert bits_equal(gw, torch.from_numpy(K.apply32(2 * gx.numpy(), mat, False, False)))
    # the second order may not depend on t
    bumped = matd.clone()
    bumped[:, 9:] += 1.5
    y_b, gx_b, gw_b = second_order(bumped)
    assert not torch.equal(y_b, y) and bits_equal(gx_b, gx) and bits_equal(gw_b, gw)
    # the D step's fakes: no input gradient is asked for, none is computed
    ctx = types.SimpleNamespace(needs_input_grad=(False, False), saved_tensors=(matd,))
    assert F.AdaColorFn.backward(ctx, w.to(DEV)) == (None, None)
    assert not F.call(F.AdaColorFn, x.to(DEV), matd).requires_grad


# ------------------------------------------------------------------------------------------------------------------- 9. network
@pytest.mark.parametrize("depth,alpha", [(5, 0.5), (3, 0.3)])
def test_network_first_and_second_order_vs_oracle(monkeypatch, dparams, depth, alpha):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss under the thirteen-op policy with per-image gates
    (p = 0.5 against pinned uniforms), against the fp64 composition color_ref o geom_ref o blit_ref o the oracle's D; the criterion
    and the tolerances of tests/test_gpu_geom.py's network test.  As there, the reference maps under the tables the device produced,
    which this test first holds against the fp64 matrices to their measured tolerances."""
    from stylegan.pytorch_amd import Losses
    from stylegan.pytorch_amd import functional as F
    from test_gpu_geom import MATRIX_TOL as GEOM_TOL
    B, res = CC.NET_B, 4 * 2 ** depth
    dp = dparams
    dis = load_ada(mid_dis(CC.FULL13, ada_target=0.6, ada_p_init=CC.NET_P, ada_kimg=BIG_KIMG), dp)
    dis.train()
    u9, gates5, bits5 = GC.C.network_draws(depth)
    u5, gates3, bits3 = GC.network_draws(depth)
    u8, cgates, cbits = CC.network_draws(depth)
    for op in K.OP_BITS:
        assert any(b & op for b in cbits) and any(not b & op for b in cbits), cbits                 # mixed
    assert any(b == 0 for b in cbits)
    dis.diffaug_override, dis.ada_gate_override = torch.from_numpy(u9).to(DEV), gates5.to(DEV)
    dis.geom_override, dis.geom_gate_override = torch.from_numpy(u5).to(DEV), gates3.to(DEV)
    dis.color_override, dis.color_gate_override = torch.from_numpy(u8).to(DEV), cgates.to(DEV)
    gmat = F.ada_geom_matrix(dis.geom_override, G.ALL, dis.geom_gate_override, dis.ada_state).cpu().numpy()
    assert float(np.abs(gmat.astype(np.float64) - G.matrices(u5, bits3)).max()) <= GEOM_TOL
    cmat = F.ada_color_matrix(dis.color_override, K.ALL, dis.color_gate_override, dis.ada_state).cpu().numpy()
    mat_err = float(np.abs(cmat.astype(np.float64) - K.matrices(u8, cbits)).max())
    print("table: largest |entry - fp64| =", mat_err, "bound", MATRIX_TOL)
    assert mat_err <= MATRIX_TOL
    orig = O.discriminator

    def discriminator(p, img, depth_, alpha_, total_depth, **kw):
        return orig(p, K.apply(G.apply(Bl.apply_gated(img, u9, bits5), gmat), cmat), depth_, alpha_, total_depth, **kw)
    monkeypatch.setattr(O, "discriminator", discriminator)
    real = gu.seeded((B, 3, res, res), 300 + depth); fake = gu.seeded((B, 3, res, res), 400 + depth)

    score = dis(real.to(DEV), depth, alpha)
    ref = O.discriminator(dp, real.double(), depth, alpha, MID_DEPTH)
    score_err = float((score.detach().double().cpu() - ref.detach()).norm())
    print("score err", score_err, "bound", 2e-5 * float(ref.detach().norm()))
    assert score_err <= 2e-5 * float(ref.detach().norm()), (score, ref)

    loss_fn = Losses.LogisticGAN(dis)
    rd = real.to(DEV).requires_grad_(True)
    r1 = loss_fn._r1_from_logit(dis(rd, depth, alpha), rd)
    r1_ref = O.r1_penalty(dp, real.double(), depth, alpha, MID_DEPTH)
    print("r1", float(r1.detach()), float(r1_ref.detach()))
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
    assert dis._ada_real is not None and dis.ada_p == CC.NET_P


# ------------------------------------------------------------------------------------------------ 10. graph replay, moving p
def train_run(use_graphs, iters=4, seed=5):
    # 1 / (0.02 * 1000) = 0.05 per image: one update (interval 1) at batch 4 moves p by 0.2
    sg = make_sg(CC.FULL13, use_graphs, ada_target=0.6, ada_interval=1, ada_kimg=0.02, ada_p_init=0.5)
    gp, dp = mid_params(torch.float64)
    load_into(sg.gen, gp); load_ada(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, mid_noises(4))
    sg.dis.diffaug_override = torch.from_numpy(Bl.edge_draws9(8, seed=3)[[0, 3, 4, 7]]).to(DEV)
    sg.dis.ada_gate_override = GC.C.spread_gates5(4).to(DEV)
    sg.dis.geom_override = torch.from_numpy(G.edge_draws5(8, seed=3)[[0, 1, 3, 7]]).to(DEV)
    sg.dis.geom_gate_override = GC.spread_gates3(4).to(DEV)
    sg.dis.color_override = torch.from_numpy(K.edge_draws8(10, seed=3)[[3, 5, 6, 9]]).to(DEV)
    sg.dis.color_gate_override = GC.C.spread_gates5(4).to(DEV)
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
    assert len({float(s[0]) for s in se}) > 1                               # p moved between the replays
    losses_agree(le, lg)


# --------------------------------------------------------------------------------------------------------------- 11. rejections
def test_c_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    B, H, W = 2, 8, 8
    x = torch.randn(B, H, W, 3, device=DEV)
    y = torch.full((B, H, W, 3), SENTINEL, device=DEV)
    mat = torch.tensor([K.IDENTITY] * B, dtype=torch.float32, device=DEV) * 2.0
    u, gates_, state = torch.rand(B, 13, device=DEV), torch.rand(B, 5, device=DEV), dev_state(0.5)
    out = torch.full((B, 12), SENTINEL, device=DEV)
    s = N.stream()

    def refused(fn):
        N.prof_start(1)
        try:
            rc = fn()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], "a kernel was launched"
        assert bool((y == SENTINEL).all()) and bool((out == SENTINEL).all())
        return rc != 0
    c = lambda *a: L.sgx_ada_color(*a)
    assert refused(lambda: c(N.ptr(y), N.ptr(y), N.ptr(mat), B, H, W, 0, 1, s))                           # in place
    assert refused(lambda: c(N.ptr(y), N.ptr(y), N.ptr(mat), B, H, W, 1, 0, s))
    assert refused(lambda: c(None, N.ptr(y), N.ptr(mat), B, H, W, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), None, N.ptr(mat), B, H, W, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), None, B, H, W, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), 0, H, W, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), -1, H, W, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, 0, W, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, -3, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, 40000, 40000, 0, 1, s))                   # beyond 2^31 floats per image
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, W, 1, 1, s))                           # the adjoint has no bias
    m = lambda *a: L.sgx_ada_color_matrix(*a)
    assert refused(lambda: m(N.ptr(u), 7, None, 0, None, 7936, N.ptr(out), B, s))                         # rows too close
    assert refused(lambda: m(N.ptr(u), 13, N.ptr(gates_), 4, N.ptr(state), 7936, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 13, N.ptr(gates_), 5, None, 7936, N.ptr(out), B, s))               # gates without the state
    assert refused(lambda: m(N.ptr(u), 13, None, 0, N.ptr(state), 7936, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 13, None, 0, None, 255, N.ptr(out), B, s))                         # bits of the other entries
    assert refused(lambda: m(N.ptr(u), 13, None, 0, None, 8192, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 13, None, 0, None, -1, N.ptr(out), B, s))
    assert refused(lambda: m(None, 13, None, 0, None, 7936, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 13, None, 0, None, 7936, None, B, s))
    assert refused(lambda: m(N.ptr(u), 13, None, 0, None, 7936, N.ptr(out), 0, s))


def test_python_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B = 2
    x = torch.randn(B, 8, 8, 3, device=DEV)
    mat = torch.tensor([K.IDENTITY] * B, dtype=torch.float32, device=DEV) * 2.0
    bad = [lambda: F._ada_color(torch.randn(B, 8, 8, 4, device=DEV), mat, False, True),                   # a 4-channel tensor
           lambda: F._ada_color(x.double(), mat, False, True), lambda: F._ada_color(x[0], mat, False, True),
           lambda: F._ada_color(x, mat[:, :8].contiguous(), False, True), lambda: F._ada_color(x, torch.zeros(B + 1, 12, device=DEV), True, False),
           lambda: F._ada_color(x, mat.double(), False, True), lambda: F._ada_color(x, mat.reshape(-1), False, False),   # the table's shape or dtype
           lambda: F._ada_color(x.cpu(), mat.cpu(), False, True), lambda: F._ada_color(x, mat.cpu(), False, True),       # CPU tensors
           lambda: F._ada_color(x.cpu(), mat, True, False),
           lambda: F._ada_color(x, mat, True, True),                                                       # the adjoint has no bias
           lambda: F.ada_color_matrix(torch.rand(B, 8), 7936),
           lambda: F.ada_color_matrix(torch.rand(B, 5, device=DEV), 7936), lambda: F.ada_color_matrix(torch.rand(B, 8, device=DEV).double(), 7936),
           lambda: F.ada_color_matrix(torch.rand(B, 8, device=DEV), 7936, torch.rand(B, 5, device=DEV)),
           lambda: F.ada_color_matrix(torch.rand(B, 8, device=DEV), 7936, torch.rand(B, 3, device=DEV), dev_state(0.5)),
           lambda: F.ada_color_matrix(torch.rand(B, 8, device=DEV), 7936, torch.rand(B, 5, device=DEV), torch.zeros(8))]
    for k, fn in enumerate(bad):
        N.prof_start(1)
        try:
            with pytest.raises(N.SgxError):
                fn()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], (k, "a kernel was launched")
    dis = small_dis(diffaug_policy=",".join(K.OPS), ada_target=0.6)
    dis.train()
    dis.color_override = torch.rand(B, 7, device=DEV)
    with pytest.raises(ValueError, match="color_override"):
        dis._diffaug(x)
    dis.color_override = torch.rand(B + 1, 8, device=DEV)
    with pytest.raises(ValueError, match="color_override"):
        dis._diffaug(x)
    dis.color_override, dis.color_gate_override = torch.rand(B, 8, device=DEV), torch.rand(B, 3, device=DEV)
    with pytest.raises(ValueError, match="color_gate_override"):
        dis._diffaug(x)
