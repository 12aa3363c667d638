"""-m gpu: ADA's general geometric group -- scale, rotate, aniso composed into one affine map per image and applied by one bilinear
resample (csrc/adageom.hip: sgx_ada_geom_matrix, sgx_ada_geom; functional.ada_geom_matrix / AdaGeomFn / AdaGeomAdjFn;
Discriminator(diffaug_policy="...,scale,rotate,aniso")) against the restatement in tests/geom_ref.py: the matrix kernel, the resample
on every launch path with a per-element bound, exact cases bit for bit, the transpose property on the device, continuity with the
policies of today, D with its R1 double backward under mixed per-image gates, graph replay with a moving p, and the rejections."""
import random
import types

import numpy as np
import pytest
import torch

import aug_ref as AR
import blit_ref as Bl
import geom_cases as GC
import geom_ref as G
import golden_util as gu
from aug_gpu_util import dev_state, dparams, load_ada, make_sg, mid_dis, nchw, nhwc, on_device, recorded, small_dis
from gpu_util import DEV, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

OPT = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
f32 = np.float32
BIG_KIMG = 1e9                                   # p does not move within a test
GUARD = 64                                       # floats around y (a multiple of 4: y keeps its 16-byte alignment)
SENTINEL = 12345.5
EPS = 2.0 ** -24
# Entries of the device's fp32 table against the fp64 restatement over the draws of test_matrix_kernel_vs_restatement.  The inputs of
# an entry are logf / cosf / sinf / exp2f results of a few ulp and theta itself is rounded to fp32 (half an ulp of pi, 1.2e-7, times
# entries of up to 2^1.2); the largest error measured on the MI355X over these draws is MATRIX_ERR_MEASURED, the bound four times that.
MATRIX_ERR_MEASURED = 2.11e-7
MATRIX_TOL = 4 * MATRIX_ERR_MEASURED
assert MATRIX_TOL <= 1e-5


def run_geom(xd, matd, adjoint):
    """sgx_ada_geom into a buffer with guard floats on both sides of y; -> (y (a copy), the note names of the launches), the guards
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
        rc = L.sgx_ada_geom(N.ptr(xd), N.ptr(y), N.ptr(matd), B, H, W, int(adjoint), N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    notes = [r[4].split(" ")[0] for r in N.prof_records()]
    N.check(rc, "sgx_ada_geom")
    AR.assert_recorded_is_planned(N, AR.GEOM, xd, y, 0, adjoint)                        # kernel, template argument, grid: sgx_aug_plan's
    assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + n:] == SENTINEL).all()), "guard floats were written"
    return y.clone(), notes


def expected_note(W, off):
    return "ada_geom_tile" if W % 4 == 0 and off == 0 else "ada_geom_px"


def rot(deg):
    t = np.deg2rad(deg)
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


def row_from_t(T):
    """A test-supplied table row from T (2x2, fp64): both halves rounded to fp32."""
    T = np.asarray(T, np.float64)
    return np.concatenate([np.linalg.inv(T).reshape(-1), T.reshape(-1)]).astype(f32)


BIG, SMALL = 2.0 ** 0.6, 2.0 ** -0.6
# mixed identity and other rows: the largest magnification the clamp allows (s = a = 2^0.6: T = Rot diag(2^1.2, 1)) at the angle of its
# widest adjoint window and at 45 degrees, the largest minification (s = a = 2^-0.6), the largest isotropic pair, a pure 45 degree turn
SUPPLIED = np.stack([
    np.array(G.IDENTITY, f32),
    row_from_t(rot(np.rad2deg(np.arctan(1.0 / BIG ** 2))) @ np.diag([BIG * BIG, 1.0])),
    row_from_t(rot(30.0) @ np.diag([SMALL * SMALL, 1.0])),
    row_from_t(rot(45.0) @ np.diag([BIG, BIG])),
    np.array(G.IDENTITY, f32),
    row_from_t(rot(-45.0) @ np.diag([SMALL, SMALL])),
    row_from_t(rot(45.0)),
    row_from_t(rot(45.0) @ np.diag([BIG * BIG, 1.0])),
])


def device_table(B, seed, p=0.5):
    """The device-produced table of the edge draws gated at p (mixed identity and other rows), with what the reference says its bits are."""
    from stylegan.pytorch_amd import functional as F
    u = G.edge_draws5(B, seed)
    gates = np.random.default_rng(seed + 1).random((B, 3), dtype=f32)
    gates[3], gates[4 % B] = (0.9, 0.9, 0.9), (0.1, 0.1, 0.1)               # one row off whatever else is drawn, one row fully on
    bits = G.gates(gates, p, G.ALL)
    mat = F.ada_geom_matrix(torch.from_numpy(u).to(DEV), G.ALL, torch.from_numpy(gates).to(DEV), dev_state(p))
    return mat, u, bits


# --------------------------------------------------------------------------------------------------------- 1. the matrix kernel
def test_matrix_kernel_vs_restatement():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B = 8
    u = G.edge_draws5(B, seed=3)
    ud = torch.from_numpy(u).to(DEV)
    gates = GC.spread_gates3(B).numpy().copy()
    gates[5], gates[6] = (0.5, 0.5, 0.5), (0.0, float(G.EDGE), 0.5)           # values equal to p = 0.5 (strict <), the edges of [0,1)
    gd = torch.from_numpy(gates).to(DEV)
    wide = torch.rand(B, 8, device=DEV)                                     # the same draws and gates as rows of one [B,8] tensor
    wide[:, :5], wide[:, 5:] = ud, gd
    worst = 0.0

    def check(mat, bits, what):
        nonlocal worst
        ref = G.matrices(u, bits)
        got = mat.cpu().numpy()
        assert got.dtype == f32 and got.shape == (B, 8)
        for b in range(B):
            if not bits[b] & G.ALL:
                assert tuple(got[b].tolist()) == G.IDENTITY and not np.signbit(got[b]).any(), (what, b, got[b])      # the flag
            else:
                err = float(np.abs(got[b].astype(np.float64) - ref[b]).max())
                worst = max(worst, err)
                assert err <= MATRIX_TOL, (what, b, err, got[b], ref[b])
    for policy in (G.ALL, G.SCALE, G.ROTATE, G.ANISO, G.SCALE | G.ANISO, G.ROTATE | G.ANISO):
        N.prof_start(1)
        try:
            mat = F.ada_geom_matrix(ud, policy)
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert [r[4].split(" ")[0] for r in N.prof_records()] == ["ada_geom_matrix"]
        check(mat, [policy] * B, ("ungated", policy))
        assert torch.equal(mat, F.ada_geom_matrix(wide[:, :5], policy))      # the row stride; and bit-reproducible
        for p in (0.0, 0.5, 1.0):
            bits = G.gates(gates, p, policy)
            mat = F.ada_geom_matrix(ud, policy, gd, dev_state(p))
            check(mat, bits, ("gated", policy, p))
            assert torch.equal(mat, F.ada_geom_matrix(wide[:, :5], policy, wide[:, 5:], dev_state(p)))
            if p == 0.0:
                assert not bits.any()
            if p == 1.0:
                assert (bits == policy).all()
    assert F.ada_geom_matrix(ud, 0).cpu().numpy().tolist() == [list(G.IDENTITY)] * B                   # no geometric op in the policy
    print("matrix kernel: largest |entry - fp64| =", worst, "bound", MATRIX_TOL)


# ------------------------------------------------------------------------------------------- 2. the resample, forward and adjoint
SHAPES = [(1, 1, 0), (2, 2, 0), (5, 7, 0), (8, 8, 0), (16, 16, 0), (33, 31, 0), (36, 36, 0), (16, 16, 1)]


def check_elements(y, x, mat, adjoint, what):
    """|y - y64| <= 2 (n + 1) 2^-24 sum |w x| per element (n non-zero coefficients: one rounding per product and per addition, a margin
    of 2), y64 the fp64 sum with the weights geom_ref reproduces bit for bit; an element with no coefficient is +0 exactly; an
    identity row is a copy."""
    mat = np.asarray(mat)
    B, H, W, _ = x.shape
    x64 = nchw(x).double()
    ref = nhwc(G.apply(x64, mat, adjoint))
    mag = nhwc(G.apply(x64.abs(), mat, adjoint))
    yc = y.cpu()
    worst = 0.0
    for b in range(B):
        if G.is_identity(mat[b]):
            assert torch.equal(yc[b], x[b]), (what, b)
            continue
        n = torch.from_numpy(G.tap_counts(mat[b], H, W, adjoint)).unsqueeze(-1)
        bound = 2.0 * (n + 1).double() * EPS * mag[b]
        err = (yc[b].double() - ref[b]).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (what, b, float((err - bound).max()))
        empty = (n == 0).expand(H, W, 3)
        assert bool((yc[b].view(torch.int32)[empty] == 0).all()), (what, b, "an element without a tap must be +0")
    return worst


@pytest.mark.parametrize("H,W,off", SHAPES)
def test_resample_vs_restatement(H, W, off):
    B = 8
    g = torch.Generator().manual_seed(H * 1000 + W + off)
    x = torch.randn(B, H, W, 3, generator=g)
    xd = on_device(x, off)
    assert (xd.data_ptr() % 16 == 0) == (off == 0)
    dev_mat, _, bits = device_table(B, seed=H + W)
    assert any(not b & G.ALL for b in bits) and any(b & G.ALL for b in bits)                 # mixed identity and other rows
    for name, matd in (("device", dev_mat), ("supplied", torch.from_numpy(SUPPLIED).to(DEV))):
        mat = matd.cpu().numpy()
        for adjoint in (False, True):
            y, notes = run_geom(xd, matd, adjoint)
            assert notes == [expected_note(W, off)], notes
            worst = check_elements(y, x, mat, adjoint, (name, adjoint))
            print(name, "adjoint" if adjoint else "forward", "largest err / bound", worst)
            y2, _ = run_geom(xd, matd, adjoint)
            assert torch.equal(y, y2)                                       # bit-reproducible
        ax = run_geom(xd, matd, False)[0].double().cpu()
        gy = torch.randn(B, H, W, 3, generator=g)
        aty = run_geom(on_device(gy, off), matd, True)[0].double().cpu()
        lhs, rhs = float((ax * gy.double()).sum()), float((x.double() * aty).sum())
        scale = float((nhwc(G.apply(nchw(x).double().abs(), mat)) * gy.double().abs()).sum())
        # <R x, g> = <x, R^T g>: each side within its per-element bound (n <= 4 forward, n <= 49 adjoint)
        assert abs(lhs - rhs) <= 2 * (5 + 50) * EPS * scale + 1e-30, (name, lhs, rhs)


def test_adjoint_window_reaches_its_largest():
    """The supplied rows include the widest candidate box the clamp allows: at 36x36 some element of the adjoint sums more coefficients
    than a 4x4 box holds, and none more than 7x7."""
    counts = [int(G.tap_counts(SUPPLIED[b], 36, 36, True).max()) for b in range(8)]
    print("largest number of coefficients per adjoint element:", counts)
    assert max(counts) > 9 and max(counts) <= 49


# --------------------------------------------------------------------------------------------------- 3. exact rows, bit for bit
def ints(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (B, H, W, 3), generator=g).float()


@pytest.mark.parametrize("H,W,off,tinv", [
    (1, 1, 0, (1, 0, 0, 1)), (5, 7, 0, (1, 0, 0, 1)), (36, 36, 0, (1, 0, 0, 1)), (16, 16, 1, (1, 0, 0, 1)),
    (8, 8, 0, (0.5, 0, 0, 0.5)), (6, 10, 0, (0.5, 0, 0, 0.5)), (36, 36, 0, (0.5, 0, 0, 0.5)),
    (8, 8, 0, (2, 0, 0, 2)), (6, 10, 0, (2, 0, 0, 2)), (36, 36, 0, (2, 0, 0, 2)), (16, 16, 1, (2, 0, 0, 2)),
    (8, 8, 0, (0, -1, 1, 0)), (36, 36, 0, (0, -1, 1, 0)), (9, 9, 0, (0, -1, 1, 0))])
def test_exact_rows_bit_for_bit(H, W, off, tinv):
    B = 3
    x = ints(B, H, W, H * 100 + W)
    xd = on_device(x, off)
    row = G.table(tinv)
    assert G.is_identity(row) == (tinv == (1, 0, 0, 1))
    mat = np.stack([row] * B)
    matd = torch.from_numpy(mat).to(DEV)
    for adjoint in (False, True):
        y, notes = run_geom(xd, matd, adjoint)
        assert notes == [expected_note(W, off)]
        ref = nhwc(G.apply(nchw(x).double(), mat, adjoint))
        assert torch.equal(y.cpu().double(), ref), (tinv, adjoint)
        if tinv == (0, -1, 1, 0):
            assert torch.equal(y.cpu(), torch.rot90(x, -1 if adjoint else 1, [1, 2]))
        if tinv == (1, 0, 0, 1):
            assert torch.equal(y.cpu(), x)
    if tinv == (1, 0, 0, 1):                                                 # the same map through the general path (T off by one ulp)
        almost = mat.copy()
        almost[:, 4] = np.nextafter(f32(1), f32(2))
        for adjoint in (False, True):
            assert torch.equal(run_geom(xd, torch.from_numpy(almost).to(DEV), adjoint)[0].cpu(), x)


# ------------------------------------------------------------------------------------------ 4. the transpose property, on the device
def test_forward_column_is_adjoint_row_bit_for_bit():
    """One-hot inputs at 5x7: image q of the forward batch holds column q of R, image p of the adjoint batch row p of R^T.  The two
    are the same fp32 numbers (the shared weight expression), and they are geom_ref's float32 weights."""
    H, W = 5, 7
    n = H * W
    dev_mat, _, _ = device_table(8, seed=11, p=1.0)
    rows = np.concatenate([SUPPLIED[[1, 2, 3, 5, 6, 7]], dev_mat.cpu().numpy()])
    onehot = torch.eye(n).reshape(n, H, W, 1).expand(n, H, W, 3).contiguous()
    xd = on_device(onehot)
    for k, row in enumerate(rows):
        matd = torch.from_numpy(np.stack([row] * n)).to(DEV)
        fwd = run_geom(xd, matd, False)[0].cpu()                            # fwd[q, p] = R[p, q]
        adj = run_geom(xd, matd, True)[0].cpu()                             # adj[p, q] = R^T[q, p] = R[p, q]
        for ch in range(3):
            Rf, Ra = fwd[..., ch].reshape(n, n), adj[..., ch].reshape(n, n)
            assert torch.equal(Rf.view(torch.int32), Ra.t().contiguous().view(torch.int32)), (k, ch)
        dense = np.zeros((n, n), f32)                                       # dense[p, q] from the restatement
        for idx, w in G.taps(row, H, W):
            np.add.at(dense, (np.arange(n), idx.reshape(-1)), w.reshape(-1))
        assert np.array_equal(adj[..., 0].reshape(n, n).numpy(), dense), k


# ------------------------------------------------------------------------------------------------------------- 5. continuity
def test_old_policies_launch_what_they_launched():
    from stylegan.pytorch_amd import functional as F
    B = 8
    img = torch.randn(B, 16, 16, 3, device=DEV)
    u9 = torch.from_numpy(Bl.edge_draws9(B, seed=2)).to(DEV)
    dis = small_dis(diffaug_policy=GC.C.FULL)
    dis.train()
    dis.diffaug_override = u9
    y, notes = recorded(lambda: dis._diffaug(img))
    assert notes and not any(n.startswith("ada_geom") for n in notes), notes
    assert torch.equal(y, F.call(F.DiffAugFn, img, u9, 31))
    three = small_dis(diffaug_policy="color,translation,cutout")
    three.train()
    three.diffaug_override = u9[:, :7].contiguous()
    y, notes = recorded(lambda: three._diffaug(img))
    assert notes == ["diffaug_sum", "diffaug"], notes
    assert torch.equal(y, F.call(F.DiffAugFn, img, u9[:, :7].contiguous(), 7))


@pytest.mark.parametrize("base", [GC.C.FULL, "color,cutout", ""])
def test_new_ops_at_p_zero_change_nothing(base):
    B = 8
    img = torch.randn(B, 16, 16, 3, device=DEV)
    policy8 = (base + "," if base else "") + "scale,rotate,aniso"
    with8 = small_dis(diffaug_policy=policy8, ada_target=0.6, ada_p_init=0.0, ada_kimg=BIG_KIMG)
    with8.train()
    width = 9 if "xflip" in base else 7
    u = torch.from_numpy(Bl.edge_draws9(B, seed=4)).to(DEV)[:, :width].contiguous()
    gates_ = torch.rand(B, 5 if width == 9 else 3, device=DEV)
    with8.diffaug_override, with8.ada_gate_override = u, gates_
    with8.geom_override, with8.geom_gate_override = torch.from_numpy(G.edge_draws5(B)).to(DEV), torch.rand(B, 3, device=DEV)
    y8, notes = recorded(lambda: with8._diffaug(img))
    assert notes[-2:] == ["ada_geom_matrix", "ada_geom_tile"], notes
    if base:
        without = small_dis(diffaug_policy=base, ada_target=0.6, ada_p_init=0.0, ada_kimg=BIG_KIMG)
        without.train()
        without.diffaug_override, without.ada_gate_override = u, gates_
        assert torch.equal(y8, without._diffaug(img))
    assert torch.equal(y8, img)                                             # and p = 0 gates every op off: the image itself


def test_training_forward_draws_its_own_five_or_eight():
    B = 4
    img = torch.randn(B, 16, 16, 3, device=DEV)
    for ada in (False, True):
        kw = dict(ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG) if ada else {}
        dis = small_dis(diffaug_policy=GC.FULL8, **kw)
        dis.train()
        torch.cuda.manual_seed(77)
        y = dis._diffaug(img)
        after = torch.cuda.get_rng_state()
        torch.cuda.manual_seed(77)
        r1 = torch.rand(B, 14 if ada else 9, device=DEV)                     # what the five-op policy draws today, then the stage's own
        r2 = torch.rand(B, 8 if ada else 5, device=DEV)
        assert torch.equal(after, torch.cuda.get_rng_state())
        dis.diffaug_override, dis.geom_override = r1[:, :9], r2[:, :5]
        if ada:
            dis.ada_gate_override, dis.geom_gate_override = r1[:, 9:], r2[:, 5:]
        assert torch.equal(y, dis._diffaug(img))
        assert ("ada_state" in dis.state_dict()) == ada


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_first_and_second_order_through_the_functions():
    """(y . w).sum() and the R1-shaped grad(...).pow(2).sum() through AdaGeomFn against torch autograd on the fp64 restatement under
    the device's table.  Bounds: each pass the per-element bound of check_elements on the input that pass was given (read back from
    the device), plus the reference map applied to the bound of the pass before (R has non-negative coefficients)."""
    from stylegan.pytorch_amd import functional as F
    B, N_ = 8, 16
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N_, N_, 3, generator=g)
    w = torch.randn(B, N_, N_, 3, generator=g)
    matd, _, _ = device_table(B, seed=21)
    mat = matd.cpu().numpy()
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y = F.call(F.AdaGeomFn, xd, matd)
    gx, = torch.autograd.grad((y * wd).sum(), xd, create_graph=True)
    gw, = torch.autograd.grad(gx.pow(2).sum(), wd)

    def R(t, adjoint=False):
        return nhwc(G.apply(nchw(t), mat, adjoint))

    def bound(t, adjoint):
        n = torch.stack([torch.from_numpy(G.tap_counts(mat[b], N_, N_, adjoint)) for b in range(B)]).unsqueeze(-1)
        return 2.0 * (n + 1).double() * EPS * R(t.abs(), adjoint)
    x64, w64 = x.double(), w.double()
    e_y = (y.detach().cpu().double() - R(x64)).abs()
    assert bool((e_y <= bound(x64, False)).all())
    e1 = bound(w64, True)
    assert bool(((gx.detach().cpu().double() - R(w64, True)).abs() <= e1).all())
    v = 2.0 * gx.detach().cpu().double()                                    # what the second pass was given (2 gx is exact in fp32)
    e2 = bound(v, False) + R(2.0 * e1)
    err = (gw.cpu().double() - 2.0 * R(R(w64, True))).abs()
    print("d2w: largest err / bound", float((err / e2.clamp_min(1e-300)).max()))
    assert bool((err <= e2).all())
    # the D step's fakes: no input gradient is asked for, none is computed
    ctx = types.SimpleNamespace(needs_input_grad=(False, False), saved_tensors=(matd,))
    assert F.AdaGeomFn.backward(ctx, wd.detach()) == (None, None)
    assert not F.call(F.AdaGeomFn, x.to(DEV), matd).requires_grad


# ------------------------------------------------------------------------------------------------------------------- 6. network
@pytest.mark.parametrize("depth,alpha", [(5, 0.5), (3, 0.3)])
def test_network_first_and_second_order_vs_oracle(monkeypatch, dparams, depth, alpha):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss under the eight-op policy with per-image gates (p = 0.5
    against pinned uniforms), against the fp64 composition geom_ref o blit_ref o the oracle's D; the criterion of
    tests/test_gpu_blit.py's network test.

    The reference resamples under the table the device produced (as the resample tests do), which this test first holds against
    geom_ref's fp64 matrices to MATRIX_TOL.  A matrix entry off by 1e-6 moves a source position by up to 64e-6 pixels at 128x128; on
    the white-noise images of this test that changes a pixel by about 1e-4 of its size, which is the matrix kernel's error
    (test_matrix_kernel_vs_restatement), not the resample's, and is above what the network criterion allows for kernel rounding."""
    from stylegan.pytorch_amd import Losses
    from stylegan.pytorch_amd import functional as F
    B, res = GC.NET_B, 4 * 2 ** depth
    dp = dparams
    dis = load_ada(mid_dis(GC.FULL8, ada_target=0.6, ada_p_init=GC.NET_P, ada_kimg=BIG_KIMG), dp)
    dis.train()
    u9, gates5, bits5 = GC.C.network_draws(depth)
    u5, gates3, bits3 = GC.network_draws(depth)
    for op in (G.SCALE, G.ROTATE, G.ANISO):
        assert any(b & op for b in bits3) and any(not b & op for b in bits3), bits3           # mixed
    dis.diffaug_override, dis.ada_gate_override = torch.from_numpy(u9).to(DEV), gates5.to(DEV)
    dis.geom_override, dis.geom_gate_override = torch.from_numpy(u5).to(DEV), gates3.to(DEV)
    mat = F.ada_geom_matrix(dis.geom_override, G.ALL, dis.geom_gate_override, dis.ada_state).cpu().numpy()
    mat_err = float(np.abs(mat.astype(np.float64) - G.matrices(u5, bits3)).max())
    print("table: largest |entry - fp64| =", mat_err, "bound", MATRIX_TOL)
    assert mat_err <= MATRIX_TOL
    orig = O.discriminator

    def discriminator(p, img, depth_, alpha_, total_depth, **kw):
        return orig(p, G.apply(Bl.apply_gated(img, u9, bits5), mat), depth_, alpha_, total_depth, **kw)
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
    assert dis._ada_real is not None and dis.ada_p == GC.NET_P


# ------------------------------------------------------------------------------------------------------ graph replay, moving p
def train_run(use_graphs, iters=4, seed=5):
    # 1 / (0.02 * 1000) = 0.05 per image: one update (interval 1) at batch 4 moves p by 0.2
    sg = make_sg(GC.FULL8, use_graphs, ada_target=0.6, ada_interval=1, ada_kimg=0.02, ada_p_init=0.5)
    gp, dp = mid_params(torch.float64)
    load_into(sg.gen, gp); load_ada(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, mid_noises(4))
    sg.dis.diffaug_override = torch.from_numpy(Bl.edge_draws9(8, seed=3)[[0, 3, 4, 7]]).to(DEV)
    sg.dis.ada_gate_override = GC.C.spread_gates5(4).to(DEV)
    sg.dis.geom_override = torch.from_numpy(G.edge_draws5(8, seed=3)[[0, 1, 3, 7]]).to(DEV)
    sg.dis.geom_gate_override = GC.spread_gates3(4).to(DEV)
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


# ---------------------------------------------------------------------------------------------------------------- 7. rejections
def test_c_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    B, H, W = 2, 8, 8
    x = torch.randn(B, H, W, 3, device=DEV)
    y = torch.full((B, H, W, 3), SENTINEL, device=DEV)
    mat = torch.from_numpy(SUPPLIED[:B].copy()).to(DEV)
    u, gates_, state = torch.rand(B, 8, device=DEV), torch.rand(B, 3, device=DEV), dev_state(0.5)
    out = torch.full((B, 8), SENTINEL, device=DEV)
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
    assert refused(lambda: L.sgx_ada_geom(N.ptr(y), N.ptr(y), N.ptr(mat), B, H, W, 0, s))                 # in place
    assert refused(lambda: L.sgx_ada_geom(N.ptr(y), N.ptr(y), N.ptr(mat), B, H, W, 1, s))
    assert refused(lambda: L.sgx_ada_geom(None, N.ptr(y), N.ptr(mat), B, H, W, 0, s))
    assert refused(lambda: L.sgx_ada_geom(N.ptr(x), N.ptr(y), None, B, H, W, 0, s))
    assert refused(lambda: L.sgx_ada_geom(N.ptr(x), N.ptr(y), N.ptr(mat), 0, H, W, 0, s))
    assert refused(lambda: L.sgx_ada_geom(N.ptr(x), N.ptr(y), N.ptr(mat), B, 0, W, 0, s))
    assert refused(lambda: L.sgx_ada_geom(N.ptr(x), N.ptr(y), N.ptr(mat), B, 40000, 40000, 0, s))         # beyond 2^31 floats per image
    m = lambda *a: L.sgx_ada_geom_matrix(*a)
    assert refused(lambda: m(N.ptr(u), 4, None, 0, None, 224, N.ptr(out), B, s))                          # rows too close
    assert refused(lambda: m(N.ptr(u), 8, N.ptr(gates_), 2, N.ptr(state), 224, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, N.ptr(gates_), 3, None, 224, N.ptr(out), B, s))                 # gates without the state
    assert refused(lambda: m(N.ptr(u), 8, None, 0, N.ptr(state), 224, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 31, N.ptr(out), B, s))                           # bits of the other entries
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 256, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, -1, N.ptr(out), B, s))
    assert refused(lambda: m(None, 8, None, 0, None, 224, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 224, N.ptr(out), 0, s))


def test_python_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B = 2
    x = torch.randn(B, 8, 8, 3, device=DEV)
    mat = torch.from_numpy(SUPPLIED[:B].copy()).to(DEV)
    bad = [lambda: F._ada_geom(torch.randn(B, 8, 8, 4, device=DEV), mat, False),                          # a 4-channel tensor
           lambda: F._ada_geom(x.double(), mat, False), lambda: F._ada_geom(x[0], mat, False),
           lambda: F._ada_geom(x, mat[:, :4].contiguous(), False), lambda: F._ada_geom(x, torch.zeros(B + 1, 8, device=DEV), True),
           lambda: F._ada_geom(x, mat.double(), False), lambda: F._ada_geom(x, mat.reshape(-1), False),   # the table's shape or dtype
           lambda: F._ada_geom(x.cpu(), mat.cpu(), False), lambda: F._ada_geom(x, mat.cpu(), False),      # CPU tensors
           lambda: F._ada_geom(x.cpu(), mat, True),
           lambda: F.ada_geom_matrix(torch.rand(B, 5), 224),
           lambda: F.ada_geom_matrix(torch.rand(B, 4, device=DEV), 224), lambda: F.ada_geom_matrix(torch.rand(B, 5, device=DEV).double(), 224),
           lambda: F.ada_geom_matrix(torch.rand(B, 5, device=DEV), 224, torch.rand(B, 3, device=DEV)),
           lambda: F.ada_geom_matrix(torch.rand(B, 5, device=DEV), 224, torch.rand(B, 5, device=DEV), dev_state(0.5)),
           lambda: F.ada_geom_matrix(torch.rand(B, 5, device=DEV), 224, torch.rand(B, 3, device=DEV), torch.zeros(8))]
    for k, fn in enumerate(bad):
        N.prof_start(1)
        try:
            with pytest.raises(N.SgxError):
                fn()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], (k, "a kernel was launched")
    dis = small_dis(diffaug_policy="scale,rotate,aniso", ada_target=0.6)
    dis.train()
    dis.geom_override = torch.rand(B, 7, device=DEV)
    with pytest.raises(ValueError, match="geom_override"):
        dis._diffaug(x)
    dis.geom_override, dis.geom_gate_override = torch.rand(B, 5, device=DEV), torch.rand(B, 5, device=DEV)
    with pytest.raises(ValueError, match="geom_gate_override"):
        dis._diffaug(x)
