"""-m gpu: ADA's image-space filtering -- four per-image band gains folded into one symmetric 43-tap filter, applied separably with
whole-sample reflection, y = A_v A_h x, one axis per launch (csrc/adafilter.hip: sgx_ada_filter_matrix, sgx_ada_filter,
sgx_ada_filter_plan; functional.ada_filter_matrix / AdaFilterFn / AdaFilterAdjFn; Discriminator(diffaug_policy="...,imgfilter"))
against the fp64 restatement tests/filter_ref.py: the table kernel, the forward and the true adjoint per element on both kernels,
tile against general bit for bit, the copy branch, planted errors against the bounds, continuity with the policies of today, the
draws, the R1-shaped double backward, D under the fourteen-op policy against the oracle, graph replay with a moving p, and the
rejections."""
import ctypes
import random
import types

import numpy as np
import pytest
import torch

import aug_ref as AR
import blit_ref as Bl
import color_cases as CC
import color_ref as K
import filter_ref as R
import geom_cases as GC
import geom_ref as G
import golden_util as gu
import streaming_ref as SR
from aug_gpu_util import bits_equal, dev_state, load_ada, make_sg, mid_dis, on_device, small_dis
from gpu_util import DEV, MID, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise  # noqa: F401  (MID: test_gpu_corrupt reads it here)
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu

OPT = dict(learning_rate=0.003, beta_1=0, beta_2=0.99, eps=1e-8)
f32 = np.float32
BIG_KIMG = 1e9                                   # p does not move within a test
GUARD = 64                                       # floats around y and the workspace (a multiple of 4: both keep their alignment)
SENTINEL = 12345.5
FULL14 = CC.FULL13 + ",imgfilter"
TILE_MIN = 44                                    # the tile kernel's least H and W (include/sgx.h)
# Entries of the device's fp32 [B][22] table against the fp64 restatement over the draws of test_matrix_kernel_vs_restatement (every z
# at both clamp ends, u at 0 and just under 1, all sixteen gate patterns): the gains are products of four quotients of exp2f / sqrtf
# results (logf, cosf behind them), an entry four products and three sums of gains of at most 3 with taps of at most 1/2.  The largest
# error measured on the MI355X over these draws is MATRIX_ERR_MEASURED, the bound four times that (libm differences between releases).
MATRIX_ERR_MEASURED = 3.35e-7
MATRIX_TOL = 4 * MATRIX_ERR_MEASURED
assert MATRIX_TOL <= 1e-5
MATRIX_B = 16


def lib_plan(B, H, W, adjoint, aligned):
    from stylegan.pytorch_amd import native as N
    out = (ctypes.c_int * 13)(*([7] * 13))
    rc = N.lib().sgx_ada_filter_plan(B, H, W, int(adjoint), int(aligned), ctypes.addressof(out))
    assert rc == 0 and out[0] == 2, (rc, list(out))
    return [tuple(out[1 + 6 * i:7 + 6 * i]) for i in range(2)]                 # (kernel, axis, adjoint, gx, gy, tiles_x)


def planned_launches(B, H, W, adjoint, aligned):
    tf = lambda v: "true" if v else "false"
    plan = lib_plan(B, H, W, adjoint, aligned)
    ids = [f"ada_filter_{'tile' if k else 'px'}_kernel<{axis}, {tf(adj)}>" for k, axis, adj, *_ in plan]
    notes = [f"ada_filter_{'tile' if k else 'px'}" for k, *_ in plan]
    return ids, [((gx, gy, 1), (256, 1, 1), 0) for _, _, _, gx, gy, _ in plan], notes, plan


def run_filter(xd, matd, adjoint):
    """sgx_ada_filter into a buffer with guard floats on both sides of y and of the workspace; -> (y (a copy), the note names), the
    launches held against sgx_ada_filter_plan and the guards checked."""
    from stylegan.pytorch_amd import native as N
    B, H, W, _ = xd.shape
    n = xd.numel()
    off = (xd.data_ptr() // 4) % 4                                          # y gets x's alignment
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=DEV)
    y = buf[GUARD + off:GUARD + off + n].view(B, H, W, 3)
    L = N.lib()
    nb = L.sgx_ada_filter_workspace_bytes(B, H, W)
    assert nb == 4 * n
    wbuf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    ws = wbuf[GUARD:GUARD + n]
    N.prof_start(1)
    try:
        rc = L.sgx_ada_filter(N.ptr(xd), N.ptr(y), N.ptr(matd), B, H, W, int(adjoint), ws.data_ptr(), nb, N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    recs = N.prof_records()
    notes = [r[4].split(" ")[0] for r in recs]
    N.check(rc, "sgx_ada_filter")
    aligned = xd.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    ids, geo, want_notes, plan = planned_launches(B, H, W, adjoint, aligned)
    got = ([SR.kernel_id(r[0]) for r in recs], [(tuple(g), tuple(b), int(lds)) for g, b, lds in N.prof_launches()])
    assert got == (ids, geo) and notes == want_notes, (got, ids, geo, notes)
    assert [p[1] for p in plan] == ([1, 0] if adjoint else [0, 1])          # along W then along H; the adjoint the other way round
    assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + n:] == SENTINEL).all()), "guard floats of y were written"
    assert bool((wbuf[:GUARD] == SENTINEL).all()) and bool((wbuf[GUARD + n:] == SENTINEL).all()), "guard floats of the workspace were written"
    return y.clone(), notes


def expected_note(H, W, off):
    return "ada_filter_tile" if W % 4 == 0 and off == 0 and H >= TILE_MIN and W >= TILE_MIN else "ada_filter_px"


def device_table(B, seed=0, identity=()):
    """The device's own table for edge draws; the images of ``identity`` gated off."""
    from stylegan.pytorch_amd import functional as F
    u = R.edge_draws8(B, seed)
    gates = np.full((B, 4), 0.25, f32)
    gates[list(identity)] = 0.75
    mat = F.ada_filter_matrix(torch.from_numpy(u).to(DEV), R.BIT, torch.from_numpy(gates).to(DEV), dev_state(0.5))
    rows = mat.cpu().numpy()
    assert [R.is_identity(r) for r in rows] == [b in identity for b in range(B)]
    return mat, rows


# --------------------------------------------------------------------------------------------------------- 1. the table kernel
def test_matrix_kernel_vs_restatement():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B = MATRIX_B
    u = R.edge_draws8(B, seed=3)
    ud = torch.from_numpy(u).to(DEV)
    gates = R.gate_patterns()                                                 # against p = 0.5: all sixteen on / off patterns
    gates[5, 0] = 0.5                                                         # a value equal to p (strict <): band 0 of row 5 goes off
    gd = torch.from_numpy(gates).to(DEV)
    wide = torch.rand(B, 12, device=DEV)                                    # the same draws and gates as rows of one [B,12] tensor
    wide[:, :8], wide[:, 8:] = ud, gd
    worst = 0.0

    def check(mat, on, what):
        nonlocal worst
        ref = R.rows(u, on)
        got = mat.cpu().numpy()
        assert got.dtype == f32 and got.shape == (B, 22)
        for b in range(B):
            if not on[b].any():
                assert tuple(got[b].tolist()) == R.IDENTITY and not np.signbit(got[b]).any(), (what, b, got[b])      # the flag
                continue
            err = float(np.abs(got[b].astype(np.float64) - ref[b]).max())
            worst = max(worst, err)
            assert err <= MATRIX_TOL, (what, b, err, got[b], ref[b])
    N.prof_start(1)
    try:
        mat = F.ada_filter_matrix(ud, R.BIT)
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    assert [r[4].split(" ")[0] for r in N.prof_records()] == ["ada_filter_matrix"]
    check(mat, np.ones((B, 4), bool), "ungated")
    assert torch.equal(mat, F.ada_filter_matrix(wide[:, :8], R.BIT))          # the row stride; and bit-reproducible
    assert torch.equal(mat, F.ada_filter_matrix(ud, 16383))                   # the other stages' bits are masked by the wrapper
    for p in (0.0, 0.5, 1.0):
        on = R.gates(gates, p)
        mat = F.ada_filter_matrix(ud, R.BIT, gd, dev_state(p))
        check(mat, on, ("gated", p))
        assert torch.equal(mat, F.ada_filter_matrix(wide[:, :8], R.BIT, wide[:, 8:], dev_state(p)))
        if p == 0.0:
            assert not on.any()
        if p == 1.0:
            assert on.all()
        if p == 0.5:
            assert sorted(int(sum(1 << i for i in range(4) if r[i])) for r in on) == sorted([4 if k == 5 else k for k in range(16)])
    assert F.ada_filter_matrix(ud, 0).cpu().numpy().tolist() == [list(R.IDENTITY)] * B                   # imgfilter not in the policy
    assert F.ada_filter_matrix(ud, 8191).cpu().numpy().tolist() == [list(R.IDENTITY)] * B                # the other stages' bits
    print("matrix kernel: largest |entry - fp64| =", worst, "bound", MATRIX_TOL)


# ------------------------------------------------------------------------------------- 2. / 3. / 5. the passes, on both kernels
SHAPES = [(2, 2), (4, 4), (5, 7), (8, 8), (16, 16), (21, 43), (22, 22), (33, 31), (43, 44), (64, 64), (72, 132), (128, 128),
          (TILE_MIN + 1, TILE_MIN), (TILE_MIN, TILE_MIN), (TILE_MIN, TILE_MIN - 1), (TILE_MIN, TILE_MIN + 1),
          (TILE_MIN, TILE_MIN + 4)]
_REF = {}


def reference(H, W):
    """x, the device's table, and per direction (y64, the bound) -- computed once per shape, shared by the offsets, left unchanged."""
    if (H, W) not in _REF:
        B = 3
        x = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(H * 1000 + W))
        matd, c = device_table(B, seed=H + W)
        x64, c64 = x.double().numpy(), c.astype(np.float64)
        out = {}
        for adjoint in (False, True):
            n = 2 * (43 * max(R.folds(H), R.folds(W)) + 1) if adjoint else 88
            out[adjoint] = (R.apply_dense(x64, c64, adjoint), R.gamma(n) * R.apply_dense(np.abs(x64), c64, adjoint, absolute=True))
        _REF[(H, W)] = (x, matd, c64, out)
    return _REF[(H, W)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_passes_vs_fp64_on_both_kernels(H, W):
    """|y - y64| <= gamma_n (|A_v| |A_h| |x|) per element, n = 88 forward and 2 (43 r + 1) adjoint (r the largest fold count), under the
    device's own fp32 table on both sides; at float offsets 0 and 1, the kernel that launched held against the plan query; where the
    tile kernel serves the shape, the general kernel (the offset run) gives the same bits."""
    x, matd, c64, ref = reference(H, W)
    ys = {}
    for off in (0, 1):
        xd = on_device(x, off)
        assert (xd.data_ptr() % 16 == 0) == (off == 0)
        for adjoint in (False, True):
            y, notes = run_filter(xd, matd, adjoint)
            assert notes == [expected_note(H, W, off)] * 2, notes
            y64, bound = ref[adjoint]
            err = np.abs(y.cpu().double().numpy() - y64)
            print(H, W, off, "adj" if adjoint else "fwd", notes[0], "largest err / bound", float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all(), (adjoint, off, float((err - bound).max()))
            ys[(off, adjoint)] = y
    for adjoint in (False, True):                                             # tile == general, bit for bit (and px == px where no tile)
        assert bits_equal(ys[(0, adjoint)], ys[(1, adjoint)]), (H, W, adjoint)


# ----------------------------------------------------------------------------------------------------------- 5. planted errors
def test_planted_errors_break_the_bounds():
    """Through filter_ref only: a row shifted by one tap, reflection that repeats the edge sample, and the adjoint computed as the
    forward each leave the operator by more than twice the bound somewhere on a listed shape -- a result within the bound of the
    operator cannot be within the bound of the planted one."""
    broke = {"shift": [], "edge": [], "adjoint as forward": []}
    for H, W in ((5, 7), (22, 22), (64, 64)):
        x, matd, c64, ref = reference(H, W)
        x64 = x.double().numpy()
        for name, adjoint, wrong in (("shift", False, R.apply_dense(x64, c64, shift=1)), ("edge", False, R.apply_dense(x64, c64, edge=True)),
                                     ("adjoint as forward", True, R.apply_dense(x64, c64, adjoint=False))):
            y64, bound = ref[adjoint]
            if (np.abs(wrong - y64) > 2 * bound).any():
                broke[name].append((H, W))
    assert all(broke.values()), broke


# ------------------------------------------------------------------------------------------------------ 4. identity rows copy
@pytest.mark.parametrize("off,H,W", [(0, 64, 48), (1, 64, 48), (0, 5, 4)])
def test_identity_rows_copy_special_values(off, H, W):
    B = 4
    # -0, +inf, -inf, quiet NaNs with payloads of either sign, a signalling NaN, the smallest denormals
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001, 0x7f800123, 0x00000001, 0x80000001], np.uint32)
    words = torch.from_numpy(np.resize(special, B * H * W * 3).view(np.int32).copy())
    buf = torch.zeros(words.numel() + off, dtype=torch.int32, device=DEV)
    buf[off:] = words.to(DEV)
    xd = buf[off:].view(torch.float32).view(B, H, W, 3)
    xd[0], xd[2] = torch.randn(H, W, 3, device=DEV), torch.randn(H, W, 3, device=DEV)      # the drawn rows filter ordinary numbers
    words = xd.view(torch.int32).cpu().reshape(B, -1)
    matd, rows = device_table(B, seed=7, identity=(1, 3))                   # identity and drawn rows in one batch: the branch is per block
    for adjoint in (False, True):
        y, notes = run_filter(xd, matd, adjoint)
        assert notes == [expected_note(H, W, off)] * 2
        got = y.view(torch.int32).cpu().reshape(B, -1)
        assert torch.equal(got[1], words[1]) and torch.equal(got[3], words[3]), adjoint
        assert not torch.equal(got[0], words[0]) and bool(torch.isfinite(y[0]).all()) and bool(torch.isfinite(y[2]).all())


# ------------------------------------------------------------------------------------------------------------- 6. continuity
def recorded(fn):
    from stylegan.pytorch_amd import native as N
    N.prof_start(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    AR.assert_records_are_planned(N)                                        # every launch of the older passes: what sgx_aug_plan reports
    return out, [r[4].split(" ")[0] for r in N.prof_records()], [tuple(g) for g, _, _ in N.prof_launches()]


def test_old_policies_launch_what_they_launched():
    from stylegan.pytorch_amd import functional as F
    B = 8
    img = torch.randn(B, 16, 16, 3, device=DEV)
    u9 = torch.from_numpy(Bl.edge_draws9(B, seed=2)).to(DEV)
    u5 = torch.from_numpy(G.edge_draws5(B, seed=2)).to(DEV)
    u8 = torch.from_numpy(K.edge_draws8(B, seed=2)).to(DEV)
    dis = small_dis(diffaug_policy=CC.FULL13)
    dis.train()
    dis.diffaug_override, dis.geom_override, dis.color_override = u9, u5, u8
    y, notes, grids = recorded(lambda: dis._diffaug(img))
    assert notes == ["diffaug_blit_sum", "diffaug_blit_tile", "ada_geom_matrix", "ada_geom_tile", "ada_color_matrix", "ada_color_vec"], notes
    assert grids == [(1, B, 1), (1, B, 1), (1, 1, 1), (1, B, 1), (1, 1, 1), (1, B, 1)], grids
    want = F.call(F.AdaColorFn, F.call(F.AdaGeomFn, F.call(F.DiffAugFn, img, u9, 31), F.ada_geom_matrix(u5, 224)), F.ada_color_matrix(u8, 7936))
    assert torch.equal(y, want)
    two = small_dis(diffaug_policy="color,cutout")
    two.train()
    two.diffaug_override = u9[:, :7].contiguous()
    y2, notes, grids = recorded(lambda: two._diffaug(img))
    assert notes == ["diffaug_sum", "diffaug"] and grids == [(1, B, 1), (1, B, 1)], (notes, grids)
    assert torch.equal(y2, F.call(F.DiffAugFn, img, u9[:, :7].contiguous(), 5))
    # with imgfilter added and p = 0: the thirteen-op result, bit for bit, and the thirteen-op launches in front of the new stage's
    ada = dict(ada_target=0.6, ada_p_init=0.0, ada_kimg=BIG_KIMG)
    gates5, gates3 = torch.rand(B, 5, device=DEV), torch.rand(B, 3, device=DEV)
    outs = []
    for policy in (CC.FULL13, FULL14):
        d = small_dis(diffaug_policy=policy, **ada)
        d.train()
        d.diffaug_override, d.geom_override, d.color_override = u9, u5, u8
        d.ada_gate_override, d.geom_gate_override, d.color_gate_override = gates5, gates3, gates5
        d.filter_override, d.filter_gate_override = torch.from_numpy(R.edge_draws8(B)).to(DEV), torch.rand(B, 4, device=DEV)
        outs.append(recorded(lambda: d._diffaug(img)))
    (y13, n13, g13), (y14, n14, g14) = outs
    assert n14 == n13 + ["ada_filter_matrix", "ada_filter_px", "ada_filter_px"] and g14[:len(g13)] == g13, (n13, n14)
    assert torch.equal(y14, y13) and torch.equal(y14, img)


# ------------------------------------------------------------------------------------------------------------------ 7. draws
def test_training_forward_draws_its_own_eight_or_twelve():
    from stylegan.pytorch_amd import functional as F
    B = 4
    img = torch.randn(B, 16, 16, 3, device=DEV)
    for ada in (False, True):
        kw = dict(ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG) if ada else {}
        dis = small_dis(diffaug_policy=FULL14, **kw)
        dis.train()
        torch.cuda.manual_seed(77)
        y = dis._diffaug(img)
        after = torch.cuda.get_rng_state()
        old = small_dis(diffaug_policy=CC.FULL13, **kw)
        old.train()
        torch.cuda.manual_seed(77)
        y13 = old._diffaug(img)                                              # what the thirteen-op policy draws today, then the stage's own
        r = torch.rand(B, 12 if ada else 8, device=DEV)
        assert torch.equal(after, torch.cuda.get_rng_state())
        mat = F.ada_filter_matrix(r[:, :8], R.BIT, *((r[:, 8:], dis.ada_state) if ada else ()))
        assert torch.equal(y, F.call(F.AdaFilterFn, y13, mat))
        dis.filter_override = r[:, :8]                                        # the overrides suppress the draw
        if ada:
            dis.filter_gate_override = r[:, 8:]
        torch.cuda.manual_seed(77)
        assert torch.equal(y, dis._diffaug(img))
        torch.cuda.manual_seed(77)
        dis._diffaug(img)
        s14 = torch.cuda.get_rng_state()
        torch.cuda.manual_seed(77)
        old._diffaug(img)
        assert torch.equal(s14, torch.cuda.get_rng_state())                  # with both overrides set the new stage draws nothing
        assert ("ada_state" in dis.state_dict()) == ada


# ---------------------------------------------------------------------------------------------------------------- 8. autograd
def test_first_and_second_order_through_the_functions():
    """An R1-shaped double backward with a linear head at 36 x 36, batch 4: logit_b = <w, A x_b>, gx = d sum(logit) / dx (create_graph),
    the penalty sum gx^2, its gradient in w -- against torch-double autograd of the restatement under the device's table.  Criterion
    (the project's for gradients): err <= max(1e-3 |g64|, 4 err(the restatement run in fp32), floor) in the L2 norm."""
    from stylegan.pytorch_amd import functional as F
    B, N_ = 4, 36
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N_, N_, 3, generator=g)
    w = torch.randn(N_, N_, 3, generator=g)
    matd, rows = device_table(B, seed=21, identity=(2,))
    c64 = rows.astype(np.float64)

    def chain(xt, wt, op):
        xt, wt = xt.requires_grad_(True), wt.requires_grad_(True)
        y = op(xt)
        gx, = torch.autograd.grad((y * wt).sum(), xt, create_graph=True)
        pen = gx.pow(2).sum()
        gw, = torch.autograd.grad(pen, wt)
        return y.detach().cpu().double(), gx.detach().cpu().double(), gw.detach().cpu().double()
    from stylegan.pytorch_amd import native as N
    N.prof_start(1)
    try:
        got = chain(x.to(DEV), w.to(DEV), lambda t: F.call(F.AdaFilterFn, t, matd))
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    names = [SR.kernel_id(r[0]) for r in N.prof_records() if r[4].startswith("ada_filter")]
    assert names == ["ada_filter_px_kernel<0, false>", "ada_filter_px_kernel<1, false>", "ada_filter_px_kernel<1, true>", "ada_filter_px_kernel<0, true>",
                     "ada_filter_px_kernel<0, false>", "ada_filter_px_kernel<1, false>"], names         # A x, A^T w, A (2 gx): the chain closes
    ref = chain(x.double(), w.double(), lambda t: R.apply_torch(t, c64))
    AH = [torch.from_numpy(R.dense(c64[b], N_)).float() for b in range(B)]
    low = chain(x.clone(), w.clone(), lambda t: torch.stack([torch.einsum("ikc,lk->ilc", torch.einsum("ij,jkc->ikc", AH[b], t[b]), AH[b]) for b in range(B)]))
    for name, a, b, l in zip(("y", "gx", "gw"), got, ref, low):
        err, err32, norm = float((a - b).norm()), float((l - b).norm()), float(b.norm())
        print(name, "err", err, "fp32 restatement err", err32, "|g64|", norm)
        assert err <= max(1e-3 * norm, 4 * err32, 1e-30), (name, err, err32, norm)
    assert torch.equal(got[0][2].float(), x[2])                                                          # the identity row copies
    # the D step's fakes: no input gradient is asked for, none is computed
    ctx = types.SimpleNamespace(needs_input_grad=(False, False), saved_tensors=(matd,))
    assert F.AdaFilterFn.backward(ctx, x.to(DEV)) == (None, None)
    assert not F.call(F.AdaFilterFn, x.to(DEV), matd).requires_grad


# ------------------------------------------------------------------------------------------------------------------- 9. network
def filter_network_draws(depth):
    """-> (u [4,8], gate uniforms [4,4], on [4,4]) at p = 0.5: image 0 every band off, image 3 every band on, 1 and 2 split them."""
    on_, off_ = 0.25, 0.75
    gates = np.array([[off_] * 4, [on_, off_, on_, off_], [off_, on_, off_, on_], [on_] * 4], f32)
    return R.edge_draws8(CC.NET_B, seed=depth), gates, R.gates(gates, CC.NET_P)


def test_network_first_and_second_order_vs_oracle(monkeypatch):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss under the fourteen-op policy with per-image gates
    (p = 0.5, all six override pairs pinned) at one depth with fade-in, against the fp64 composition filter_ref o color_ref o geom_ref
    o blit_ref o the oracle's D, under the tables the device produced; the criteria of tests/test_gpu_color.py's network test."""
    from stylegan.pytorch_amd import Losses
    from stylegan.pytorch_amd import functional as F
    depth, alpha = 3, 0.3
    B, res = CC.NET_B, 4 * 2 ** depth
    dp = mid_params(torch.float64)[1]
    dis = load_ada(mid_dis(FULL14, ada_target=0.6, ada_p_init=CC.NET_P, ada_kimg=BIG_KIMG), dp)
    dis.train()
    u9, gates5, bits5 = GC.C.network_draws(depth)
    u5, gates3, bits3 = GC.network_draws(depth)
    u8, cgates, cbits = CC.network_draws(depth)
    uf, fgates, fon = filter_network_draws(depth)
    dis.diffaug_override, dis.ada_gate_override = torch.from_numpy(u9).to(DEV), gates5.to(DEV)
    dis.geom_override, dis.geom_gate_override = torch.from_numpy(u5).to(DEV), gates3.to(DEV)
    dis.color_override, dis.color_gate_override = torch.from_numpy(u8).to(DEV), cgates.to(DEV)
    dis.filter_override, dis.filter_gate_override = torch.from_numpy(uf).to(DEV), torch.from_numpy(fgates).to(DEV)
    gmat = F.ada_geom_matrix(dis.geom_override, G.ALL, dis.geom_gate_override, dis.ada_state).cpu().numpy()
    cmat = F.ada_color_matrix(dis.color_override, K.ALL, dis.color_gate_override, dis.ada_state).cpu().numpy()
    fmat = F.ada_filter_matrix(dis.filter_override, R.BIT, dis.filter_gate_override, dis.ada_state).cpu().numpy()
    assert float(np.abs(fmat.astype(np.float64) - R.rows(uf, fon)).max()) <= MATRIX_TOL
    assert [R.is_identity(r) for r in fmat] == [True, False, False, False]
    f64 = fmat.astype(np.float64)
    orig = O.discriminator

    def discriminator(p, img, depth_, alpha_, total_depth, **kw):
        aug = K.apply(G.apply(Bl.apply_gated(img, u9, bits5), gmat), cmat)
        aug = R.apply_torch(aug.permute(0, 2, 3, 1), f64).permute(0, 3, 1, 2)
        return orig(p, aug, depth_, alpha_, total_depth, **kw)
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


# ------------------------------------------------------------------------------------------------ 10. graph replay, moving p
def train_run(use_graphs, iters=4, seed=5):
    # 1 / (0.02 * 1000) = 0.05 per image: one update (interval 1) at batch 4 moves p by 0.2
    sg = make_sg(FULL14, use_graphs, ada_target=0.6, ada_interval=1, ada_kimg=0.02, ada_p_init=0.5)
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
    sg.dis.filter_override = torch.from_numpy(R.edge_draws8(8, seed=3)[[0, 2, 5, 7]]).to(DEV)
    sg.dis.filter_gate_override = GC.C.spread_gates5(4)[:, :4].contiguous().to(DEV)
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
    wbuf = torch.full((B * H * W * 3 + 4,), SENTINEL, device=DEV)
    ws, nb = wbuf.data_ptr(), 4 * B * H * W * 3
    mat = torch.tensor([R.IDENTITY] * B, dtype=torch.float32, device=DEV) * 2.0
    u, gates_, state = torch.rand(B, 12, device=DEV), torch.rand(B, 4, device=DEV), dev_state(0.5)
    out = torch.full((B, 22), SENTINEL, device=DEV)
    s = N.stream()
    assert L.sgx_ada_filter_workspace_bytes(B, H, W) == nb and L.sgx_ada_filter_workspace_bytes(B, 1, W) == 0

    def refused(fn):
        N.prof_start(1)
        try:
            rc = fn()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], "a kernel was launched"
        assert bool((y == SENTINEL).all()) and bool((out == SENTINEL).all()) and bool((wbuf == SENTINEL).all())
        return rc != 0
    c = lambda *a: L.sgx_ada_filter(*a)
    for adj in (0, 1):
        assert refused(lambda: c(N.ptr(y), N.ptr(y), N.ptr(mat), B, H, W, adj, ws, nb, s))               # in place
    assert refused(lambda: c(None, N.ptr(y), N.ptr(mat), B, H, W, 0, ws, nb, s))
    assert refused(lambda: c(N.ptr(x), None, N.ptr(mat), B, H, W, 0, ws, nb, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), None, B, H, W, 0, ws, nb, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, W, 0, None, nb, s))                   # no workspace
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, W, 0, ws, nb - 1, s))                 # short
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, W, 1, ws, 0, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, W, 0, ws + 4, nb, s))                 # unaligned
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, W, 0, N.ptr(x), nb, s))               # the workspace is x
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), 0, H, W, 0, ws, nb, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), -1, H, W, 0, ws, nb, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, 1, W, 0, ws, nb, s))                     # H or W < 2: no reflection
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, H, 1, 1, ws, nb, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, 0, W, 0, ws, nb, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(mat), B, 40000, 40000, 0, ws, nb, s))             # beyond 2^31 floats per image
    m = lambda *a: L.sgx_ada_filter_matrix(*a)
    assert refused(lambda: m(N.ptr(u), 7, None, 0, None, 8192, N.ptr(out), B, s))                        # rows too close
    assert refused(lambda: m(N.ptr(u), 12, N.ptr(gates_), 3, N.ptr(state), 8192, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 12, N.ptr(gates_), 4, None, 8192, N.ptr(out), B, s))              # gates without the state
    assert refused(lambda: m(N.ptr(u), 12, None, 0, N.ptr(state), 8192, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 12, None, 0, None, 4096, N.ptr(out), B, s))                       # bits of the other entries
    assert refused(lambda: m(N.ptr(u), 12, None, 0, None, 16383, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 12, None, 0, None, -1, N.ptr(out), B, s))
    assert refused(lambda: m(None, 12, None, 0, None, 8192, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 12, None, 0, None, 8192, None, B, s))
    assert refused(lambda: m(N.ptr(u), 12, None, 0, None, 8192, N.ptr(out), 0, s))
    q = (ctypes.c_int * 13)(*([7] * 13))
    for bad in ((0, 8, 8), (65536, 8, 8), (1, 1, 8), (1, 8, 1), (1, 40000, 40000)):
        assert L.sgx_ada_filter_plan(*bad, 0, 1, ctypes.addressof(q)) != 0 and list(q) == [0] * 13
    assert L.sgx_ada_filter_plan(1, 8, 8, 0, 1, None) != 0
    L.sgx_clear_error()


def test_python_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B = 2
    x = torch.randn(B, 8, 8, 3, device=DEV)
    mat = torch.tensor([R.IDENTITY] * B, dtype=torch.float32, device=DEV) * 2.0
    bad = [lambda: F._ada_filter(torch.randn(B, 8, 8, 4, device=DEV), mat, False),                       # a 4-channel tensor
           lambda: F._ada_filter(x.double(), mat, False), lambda: F._ada_filter(x[0], mat, False),
           lambda: F._ada_filter(x, mat[:, :12].contiguous(), False), lambda: F._ada_filter(x, torch.zeros(B + 1, 22, device=DEV), True),
           lambda: F._ada_filter(x, mat.double(), False), lambda: F._ada_filter(x, mat.reshape(-1), False),  # the table's width, shape or dtype
           lambda: F._ada_filter(x.cpu(), mat.cpu(), False), lambda: F._ada_filter(x, mat.cpu(), False),     # CPU tensors
           lambda: F._ada_filter(x[:, :1].contiguous(), mat, False), lambda: F._ada_filter(x[:, :, :1].contiguous(), mat, True),   # H or W < 2
           lambda: F.ada_filter_matrix(torch.rand(B, 8), 8192),
           lambda: F.ada_filter_matrix(torch.rand(B, 5, device=DEV), 8192), lambda: F.ada_filter_matrix(torch.rand(B, 8, device=DEV).double(), 8192),
           lambda: F.ada_filter_matrix(torch.rand(B, 8, device=DEV), 8192, torch.rand(B, 4, device=DEV)),
           lambda: F.ada_filter_matrix(torch.rand(B, 8, device=DEV), 8192, torch.rand(B, 5, device=DEV), dev_state(0.5)),
           lambda: F.ada_filter_matrix(torch.rand(B, 8, device=DEV), 8192, torch.rand(B, 4, device=DEV), torch.zeros(8))]
    for k, fn in enumerate(bad):
        N.prof_start(1)
        try:
            with pytest.raises(N.SgxError):
                fn()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], (k, "a kernel was launched")
    dis = small_dis(diffaug_policy="imgfilter", ada_target=0.6)
    dis.train()
    dis.filter_override = torch.rand(B, 7, device=DEV)
    with pytest.raises(ValueError, match="filter_override"):
        dis._diffaug(x)
    dis.filter_override, dis.filter_gate_override = torch.rand(B, 8, device=DEV), torch.rand(B, 5, device=DEV)
    with pytest.raises(ValueError, match="filter_gate_override"):
        dis._diffaug(x)
