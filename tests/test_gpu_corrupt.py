"""-m gpu: ADA's image-space corruptions -- additive noise from an in-kernel Philox4x32-10 field and one cutout rectangle per image in
one streaming pass, y = M (x + sigma n) (csrc/adacorrupt.hip: sgx_ada_corrupt_table, sgx_ada_corrupt, sgx_ada_corrupt_plan;
functional.ada_corrupt_table / AdaCorruptFn / AdaCorruptLinFn; Discriminator(diffaug_policy="...,noise,imgcutout")) against the
restatement tests/corrupt_ref.py: the table kernel, both modes per element on both kernels under the device's table and under crafted
rows, vector against px bit for bit, reproducibility, the R1-shaped double backward, continuity with the policies of today, D under
the sixteen-op policy against the oracle, graph replay, and the rejections."""
import ctypes
import random
import types

import numpy as np
import pytest
import torch

import blit_ref as Bl
import color_cases as CC
import color_ref as K
import corrupt_ref as R
import filter_ref as FR
import geom_cases as GC
import geom_ref as G
import golden_util as gu
import streaming_ref as SR
import test_gpu_filter as TF
from aug_gpu_util import bits_equal, dev_state, small_dis
from gpu_util import DEV, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise
from oracle import stylegan_oracle as O
from test_gpu_filter import BIG_KIMG, FULL14, recorded

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64                                       # floats around y (a multiple of 4: y keeps its alignment)
SENTINEL = 12345.5
FULL16 = FULL14 + ",noise,imgcutout"
# sigma = 0.1 |z| of the device's table against fp64 over the draws of test_table_kernel_vs_restatement (z at both clamp ends, u0 = 0, u
# just under 1): logf, sqrtf, cosf and two products of values of at most 0.3.  The largest error measured on the MI355X is
# SIGMA_ERR_MEASURED, the bound four times that (libm differences between releases), under the cap tests/test_gpu_filter.py uses.
SIGMA_ERR_MEASURED = 4.62e-8
SIGMA_TOL = 4 * SIGMA_ERR_MEASURED
assert SIGMA_TOL <= 1e-5
# A normal of the kernels (logf, sqrtf, sincospif, one product, |n| <= 5.77) against fp64 from the same generator outputs: the largest
# |n - n64| measured on the MI355X over SHAPES (the sigma = 1, x = 0 image of test_passes_under_crafted_rows) is N_ERR_MEASURED, N_TOL
# four times that, under the cap.
N_ERR_MEASURED = 4.81e-7                        # (at 300 x 300; 1.3e-7 .. 3.2e-7 at the smaller shapes)
N_TOL = 4 * N_ERR_MEASURED
assert N_TOL <= 1e-5
# (B, H, W, base offset in floats)
SHAPES = [(2, 4, 4, 0), (3, 8, 12, 0), (2, 5, 7, 0), (1, 1, 1, 0), (2, 8, 8, 1), (2, 44, 48, 0), (1, 300, 300, 0)]
SPECIAL = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffc00001, 0x7f800123, 0x00000001, 0x80000001], np.uint32)


def lib_plan(B, H, W, mode, aligned):
    from stylegan.pytorch_amd import native as N
    out = (ctypes.c_int * 5)(*([7] * 5))
    rc = N.lib().sgx_ada_corrupt_plan(B, H, W, int(mode), int(aligned), ctypes.addressof(out))
    assert rc == 0 and out[0] == 1, (rc, list(out))
    return tuple(out[1:])                                                     # (kernel, mode, gx, gy)


def expected_note(H, W, off):
    return "ada_corrupt_vec" if (H * W) % 4 == 0 and off == 0 else "ada_corrupt_px"


def run_corrupt(xd, tabd, mode):
    """sgx_ada_corrupt into a buffer with guard floats on both sides of y; -> y (a copy), the launch held against
    sgx_ada_corrupt_plan, the note's name asserted and the guards checked."""
    from stylegan.pytorch_amd import native as N
    B, H, W, _ = xd.shape
    n = xd.numel()
    off = (xd.data_ptr() // 4) % 4                                          # y gets x's alignment
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=DEV)
    y = buf[GUARD + off:GUARD + off + n].view(B, H, W, 3)
    before = xd.clone()
    N.prof_start(1)
    try:
        rc = N.lib().sgx_ada_corrupt(N.ptr(xd), N.ptr(y), N.ptr(tabd), B, H, W, int(mode), N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    recs = N.prof_records()
    N.check(rc, "sgx_ada_corrupt")
    aligned = xd.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    kernel, pmode, gx, gy = lib_plan(B, H, W, mode, aligned)
    assert pmode == mode and gy == B and kernel == int(aligned and (H * W) % 4 == 0)
    assert gx == ((H * W // 4 if kernel else H * W) + 255) // 256
    want_id = f"ada_corrupt_{'vec' if kernel else 'px'}_kernel<{mode}>"
    got = ([SR.kernel_id(r[0]) for r in recs], [(tuple(g), tuple(b), int(lds)) for g, b, lds in N.prof_launches()])
    assert got == ([want_id], [((gx, gy, 1), (256, 1, 1), 0)]), (got, want_id, gx, gy)
    notes = [r[4].split(" ")[0] for r in recs]
    assert notes == [expected_note(H, W, off)] and recs[0][4].endswith(" lin" if mode else " fwd"), recs
    assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + n:] == SENTINEL).all()), "guard floats of y were written"
    assert bits_equal(xd, before), "x was written"
    return y.clone()


def images(B, H, W, seed, special=True):
    """fp32 [B,H,W,3] normals; with ``special`` every seventh element (from a start that differs per image) is one of -0, the
    infinities, NaNs with payloads of either sign and the smallest denormals."""
    x = np.random.default_rng(seed).standard_normal((B, H, W, 3)).astype(f32)
    if special:
        w = x.view(np.uint32).reshape(B, -1)
        for b in range(B):
            idx = np.arange(b % 7, w.shape[1], 7)
            w[b, idx] = np.resize(SPECIAL, idx.size)
    return x


def to_dev(x, off=0):
    """The fp32 array on the device at a base ``off`` floats past a 16-byte boundary, its bits kept (NaN payloads included)."""
    words = torch.from_numpy(np.ascontiguousarray(x).view(np.int32).reshape(-1).copy())
    buf = torch.zeros(words.numel() + off, dtype=torch.int32, device=DEV)
    buf[off:] = words.to(DEV)
    v = buf[off:].view(torch.float32).view(x.shape)
    assert (v.data_ptr() % 16 == 0) == (off == 0)
    return v


def to_host(y):
    return y.contiguous().view(torch.int32).cpu().numpy().view(f32)


def device_table(B, H, W, seed=0, off_rows=()):
    """The device's own table for edge draws, both ops on; the images of ``off_rows`` gated off."""
    from stylegan.pytorch_amd import functional as F
    u = R.edge_draws6(B, seed)
    g = np.full((B, 2), 0.25, f32)
    g[list(off_rows)] = 0.75
    tab = F.ada_corrupt_table(torch.from_numpy(u).to(DEV), R.ALL, H, W, torch.from_numpy(g).to(DEV), dev_state(0.5))
    return tab, tab.cpu().numpy()


def check_passes(x, tab_np, off, what):
    """Both modes of one batch under one table, per element against the restatement."""
    xd, tabd = to_dev(x, off), torch.from_numpy(tab_np).to(DEV)
    out = {}
    for mode in (0, 1):
        y = to_host(run_corrupt(xd, tabd, mode))
        bad = R.violations(y, x, tab_np, mode, N_TOL)
        assert not bad.any(), (what, mode, off, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        out[mode] = y
    return out


# ------------------------------------------------------------------------------------------------------------ 1. the table kernel
def test_table_kernel_vs_restatement():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B, H, W = 12, 44, 100
    u = R.edge_draws6(B, seed=3)
    ud = torch.from_numpy(u).to(DEV)
    gates = np.resize(R.gate_patterns(), (B, 2)).astype(f32)                 # against p = 0.5: all four on / off patterns, three times over
    gates[5, 0] = 0.5                                                         # a value equal to p (strict <): the noise of row 5 goes off
    gd = torch.from_numpy(gates).to(DEV)
    wide = torch.rand(B, 8, device=DEV)                                      # the same draws and gates as rows of one [B,8] tensor
    wide[:, :6], wide[:, 6:] = ud, gd
    worst = 0.0

    def check(tab, on, what, h=H, w=W):
        nonlocal worst
        ref = R.table(u, h, w, on)
        got = tab.cpu().numpy()
        assert got.dtype == f32 and got.shape == (B, 8)
        assert np.array_equal(R.bits(got[:, 1:]), R.bits(ref[:, 1:])), (what, got, ref)        # the keys, the bounds, the zeros: exact
        for b in range(B):
            if not on[b].any():
                assert not R.bits(got[b]).any(), (what, b, got[b])                              # the all-zero row, +0 throughout
            if not on[b, 0]:
                assert R.bits(got[b, :1])[0] == 0
                continue
            err = abs(float(got[b, 0]) - float(R.sigma64(u[b:b + 1])[0]))
            worst = max(worst, err)
            assert err <= SIGMA_TOL, (what, b, err)
    N.prof_start(1)
    try:
        tab = F.ada_corrupt_table(ud, R.ALL, H, W)
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    assert [r[4].split(" ")[0] for r in N.prof_records()] == ["ada_corrupt_table"]
    every = np.ones((B, 2), bool)
    check(tab, every, "ungated")
    assert float(tab[2, 0]) == 0.0 and float(tab[0, 0]) == pytest.approx(0.3, abs=SIGMA_TOL)                 # u0 = 0; the clamp
    assert torch.equal(tab, F.ada_corrupt_table(wide[:, :6], R.ALL, H, W))     # the row stride; and bit-reproducible
    assert torch.equal(tab, F.ada_corrupt_table(ud, 65535, H, W))              # the other stages' bits are masked by the wrapper
    for h, w in ((1, 1), (5, 7), (1024, 3)):
        check(F.ada_corrupt_table(ud, R.ALL, h, w), every, ("size", h, w), h, w)
    check(F.ada_corrupt_table(ud, R.NOISE, H, W), every & np.array([True, False]), "noise alone")
    check(F.ada_corrupt_table(ud, R.CUTOUT, H, W), every & np.array([False, True]), "cutout alone")
    for p in (0.0, 0.5, 1.0):
        on = R.gates(gates, p)
        tab = F.ada_corrupt_table(ud, R.ALL, H, W, gd, dev_state(p))
        check(tab, on, ("gated", p))
        assert torch.equal(tab, F.ada_corrupt_table(wide[:, :6], R.ALL, H, W, wide[:, 6:], dev_state(p)))
        if p == 0.0:
            assert not on.any()
        if p == 1.0:
            assert on.all()
        if p == 0.5:
            assert [int(a) + 2 * int(b) for a, b in on] == [0, 1, 2, 3, 0, 0, 2, 3, 0, 1, 2, 3]
    assert not R.bits(F.ada_corrupt_table(ud, 0, H, W).cpu().numpy()).any()                             # neither op in the policy
    assert not R.bits(F.ada_corrupt_table(ud, 16383, H, W).cpu().numpy()).any()                         # the other stages' bits
    print("table kernel: largest |sigma - fp64| =", worst, "bound", SIGMA_TOL)


# ----------------------------------------------------------------------------------------------------- 2. / 3. the passes, per shape
def crafted_rows(H, W):
    """sigma = 1 (on x = 0: the field itself), sigma = 0 with a rectangle, a rectangle over the whole image, an empty rectangle with
    sigma != 0, the identity row."""
    return np.array([[1.0, 77.0, 16777215.0, 0, 0, 0, 0, 0], [0.0, 0.0, 0.0, W // 3, W, 0, (H + 1) // 2, 0],
                     [0.25, 5.0, 6.0, 0, W, 0, H, 0], [0.125, 123456.0, 654321.0, W, W // 2, 0, H, 0], [0.0] * 8], f32)


@pytest.mark.parametrize("B,H,W,off", SHAPES)
def test_passes_under_the_device_table(B, H, W, off):
    """Both modes under the device's own table for edge draws (the last image gated off where there is more than one): mode 1, cut
    pixels and images without noise bit for bit (the inputs hold -0, the infinities and NaN payloads), noisy elements within
    2^-24 (|sigma n64| + |y64|) + sigma N_TOL of the fp64 restatement under the same fp32 row."""
    tabd, tab = device_table(B, H, W, seed=H + W, off_rows=(B - 1,) if B > 1 else ())
    assert B == 1 or not tab[B - 1].any()
    x = images(B, H, W, seed=H * 1000 + W)
    ys = check_passes(x, tab, off, "device table")
    if B > 1:
        assert np.array_equal(R.bits(ys[0][B - 1]), R.bits(x[B - 1])) and np.array_equal(R.bits(ys[1][B - 1]), R.bits(x[B - 1]))


@pytest.mark.parametrize("B,H,W,off", SHAPES)
def test_passes_under_crafted_rows(B, H, W, off):
    rows = crafted_rows(H, W)
    x = images(5, H, W, seed=H * 1000 + W + 1)
    x[0] = 0.0
    ys = check_passes(x, rows, off, "crafted rows")
    n64 = R.field(77, 16777215, 3 * H * W).reshape(H, W, 3)
    err = float(np.abs(ys[0][0].astype(np.float64) - n64).max())
    print(H, W, off, "largest |n - n64| =", err, "N_TOL", N_TOL)
    assert err <= N_TOL + 2.0 ** -24 * float(np.abs(n64).max())                      # sigma = 1 on x = 0: the field itself
    assert not R.bits(ys[0][2]).any() and not R.bits(ys[1][2]).any()                 # the whole image cut: +0 everywhere
    assert np.array_equal(R.bits(ys[1][3]), R.bits(x[3]))                            # an empty rectangle: mode 1 is the copy
    for mode in (0, 1):
        assert np.array_equal(R.bits(ys[mode][4]), R.bits(x[4]))                     # the identity row copies


# ----------------------------------------------------------------------------------------------- 4. / 5. vector == px, reproducibility
@pytest.mark.parametrize("H,W", [(4, 4), (8, 12), (44, 48)])
def test_vector_and_px_kernels_agree_bit_for_bit(H, W):
    B = 3
    tabd, tab = device_table(B, H, W, seed=9)
    rows = torch.from_numpy(crafted_rows(H, W)[[0, 2, 3]]).to(DEV)
    x = images(B, H, W, seed=5, special=False)
    for t in (tabd, rows):
        for mode in (0, 1):
            a = run_corrupt(to_dev(x, 0), t, mode)
            b = run_corrupt(to_dev(x, 1), t, mode)
            assert bits_equal(a, b), (H, W, mode)


def test_reproducible_under_one_table_and_fresh_under_another():
    B, H, W = 2, 16, 20
    x = to_dev(images(B, H, W, seed=1, special=False))
    t1 = torch.tensor([[0.2, 11.0, 12.0, 0, 0, 0, 0, 0]] * B, device=DEV)
    t2 = torch.tensor([[0.2, 11.0, 13.0, 0, 0, 0, 0, 0], [0.2, 12.0, 12.0, 0, 0, 0, 0, 0]], device=DEV)
    a, b, c = run_corrupt(x, t1, 0), run_corrupt(x, t1, 0), run_corrupt(x, t2, 0)
    assert bits_equal(a, b)                                                               # one table: the same bits
    assert float(((a - c).abs() > 1e-3).float().mean()) > 0.9                             # another key (k1, or k0): another field
    z0 = torch.zeros_like(x)                                                              # two images under one key: one field
    f = run_corrupt(z0, t1, 0)
    assert bits_equal(f[0], f[1]) and float(f.std()) == pytest.approx(0.2, rel=0.1)


# ---------------------------------------------------------------------------------------------------------------------- 6. autograd
def test_first_and_second_order_through_the_functions():
    """logit = <w, y(x)>: grad in x is linear(w) bit for bit (the noise carries no gradient); the R1-shaped double backward -- gx with
    create_graph, the penalty sum gx^2, its gradient in w -- runs forward, linear, linear and gives linear(2 linear(w)) = 2 linear(w)
    on the 0/1 mask, bit for bit."""
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B, H, W = 3, 12, 20
    tabd, tab = device_table(B, H, W, seed=4)
    assert (tab[:, 0] != 0).sum() >= 2 and R.cut_mask(tab, H, W).any()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, H, W, 3, generator=g)
    w = torch.randn(B, H, W, 3, generator=g)
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    N.prof_start(1)
    try:
        y = F.call(F.AdaCorruptFn, xd, tabd)
        gx, = torch.autograd.grad((y * wd).sum(), xd, create_graph=True)
        gw, = torch.autograd.grad(gx.pow(2).sum(), wd)
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    names = [SR.kernel_id(r[0]) for r in N.prof_records() if r[4].startswith("ada_corrupt")]
    assert names == ["ada_corrupt_vec_kernel<0>", "ada_corrupt_vec_kernel<1>", "ada_corrupt_vec_kernel<1>"], names   # the noise: once
    lin_w = R.linear(w.numpy(), tab)
    assert not R.violations(to_host(y.detach()), x.numpy(), tab, 0, N_TOL).any()
    assert np.array_equal(R.bits(to_host(gx.detach())), R.bits(lin_w))
    assert np.array_equal(R.bits(to_host(gw.detach())), R.bits(R.linear(2.0 * lin_w, tab)))
    # the D step's fakes: no input gradient is asked for, none is computed
    ctx = types.SimpleNamespace(needs_input_grad=(False, False), saved_tensors=(tabd,))
    assert F.AdaCorruptFn.backward(ctx, x.to(DEV)) == (None, None)
    assert not F.call(F.AdaCorruptFn, x.to(DEV), tabd).requires_grad


# -------------------------------------------------------------------------------------------------------------------- 7. continuity
def test_old_policies_launch_what_they_launched():
    B = 8
    img = torch.randn(B, 16, 16, 3, device=DEV)
    u9 = torch.from_numpy(Bl.edge_draws9(B, seed=2)).to(DEV)
    u5 = torch.from_numpy(G.edge_draws5(B, seed=2)).to(DEV)
    u8 = torch.from_numpy(K.edge_draws8(B, seed=2)).to(DEV)
    uf = torch.from_numpy(FR.edge_draws8(B, seed=2)).to(DEV)
    ada = dict(ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG)
    gates5, gates3, gates4 = torch.rand(B, 5, device=DEV), torch.rand(B, 3, device=DEV), torch.rand(B, 4, device=DEV)
    outs = []
    for policy in (FULL14, FULL16):
        d = small_dis(diffaug_policy=policy, **ada)
        d.train()
        d.diffaug_override, d.geom_override, d.color_override, d.filter_override = u9, u5, u8, uf
        d.ada_gate_override, d.geom_gate_override, d.color_gate_override, d.filter_gate_override = gates5, gates3, gates5, gates4
        d.corrupt_override = torch.from_numpy(R.edge_draws6(B)).to(DEV)
        d.corrupt_gate_override = torch.full((B, 2), 0.75, device=DEV)      # both ops gated off for every image
        outs.append(recorded(lambda: d._diffaug(img)))
    (y14, n14, g14), (y16, n16, g16) = outs
    # the fourteen-op launches in front of the new stage's, and with both ops gated off the fourteen-op result, bit for bit
    assert n16 == n14 + ["ada_corrupt_table", "ada_corrupt_vec"] and g16[:len(g14)] == g14 and g16[len(g14):] == [(1, 1, 1), (1, B, 1)], (n16, g16)
    assert bits_equal(y16, y14)
    plain = small_dis(diffaug_policy=FULL14)                                 # the fourteen-op policy launches what it launched
    plain.train()
    plain.diffaug_override, plain.geom_override, plain.color_override, plain.filter_override = u9, u5, u8, uf
    plain.corrupt_override = torch.rand(B, 5, device=DEV)                   # (never looked at: the policy has neither op)
    _, notes, grids = recorded(lambda: plain._diffaug(img))
    assert notes == ["diffaug_blit_sum", "diffaug_blit_tile", "ada_geom_matrix", "ada_geom_tile", "ada_color_matrix", "ada_color_vec",
                     "ada_filter_matrix", "ada_filter_px", "ada_filter_px"], notes
    assert grids[:6] == [(1, B, 1), (1, B, 1), (1, 1, 1), (1, B, 1), (1, 1, 1), (1, B, 1)], grids
    default = small_dis()                                                    # the default policy launches none of it
    default.train()
    _, notes, _ = recorded(lambda: default(torch.randn(4, 3, 8, 8, device=DEV), 1, 1.0))
    assert notes and not [n for n in notes if n.startswith(("ada_", "diffaug"))], notes


def test_training_forward_draws_its_own_six_or_eight():
    from stylegan.pytorch_amd import functional as F
    B = 4
    img = torch.randn(B, 16, 16, 3, device=DEV)
    for ada in (False, True):
        kw = dict(ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG) if ada else {}
        dis = small_dis(diffaug_policy=FULL16, **kw)
        dis.train()
        torch.cuda.manual_seed(77)
        y = dis._diffaug(img)
        after = torch.cuda.get_rng_state()
        old = small_dis(diffaug_policy=FULL14, **kw)
        old.train()
        torch.cuda.manual_seed(77)
        y14 = old._diffaug(img)                                              # what the fourteen-op policy draws today, then the stage's own
        r = torch.rand(B, 8 if ada else 6, device=DEV)
        assert torch.equal(after, torch.cuda.get_rng_state())
        tab = F.ada_corrupt_table(r[:, :6], R.ALL, 16, 16, *((r[:, 6:], dis.ada_state) if ada else ()))
        assert bits_equal(y, F.call(F.AdaCorruptFn, y14, tab))
        assert ("ada_state" in dis.state_dict()) == ada


# ----------------------------------------------------------------------------------------------------------------------- 8. network
def corrupt_network_draws(depth):
    """-> (u [4,6], gate uniforms [4,2], on [4,2]) at p = 0.5: image 0 both ops off, 1 the noise, 2 the cutout, 3 both."""
    gates = R.gate_patterns()
    return R.edge_draws6(5, seed=depth)[[4, 1, 2, 3]], gates, R.gates(gates, CC.NET_P)


def test_network_first_and_second_order_vs_oracle(monkeypatch):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss under the sixteen-op policy with per-image gates
    (p = 0.5, all seven override pairs pinned) at one depth with fade-in, against the fp64 composition corrupt_ref o filter_ref o
    color_ref o geom_ref o blit_ref o the oracle's D, under the tables the device produced; the criteria of tests/test_gpu_filter.py's
    network test."""
    from stylegan.pytorch_amd import Losses
    from stylegan.pytorch_amd import functional as F
    depth, alpha = 3, 0.3
    B, res = CC.NET_B, 4 * 2 ** depth
    dp = mid_params(torch.float64)[1]
    dis = TF.load_ada(TF.mid_dis(FULL16, ada_target=0.6, ada_p_init=CC.NET_P, ada_kimg=BIG_KIMG), dp)
    dis.train()
    u9, gates5, bits5 = GC.C.network_draws(depth)
    u5, gates3, bits3 = GC.network_draws(depth)
    u8, cgates, cbits = CC.network_draws(depth)
    uf, fgates, fon = TF.filter_network_draws(depth)
    uc, ngates, non = corrupt_network_draws(depth)
    dis.diffaug_override, dis.ada_gate_override = torch.from_numpy(u9).to(DEV), gates5.to(DEV)
    dis.geom_override, dis.geom_gate_override = torch.from_numpy(u5).to(DEV), gates3.to(DEV)
    dis.color_override, dis.color_gate_override = torch.from_numpy(u8).to(DEV), cgates.to(DEV)
    dis.filter_override, dis.filter_gate_override = torch.from_numpy(uf).to(DEV), torch.from_numpy(fgates).to(DEV)
    dis.corrupt_override, dis.corrupt_gate_override = torch.from_numpy(uc).to(DEV), torch.from_numpy(ngates).to(DEV)
    gmat = F.ada_geom_matrix(dis.geom_override, G.ALL, dis.geom_gate_override, dis.ada_state).cpu().numpy()
    cmat = F.ada_color_matrix(dis.color_override, K.ALL, dis.color_gate_override, dis.ada_state).cpu().numpy()
    fmat = F.ada_filter_matrix(dis.filter_override, FR.BIT, dis.filter_gate_override, dis.ada_state).cpu().numpy()
    ntab = F.ada_corrupt_table(dis.corrupt_override, R.ALL, res, res, dis.corrupt_gate_override, dis.ada_state).cpu().numpy()
    ref_tab = R.table(uc, res, res, non)
    assert np.array_equal(ntab[:, 1:], ref_tab[:, 1:]) and float(np.abs(ntab[:, 0].astype(np.float64) - R.sigma64(uc) * non[:, 0]).max()) <= SIGMA_TOL
    assert [bool(r[0] != 0) for r in ntab] == [False, True, False, True] and R.cut_mask(ntab, res, res).any(axis=(1, 2)).tolist() == [False, False, True, True]
    f64 = fmat.astype(np.float64)
    keep = torch.from_numpy(~R.cut_mask(ntab, res, res)).double()[..., None]
    sn = torch.from_numpy(R.noise_term(ntab, res, res))
    orig = O.discriminator

    def discriminator(p, img, depth_, alpha_, total_depth, **kw):
        aug = K.apply(G.apply(Bl.apply_gated(img, u9, bits5), gmat), cmat)
        aug = FR.apply_torch(aug.permute(0, 2, 3, 1), f64)
        aug = (keep * (aug + sn)).permute(0, 3, 1, 2)
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


# ------------------------------------------------------------------------------------------------------------------ 9. graph replay
def capture(dis, img):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dis._diffaug(img)                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = dis._diffaug(img)
    return g, out


def test_stage_replay_fresh_noise_a_moving_p_and_overrides():
    """The stage captured on its own: without overrides two replays draw different noise, and p is read on the device at every replay
    (p = 0 copies the image, p = 1 corrupts it); with both overrides set a replay is the eager result, bit for bit."""
    B = 4
    img = torch.randn(B, 16, 16, 3, device=DEV)
    dis = small_dis(diffaug_policy="noise,imgcutout", ada_target=0.6, ada_p_init=1.0, ada_kimg=BIG_KIMG)
    dis.train()
    g, out = capture(dis, img)
    g.replay(); a = out.clone()
    g.replay(); b = out.clone()
    assert not bits_equal(a, b) and not bits_equal(a, img)
    dis.ada_state[0] = 0.0
    g.replay()
    assert bits_equal(out, img)
    dis.ada_state[0] = 1.0
    g.replay()
    assert not bits_equal(out, img)
    dis.corrupt_override = torch.from_numpy(R.edge_draws6(B, seed=1)).to(DEV)
    dis.corrupt_gate_override = torch.from_numpy(R.gate_patterns()).to(DEV)
    dis.ada_state[0] = 0.5
    eager = dis._diffaug(img).clone()
    g2, out2 = capture(dis, img)
    g2.replay(); first = out2.clone()
    g2.replay()
    assert bits_equal(first, eager) and bits_equal(out2, eager)
    assert bits_equal(eager[0], img[0]) and not bits_equal(eager[1], img[1])


def train_run(use_graphs, iters=4, seed=5):
    from stylegan.pytorch_amd.GAN import StyleGAN
    MID = TF.MID
    # 1 / (0.02 * 1000) = 0.05 per image: one update (interval 1) at batch 4 moves p by 0.2
    sg = StyleGAN(structure="linear", resolution=128, num_channels=3, latent_size=512,
                  g_args=dict(latent_size=512, mapping_layers=MID["mapping_layers"], blur_filter=[1, 2, 1], truncation_psi=0.7,
                              truncation_cutoff=8, fmap_base=MID["fmap_base"], fmap_max=MID["fmap_max"]),
                  d_args=dict(use_wscale=True, blur_filter=[1, 2, 1], fmap_base=MID["fmap_base"], fmap_max=MID["fmap_max"],
                              diffaug_policy=FULL16, ada_target=0.6, ada_interval=1, ada_kimg=0.02, ada_p_init=0.5),
                  g_opt_args=TF.OPT, d_opt_args=TF.OPT, loss="logistic", d_repeats=1, use_ema=True, ema_decay=0.999,
                  device=torch.device(DEV), use_graphs=use_graphs)
    gp, dp = mid_params(torch.float64)
    load_into(sg.gen, gp); TF.load_ada(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, mid_noises(4))
    sg.dis.diffaug_override = torch.from_numpy(Bl.edge_draws9(8, seed=3)[[0, 3, 4, 7]]).to(DEV)
    sg.dis.ada_gate_override = GC.C.spread_gates5(4).to(DEV)
    sg.dis.geom_override = torch.from_numpy(G.edge_draws5(8, seed=3)[[0, 1, 3, 7]]).to(DEV)
    sg.dis.geom_gate_override = GC.spread_gates3(4).to(DEV)
    sg.dis.color_override = torch.from_numpy(K.edge_draws8(10, seed=3)[[3, 5, 6, 9]]).to(DEV)
    sg.dis.color_gate_override = GC.C.spread_gates5(4).to(DEV)
    sg.dis.filter_override = torch.from_numpy(FR.edge_draws8(8, seed=3)[[0, 2, 5, 7]]).to(DEV)
    sg.dis.filter_gate_override = GC.C.spread_gates5(4)[:, :4].contiguous().to(DEV)
    sg.dis.corrupt_override = torch.from_numpy(R.edge_draws6(8, seed=3)[[0, 2, 5, 7]]).to(DEV)
    sg.dis.corrupt_gate_override = GC.C.spread_gates5(4)[:, 1:3].contiguous().to(DEV)
    torch.manual_seed(seed); random.seed(seed)
    losses, states = [], []
    for i in range(iters):
        alpha = min(1.0, 0.25 + 0.15 * i)
        zl = gu.seeded((4, 512), 100 + i).to(DEV); real = gu.seeded((4, 3, 128, 128), 200 + i).to(DEV)
        losses.append((float(sg.optimize_discriminator(zl, real, 5, alpha)), float(sg.optimize_generator(zl, real, 5, alpha))))
        states.append(sg.dis.ada_state.cpu().clone())
    torch.cuda.synchronize()
    return losses, states, sg


def test_step_graph_replay_matches_eager_with_a_moving_p():
    """The whole training step under the sixteen-op policy, p moved by the controller at every step (ada_interval 1, a small ada_kimg),
    replayed against eager.  The overrides are pinned: without them eager and replay draw from different generator streams and have
    no common value to compare.  The step is held to the loss tolerance of tests/test_gpu_graphs.py, not to bits: the eager step
    takes the fade-in alpha from the host and folds it into from_rgb's weights, a replay reads it from device memory, so the two
    round the residual branch differently whatever the policy.  The bit-for-bit replay of THIS stage, its fresh noise without
    overrides and its reading p on the device at every replay are asserted on the captured stage above, where nothing else differs."""
    from test_gpu_graphs import losses_agree
    le, se, _ = train_run(False)
    lg, sg_, sg = train_run(True)
    assert all(g.graph is not None for g in sg._step_graphs.values()) and len(sg._step_graphs) == 2
    for i, (a, b) in enumerate(zip(se, sg_)):
        assert torch.equal(a, b), (i, a, b)
    assert [float(s[5]) for s in se] == [1.0, 2.0, 3.0, 4.0]
    assert len({float(s[0]) for s in se}) > 1                               # p moved between the replays
    losses_agree(le, lg)
    n = len(sg._step_graphs)                                                # the overrides' pointers are part of the step-graph key
    sg.dis.corrupt_override = sg.dis.corrupt_override.clone()
    zl, real = gu.seeded((4, 512), 100).to(DEV), gu.seeded((4, 3, 128, 128), 200).to(DEV)
    sg.optimize_discriminator(zl, real, 5, 0.5)
    assert len(sg._step_graphs) == n + 1


# ------------------------------------------------------------------------------------------------------------------ 10. rejections
def test_c_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    B, H, W = 2, 8, 8
    x = torch.randn(B, H, W, 3, device=DEV)
    y = torch.full((B, H, W, 3), SENTINEL, device=DEV)
    tab = torch.tensor([[0.5, 1.0, 2.0, 0, 4, 0, 4, 0]] * B, dtype=torch.float32, device=DEV)
    u, gates_, state = torch.rand(B, 8, device=DEV), torch.rand(B, 2, device=DEV), dev_state(0.5)
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
    c = lambda *a: L.sgx_ada_corrupt(*a)
    for mode in (0, 1):
        assert refused(lambda: c(N.ptr(y), N.ptr(y), N.ptr(tab), B, H, W, mode, s))                      # in place
    assert refused(lambda: c(None, N.ptr(y), N.ptr(tab), B, H, W, 0, s))
    assert refused(lambda: c(N.ptr(x), None, N.ptr(tab), B, H, W, 0, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), None, B, H, W, 0, s))
    for bad_b in (0, -1, 65536):
        assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(tab), bad_b, H, W, 0, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(tab), B, 0, W, 0, s))                             # H or W < 1
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(tab), B, H, 0, 1, s))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(tab), B, H, -3, 0, s))
    assert c(N.ptr(x), N.ptr(y), N.ptr(tab), B, 40000, 40000, 0, s) == L.sgx_ada_corrupt_plan(B, 40000, 40000, 0, 1, ctypes.addressof((ctypes.c_int * 5)()))
    assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(tab), B, 40000, 40000, 0, s))                     # beyond 2^31 floats per image
    for bad_mode in (-1, 2, 3):
        assert refused(lambda: c(N.ptr(x), N.ptr(y), N.ptr(tab), B, H, W, bad_mode, s))
    m = lambda *a: L.sgx_ada_corrupt_table(*a)
    assert refused(lambda: m(N.ptr(u), 5, None, 0, None, 49152, H, W, N.ptr(out), B, s))                 # rows too close
    assert refused(lambda: m(N.ptr(u), 8, N.ptr(gates_), 1, N.ptr(state), 49152, H, W, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, N.ptr(gates_), 2, None, 49152, H, W, N.ptr(out), B, s))        # gates without the state
    assert refused(lambda: m(N.ptr(u), 8, None, 0, N.ptr(state), 49152, H, W, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 8192, H, W, N.ptr(out), B, s))                  # bits of the other entries
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 65535, H, W, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, -1, H, W, N.ptr(out), B, s))
    assert refused(lambda: m(None, 8, None, 0, None, 49152, H, W, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 49152, H, W, None, B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 49152, H, W, N.ptr(out), 0, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 49152, 0, W, N.ptr(out), B, s))
    assert refused(lambda: m(N.ptr(u), 8, None, 0, None, 49152, H, 0, N.ptr(out), B, s))
    q = (ctypes.c_int * 5)(*([7] * 5))
    for bad in ((0, 8, 8, 0), (65536, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 1), (1, 40000, 40000, 0), (1, 8, 8, 2), (1, 8, 8, -1)):
        for i in range(5):
            q[i] = 7
        assert L.sgx_ada_corrupt_plan(*bad, 1, ctypes.addressof(q)) != 0 and list(q) == [0] * 5, bad
    assert L.sgx_ada_corrupt_plan(1, 8, 8, 0, 1, None) != 0
    assert L.sgx_ada_corrupt_plan(1, 1, 1, 1, 0, ctypes.addressof(q)) == 0 and list(q) == [1, 0, 1, 1, 1]
    L.sgx_clear_error()


def test_python_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    B = 2
    x = torch.randn(B, 8, 8, 3, device=DEV)
    tab = torch.zeros(B, 8, device=DEV)
    r6 = lambda: torch.rand(B, 6, device=DEV)
    bad = [lambda: F._ada_corrupt(torch.randn(B, 8, 8, 4, device=DEV), tab, 0),                          # a 4-channel tensor
           lambda: F._ada_corrupt(x.double(), tab, 0), lambda: F._ada_corrupt(x[0], tab, 1),
           lambda: F._ada_corrupt(x, tab[:, :6].contiguous(), 0), lambda: F._ada_corrupt(x, torch.zeros(B + 1, 8, device=DEV), 1),
           lambda: F._ada_corrupt(x, tab.double(), 0), lambda: F._ada_corrupt(x, tab.reshape(-1), 0),      # the table's width, shape or dtype
           lambda: F._ada_corrupt(x.cpu(), tab.cpu(), 0), lambda: F._ada_corrupt(x, tab.cpu(), 0),         # CPU tensors
           lambda: F._ada_corrupt(x, tab, 2), lambda: F._ada_corrupt(x, tab, -1),                          # the mode
           lambda: F.ada_corrupt_table(torch.rand(B, 6), 49152, 8, 8),
           lambda: F.ada_corrupt_table(torch.rand(B, 5, device=DEV), 49152, 8, 8), lambda: F.ada_corrupt_table(r6().double(), 49152, 8, 8),
           lambda: F.ada_corrupt_table(r6(), 49152, 0, 8), lambda: F.ada_corrupt_table(r6(), 49152, 8, 0),
           lambda: F.ada_corrupt_table(r6(), 49152, 8, 8, torch.rand(B, 2, device=DEV)),
           lambda: F.ada_corrupt_table(r6(), 49152, 8, 8, torch.rand(B, 3, device=DEV), dev_state(0.5)),
           lambda: F.ada_corrupt_table(r6(), 49152, 8, 8, torch.rand(B, 2, device=DEV), torch.zeros(8))]
    for k, fn in enumerate(bad):
        N.prof_start(1)
        try:
            with pytest.raises(N.SgxError):
                fn()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], (k, "a kernel was launched")
    dis = small_dis(diffaug_policy="noise", ada_target=0.6)
    dis.train()
    dis.corrupt_override = torch.rand(B, 5, device=DEV)
    with pytest.raises(ValueError, match="corrupt_override"):
        dis._diffaug(x)
    dis.corrupt_override, dis.corrupt_gate_override = torch.rand(B, 6, device=DEV), torch.rand(B, 3, device=DEV)
    with pytest.raises(ValueError, match="corrupt_gate_override"):
        dis._diffaug(x)
