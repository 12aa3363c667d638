"""-m gpu: the geometric resample with reflection padding (csrc/adageompad.hip: sgx_ada_geom_reflect, sgx_ada_geom_reflect_plan;
functional.AdaGeomReflectFn / AdaGeomReflectAdjFn; Discriminator(geom_padding="reflect")) against the restatement in
tests/geom_pad_ref.py: both kernels per element with the project's bound, exact rows and one-hot columns bit for bit, sgx_ada_geom's
bits where no tap leaves the image, the default path unchanged, D with its R1 double backward under mixed per-image gates, graph replay
with a moving p, and the rejections.  Tables, draws and helpers are those of tests/test_gpu_geom.py."""
import ctypes
import random

import numpy as np
import pytest
import torch

import blit_ref as Bl
import geom_cases as GC
import geom_pad_ref as GP
import geom_ref as G
import golden_util as gu
import streaming_ref as SR
from aug_gpu_util import bits_equal, dparams, load_ada, make_sg, mid_dis, nchw, nhwc, on_device, recorded, small_dis
from gpu_util import DEV, MID_DEPTH, load_into, mid_noises, mid_params, pin_noise
from oracle import stylegan_oracle as O
from test_gpu_geom import BIG_KIMG, EPS, GUARD, MATRIX_TOL, SENTINEL, SUPPLIED, device_table, ints, run_geom

pytestmark = pytest.mark.gpu

f32 = np.float32
PLAN_INTS = 6


def lib_plan(B, H, W, adjoint, aligned):
    from stylegan.pytorch_amd import native as N
    out = (ctypes.c_int * PLAN_INTS)(*([7] * PLAN_INTS))
    rc = N.lib().sgx_ada_geom_reflect_plan(B, H, W, int(adjoint), int(aligned), ctypes.addressof(out))
    assert rc == 0 and out[0] == 1, (rc, list(out))
    return tuple(out[1:])                                                     # (kernel, ADJ, gx, gy, tiles)


def expected_note(W, off):
    return "ada_geom_reflect_tile" if W % 4 == 0 and off == 0 else "ada_geom_reflect_px"


def run_reflect(xd, matd, adjoint):
    """sgx_ada_geom_reflect into a buffer with guard floats on both sides of y; -> y (a copy).  The recorded launch is the plan
    query's, the note's name is the path's, the guards and x are untouched."""
    from stylegan.pytorch_amd import native as N
    B, H, W, _ = xd.shape
    n = xd.numel()
    off = (xd.data_ptr() // 4) % 4                                          # y gets x's alignment
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device=DEV)
    y = buf[GUARD + off:GUARD + off + n].view(B, H, W, 3)
    before = xd.clone()
    N.prof_start(1)
    try:
        rc = N.lib().sgx_ada_geom_reflect(N.ptr(xd), N.ptr(y), N.ptr(matd), B, H, W, int(adjoint), N.stream())
        torch.cuda.synchronize()
    finally:
        N.prof_start(0)
    recs = N.prof_records()
    N.check(rc, "sgx_ada_geom_reflect")
    aligned = xd.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    kernel, adj, gx, gy, tiles = lib_plan(B, H, W, adjoint, aligned)
    assert kernel == int(aligned and W % 4 == 0) and adj == int(adjoint) and gy == B
    assert (gx, tiles) == ((-(-H // 32) * -(-W // 32), -(-W // 32)) if kernel else (-(-H * W // 256), 0))
    want_id = f"ada_geom_reflect_{'tile' if kernel else 'px'}_kernel<{'true' if adjoint else 'false'}>"
    got = ([SR.kernel_id(r[0]) for r in recs], [(tuple(g), tuple(b), int(lds)) for g, b, lds in N.prof_launches()])
    assert got == ([want_id], [((gx, gy, 1), (256, 1, 1), 0)]), (got, want_id, gx, gy)
    assert [r[4].split(" ")[0] for r in recs] == [expected_note(W, off)] and recs[0][4].endswith(" adj" if adjoint else " fwd"), recs
    assert bool((buf[:GUARD + off] == SENTINEL).all()) and bool((buf[GUARD + off + n:] == SENTINEL).all()), "guard floats were written"
    assert bits_equal(xd, before), "x was written"
    return y.clone()


# ------------------------------------------------------------------------------------------- 1. per element against fp64
SHAPES = [(2, 2, 0), (2, 5, 0), (5, 7, 0), (8, 8, 0), (16, 16, 0), (33, 31, 0), (36, 36, 0), (33, 64, 0), (16, 16, 1)]
_bounds = {}


def counts(mat, H, W, adjoint):
    """[B,H,W,1] coefficients per output element, computed once per (table, shape, direction)."""
    key = (mat.tobytes(), H, W, bool(adjoint))
    if key not in _bounds:
        _bounds[key] = torch.stack([torch.from_numpy(GP.tap_counts(row, H, W, adjoint)) for row in mat]).unsqueeze(-1)
    return _bounds[key]


def element_bound(x, mat, adjoint):
    """2 (n + 1) 2^-24 sum |w x| per element: one rounding per product and per addition, a margin of 2 (the project's bound)."""
    B, H, W, _ = x.shape
    return 2.0 * (counts(mat, H, W, adjoint) + 1).double() * EPS * nhwc(GP.apply(nchw(x).double().abs(), mat, adjoint))


def check_elements(y, x, mat, adjoint, what):
    B, H, W, _ = x.shape
    ref = nhwc(GP.apply(nchw(x).double(), mat, adjoint))
    bound = element_bound(x, mat, adjoint)
    n = counts(mat, H, W, adjoint)
    yc = y.cpu()
    worst = 0.0
    for b in range(B):
        if G.is_identity(mat[b]):
            assert bits_equal(yc[b], x[b]), (what, b)
            continue
        err = (yc[b].double() - ref[b]).abs()
        worst = max(worst, float((err / bound[b].clamp_min(1e-300)).max()))
        assert bool((err <= bound[b]).all()), (what, b, float((err - bound[b]).max()))
        empty = (n[b] == 0).expand(H, W, 3)
        assert bool((yc[b].view(torch.int32)[empty] == 0).all()), (what, b, "an element without a coefficient must be +0")
    return worst


@pytest.mark.parametrize("H,W,off", SHAPES)
def test_resample_vs_restatement(H, W, off):
    B = 8
    g = torch.Generator().manual_seed(H * 1000 + W + off)
    x = torch.randn(B, H, W, 3, generator=g)
    gy = torch.randn(B, H, W, 3, generator=g)
    xd, gd = on_device(x, off), on_device(gy, off)
    assert (xd.data_ptr() % 16 == 0) == (off == 0)
    dev_mat, _, bits = device_table(B, seed=H + W)
    assert any(not b & G.ALL for b in bits) and any(b & G.ALL for b in bits)                 # mixed identity and other rows
    for name, matd in (("device", dev_mat), ("supplied", torch.from_numpy(SUPPLIED).to(DEV))):
        mat = matd.cpu().numpy()
        ax = run_reflect(xd, matd, False)
        aty = run_reflect(gd, matd, True)
        for adjoint, inp, out in ((False, x, ax), (True, gy, aty)):
            worst = check_elements(out, inp, mat, adjoint, (name, adjoint))
            print(name, "adjoint" if adjoint else "forward", "largest err / bound", worst)
            assert bits_equal(out, run_reflect(on_device(inp, off), matd, adjoint))          # bit-reproducible
        # <R x, g> = <x, R^T g>: each side within the sum of its per-element bounds (and the fp64 reference's own rounding)
        lhs, rhs = float((ax.double().cpu() * gy.double()).sum()), float((x.double() * aty.double().cpu()).sum())
        tol_l = float((element_bound(x, mat, False) * gy.double().abs()).sum())
        tol_r = float((element_bound(gy, mat, True) * x.double().abs()).sum())
        scale = float((nhwc(GP.apply(nchw(x).double().abs(), mat)) * gy.double().abs()).sum())
        print(name, "transpose: |lhs - rhs|", abs(lhs - rhs), "bound", tol_l + tol_r)
        assert abs(lhs - rhs) <= tol_l + tol_r + 1e-12 * scale + 1e-30, (name, lhs, rhs)


# --------------------------------------------------------------------------------------------------- 2. exact rows, bit for bit
SCALES = [(2, 0, 0, 2), (2, 0, 0, 1), (1, 0, 0, 2)]
EXACT = ([(H, W, off, (1, 0, 0, 1)) for H, W, off in ((2, 2, 0), (5, 7, 0), (36, 36, 0), (16, 16, 1))]
         + [(H, W, off, t) for t in SCALES for H, W, off in ((8, 8, 0), (6, 10, 0), (36, 36, 0), (16, 16, 1))]
         + [(8, 8, 0, (0, -1, 1, 0)), (9, 9, 0, (0, -1, 1, 0))])


@pytest.mark.parametrize("H,W,off,tinv", EXACT)
def test_exact_rows_bit_for_bit(H, W, off, tinv):
    """Integer images in -8..8.  Under T^-1 = diag of 1s and 2s at even sizes the positions are half-integers, the weights 1/2 or 1/4
    and reflected taps are present, so every sum is exact in fp32 and the fp64 restatement is the result."""
    B = 3
    x = ints(B, H, W, H * 100 + W)
    xd = on_device(x, off)
    row = G.table(tinv)
    mat = np.stack([row] * B)
    matd = torch.from_numpy(mat).to(DEV)
    if tinv in SCALES:
        assert GP.census(row, H, W)["reflected"] > 0
        assert all(set(np.unique(w).tolist()) <= {0.0, 0.25, 0.5} for _, _, _, w in GP.tap_info(row, H, W))
    for adjoint in (False, True):
        y = run_reflect(xd, matd, adjoint).cpu()
        ref = nhwc(GP.apply(nchw(x).double(), mat, adjoint))
        assert torch.equal(y.double(), ref), (tinv, adjoint)
        if tinv == (0, -1, 1, 0):
            assert torch.equal(y, torch.rot90(x, -1 if adjoint else 1, [1, 2]))
        if tinv == (1, 0, 0, 1):
            assert bits_equal(y, x)


# ---------------------------------------------------------------------------------------------------------- 3. one-hot at 5 x 7
def test_forward_column_is_adjoint_row_bit_for_bit():
    """Image q of the forward batch holds column q of R, image p of the adjoint batch row p of R^T: the same fp32 numbers, and the
    restatement's dense float32 matrix (the four taps of a pixel read four different pixels, so an entry is one weight)."""
    H, W = 5, 7
    n = H * W
    dev_mat, _, _ = device_table(8, seed=11, p=1.0)
    rows = np.concatenate([SUPPLIED[[1, 2, 3, 5, 6, 7]], dev_mat.cpu().numpy()])
    onehot = torch.eye(n).reshape(n, H, W, 1).expand(n, H, W, 3).contiguous()
    xd = on_device(onehot)
    reflected = 0
    for k, row in enumerate(rows):
        matd = torch.from_numpy(np.stack([row] * n)).to(DEV)
        fwd = run_reflect(xd, matd, False).cpu()                            # fwd[q, p] = R[p, q]
        adj = run_reflect(xd, matd, True).cpu()                             # adj[p, q] = R^T[q, p] = R[p, q]
        for ch in range(3):
            Rf, Ra = fwd[..., ch].reshape(n, n), adj[..., ch].reshape(n, n)
            assert bits_equal(Rf, Ra.t().contiguous()), (k, ch)
        dense = np.zeros((n, n), f32)                                       # dense[p, q] from the restatement
        for idx, w in GP.taps(row, H, W):
            assert (dense[np.arange(n), idx.reshape(-1)][w.reshape(-1) > 0] == 0).all()     # one weight per entry
            np.add.at(dense, (np.arange(n), idx.reshape(-1)), w.reshape(-1))
        assert np.array_equal(adj[..., 0].reshape(n, n).numpy(), dense), k
        reflected += GP.census(row, H, W)["reflected"]
    assert reflected > 0


# ------------------------------------------------------------------------- 4. taps that stay inside give sgx_ada_geom's bits
@pytest.mark.parametrize("H,W,off", [(5, 7, 0), (8, 8, 0), (9, 9, 0), (36, 36, 0), (16, 16, 1)])
def test_inside_rows_equal_the_zero_padded_entry_bit_for_bit(H, W, off):
    g = torch.Generator().manual_seed(H + W)
    rows = [np.array(G.IDENTITY, f32), G.table((0.5, 0, 0, 0.5))] + ([G.table((0, -1, 1, 0))] if H == W else [])
    B = len(rows)
    xd = on_device(torch.randn(B, H, W, 3, generator=g), off)
    mat = np.stack(rows)
    for row in rows[1:]:
        for tx, ty, _, w in GP.tap_info(row, H, W):                        # the premise, on the reference
            assert ((tx >= 0) & (tx < W) & (ty >= 0) & (ty < H))[w > 0].all()
    matd = torch.from_numpy(mat).to(DEV)
    for adjoint in (False, True):
        assert bits_equal(run_reflect(xd, matd, adjoint), run_geom(xd, matd, adjoint)[0]), adjoint


# ----------------------------------------------------------------------------------------------------- 5. the default is unchanged
def test_default_padding_launches_and_computes_what_it_did():
    from stylegan.pytorch_amd import functional as F
    B = 8
    u9 = torch.from_numpy(Bl.edge_draws9(B, seed=2)).to(DEV)
    u5 = torch.from_numpy(G.edge_draws5(B, seed=2)).to(DEV)
    for N_, path in ((16, "tile"), (18, "px")):                              # rows of whole groups of four, and not
        img = torch.randn(B, N_, N_, 3, device=DEV)
        mid = F.call(F.DiffAugFn, img, u9, 31)
        want = F.call(F.AdaGeomFn, mid, F.ada_geom_matrix(u5, G.ALL))
        outs = {}
        for pad in (None, "zeros", "reflect"):
            dis = small_dis(diffaug_policy=GC.FULL8, **({} if pad is None else dict(geom_padding=pad)))
            dis.train()
            dis.diffaug_override, dis.geom_override = u9, u5
            outs[pad], notes = recorded(lambda: dis._diffaug(img))
            name = "ada_geom_reflect_" if pad == "reflect" else "ada_geom_"
            assert notes[-2:] == ["ada_geom_matrix", name + path], (pad, notes)
            assert len([n for n in notes if n.startswith("ada_geom")]) == 2, notes
        assert bits_equal(outs[None], want) and bits_equal(outs["zeros"], want) and not bits_equal(outs["reflect"], want)
        assert bits_equal(outs["reflect"], F.call(F.AdaGeomReflectFn, mid, F.ada_geom_matrix(u5, G.ALL)))
    img = torch.randn(B, 16, 16, 3, device=DEV)
    # a policy without a geometric op: "reflect" is inert
    got = {}
    for pad in ("zeros", "reflect"):
        dis = small_dis(diffaug_policy=GC.C.FULL + ",brightness,contrast", geom_padding=pad)
        dis.train()
        dis.diffaug_override, dis.color_override = u9, torch.rand(B, 8, generator=torch.Generator().manual_seed(1)).to(DEV)
        got[pad] = recorded(lambda: dis._diffaug(img))
    assert got["zeros"][1] == got["reflect"][1] and not any("geom" in n for n in got["reflect"][1]), got["reflect"][1]
    assert bits_equal(got["zeros"][0], got["reflect"][0])


def test_first_and_second_order_through_the_functions():
    """(y . w).sum() and the R1-shaped grad(...).pow(2).sum() through AdaGeomReflectFn: the backward is the adjoint kernel, the double
    backward the forward kernel again, each the bits of the entry called directly."""
    from stylegan.pytorch_amd import functional as F
    B, N_ = 8, 16
    g = torch.Generator().manual_seed(3)
    matd, _, _ = device_table(B, seed=21)
    xd = torch.randn(B, N_, N_, 3, generator=g).to(DEV).requires_grad_(True)
    wd = torch.randn(B, N_, N_, 3, generator=g).to(DEV).requires_grad_(True)
    (y, gx, gw), notes = recorded(lambda: _orders(F, xd, wd, matd))
    assert notes == ["ada_geom_reflect_tile"] * 3, notes
    assert bits_equal(y, run_reflect(xd.detach(), matd, False))
    assert bits_equal(gx, run_reflect(wd.detach(), matd, True))
    assert bits_equal(gw, run_reflect((2.0 * gx).detach(), matd, False))
    assert not F.call(F.AdaGeomReflectFn, xd.detach(), matd).requires_grad


def _orders(F, xd, wd, matd):
    y = F.call(F.AdaGeomReflectFn, xd, matd)
    gx, = torch.autograd.grad((y * wd).sum(), xd, create_graph=True)
    gw, = torch.autograd.grad(gx.pow(2).sum(), wd)
    return y.detach(), gx.detach(), gw


# ------------------------------------------------------------------------------------------------------------------- 6. network
@pytest.mark.parametrize("depth,alpha", [(5, 0.5), (3, 0.3)])
def test_network_first_and_second_order_vs_oracle(monkeypatch, dparams, depth, alpha):
    """D(x), the R1 value and every D parameter gradient of the logistic D loss under the eight-op policy with geom_padding="reflect"
    and per-image gates (p = 0.5 against pinned uniforms), against the fp64 composition geom_pad_ref o blit_ref o the oracle's D under
    the device's table: the check, the draws and the tolerances of tests/test_gpu_geom.py's network test."""
    from stylegan.pytorch_amd import Losses
    from stylegan.pytorch_amd import functional as F
    B, res = GC.NET_B, 4 * 2 ** depth
    dp = dparams
    dis = load_ada(mid_dis(GC.FULL8, ada_target=0.6, ada_p_init=GC.NET_P, ada_kimg=BIG_KIMG, geom_padding="reflect"), dp)
    dis.train()
    u9, gates5, bits5 = GC.C.network_draws(depth)
    u5, gates3, bits3 = GC.network_draws(depth)
    for op in (G.SCALE, G.ROTATE, G.ANISO):
        assert any(b & op for b in bits3) and any(not b & op for b in bits3), bits3           # mixed
    dis.diffaug_override, dis.ada_gate_override = torch.from_numpy(u9).to(DEV), gates5.to(DEV)
    dis.geom_override, dis.geom_gate_override = torch.from_numpy(u5).to(DEV), gates3.to(DEV)
    mat = F.ada_geom_matrix(dis.geom_override, G.ALL, dis.geom_gate_override, dis.ada_state).cpu().numpy()
    assert float(np.abs(mat.astype(np.float64) - G.matrices(u5, bits3)).max()) <= MATRIX_TOL
    assert sum(GP.census(row, res, res)["reflected"] for row in mat if not G.is_identity(row)) > 0
    orig = O.discriminator

    def discriminator(p, img, depth_, alpha_, total_depth, **kw):
        return orig(p, GP.apply(Bl.apply_gated(img, u9, bits5), mat), depth_, alpha_, total_depth, **kw)
    monkeypatch.setattr(O, "discriminator", discriminator)
    real = gu.seeded((B, 3, res, res), 300 + depth); fake = gu.seeded((B, 3, res, res), 400 + depth)

    score, notes = recorded(lambda: dis(real.to(DEV), depth, alpha))
    assert "ada_geom_reflect_tile" in notes and "ada_geom_tile" not in notes, notes
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


# ------------------------------------------------------------------------------------------------------ 7. graph replay, moving p
def pin(dis):
    dis.diffaug_override = torch.from_numpy(Bl.edge_draws9(8, seed=3)[[0, 3, 4, 7]]).to(DEV)
    dis.ada_gate_override = GC.C.spread_gates5(4).to(DEV)
    dis.geom_override = torch.from_numpy(G.edge_draws5(8, seed=3)[[0, 1, 3, 7]]).to(DEV)
    dis.geom_gate_override = GC.spread_gates3(4).to(DEV)


def test_stage_replay_is_eager_bit_for_bit_with_a_moving_p():
    """The augmentation stages of the MID discriminator captured on their own: p is read on the device at every replay, and a replay
    is the eager result bit for bit at each p."""
    img = gu.seeded((4, 128, 128, 3), 7).float().to(DEV)
    dis = mid_dis(GC.FULL8, ada_target=0.6, ada_p_init=0.5, ada_kimg=BIG_KIMG, geom_padding="reflect")
    dis.train()
    pin(dis)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dis._diffaug(img)                                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = dis._diffaug(img)
    seen = []
    for p in (0.5, 0.1, 0.9, 0.0, 0.5):
        dis.ada_state[0] = p
        g.replay()
        got = out.clone()
        assert bits_equal(got, dis._diffaug(img)), p
        seen.append(got)
    assert bits_equal(seen[0], seen[4]) and not bits_equal(seen[0], seen[2]) and bits_equal(seen[3], img)
    zeros = mid_dis(GC.FULL8, ada_target=0.6, ada_p_init=0.9, ada_kimg=BIG_KIMG)
    zeros.train()
    pin(zeros)
    assert not bits_equal(seen[2], zeros._diffaug(img))                      # and the padding mode is what differs


def train_run(use_graphs, iters=4, seed=5):
    # 1 / (0.02 * 1000) = 0.05 per image: one update (interval 1) at batch 4 moves p by 0.2
    sg = make_sg(GC.FULL8, use_graphs, ada_target=0.6, ada_interval=1, ada_kimg=0.02, ada_p_init=0.5, geom_padding="reflect")
    if not use_graphs:
        sg.alpha_on_device = True                    # the replay's arithmetic: the fade-in coefficient read from device memory
    gp, dp = mid_params(torch.float64)
    load_into(sg.gen, gp); load_ada(sg.dis, dp); load_into(sg.gen_shadow, gp)
    sg.gen.train(); sg.dis.train()
    pin_noise(sg.gen, mid_noises(4))
    pin(sg.dis)
    torch.manual_seed(seed); random.seed(seed)
    losses, states = [], []
    for i in range(iters):
        alpha = min(1.0, 0.25 + 0.15 * i)
        z = gu.seeded((4, 512), 100 + i).to(DEV); real = gu.seeded((4, 3, 128, 128), 200 + i).to(DEV)
        losses.append((float(sg.optimize_discriminator(z, real, 5, alpha)), float(sg.optimize_generator(z, real, 5, alpha))))
        states.append(sg.dis.ada_state.cpu().clone())
    torch.cuda.synchronize()
    return losses, states, sg


def test_step_graph_replay_matches_eager_with_a_moving_p():
    """The whole step with geom_padding="reflect", p moved by the controller at every step, replayed against eager: the ADA state bit
    for bit, the losses to the schedule of tests/test_gpu_graphs.py.  The eager run reads the fade-in coefficient from device memory
    (alpha_on_device), launch for launch the replay's arithmetic, as test_data_parallel_graphs_split_around_the_all_reduce does: with
    the host form, which folds (1 - alpha) into from_rgb's weights, the third generator loss of this run sat at 1.8e-4 against the
    schedule's 1e-4 (measured on the MI355X; iterations 0 and 1 at 1e-7 and 2e-7) -- the documented difference between the two eager
    forms, amplified by Adam with beta1 = 0, not the stage's: its own bit-for-bit replay is asserted above."""
    from test_gpu_graphs import losses_agree
    le, se, eager = train_run(False)
    lg, sg_, sg = train_run(True)
    assert eager.dis.geom_padding == sg.dis.geom_padding == "reflect"
    assert all(g.graph is not None for g in sg._step_graphs.values()) and len(sg._step_graphs) == 2
    for i, (a, b) in enumerate(zip(se, sg_)):
        assert torch.equal(a, b), (i, a, b)
    assert [float(s[5]) for s in se] == [1.0, 2.0, 3.0, 4.0]
    assert len({float(s[0]) for s in se}) > 1                               # p moved between the replays
    losses_agree(le, lg)


# ---------------------------------------------------------------------------------------------------------------- 8. rejections
def test_entry_rejections_launch_nothing():
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd import native as N
    L = N.lib()
    B, H, W = 2, 8, 8
    x = torch.randn(B, H, W, 3, device=DEV)
    y = torch.full((B, H, W, 3), SENTINEL, device=DEV)
    mat = torch.from_numpy(SUPPLIED[:B].copy()).to(DEV)
    s = N.stream()
    r = lambda *a: L.sgx_ada_geom_reflect(*a)

    def refused(fn):
        N.prof_start(1)
        try:
            rc = fn()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        assert N.prof_records() == [], "a kernel was launched"
        assert bool((y == SENTINEL).all())
        L.sgx_clear_error()
        return rc
    for h, w in ((1, 8), (8, 1), (1, 1)):                                                                  # no reflection period
        for adjoint in (0, 1):
            assert refused(lambda: r(N.ptr(x), N.ptr(y), N.ptr(mat), B, h, w, adjoint, s)) == -1
    assert refused(lambda: r(N.ptr(y), N.ptr(y), N.ptr(mat), B, H, W, 0, s)) == -1                         # in place
    assert refused(lambda: r(N.ptr(y), N.ptr(y), N.ptr(mat), B, H, W, 1, s)) == -1
    assert refused(lambda: r(None, N.ptr(y), N.ptr(mat), B, H, W, 0, s)) == -1                             # NULL pointers
    assert refused(lambda: r(N.ptr(x), None, N.ptr(mat), B, H, W, 0, s)) == -1
    assert refused(lambda: r(N.ptr(x), N.ptr(y), None, B, H, W, 1, s)) == -1
    assert refused(lambda: r(N.ptr(x), N.ptr(y), N.ptr(mat), 0, H, W, 0, s)) == -1                         # sgx_ada_geom's own
    assert refused(lambda: r(N.ptr(x), N.ptr(y), N.ptr(mat), 65536, H, W, 0, s)) == -1
    assert refused(lambda: r(N.ptr(x), N.ptr(y), N.ptr(mat), B, 0, W, 0, s)) == -1
    assert refused(lambda: r(N.ptr(x), N.ptr(y), N.ptr(mat), B, 40000, 40000, 0, s)) == -2                 # beyond 2^31 floats per image

    def raises(fn):
        with pytest.raises(N.SgxError):
            fn()
        return 0
    assert refused(lambda: raises(lambda: F.call(F.AdaGeomReflectFn, x[:, :1].contiguous(), mat))) == 0    # H = 1 through the Function
    assert refused(lambda: raises(lambda: F.call(F.AdaGeomReflectFn, x, mat[:, :4].contiguous()))) == 0
    assert refused(lambda: raises(lambda: F.call(F.AdaGeomReflectAdjFn, x.cpu(), mat))) == 0
