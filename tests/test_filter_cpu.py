"""CPU: the policy surface of ADA's image-space filtering (imgfilter, bit 8192) and its restatement tests/filter_ref.py on its own --
the parsing, the constructor and the override widths, the filter bank's stated properties, pad-and-convolve against the dense
matrix, the adjoint identity, the exact rows, the DC gain, the power-preserving gains and the double backward."""
import itertools

import numpy as np
import pytest
import torch

import filter_ref as R
from aug_gpu_util import small_dis_cpu as small_dis

f32 = np.float32
OLD_OPS = ("color", "xflip", "rot90", "translation", "cutout", "scale", "rotate", "aniso", "brightness", "contrast", "lumaflip", "hue",
           "saturation")
OLD_BITS = {"color": 1, "translation": 2, "cutout": 4, "xflip": 8, "rot90": 16, "scale": 32, "rotate": 64, "aniso": 128, "brightness": 256,
            "contrast": 512, "lumaflip": 1024, "hue": 2048, "saturation": 4096}
FULL14 = ",".join(OLD_OPS) + ",imgfilter"


# ---------------------------------------------------------------------------------------------------------------------- parsing
def test_policy_surface():
    from stylegan.pytorch_amd import functional as F
    assert F.DIFFAUG_FILTER_OPS == ("imgfilter",) and F.DIFFAUG_FILTER_BITS == {"imgfilter": 8192} and F.DIFFAUG_FILTER_MASK == 8192 == R.BIT
    assert F.diffaug_policy_bits(FULL14) == 16383
    n = 0
    for k in range(len(OLD_OPS) + 1):
        for old in itertools.combinations(OLD_OPS, k):
            want = sum(OLD_BITS[o] for o in old)
            s = ",".join(old)
            assert F.diffaug_policy_bits(s) == want                                    # every string accepted today keeps its bits
            assert F.diffaug_policy_bits(s + ",imgfilter" if s else "imgfilter") == want + 8192
            n += 1
    assert n == 8192
    assert F.diffaug_policy_bits(" hue , imgfilter ") == 2048 + 8192


@pytest.mark.parametrize("bad", ["imgfilter,hue", "imgfilter,imgfilter", "Imgfilter", "filter", "imgfilter,", "imgfilter,color", ",imgfilter",
                                 "img_filter", "saturation,imgfilter,imgfilter"])
def test_misordered_duplicated_or_unknown_names_are_refused(bad):
    from stylegan.pytorch_amd import functional as F
    with pytest.raises(ValueError):
        F.diffaug_policy_bits(bad)


# ---------------------------------------------------------------------------------------------------- constructor, override widths
def test_constructor_and_state_dict():
    plain = small_dis(diffaug_policy="color")
    dis = small_dis(diffaug_policy="color,hue,imgfilter")
    assert dis._diffaug_bits == 1 + 2048 + 8192
    assert set(dis.state_dict()) == set(plain.state_dict())                          # no new key
    ada = small_dis(diffaug_policy="imgfilter", ada_target=0.6)
    assert set(ada.state_dict()) == set(small_dis(diffaug_policy="color", ada_target=0.6).state_dict())
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="num_channels"):
            small_dis(diffaug_policy="imgfilter", num_channels=c)
    assert dis.filter_override is None and dis.filter_gate_override is None


def test_override_widths():
    img = torch.zeros(2, 8, 8, 3)
    dis = small_dis(diffaug_policy="imgfilter")
    for w in (4, 7, 9, 12):
        dis.filter_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="filter_override"):
            dis._diffaug(img)
    dis.filter_override = torch.rand(3, 8)
    with pytest.raises(ValueError, match="filter_override"):
        dis._diffaug(img)
    ada = small_dis(diffaug_policy="imgfilter", ada_target=0.6)
    ada.filter_override = torch.rand(2, 8)
    for w in (3, 5, 8, 12):
        ada.filter_gate_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="filter_gate_override"):
            ada._diffaug(img)
    ada.filter_gate_override = torch.rand(3, 4)
    with pytest.raises(ValueError, match="filter_gate_override"):
        ada._diffaug(img)


# -------------------------------------------------------------------------------------------------------------------- the bank
def test_bank_properties():
    fb = R.FB
    assert fb.shape == (4, 43) and fb.dtype == np.float64
    assert np.abs(fb - fb[:, ::-1]).max() <= 1e-16                                     # symmetric about tap 21
    assert [int(np.count_nonzero(r)) for r in fb] == [37, 37, 15, 5]
    assert np.abs(fb.sum(axis=0) - np.eye(43)[21]).max() <= 1e-15                      # the rows sum to the impulse
    assert abs(fb[0].sum() - 1.0) <= 1e-15 and np.abs(fb[1:].sum(axis=1)).max() <= 1e-15
    assert R.FBH.shape == (4, 22) and R.FBH.dtype == f32
    assert np.array_equal(R.FBH, fb[:, 21:].astype(f32)) and np.array_equal(R.full(R.FBH), fb.astype(f32))
    assert np.abs(R.FBH.astype(np.float64) - fb[:, 21:]).max() <= 1e-15                # the taps are dyadic rationals: fp32 loses nothing


# ------------------------------------------------------------------------------------------------- the restatement against itself
SIZES = (2, 3, 4, 5, 8, 21, 22, 43, 64)


def case(N, seed=0, B=3):
    g = np.random.default_rng(1000 * N + seed)
    M = N + 1 if N in (4, 5, 21) else N                                                # some not square
    x = g.standard_normal((B, N, M, 3))
    c = R.rows(R.edge_draws8(B, seed=N))
    return g, x, c


@pytest.mark.parametrize("N", SIZES)
def test_pad_and_convolve_is_the_dense_matrix(N):
    g, x, c = case(N)
    assert np.abs(R.apply_pad(x, c) - R.apply_dense(x, c)).max() <= 1e-13
    assert np.abs(R.apply_pad(x, c, adjoint=True) - R.apply_dense(x, c, adjoint=True)).max() <= 1e-13
    # refl is np.pad's reflection at any width
    idx = np.pad(np.arange(N), (21, 21), mode="reflect")
    assert np.array_equal(idx, R.refl(np.arange(-21, N + 21), N))


@pytest.mark.parametrize("N", SIZES)
def test_adjoint_identity(N):
    g, x, c = case(N, seed=1)
    w = g.standard_normal(x.shape)
    for fn in (R.apply_pad, R.apply_dense):
        lhs, rhs = float((fn(x, c) * w).sum()), float((x * fn(w, c, adjoint=True)).sum())
        scale = float((R.apply_dense(np.abs(x), c, absolute=True) * np.abs(w)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(scale, 1.0)


def test_fold_counts():
    assert [R.folds(N) for N in (2, 4, 22, 43, 64)] == [22, 15, 3, 3, 2]


def test_all_off_is_the_identity_and_rows_are_exact():
    u = R.edge_draws8(6)
    off = np.zeros((6, 4), bool)
    c = R.rows(u, off)
    assert all(R.is_identity(r) for r in c)
    x = np.random.default_rng(2).standard_normal((6, 5, 7, 3))
    assert np.array_equal(R.apply_dense(x, c), x) and np.array_equal(R.apply_pad(x, c, adjoint=True), x)
    assert np.array_equal(R.gains(u, off), np.ones((6, 4)))                            # a band that is off: t = (1,1,1,1) exactly
    assert not any(R.is_identity(r) for r in R.rows(u)[:5])
    assert np.abs(R.rows(u)[5] - np.array(R.IDENTITY)).max() <= 1e-15               # z = 0 in every band: unit gains, the rows sum to the impulse
    assert not R.gates(np.zeros((2, 4), f32), 1.0, policy=4096).any() and R.gates(np.zeros((2, 4), f32), 1.0).all()
    gu = np.array([[0.5, 0.25, 0.75, float(np.nextafter(f32(0.5), f32(0)))]], f32)
    assert R.gates(gu, 0.5).tolist() == [[False, True, False, True]]                   # strict <


def test_constant_image_gets_the_dc_gain():
    u = R.edge_draws8(8, seed=3)
    g = R.gains(u)
    c = R.rows(u)
    x = np.full((8, 6, 9, 3), 1.5)
    y = R.apply_dense(x, c)
    assert np.abs(y - 1.5 * (g[:, 0] ** 2)[:, None, None, None]).max() <= 1e-13 * float(g.max()) ** 2      # only band 0 has DC gain


def test_gains_preserve_power_after_any_single_band():
    u = np.concatenate([R.edge_draws8(5), np.random.default_rng(4).random((16, 8), dtype=f32)])
    for i in range(4):
        on = np.zeros((u.shape[0], 4), bool)
        on[:, i] = True
        g = R.gains(u, on)
        assert np.abs((g * g).mean(axis=1) - 1.0).max() <= 1e-14
    g = R.gains(u)
    assert 0.005 < float(g.min()) and float(g.max()) < 3.1                             # the scale of the gains under the clamp at +-3
    assert R.z(R.EDGE, 0.0) == 3.0 and R.z(R.EDGE, 0.5) == -3.0 and R.z(0.0, 0.0) == 0.0
    assert np.array_equal(R.gains(R.edge_draws8(6)[5:6]), np.ones((1, 4)))


def test_double_backward_of_the_restated_op():
    c = R.rows(R.edge_draws8(1, seed=5))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 5, 6, 3, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: R.apply_torch(t, c), (x,))
    assert torch.autograd.gradgradcheck(lambda t: R.apply_torch(t, c).pow(2), (x,))
    w = torch.randn(1, 5, 6, 3, generator=g, dtype=torch.float64)
    gx, = torch.autograd.grad((R.apply_torch(x, c) * w).sum(), x)
    assert np.abs(gx.numpy() - R.apply_pad(w.numpy(), c, adjoint=True)).max() <= 1e-13


# ----------------------------------------------------------------------------------------------------------- planted errors
def test_planted_errors_are_visible_in_fp64():
    """What tests/test_gpu_filter.py plants against its bounds differs from the operator by far more than a bound."""
    _, x, c = case(8)
    y = R.apply_dense(x, c)
    mag = R.gamma(88) * R.apply_dense(np.abs(x), c, absolute=True)
    for wrong in (R.apply_dense(x, c, shift=1), R.apply_dense(x, c, edge=True), R.apply_dense(x, c, adjoint=True)):
        assert (np.abs(wrong - y) > mag).any()
