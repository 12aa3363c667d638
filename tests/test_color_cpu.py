"""CPU: the policy surface of ADA's colour group (brightness, contrast, lumaflip, hue, saturation) and its restatement
tests/color_ref.py on its own -- the parsing, the constructor and the override widths, the reference's algebra against the paper's
five homogeneous matrices, its adjoint and double backward, the exact rows, and that the pinned draws and gates of
tests/test_gpu_color.py reach the edges those tests claim to reach."""
import itertools

import numpy as np
import pytest
import torch

import color_cases as CC
import color_ref as K
from aug_gpu_util import small_dis_cpu as small_dis

f32 = np.float32
OLD_OPS = ("color", "xflip", "rot90", "translation", "cutout", "scale", "rotate", "aniso")
OLD_BITS = {"color": 1, "translation": 2, "cutout": 4, "xflip": 8, "rot90": 16, "scale": 32, "rotate": 64, "aniso": 128}
NEW_BITS = {"brightness": 256, "contrast": 512, "lumaflip": 1024, "hue": 2048, "saturation": 4096}


def subsets(names):
    return [c for n in range(len(names) + 1) for c in itertools.combinations(names, n)]


# ---------------------------------------------------------------------------------------------------------------------- parsing
def test_new_tables_exist():
    from stylegan.pytorch_amd import functional as F
    assert F.DIFFAUG_COLOR_OPS == K.OPS == ("brightness", "contrast", "lumaflip", "hue", "saturation")
    assert F.DIFFAUG_COLOR_BITS == NEW_BITS and F.DIFFAUG_COLOR_MASK == 7936 == K.ALL
    assert F.DIFFAUG_PIXEL_MASK == 31 and F.DIFFAUG_GEOM_MASK == 224


def test_every_policy_string_in_canonical_order():
    from stylegan.pytorch_amd import functional as F
    for old in subsets(OLD_OPS):
        want_old = sum(OLD_BITS[n] for n in old)
        assert F.diffaug_policy_bits(",".join(old)) == want_old                        # every string accepted today keeps its bits
    for new in subsets(K.OPS):
        add = sum(NEW_BITS[n] for n in new)
        for old in ((), ("color",), ("color", "cutout"), ("xflip", "translation", "rotate"), OLD_OPS):
            assert F.diffaug_policy_bits(",".join(old + new)) == sum(OLD_BITS[n] for n in old) + add, (old, new)
    assert F.diffaug_policy_bits(CC.FULL13) == 8191
    assert F.diffaug_policy_bits(" brightness , hue ") == 256 + 2048
    assert F.diffaug_policy_bits("") == 0 and F.diffaug_policy_bits(None) == 0


@pytest.mark.parametrize("bad", ["hue,brightness", "brightness,scale", "saturation,color", "contrast,brightness", "saturation,hue",
                                 "lumaflip,contrast", "hue,aniso", "brightness,cutout", "hue,hue", "brightness,brightness",
                                 "brightness,contrast,lumaflip,hue,saturation,saturation", "bright", "saturate", "luma_flip", "hue;saturation",
                                 "hue,", ",contrast", "Hue", "BRIGHTNESS", "Lumaflip"])
def test_misordered_duplicated_or_unknown_names_are_refused(bad):
    from stylegan.pytorch_amd import functional as F
    with pytest.raises(ValueError):
        F.diffaug_policy_bits(bad)


# ---------------------------------------------------------------------------------------------------- constructor, override widths
def test_constructor_and_state_dict():
    plain = small_dis(diffaug_policy="color")
    dis = small_dis(diffaug_policy="color,rotate,brightness,hue")
    assert dis._diffaug_bits == 1 + 64 + 256 + 2048
    assert set(dis.state_dict()) == set(plain.state_dict())                          # no new key
    ada = small_dis(diffaug_policy="hue", ada_target=0.6)
    assert set(ada.state_dict()) == set(small_dis(diffaug_policy="color", ada_target=0.6).state_dict())
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="num_channels"):
            small_dis(diffaug_policy="saturation", num_channels=c)
    with pytest.raises(ValueError):
        small_dis(diffaug_policy="hue,brightness")
    assert dis.color_override is None and dis.color_gate_override is None
    assert dis.geom_override is None and dis.diffaug_override is None


def test_override_widths():
    img = torch.zeros(2, 8, 8, 3)
    dis = small_dis(diffaug_policy=",".join(K.OPS))
    for w in (5, 7, 9, 13):
        dis.color_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="color_override"):
            dis._diffaug(img)
    dis.color_override = torch.rand(3, 8)
    with pytest.raises(ValueError, match="color_override"):
        dis._diffaug(img)
    ada = small_dis(diffaug_policy=",".join(K.OPS), ada_target=0.6)
    ada.color_override = torch.rand(2, 8)
    for w in (3, 8, 13):
        ada.color_gate_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="color_gate_override"):
            ada._diffaug(img)
    ada.color_gate_override = torch.rand(3, 5)
    with pytest.raises(ValueError, match="color_gate_override"):
        ada._diffaug(img)


# --------------------------------------------------------------------------------------------------------------- the reference
def M_of(row):
    return np.asarray(row)[:9].reshape(3, 3)


def draws(B, seed):
    return np.random.default_rng(seed).random((B, 8), dtype=f32)


def test_hue_alone_is_a_rotation_about_grey():
    for row in np.concatenate([K.matrices(draws(16, 1), K.HUE), K.matrices(K.edge_draws8(8), K.HUE)]):
        M = M_of(row)
        assert np.abs(M.T @ M - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(M) - 1.0) <= 1e-14
        assert np.abs(M @ np.ones(3) - np.ones(3)).max() <= 1e-14 and not row[9:].any()


def test_lumaflip_alone_is_the_householder_map():
    u = K.edge_draws8(8)
    mat = K.matrices(u, K.LUMAFLIP)
    flipped = 0
    for b in range(8):
        sigma = K.params(u[b], K.LUMAFLIP)["sigma"]
        assert sigma == (-1.0 if u[b, 4] >= 0.5 else 1.0)
        want = np.eye(3) - 2.0 * K.P if sigma < 0 else np.eye(3)
        assert np.abs(M_of(mat[b]) - want).max() <= 1e-15 and not mat[b, 9:].any()
        flipped += sigma < 0
    assert 0 < flipped < 8


def test_saturation_alone_fixes_grey_and_scales_the_rest():
    u = K.edge_draws8(10)
    mat = K.matrices(u, K.SATURATION)
    w1, w2 = np.array([1.0, -1.0, 0.0]), np.array([1.0, 1.0, -2.0])            # two vectors orthogonal to v
    for b in range(10):
        s = K.params(u[b], K.SATURATION)["s"]
        M = M_of(mat[b])
        assert np.abs(M @ K.V - K.V).max() <= 1e-14
        assert np.abs(M @ w1 - s * w1).max() <= 1e-14 * max(s, 1) and np.abs(M @ w2 - s * w2).max() <= 2e-14 * max(s, 1)
    assert K.params(u[0], K.SATURATION)["s"] == 8.0 and K.params(u[1], K.SATURATION)["s"] == 0.125


def test_contrast_and_brightness_alone():
    u = K.edge_draws8(10)
    for b in range(10):
        c = K.params(u[b], K.CONTRAST)["c"]
        row = K.matrices(u[b:b + 1], K.CONTRAST)[0]
        assert np.abs(M_of(row) - c * np.eye(3)).max() <= 1e-15 * c and not row[9:].any()
        bb = K.params(u[b], K.BRIGHTNESS)["b"]
        row = K.matrices(u[b:b + 1], K.BRIGHTNESS)[0]
        assert np.abs(M_of(row) - np.eye(3)).max() <= 1e-15 and np.abs(row[9:] - bb).max() <= 1e-16
    assert abs(K.params(u[0], K.ALL)["b"] - 0.6) < 1e-15 and abs(K.params(u[0], K.ALL)["c"] - 2.0 ** 1.5) < 1e-15


def test_full_composition_is_the_papers_product():
    u = np.concatenate([K.edge_draws8(10, seed=1), draws(32, 2)])
    for policy in [K.ALL] + [sum(s) for s in subsets(K.OP_BITS) if s]:
        mat = K.matrices(u, policy)
        for b in range(u.shape[0]):
            p = K.params(u[b], policy)
            hs = K.homogeneous(p["b"], p["c"], p["sigma"], p["theta"], p["s"])
            prod = hs[4] @ hs[3] @ hs[2] @ hs[1] @ hs[0]                        # Sat Hue Luma Contrast Brightness
            assert np.abs(prod[:3, :3] - M_of(mat[b])).max() <= 1e-12 and np.abs(prod[:3, 3] - mat[b, 9:]).max() <= 1e-12
            assert prod[3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_matrix_is_circulant_with_the_stated_entries():
    u = draws(16, 3)
    for b, row in enumerate(K.matrices(u, K.ALL)):
        p = K.params(u[b], K.ALL)
        a, d, e = p["c"] * p["sigma"] / 3, p["c"] * p["s"] * np.cos(p["theta"]), p["c"] * p["s"] * np.sin(p["theta"]) / np.sqrt(3.0)
        D, L, U = a + 2 * d / 3, a - d / 3 - e, a - d / 3 + e
        assert np.abs(M_of(row) - np.array([[D, L, U], [U, D, L], [L, U, D]])).max() <= 1e-13


# ------------------------------------------------------------------------------------------------------------------ adjoints
def test_adjoint_restatement_is_the_transpose():
    B, H, W = 6, 5, 7
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    y = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    mat = K.matrices(K.edge_draws8(B, seed=2), K.ALL)
    lhs = float((K.apply(x, mat, with_bias=False) * y).sum())
    rhs = float((x * K.apply(y, mat, adjoint=True, with_bias=False)).sum())
    scale = float((K.apply(x.abs(), np.abs(mat), with_bias=False) * y.abs()).sum())
    assert abs(lhs - rhs) <= 1e-13 * scale
    # and the float32 restatement: one-hot inputs give the columns of the forward and the rows of the adjoint, the same numbers
    m32 = mat.astype(f32)
    onehot = np.eye(3, dtype=f32).reshape(1, 1, 3, 3).repeat(B, 0)                                   # [B,1,3,3]: pixel q = e_q
    fwd = K.apply32(onehot, m32, with_bias=False)                                                    # fwd[b,0,q,k] = M[k,q]
    adj = K.apply32(onehot, m32, adjoint=True, with_bias=False)                                      # adj[b,0,k,q] = M[k,q]
    assert np.array_equal(fwd[:, 0].transpose(0, 2, 1).view(np.int32), adj[:, 0].view(np.int32))
    assert np.array_equal(adj[:, 0].reshape(B, 9) + f32(0), m32[:, :9] + f32(0))


def test_autograd_gives_the_adjoint_and_the_linear_part():
    B, H, W = 4, 3, 5
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    mat = K.matrices(K.edge_draws8(B, seed=3), K.ALL)
    gx, = torch.autograd.grad((K.apply(x, mat) * w).sum(), x, create_graph=True)
    assert torch.allclose(gx, K.apply(w, mat, adjoint=True, with_bias=False), rtol=0, atol=1e-13)
    gw, = torch.autograd.grad(gx.pow(2).sum(), w)
    want = 2 * K.apply(K.apply(w, mat, adjoint=True, with_bias=False), mat, with_bias=False).detach()   # the linear part: no t
    assert torch.allclose(gw, want, rtol=0, atol=1e-11)
    bumped = mat.copy()
    bumped[:, 9:] += 1.0
    gx2, = torch.autograd.grad((K.apply(x, bumped) * w).sum(), x, create_graph=True)
    assert torch.equal(torch.autograd.grad(gx2.pow(2).sum(), w)[0], gw)                                # the second order does not see t


def test_float32_restatement_follows_the_fp64_one():
    B, H, W = 8, 4, 6
    x = np.random.default_rng(6).standard_normal((B, H, W, 3)).astype(f32)
    mat = K.matrices(K.edge_draws8(B, seed=4), [K.ALL] * (B - 1) + [0]).astype(f32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    for adjoint, bias in ((False, True), (False, False), (True, False)):
        y = K.apply32(x, mat, adjoint, bias)
        ref = K.apply(xt, mat, adjoint, bias).permute(0, 2, 3, 1).numpy()
        mag = K.apply(xt.abs(), np.abs(mat), adjoint, bias).permute(0, 2, 3, 1).numpy()
        assert np.all(np.abs(y - ref) <= 10 * 2.0 ** -24 * mag)
    assert np.array_equal(K.apply32(x, mat)[B - 1].view(np.int32), x[B - 1].view(np.int32))            # the identity row copies


# ----------------------------------------------------------------------------------------------------------------- exact rows
def test_exact_rows_of_the_reference():
    u = K.edge_draws8(10)
    assert all(K.is_identity(r) for r in K.matrices(u, 0))
    assert all(K.is_identity(r) for r in K.matrices(u, [0] * 10))
    for policy in (K.CONTRAST, K.BRIGHTNESS | K.CONTRAST, K.BRIGHTNESS):
        for b, row in enumerate(K.matrices(u, policy)):
            assert K.is_diagonal_case(u[b], policy)
            M = M_of(row)
            assert (M[~np.eye(3, dtype=bool)] == 0.0).all() and M[0, 0] == M[1, 1] == M[2, 2] == K.params(u[b], policy)["c"]
    assert K.is_diagonal_case(u[1], K.LUMAFLIP | K.CONTRAST) and not K.is_diagonal_case(u[0], K.LUMAFLIP | K.CONTRAST)
    assert not K.is_diagonal_case(u[1], K.HUE) and not K.is_diagonal_case(u[1], K.SATURATION)
    flip = M_of(K.matrices(u[:1], K.LUMAFLIP)[0])
    assert np.array_equal(flip, flip.T)


# ------------------------------------------------------------------------------------------------------------------- the pins
def test_edge_draws_reach_the_edges():
    u = K.edge_draws8(10, seed=3)
    assert u.dtype == f32 and u.shape == (10, 8) and float(u.max()) < 1.0 and float(u.min()) >= 0.0
    p = [K.params(u[b], K.ALL) for b in range(10)]
    assert (p[0]["z_b"], p[0]["z_c"], p[0]["z_s"]) == (3.0, 3.0, 3.0) and (p[1]["z_b"], p[1]["z_c"], p[1]["z_s"]) == (-3.0, -3.0, -3.0)
    assert (p[5]["z_c"], p[5]["z_s"]) == (3.0, -3.0) and (p[6]["z_c"], p[6]["z_s"], p[6]["z_b"]) == (-3.0, 3.0, 3.0)
    assert abs(p[0]["c"] * p[0]["s"] - 2.0 ** 4.5) < 1e-13                                             # the largest entries
    assert u[0, 4] == 0.5 and p[0]["sigma"] == -1.0 and u[1, 4] < 0.5 and p[1]["sigma"] == 1.0         # both sides of 0.5
    assert float(u[1, 4]) == float(np.nextafter(f32(0.5), f32(0)))
    assert p[2]["sigma"] == 1.0 and p[3]["sigma"] == -1.0
    assert p[0]["theta"] == -np.pi and p[1]["theta"] == 2 * np.pi * (float(K.EDGE) - 0.5) > 3.14159    # the ends of theta
    assert p[2]["theta"] == 0.0 and p[3]["theta"] == np.pi / 2 and p[4]["theta"] == -np.pi / 2
    assert (p[7]["b"], p[7]["c"], p[7]["sigma"], p[7]["theta"], p[7]["s"]) == (0.0, 1.0, 1.0, 0.0, 1.0)   # the all-off row
    assert np.abs(K.matrices(u[7:8], K.ALL)[0] - np.array(K.IDENTITY)).max() <= 1e-15
    off = [K.params(u[b], 0) for b in range(10)]
    assert all((q["b"], q["c"], q["sigma"], q["theta"], q["s"]) == (0.0, 1.0, 1.0, 0.0, 1.0) for q in off)


def test_gates_follow_the_strict_rule():
    gu = np.array([[0.5, 0.25, 0.75, 0.25, 0.5], [0.0, float(K.EDGE), 0.5, 0.0, float(K.BELOW_HALF)]], f32)
    assert K.gates(gu, 0.5, K.ALL).tolist() == [K.CONTRAST | K.HUE, K.BRIGHTNESS | K.HUE | K.SATURATION]
    assert K.gates(gu, 0.0, K.ALL).tolist() == [0, 0] and K.gates(gu, 1.0, K.ALL).tolist() == [K.ALL, K.ALL]
    assert K.gates(gu, 1.0, K.HUE | K.BRIGHTNESS).tolist() == [2304, 2304]
    assert K.gates(gu, 1.0, 255 | K.HUE).tolist() == [2048, 2048]                                      # the other stages' bits are not its own


@pytest.mark.parametrize("depth", [5, 3])
def test_network_test_gates_are_mixed(depth):
    u, gates, bits = CC.network_draws(depth)
    assert u.shape == (CC.NET_B, 8) and tuple(gates.shape) == (CC.NET_B, 5)
    for op in K.OP_BITS:
        assert any(b & op for b in bits) and any(not b & op for b in bits), (op, bits)
    assert any(b == 0 for b in bits) and any(b == K.ALL for b in bits)
    mat = K.matrices(u, bits)
    assert sum(K.is_identity(r) for r in mat) == 1 and len({tuple(r) for r in mat}) == CC.NET_B
