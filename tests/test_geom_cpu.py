"""CPU: the policy surface of ADA's geometric group (scale, rotate, aniso) and its restatement tests/geom_ref.py on its own -- the
parsing, the constructor and the override widths, the reference's transpose property and exact cases, and that the pinned draws and
gates of tests/test_gpu_geom.py reach the edges those tests claim to reach."""
import itertools

import numpy as np
import pytest
import torch

import geom_cases as GC
import geom_ref as G
from aug_gpu_util import small_dis_cpu as small_dis

f32 = np.float32
OLD_OPS = ("color", "xflip", "rot90", "translation", "cutout")
OLD_BITS = {"color": 1, "translation": 2, "cutout": 4, "xflip": 8, "rot90": 16}
NEW_BITS = {"scale": 32, "rotate": 64, "aniso": 128}


def subsets(names):
    return [c for n in range(len(names) + 1) for c in itertools.combinations(names, n)]


# ---------------------------------------------------------------------------------------------------------------------- parsing
def test_old_tables_are_untouched_and_new_ones_exist():
    from stylegan.pytorch_amd import functional as F
    assert F.DIFFAUG_OPS == OLD_OPS and F.DIFFAUG_BITS == OLD_BITS
    assert F.DIFFAUG_GEOM_OPS == G.OPS == ("scale", "rotate", "aniso")
    assert F.DIFFAUG_GEOM_BITS == NEW_BITS and F.DIFFAUG_GEOM_MASK == 224 == G.ALL


def test_every_policy_string_in_canonical_order():
    from stylegan.pytorch_amd import functional as F
    for old in subsets(OLD_OPS):
        want_old = sum(OLD_BITS[n] for n in old)
        assert F.diffaug_policy_bits(",".join(old)) == want_old                        # every string accepted today keeps its bits
        for new in subsets(G.OPS):
            want = want_old + sum(NEW_BITS[n] for n in new)
            assert F.diffaug_policy_bits(",".join(old + new)) == want, (old, new)
    assert F.diffaug_policy_bits(GC.FULL8) == 255
    assert F.diffaug_policy_bits(" scale , aniso ") == 160
    assert F.diffaug_policy_bits("") == 0 and F.diffaug_policy_bits(None) == 0


@pytest.mark.parametrize("bad", ["rotate,scale", "aniso,rotate", "aniso,scale", "scale,scale", "rotate,rotate", "scale,rotate,aniso,aniso",
                                 "scale,color", "rotate,cutout", "aniso,xflip", "color,scale,translation", "scaling", "rot", "scale;rotate",
                                 "scale,", ",rotate", "Scale"])
def test_misordered_duplicated_or_unknown_names_are_refused(bad):
    from stylegan.pytorch_amd import functional as F
    with pytest.raises(ValueError):
        F.diffaug_policy_bits(bad)


# ---------------------------------------------------------------------------------------------------- constructor, override widths
def test_constructor_and_state_dict():
    plain = small_dis(diffaug_policy="color")
    dis = small_dis(diffaug_policy="color,scale,rotate,aniso")
    assert dis._diffaug_bits == 225
    assert set(dis.state_dict()) == set(plain.state_dict())                          # no new key
    ada = small_dis(diffaug_policy="rotate", ada_target=0.6)
    assert set(ada.state_dict()) == set(small_dis(diffaug_policy="color", ada_target=0.6).state_dict())
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="num_channels"):
            small_dis(diffaug_policy="scale", num_channels=c)
    with pytest.raises(ValueError):
        small_dis(diffaug_policy="rotate,scale")
    assert dis.geom_override is None and dis.geom_gate_override is None


def test_override_widths():
    img = torch.zeros(2, 8, 8, 3)
    dis = small_dis(diffaug_policy="scale,rotate,aniso")
    for w in (3, 7, 8, 9):
        dis.geom_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="geom_override"):
            dis._diffaug(img)
    dis.geom_override = torch.rand(3, 5)
    with pytest.raises(ValueError, match="geom_override"):
        dis._diffaug(img)
    ada = small_dis(diffaug_policy="scale,rotate,aniso", ada_target=0.6)
    ada.geom_override = torch.rand(2, 5)
    for w in (5, 8, 2):
        ada.geom_gate_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="geom_gate_override"):
            ada._diffaug(img)


# --------------------------------------------------------------------------------------------------------------- the reference
def random_table(B, seed):
    u = np.random.default_rng(seed).random((B, 5), dtype=f32)
    return G.matrices(u, [G.ALL] * B)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 7), (16, 16), (33, 31)])
def test_reference_adjoint_is_the_transpose(H, W):
    B = 6
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    y = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    mat = np.concatenate([random_table(B - 2, H + W), G.matrices(G.edge_draws5(2), [G.ALL] * 2)])
    lhs, rhs = float((G.apply(x, mat) * y).sum()), float((x * G.apply(y, mat, adjoint=True)).sum())
    scale = float((G.apply(x.abs(), mat) * y.abs()).sum())
    print("lhs", lhs, "rhs", rhs, "rel", abs(lhs - rhs) / max(scale, 1e-300))
    assert abs(lhs - rhs) <= 1e-12 * scale + 1e-300


def test_reference_autograd_gives_the_adjoint_and_back():
    B, H, W = 3, 5, 7
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    mat = random_table(B, 5)
    gx, = torch.autograd.grad((G.apply(x, mat) * w).sum(), x, create_graph=True)
    assert torch.allclose(gx, G.apply(w, mat, adjoint=True), rtol=0, atol=1e-14)
    gw, = torch.autograd.grad(gx.pow(2).sum(), w)
    assert torch.allclose(gw, 2 * G.apply(G.apply(w, mat, adjoint=True), mat).detach(), rtol=0, atol=1e-13)


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (8, 8)])
def test_identity_is_a_copy(H, W):
    x = torch.randn(2, 3, H, W, dtype=torch.float64)
    ident = np.array([G.IDENTITY] * 2)
    assert torch.equal(G.apply(x, ident), x) and torch.equal(G.apply(x, ident, adjoint=True), x)
    # the same matrix through the general path (a row that is not flagged: T differs in the last place)
    almost = ident.copy()
    almost[:, 4] = np.nextafter(f32(1), f32(2))
    assert torch.equal(G.apply(x, almost), x) and torch.equal(G.apply(x, almost, adjoint=True), x)


@pytest.mark.parametrize("N", [8, 36, 5])
def test_quarter_turn_matrix_is_rot90(N):
    x = torch.randn(2, 3, N, N, dtype=torch.float64)
    mat = np.stack([G.table((0, -1, 1, 0))] * 2)
    assert torch.equal(G.apply(x, mat), torch.rot90(x, 1, [2, 3]))
    assert torch.equal(G.apply(x, mat, adjoint=True), torch.rot90(x, -1, [2, 3]))


def test_matrix_rows_are_inverse_pairs():
    mat = random_table(64, 1)
    for row in mat:
        prod = row[:4].reshape(2, 2) @ row[4:].reshape(2, 2)
        assert np.abs(prod - np.eye(2)).max() <= 1e-14
        assert np.abs(row[4:]).max() <= 2.0 ** 1.2 + 1e-12                              # s a <= 2^0.6 * 2^0.6


def test_adjoint_window_is_at_most_seven():
    """The candidates of the adjoint gather: integers in an interval of length 2 (|t00| + |t01|) (and the same for rows)."""
    worst = 0.0
    for th in np.linspace(-np.pi, np.pi, 2001):
        for s, a in itertools.product((2.0 ** -0.6, 1.0, 2.0 ** 0.6), repeat=2):
            t = G.matrix(s, th, a)[4:]
            worst = max(worst, abs(t[0]) + abs(t[1]), abs(t[2]) + abs(t[3]))
    print("largest half extent", worst)
    assert int(np.floor(2 * (worst + 0.03125))) + 1 <= 7


# ------------------------------------------------------------------------------------------------------------------- the pins
def test_edge_draws_reach_the_edges():
    u = G.edge_draws5(8, seed=3)
    assert u.dtype == f32 and float(u.max()) < 1.0 and float(u.min()) >= 0.0
    p = [G.params(u[b], G.ALL) for b in range(8)]
    assert p[0]["z_s"] == 3.0 and p[0]["z_a"] == 3.0 and p[1]["z_s"] == -3.0 and p[1]["z_a"] == -3.0              # both clamp ends
    assert p[5]["z_s"] == 3.0 and p[5]["z_a"] == -3.0 and p[6]["z_s"] == -3.0 and p[6]["z_a"] == 3.0
    assert p[0]["theta"] == -np.pi and p[1]["theta"] == 2 * np.pi * (float(G.EDGE) - 0.5) > 3.14159                # the ends of theta
    assert p[2]["theta"] == 0.0 and p[3]["theta"] == np.pi / 2 and p[4]["theta"] == -np.pi / 2
    # the largest magnification and minification: T = diag(2^1.2, 1) turned / diag(2^-1.2, 1) turned
    assert abs(p[0]["s"] * p[0]["a"] - 2.0 ** 1.2) < 1e-14 and abs(p[1]["s"] * p[1]["a"] - 2.0 ** -1.2) < 1e-14
    off = [G.params(u[b], 0) for b in range(8)]
    assert all(q["s"] == 1.0 and q["theta"] == 0.0 and q["a"] == 1.0 for q in off)
    assert all(G.is_identity(r) for r in G.matrices(u, 0))


@pytest.mark.parametrize("depth", [5, 3])
def test_network_test_gates_are_mixed(depth):
    u, gates, bits = GC.network_draws(depth)
    assert u.shape == (GC.NET_B, 5) and tuple(gates.shape) == (GC.NET_B, 3)
    for op in (G.SCALE, G.ROTATE, G.ANISO):
        assert any(b & op for b in bits) and any(not b & op for b in bits), (op, bits)
    mat = G.matrices(u, bits)
    assert not any(G.is_identity(r) for r in mat) and len({tuple(r) for r in mat}) == GC.NET_B


def test_gates_follow_the_strict_rule():
    gu = np.array([[0.5, 0.25, 0.75], [0.0, float(G.EDGE), 0.5]], f32)
    assert G.gates(gu, 0.5, G.ALL).tolist() == [G.ROTATE, G.SCALE]
    assert G.gates(gu, 0.0, G.ALL).tolist() == [0, 0] and G.gates(gu, 1.0, G.ALL).tolist() == [G.ALL, G.ALL]
    assert G.gates(gu, 1.0, G.SCALE | G.ANISO).tolist() == [160, 160]
