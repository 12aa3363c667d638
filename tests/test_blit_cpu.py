"""CPU: the restatement of the augmentation with pixel blitting (tests/blit_ref.py) against the index rules of include/sgx.h written
out pixel by pixel, its adjoint identity for every subset of the five ops, the policy parsing and the Discriminator's keys."""
import itertools

import numpy as np
import pytest
import torch

import blit_ref as Bl
import diffaug_ref as R


def test_edge_draws_cover_every_orientation_and_the_clamps():
    u = Bl.edge_draws9(8, seed=3)
    assert u.shape == (8, 9) and u.dtype == np.float32
    seen = {(Bl.params9(u[b], 8, 8, Bl.ALL)["f"], Bl.params9(u[b], 8, 8, Bl.ALL)["k"]) for b in range(8)}
    assert seen == set(itertools.product((0, 1), range(4)))
    for col in (7, 8):
        assert 0.0 in u[:, col] and np.float32(Bl.EDGE) in u[:, col]
    assert np.array_equal(u[:, :7], R.edge_draws(8, seed=3))                # the existing edge rows, extended
    p = Bl.params9(np.full(9, Bl.EDGE, np.float32), 8, 8, Bl.ALL)
    assert p["f"] == 1 and p["k"] == 3                                      # the clamps: 2u and 4u round up to 2 and 4 in fp32
    p = Bl.params9(np.full(9, Bl.EDGE, np.float32), 8, 8, 7)
    assert p["f"] == 0 and p["k"] == 0                                      # absent ops: whatever the uniform is


@pytest.mark.parametrize("N", [4, 7, 16])
def test_restatement_vs_literal_indices(N):
    g = torch.Generator().manual_seed(N)
    x = torch.randn(8, 3, N, N, generator=g, dtype=torch.float64)
    u = Bl.edge_draws9(8, seed=N)
    for bits in (8, 16, 24, 26, 28, 30):                                    # without the colour: gathers and zeros, exact
        for b in range(8):
            p = Bl.params9(u[b], N, N, bits)
            for adjoint in (False, True):
                ref = Bl.apply_one(x[b], p, bits, adjoint)
                assert torch.equal(ref, Bl.literal(x[b], p, adjoint)), (bits, b, adjoint, p)
    # the table of rotations, entry by entry
    a = x[0]
    i, j = 1, 2
    assert torch.equal(Bl.orient(a, 0, 1)[:, i, j], a[:, j, N - 1 - i])
    assert torch.equal(Bl.orient(a, 0, 2)[:, i, j], a[:, N - 1 - i, N - 1 - j])
    assert torch.equal(Bl.orient(a, 0, 3)[:, i, j], a[:, N - 1 - j, i])
    assert torch.equal(Bl.orient(a, 1, 0)[:, i, j], a[:, i, N - 1 - j])
    for f, k in itertools.product((0, 1), range(4)):
        assert torch.equal(Bl.orient_t(Bl.orient(a, f, k), f, k), a)


def test_old_policies_are_the_old_restatement():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 3, 7, 5, generator=g, dtype=torch.float64)
    u = Bl.edge_draws9(8, seed=1)
    for bits in range(8):
        for adjoint, with_bias in ((False, True), (False, False), (True, False)):
            assert torch.equal(Bl.apply(x, u, bits, adjoint, with_bias), R.apply(x, u[:, :7], bits, adjoint, with_bias))


@pytest.mark.parametrize("bits", list(range(32)))
def test_adjoint_identity_and_affine_part(bits):
    shapes = [(8, 8), (7, 7), (16, 16)] + ([] if bits & Bl.ROT90 else [(7, 5)])
    for H, W in shapes:
        g = torch.Generator().manual_seed(bits * 100 + H)
        x = torch.randn(8, 3, H, W, generator=g, dtype=torch.float64)
        y = torch.randn(8, 3, H, W, generator=g, dtype=torch.float64)
        u = Bl.edge_draws9(8, seed=H + W)
        ax = Bl.apply(x, u, bits, False, False)
        aty = Bl.apply(y, u, bits, True, False)
        lhs, rhs = float((ax * y).sum()), float((x * aty).sum())
        assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + float(ax.abs().sum())), (bits, H, W, lhs, rhs)
        assert torch.allclose(Bl.apply(x, u, bits), ax + Bl.apply(torch.zeros_like(x), u, bits), atol=1e-12)
        mixed = [(bits & m) for m in (31, 0, 7, 24, 17, 10, 29, 22)]        # per-image bits
        axg = Bl.apply_gated(x, u, mixed, False, False)
        atyg = Bl.apply_gated(y, u, mixed, True, False)
        lhs, rhs = float((axg * y).sum()), float((x * atyg).sum())
        assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + float(axg.abs().sum())), (bits, H, W, lhs, rhs)


def test_rot90_needs_square_images():
    u = Bl.edge_draws9(8)
    with pytest.raises(ValueError):
        Bl.apply(torch.zeros(8, 3, 7, 5, dtype=torch.float64), u, 16)


def test_gates_n_restatement():
    import ada_ref as A
    rng = np.random.default_rng(0)
    gu = rng.random((50, 5), dtype=np.float32)
    for p in (0.0, 0.3, 1.0):
        for bits in (31, 24, 7, 21):
            got = Bl.gates_n(gu, p, bits)
            want = [bits & sum((1 << g) for g in range(5) if np.float32(gu[b, g]) < np.float32(p)) for b in range(50)]
            assert got.dtype == np.int32 and got.tolist() == want
        assert np.array_equal(Bl.gates_n(gu[:, :3], p, 7), A.gates(gu[:, :3], p, 7))
    assert not Bl.gates_n(gu, 0.0, 31).any() and (Bl.gates_n(gu, 1.0, 31) == 31).all()


def test_policy_parsing():
    from stylegan.pytorch_amd import functional as F
    assert F.diffaug_policy_bits("color,xflip,rot90,translation,cutout") == 31
    assert F.diffaug_policy_bits("xflip") == 8
    assert F.diffaug_policy_bits("rot90,cutout") == 20
    assert F.diffaug_policy_bits("color, xflip") == 9
    # every string accepted before keeps its bits
    assert F.diffaug_policy_bits("") == 0 and F.diffaug_policy_bits(None) == 0
    assert F.diffaug_policy_bits("color,translation,cutout") == 7
    assert F.diffaug_policy_bits("color, cutout") == 5
    assert F.diffaug_policy_bits("translation") == 2
    for bad in ("translation,xflip", "rot90,xflip", "xflip,xflip", "bogus", "color,bogus", "cutout,color", "translation,color",
                "color,color", "color,,cutout", "Color", "Xflip", "rot180"):
        with pytest.raises(ValueError):
            F.diffaug_policy_bits(bad)
    assert [Bl.OPS, Bl.COLOR, Bl.TRANSLATION, Bl.CUTOUT, Bl.XFLIP, Bl.ROT90] == \
        [F.DIFFAUG_OPS] + [F.DIFFAUG_BITS[k] for k in ("color", "translation", "cutout", "xflip", "rot90")]


def test_discriminator_constructs_without_new_keys():
    from stylegan.pytorch_amd.GAN import Discriminator
    small = lambda **kw: Discriminator(resolution=8, blur_filter=[1, 2, 1], fmap_base=64, fmap_max=16, **kw)
    full = "color,xflip,rot90,translation,cutout"
    plain = set(small().state_dict())
    d = small(diffaug_policy=full)
    assert d._diffaug_bits == 31 and d.diffaug_policy == full and not d.ada
    assert set(d.state_dict()) == plain
    on = small(diffaug_policy=full, ada_target=0.6)
    assert set(on.state_dict()) == plain | {"ada_state"} and tuple(on.ada_state.shape) == (8,)
    with pytest.raises(ValueError):
        small(diffaug_policy="rot90,xflip")


def test_network_test_gates_are_mixed():
    """The pinned gate uniforms of tests/test_gpu_blit.py's network test: at p = 0.5 they turn rot90 on with an odd k for at least one
    image and off for at least one, on the reference alone."""
    import blit_cases as C
    for depth in (3, 5):
        u, gates, bits = C.network_draws(depth)
        ks = [Bl.params9(u[b], 32, 32, bits[b])["k"] for b in range(len(bits))]
        assert any(b & Bl.ROT90 and k & 1 for b, k in zip(bits, ks)), (bits, ks)
        assert any(not b & Bl.ROT90 for b in bits), bits
        assert len(set(bits)) >= 3 and any(b & 1 for b in bits) and any(not b & 1 for b in bits), bits
