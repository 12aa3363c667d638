"""CPU: the fp64 DiffAugment restatement (tests/diffaug_ref.py) against DiffAugment's own indexing and against its adjoint, the policy
parser, the config key and the Discriminator keyword.  No GPU, no reference tree."""
import itertools

import pytest
import torch

import diffaug_ref as R

SUBSETS = [b for b in range(1, 8)]


def test_restatement_equals_the_published_indexing():
    """Zero-fill shift + masked box == pad / clamp / gather / clamped-grid mask, for shifts and offsets across the whole range."""
    torch.manual_seed(0)
    for H, W in ((8, 8), (9, 6), (16, 12)):
        x = torch.randn(1, 3, H, W, dtype=torch.float64)
        sh, sw = int(H * 0.125 + 0.5), int(W * 0.125 + 0.5)
        ch, cw = int(H * 0.5 + 0.5), int(W * 0.5 + 0.5)
        for bits in SUBSETS:
            for tx, ty, ox, oy in itertools.product((-sh, 0, sh), (-sw, 1, sw), (0, H // 2, H - ch % 2), (0, 1, W - cw % 2)):
                p = dict(b=0.2, s=0.7, c=1.3, tx=tx, ty=ty, ox=ox, oy=oy)
                q = dict(b=0.2, s=0.7, c=1.3, tx=tx, ty=ty,
                         r0=max(ox - ch // 2, 0), r1=min(ox - ch // 2 + ch, H), c0=max(oy - cw // 2, 0), c1=min(oy - cw // 2 + cw, W))
                if not bits & R.TRANSLATION:
                    p.update(tx=0, ty=0); q.update(tx=0, ty=0)
                if not bits & R.CUTOUT:
                    q.update(r0=0, r1=0)
                a = R.apply_one(x[0], q, bits)
                b = R.literal(x, p, bits)[0]
                assert torch.allclose(a, b, rtol=0, atol=1e-12), (H, W, bits, tx, ty, ox, oy)


def test_params_clamp_the_edge_draws():
    for H in (4, 5, 8, 64, 1024):
        sh, ch = int(H * 0.125 + 0.5), int(H * 0.5 + 0.5)
        lo, hi = R.params([0.0] * 7, H, H, 7), R.params([R.EDGE] * 7, H, H, 7)
        assert lo["tx"] == -sh and hi["tx"] == sh                         # fp32 (1 - 2^-24) * n rounds to n for small n: clamped
        assert lo["r0"] == 0 and lo["r1"] == ch - ch // 2                  # cutout at the top-left corner
        assert hi["r1"] == H and hi["r0"] == H - ch % 2 - ch // 2          # ... and at the bottom-right one
        assert lo["s"] == 0.0 and lo["c"] == 0.5 and lo["b"] == -0.5


@pytest.mark.parametrize("bits", SUBSETS)
def test_adjoint_identity_fp64(bits):
    """<A x, y> = <x, A^T y> for the linear part A (no bias), on random and edge draws."""
    torch.manual_seed(bits)
    for H, W in ((4, 4), (7, 5), (16, 16)):
        u = R.edge_draws(6, seed=bits)
        x = torch.randn(6, 3, H, W, dtype=torch.float64)
        y = torch.randn(6, 3, H, W, dtype=torch.float64)
        ax = R.apply(x, u, bits, with_bias=False)
        aty = R.apply(y, u, bits, adjoint=True)
        lhs, rhs = float((ax * y).sum()), float((x * aty).sum())
        assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + float(ax.abs().sum())), (bits, H, W, lhs, rhs)
        # the bias is the only affine part: A(x) + A_b(0) == A_b(x)
        assert torch.allclose(R.apply(x, u, bits), ax + R.apply(torch.zeros_like(x), u, bits), atol=1e-12)


def test_policy_parsing():
    from stylegan.pytorch_amd import functional as F
    assert F.diffaug_policy_bits("") == 0 and F.diffaug_policy_bits(None) == 0
    assert F.diffaug_policy_bits("color,translation,cutout") == 7
    assert F.diffaug_policy_bits("color, cutout") == 5
    assert F.diffaug_policy_bits("translation") == 2
    for bad in ("bogus", "color,bogus", "cutout,color", "translation,color", "color,color", "color,,cutout", "Color"):
        with pytest.raises(ValueError):
            F.diffaug_policy_bits(bad)


def test_discriminator_rejects_a_bad_policy_at_construction():
    from stylegan.pytorch_amd.GAN import Discriminator
    with pytest.raises(ValueError):
        Discriminator(resolution=8, blur_filter=[1, 2, 1], fmap_base=64, fmap_max=16, diffaug_policy="bogus")
    with pytest.raises(ValueError):
        Discriminator(resolution=8, blur_filter=[1, 2, 1], fmap_base=64, fmap_max=16, diffaug_policy="cutout,translation")
    d = Discriminator(resolution=8, blur_filter=[1, 2, 1], fmap_base=64, fmap_max=16, diffaug_policy="color,translation,cutout")
    assert d.diffaug_policy == "color,translation,cutout" and d.diffaug_override is None


def test_config_key(tmp_path):
    from stylegan.pytorch_amd.config import default_cfg
    cfg = default_cfg()
    assert cfg.model.dis.diffaug_policy == ""
    plain = tmp_path / "plain.yaml"
    plain.write_text("model:\n  dis:\n    use_wscale: True\n")
    cfg.merge_from_file(str(plain))                                   # a yaml without the key still merges
    assert cfg.model.dis.diffaug_policy == ""
    on = tmp_path / "on.yaml"
    on.write_text('model:\n  dis:\n    diffaug_policy: "color,translation,cutout"\n')
    cfg = default_cfg()
    cfg.merge_from_file(str(on))
    assert cfg.model.dis.diffaug_policy == "color,translation,cutout"
    from stylegan.pytorch_amd.GAN import Discriminator
    d = Discriminator(resolution=8, fmap_base=64, fmap_max=16, **cfg.model.dis)   # train.py: Discriminator(**opt.model.dis)
    assert d._diffaug_bits == 7


def test_the_sample_configs_of_the_schedule_tests_still_merge(tmp_path):
    """The configs/sample.yaml and ffhq1024 values tests/test_train_schedule.py embeds merge with the new key in the defaults."""
    import test_train_schedule as ts
    from stylegan.pytorch_amd.config import default_cfg
    for name in ("SAMPLE_YAML", "FFHQ1024_YAML"):
        p = tmp_path / (name + ".yaml")
        p.write_text(getattr(ts, name))
        cfg = default_cfg()
        cfg.merge_from_file(str(p))
        assert cfg.model.dis.diffaug_policy == ""
