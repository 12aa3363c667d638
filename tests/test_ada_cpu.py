"""CPU: the ADA restatement (tests/ada_ref.py) against itself and fp64, the four config keys, the Discriminator keywords and the
state_dict surface.  No GPU, no reference tree."""
import numpy as np
import pytest

import ada_ref as A

f32 = np.float32


def run(p0, batches, target, adjust, interval):
    s, s64, out = A.new_state(p0), A.new_state(p0, np.float64), []
    for lg in batches:
        s = A.controller(s, lg, target, adjust, interval)
        s64 = A.controller64(s64, lg, target, adjust, interval)
        assert s.dtype == f32 and np.allclose(s, s64, rtol=1e-6, atol=1e-6), (s, s64)
        out.append(s.copy())
    return out


def test_gate_rule():
    gu = np.array([[0.0, 0.5, A.R.EDGE], [0.3, 0.3, 0.3], [0.29999998, 0.30000004, 0.9]], f32)
    assert A.gates(gu, 0.0, 7).tolist() == [0, 0, 0]                      # p = 0 gates nothing, not even u = 0 (strict <)
    assert A.gates(gu, 1.0, 7).tolist() == [7, 7, 7]                      # p = 1 gates everything, up to the largest fp32 below 1
    assert A.gates(gu, f32(0.3), 7).tolist() == [1, 0, 1]                 # u == p is off
    assert A.gates(gu, f32(0.3), 5).tolist() == [1, 0, 1] and A.gates(gu, 1.0, 2).tolist() == [2, 2, 2]
    assert A.gates(gu, 2.0 ** -24, 7).tolist() == [1, 0, 0]
    assert A.gates(gu, 1.0, 7).dtype == np.int32


def test_signs_of_nan_and_zero():
    lg = np.array([3.0, -2.0, 0.0, -0.0, np.nan, 1e30, -1e-45, np.inf], f32)
    assert A.signs(lg).tolist() == [1, -1, 0, 0, 0, 1, -1, 1]


@pytest.mark.parametrize("interval", [1, 4])
def test_controller_crosses_the_target_both_ways(interval):
    B, target, adjust = 8, 0.6, f32(0.01)
    up, down = np.ones(B, f32), -np.ones(B, f32)
    tr = run(0.5, [up] * interval + [down] * interval, target, adjust, interval)
    step = f32(adjust * f32(B * interval))
    for s in tr[:interval - 1]:
        assert s[0] == f32(0.5) and s[5] == 0 and s[3] > 0                 # nothing moves between updates
    assert tr[interval - 1][0] == f32(f32(0.5) + step) and tr[interval - 1][4] == 1.0 and tr[interval - 1][5] == 1
    assert tr[interval - 1][1:4].tolist() == [0, 0, 0]
    assert tr[-1][0] == f32(f32(f32(0.5) + step) - step) and tr[-1][4] == -1.0 and tr[-1][5] == 2


def test_controller_clamps_and_holds_at_the_target():
    B, adjust = 4, f32(0.1)                                                # 0.4 per update
    hi = run(0.5, [np.ones(B, f32)] * 3, 0.6, adjust, 1)
    assert [float(s[0]) for s in hi] == [float(f32(f32(0.5) + f32(adjust * f32(4)))), 1.0, 1.0]
    lo = run(0.5, [-np.ones(B, f32)] * 3, 0.6, adjust, 1)
    assert [float(s[0]) for s in lo][1:] == [0.0, 0.0]
    eq = np.array([1, 1, 1, -1], f32)                                      # r_t = 0.5 exactly
    held = run(0.25, [eq] * 2, 0.5, adjust, 1)
    assert held[-1][0] == f32(0.25) and held[-1][4] == 0.5 and held[-1][5] == 2
    odd = np.array([np.nan, 0.0, -0.0, 5.0], f32)                          # r_t = 1/4: NaN and +-0 count as images, not as signs
    s = A.controller(A.new_state(0.5), odd, 0.6, adjust, 1)
    assert s[4] == 0.25 and s[0] == f32(f32(0.5) - f32(adjust * f32(4)))


def test_config_keys(tmp_path):
    from stylegan.pytorch_amd.config import default_cfg
    cfg = default_cfg()
    d = cfg.model.dis
    assert (d.ada_target, d.ada_interval, d.ada_kimg, d.ada_p_init) == (0.0, 4, 500, 0.0)
    y = tmp_path / "ada.yaml"
    y.write_text('model:\n  dis:\n    diffaug_policy: "color,translation,cutout"\n    ada_target: 0.6\n    ada_interval: 2\n'
                 '    ada_kimg: 100\n    ada_p_init: 0.25\n')
    cfg.merge_from_file(str(y))
    d = cfg.model.dis
    assert (d.ada_target, d.ada_interval, d.ada_kimg, d.ada_p_init) == (0.6, 2, 100, 0.25)
    from stylegan.pytorch_amd.GAN import Discriminator
    dis = Discriminator(resolution=8, fmap_base=64, fmap_max=16, **cfg.model.dis)      # train.py: Discriminator(**opt.model.dis)
    assert dis.ada and float(dis.ada_state[0]) == 0.25 and dis.ada_interval == 2


def small(**kw):
    from stylegan.pytorch_amd.GAN import Discriminator
    return Discriminator(resolution=8, blur_filter=[1, 2, 1], fmap_base=64, fmap_max=16, **kw)


def test_constructor_validation():
    with pytest.raises(ValueError):
        small(ada_target=0.6)                                              # no policy to gate
    with pytest.raises(ValueError):
        small(ada_target=0.6, diffaug_policy="")
    for bad in (dict(ada_target=1.0), dict(ada_target=-0.1), dict(ada_target=1.5), dict(ada_interval=0), dict(ada_interval=-2),
                dict(ada_kimg=0), dict(ada_kimg=-1.0), dict(ada_p_init=-0.1), dict(ada_p_init=1.5)):
        kw = dict(dict(ada_target=0.6, diffaug_policy="color"), **bad)
        with pytest.raises(ValueError):
            small(**kw)
    d = small(ada_target=0.6, diffaug_policy="translation,cutout", ada_p_init=1.0)
    assert d.ada and d.ada_gate_override is None and d.ada_state.tolist() == [1.0, 0, 0, 0, 0, 0, 0, 0]


def test_state_dict_keys():
    plain = set(small().state_dict())
    assert set(small(diffaug_policy="color,translation,cutout").state_dict()) == plain
    on = small(diffaug_policy="color,translation,cutout", ada_target=0.6)
    assert set(on.state_dict()) == plain | {"ada_state"}
    assert on.ada_state.dtype.is_floating_point and tuple(on.ada_state.shape) == (8,)
    off = small(diffaug_policy="color")
    assert not off.ada and off.ada_p is None and not hasattr(off, "ada_state")
