"""CPU: the policy surface of ADA's image-space corruptions (noise 16384, imgcutout 32768), ``ada_preset``, and the restatement
tests/corrupt_ref.py on its own -- the parsing, the constructor and the override widths, Philox's known answers, the rectangle
against the paper's fp64 predicate, the moments of the restated field, and planted errors against the per-element criterion that
tests/test_gpu_corrupt.py holds the kernels to."""
import itertools

import numpy as np
import pytest
import torch

import corrupt_ref as R
from aug_gpu_util import small_dis_cpu as small_dis

f32 = np.float32
OLD_OPS = ("color", "xflip", "rot90", "translation", "cutout", "scale", "rotate", "aniso", "brightness", "contrast", "lumaflip", "hue",
           "saturation", "imgfilter")
OLD_BITS = {"color": 1, "translation": 2, "cutout": 4, "xflip": 8, "rot90": 16, "scale": 32, "rotate": 64, "aniso": 128, "brightness": 256,
            "contrast": 512, "lumaflip": 1024, "hue": 2048, "saturation": 4096, "imgfilter": 8192}
FULL14 = ",".join(OLD_OPS)
FULL16 = FULL14 + ",noise,imgcutout"
SIZES = (1, 2, 3, 4, 5, 8, 12, 16, 44, 64, 100, 128, 1024)
N_TOL_CAP = 1e-5                                  # the cap on the GPU file's N_TOL: a planted error must break the criterion even at it


# ---------------------------------------------------------------------------------------------------------------------- parsing
def test_policy_surface():
    from stylegan.pytorch_amd import functional as F
    assert F.DIFFAUG_CORRUPT_OPS == ("noise", "imgcutout") and F.DIFFAUG_CORRUPT_BITS == {"noise": 16384, "imgcutout": 32768}
    assert F.DIFFAUG_CORRUPT_MASK == 49152 == R.ALL and (R.NOISE, R.CUTOUT) == (16384, 32768)
    assert F.diffaug_policy_bits(FULL16) == 65535 and F.diffaug_policy_bits(FULL14) == 16383
    n = 0
    for k in range(len(OLD_OPS) + 1):
        for old in itertools.combinations(OLD_OPS, k):
            want = sum(OLD_BITS[o] for o in old)
            s = ",".join(old)
            join = lambda tail: s + "," + tail if s else tail
            assert F.diffaug_policy_bits(s) == want                                    # every string accepted today keeps its bits
            assert F.diffaug_policy_bits(join("noise")) == want + 16384
            assert F.diffaug_policy_bits(join("imgcutout")) == want + 32768
            assert F.diffaug_policy_bits(join("noise,imgcutout")) == want + 49152
            n += 1
    assert n == 2 ** 14
    assert F.diffaug_policy_bits(" cutout , noise , imgcutout ") == 4 + 49152


@pytest.mark.parametrize("bad", ["imgcutout,noise", "noise,noise", "noise,imgfilter", "Noise", "cutout2", "noise,", "imgcutout,imgcutout",
                                 "imgcutout,cutout", ",noise", "bgc", "bgcfnc", "blit", "geom"])
def test_misordered_duplicated_or_unknown_names_are_refused(bad):
    from stylegan.pytorch_amd import functional as F
    with pytest.raises(ValueError):
        F.diffaug_policy_bits(bad)


def test_presets():
    from stylegan.pytorch_amd import functional as F
    want = {"blit": 8 + 16 + 2, "geom": 224, "color": 7936, "filter": 8192, "noise": 16384, "cutout": 32768}
    assert F.ada_preset("blit") == "xflip,rot90,translation" and F.ada_preset("cutout") == "imgcutout"
    for name, bits in want.items():
        s = F.ada_preset(name)
        assert isinstance(s, str) and F.diffaug_policy_bits(s) == bits, (name, s)
    acc = 0
    for name, last in zip(("bg", "bgc", "bgcf", "bgcfn", "bgcfnc"), ("geom", "color", "filter", "noise", "cutout")):
        acc = (acc or want["blit"]) | want[last]
        assert F.diffaug_policy_bits(F.ada_preset(name)) == acc, name
    assert F.diffaug_policy_bits(F.ada_preset("bgcfnc")) == 65535 - 1 - 4                  # all but DiffAugment's own color and cutout
    for bad in ("", "b", "bgx", "cb", "bgcfncx", "imgcutout", None):
        with pytest.raises(ValueError):
            F.ada_preset(bad)
    with pytest.raises(ValueError):
        small_dis(diffaug_policy="bgc")                                                  # the parser does not learn the names


# ---------------------------------------------------------------------------------------------------- constructor, override widths
def test_constructor_and_state_dict():
    plain = small_dis(diffaug_policy="color")
    dis = small_dis(diffaug_policy="color,hue,noise,imgcutout")
    assert dis._diffaug_bits == 1 + 2048 + 49152
    assert set(dis.state_dict()) == set(plain.state_dict())                          # no new key
    ada = small_dis(diffaug_policy="noise", ada_target=0.6)
    assert set(ada.state_dict()) == set(small_dis(diffaug_policy="color", ada_target=0.6).state_dict())
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="num_channels"):
            small_dis(diffaug_policy="imgcutout", num_channels=c)
    assert dis.corrupt_override is None and dis.corrupt_gate_override is None
    assert small_dis()._diffaug_bits == 0


def test_override_widths():
    img = torch.zeros(2, 8, 8, 3)
    dis = small_dis(diffaug_policy="noise,imgcutout")
    for w in (4, 5, 7, 8):
        dis.corrupt_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="corrupt_override"):
            dis._diffaug(img)
    dis.corrupt_override = torch.rand(3, 6)
    with pytest.raises(ValueError, match="corrupt_override"):
        dis._diffaug(img)
    ada = small_dis(diffaug_policy="imgcutout", ada_target=0.6)
    ada.corrupt_override = torch.rand(2, 6)
    for w in (1, 3, 6, 8):
        ada.corrupt_gate_override = torch.rand(2, w)
        with pytest.raises(ValueError, match="corrupt_gate_override"):
            ada._diffaug(img)
    ada.corrupt_gate_override = torch.rand(3, 2)
    with pytest.raises(ValueError, match="corrupt_gate_override"):
        ada._diffaug(img)


# -------------------------------------------------------------------------------------------------------------- the generator
def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in kat:
        got = R.philox(counter, key)
        assert got.dtype == np.uint32 and " ".join(f"{int(v):08x}" for v in got) == want, (counter, key)
    many = R.philox((np.arange(5), 0, 0, 0), (7, 9))                                  # an array of counters is its scalars
    assert many.shape == (5, 4) and all(np.array_equal(many[q], R.philox((q, 0, 0, 0), (7, 9))) for q in range(5))
    assert not np.array_equal(R.philox((0, 0, 0, 0), (0, 0), rounds=9), R.philox((0, 0, 0, 0), (0, 0)))


def test_field_layout_and_range():
    k0, k1 = 123456, 16777215
    f = R.field(k0, k1, 23)
    nq = R.normals(np.arange(6), k0, k1)
    assert f.shape == (23,) and np.array_equal(f, nq.reshape(-1)[:23])                 # element e: normal e & 3 of counter e >> 2
    assert float(np.abs(R.field(k0, k1, 4096)).max()) <= np.sqrt(48 * np.log(2.0))
    # ua = 0 gives rad = 0 (both normals of the pair are 0), the largest ua the largest radius
    assert np.sqrt(-2.0 * np.log(1.0 - (2.0 ** 24 - 1) * 2.0 ** -24)) == pytest.approx(np.sqrt(48 * np.log(2.0)))


def test_field_moments():
    """64 x 64 x 3 x 4 = 49 152 samples at fixed keys: mean, variance and lag-1 correlation along e within 5 standard errors of 0, 1, 0
    (standard errors of N iid normals: 1 / sqrt N, sqrt(2 / N), 1 / sqrt N)."""
    n = 64 * 64 * 3
    f = np.concatenate([R.field(k0, k1, n) for k0, k1 in ((1, 2), (16777215, 0), (0xABCDEF, 0x123456), (0, 0))])
    N = f.size
    assert N == 49152
    mean, var = float(f.mean()), float(f.var())
    lag = float(np.mean((f[1:] - mean) * (f[:-1] - mean)) / var)
    print("mean", mean, "var", var, "lag-1", lag, "in standard errors", mean * np.sqrt(N), (var - 1) / np.sqrt(2 / N), lag * np.sqrt(N))
    assert abs(mean) <= 5 / np.sqrt(N) and abs(var - 1.0) <= 5 * np.sqrt(2.0 / N) and abs(lag) <= 5 / np.sqrt(N)


# ---------------------------------------------------------------------------------------------------------------------- the table
def test_rectangle_is_the_fp64_predicate():
    """The float32 interval against |(j + 0.5) / N - c| < 0.25 in fp64: 2000 draws per size (26 000 in all) and the edge centres, for
    the columns and, the same expression, for the rows.  0 mismatches: a condition, not a tolerance."""
    g = np.random.default_rng(11)
    mism = 0
    for N in SIZES:
        c = np.concatenate([g.random(2000).astype(f32), np.array([0.0, R.EDGE, 0.25, 0.75, 0.5], f32)])
        lo, hi = R.interval(c, N)
        j = np.arange(N)[None, :]
        got = (j >= lo[:, None]) & (j < hi[:, None])
        mism += int((got != R.interval64(c, N)).sum())
        assert (lo >= 0).all() and (hi <= N).all()
    assert mism == 0
    u = R.edge_draws6(6)
    t = R.table(u, 12, 44)                                                               # W from u4, H from u5
    assert np.array_equal(t[:, 3:5], np.stack(R.interval(u[:, 4], 44), 1).astype(f32))
    assert np.array_equal(t[:, 5:7], np.stack(R.interval(u[:, 5], 12), 1).astype(f32))
    assert R.cut_mask(t, 12, 44).shape == (6, 12, 44) and not t[:, 7].any()


def test_table_rows():
    u = R.edge_draws6(8)
    t = R.table(u, 16, 16)
    assert t.dtype == f32 and t.shape == (8, 8)
    assert t[0, 0] == f32(0.3) and t[1, 0] == f32(0.3) and t[2, 0] == 0.0               # both clamp ends; u0 = 0 gives z = 0
    assert t[3, 1] == t[3, 2] == 16777215.0 and t[4, 1] == t[4, 2] == 0.0
    assert tuple(t[2, 3:7]) == (0.0, 8.0, 8.0, 16.0) and tuple(t[4, 3:7]) == (4.0, 12.0, 0.0, 4.0)    # centres (0.25, 0.75), (0.5, 0)
    off = R.table(u, 16, 16, np.zeros((8, 2), bool))
    assert all(tuple(r.tolist()) == R.ZERO_ROW for r in off) and not np.signbit(off).any()
    only_n = R.table(u, 16, 16, np.array([[True, False]] * 8))
    assert not only_n[:, 3:].any() and np.array_equal(only_n[:, :3], t[:, :3])
    only_c = R.table(u, 16, 16, np.array([[False, True]] * 8))
    assert not only_c[:, :3].any() and np.array_equal(only_c[:, 3:], t[:, 3:])
    assert R.gates(np.array([[0.5, 0.25]], f32), 0.5).tolist() == [[False, True]]        # strict <
    assert not R.gates(np.zeros((2, 2), f32), 1.0, policy=8192).any() and R.gates(np.zeros((2, 2), f32), 1.0).all()
    assert R.gates(np.zeros((1, 2), f32), 1.0, policy=R.CUTOUT).tolist() == [[False, True]]
    on = R.gates(R.gate_patterns(), 0.5)
    assert [int(a) + 2 * int(b) for a, b in on] == [0, 1, 2, 3]


# -------------------------------------------------------------------------------------------------------------------- the passes
def case(B=4, H=6, W=10, seed=0):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, H, W, 3)).astype(f32)
    x[:, 0, 0, 0], x[:, 1, 1, 1] = -0.0, 0.0
    u = g.random((B, 6)).astype(f32)
    u[:, 4:] = [[0.5, 0.5], [0.1, 0.9], [0.5, 0.5], [0.7, 0.2]][:B]
    on = np.array([[True, True], [True, True], [False, True], [True, False]])[:B]
    return x, R.table(u, H, W, on)


def test_restated_passes():
    x, tab = case()
    cut = R.cut_mask(tab, 6, 10)
    assert cut[:3].any(axis=(1, 2)).all() and not cut[3].any()
    y, lin = R.forward(x, tab), R.linear(x, tab)
    assert lin.dtype == f32 and np.array_equal(R.bits(lin)[~cut], R.bits(x)[~cut]) and not R.bits(lin)[cut].any()
    assert not y[cut].any() and np.array_equal(y[2][~cut[2]], x[2][~cut[2]].astype(np.float64))          # sigma == 0: x where not cut
    assert np.array_equal(R.noise_term(tab, 6, 10)[3].reshape(-1), float(tab[3, 0]) * R.field(int(tab[3, 1]), int(tab[3, 2]), 180))
    # the restatement's own outputs (the forward rounded to fp32) meet the criterion at N_TOL = 0
    assert not R.violations(y.astype(f32), x, tab, 0, 0.0).any() and not R.violations(lin, x, tab, 1, 0.0).any()
    # infinities and NaNs in x stay what they are
    xs = x.copy()
    xs[3, 2, 2] = [np.inf, -np.inf, np.nan]
    assert not R.violations(R.forward(xs, tab).astype(f32), xs, tab, 0, 0.0).any()


def test_planted_errors_break_the_criterion():
    x, tab = case()
    cut = R.cut_mask(tab, 6, 10)
    sn = R.noise_term(tab, 6, 10)
    fwd = lambda **plant: R.forward(x, tab, **plant).astype(f32)
    inside = (x.astype(np.float64) + sn).astype(f32)                                    # noise added inside the cut (no mask)
    inside[2] = R.linear(x, tab)[2]
    mode1 = (R.linear(x, tab).astype(np.float64) + np.where(cut[..., None], 0.0, sn)).astype(f32)          # sigma n added in mode 1
    pos0 = R.linear(x, tab) + f32(0.0)                                                   # -0 turned into +0
    assert np.signbit(x[3, 0, 0, 0]) and not np.signbit(pos0[3, 0, 0, 0])
    planted = {"nine rounds": (fwd(rounds=9), 0), "counter q + 1": (fwd(q_offset=1), 0), "order 1, 0, 3, 2": (fwd(order=(1, 0, 3, 2)), 0),
               "noise inside the cut": (inside, 0), "sigma n in mode 1": (mode1, 1), "-0 to +0, mode 1": (pos0, 1)}
    for name, (y, mode) in planted.items():
        bad = R.violations(y, x, tab, mode, N_TOL_CAP)
        assert bad.any(), name
    assert R.violations(inside, x, tab, 0, N_TOL_CAP)[cut].any() and not R.violations(inside, x, tab, 0, N_TOL_CAP)[~cut].any()
    # -0 to +0 in the forward of an image with sigma == 0 (image 2 here): held bit for bit as well
    y = fwd()
    x2 = x.copy()
    x2[2, 0, 0, 0] = -0.0
    assert not cut[2, 0, 0] and R.violations(y, x2, tab, 0, N_TOL_CAP)[2, 0, 0, 0] == (R.bits(y)[2, 0, 0, 0] != 0x80000000)
    y0 = R.forward(x2, tab).astype(f32)
    assert np.signbit(y0[2, 0, 0, 0]) and not R.violations(y0, x2, tab, 0, 0.0).any()
    y0[2, 0, 0, 0] = 0.0
    assert R.violations(y0, x2, tab, 0, N_TOL_CAP)[2, 0, 0, 0]
