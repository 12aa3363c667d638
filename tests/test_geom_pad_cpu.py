"""CPU: reflection padding for the geometric stage (sgx_ada_geom_reflect, Discriminator(geom_padding="reflect")) without a GPU -- the
restatement tests/geom_pad_ref.py against an independent construction (np.pad, then the zero-padded gather) and against geom_ref where
no tap leaves the image, that the case table of tests/test_gpu_geom_pad.py reaches what those tests claim, and the surface: the
constructor keyword, the config key, header / binding table / exported symbols, and the host-only plan query with its rejections."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import geom_pad_ref as GP
import geom_ref as G
from aug_gpu_util import small_dis_cpu as small_dis
from test_aug_plan import SIZES
from test_gpu_geom import SUPPLIED

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
PLAN_INTS = 6
INSIDE_ROWS = [G.IDENTITY, tuple(G.table((0.5, 0, 0, 0.5))), tuple(G.table((0, -1, 1, 0)))]   # identity, the 0.5 magnification, 90 degrees


# ----------------------------------------------------------------------------------------------------------- the restatement
def padded_gather(img, row):
    """The independent construction: np.pad(mode="reflect") by N-1 on each side, then the ZERO-padded bilinear gather of the padded
    image in fp64, the tap indices shifted by the pad; weights are geom_ref's float32 ones at the unshifted position."""
    C, H, W = img.shape
    pad = np.pad(img, ((0, 0), (H - 1, H - 1), (W - 1, W - 1)), mode="reflect")
    PH, PW = pad.shape[1:]
    sx, sy = G.positions(row, H, W)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    out = np.zeros((C, H, W), np.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = x0 + dx, y0 + dy
            px, py = tx + (W - 1), ty + (H - 1)
            inside = (px >= 0) & (px < PW) & (py >= 0) & (py < PH)
            w = np.where(inside, G.weight(sx, sy, tx, ty), f32(0)).astype(np.float64)
            out += w * pad[:, np.clip(py, 0, PH - 1), np.clip(px, 0, PW - 1)]
    return out


@pytest.mark.parametrize("H,W", [(2, 2), (2, 5), (5, 7), (16, 16), (33, 31), (36, 36)])
def test_restatement_is_np_pad_then_the_zero_padded_gather(H, W):
    g = np.random.default_rng(H * 100 + W)
    img = g.standard_normal((3, H, W))
    rows = [r for r in SUPPLIED if not G.is_identity(r)] + list(G.matrices(G.edge_draws5(8, seed=H), [G.ALL] * 8).astype(f32))
    worst = 0.0
    for row in rows:
        got = GP.apply_one(torch.from_numpy(img), row).numpy()
        worst = max(worst, float(np.abs(got - padded_gather(img, row)).max()))
    print("largest |restatement - np.pad construction|", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (8, 8), (9, 9), (36, 36)])
def test_rows_whose_taps_stay_inside_equal_the_zero_padded_reference(H, W):
    x = torch.randn(1, 3, H, W, dtype=torch.float64)
    for row in INSIDE_ROWS:
        if row == INSIDE_ROWS[2] and H != W:
            continue                                                       # a quarter turn of a rectangle leaves it
        row = np.array(row, f32)
        for tx, ty, _, w in GP.tap_info(row, H, W):                        # the premise: every non-zero tap is inside the image
            assert ((tx >= 0) & (tx < W) & (ty >= 0) & (ty < H))[w > 0].all()
        for adjoint in (False, True):
            assert torch.equal(GP.apply(x, row[None], adjoint), G.apply(x, row[None], adjoint)), (row, adjoint)
            assert np.array_equal(GP.tap_counts(row, H, W, adjoint), G.tap_counts(row, H, W, adjoint))


@pytest.mark.parametrize("H,W", [(2, 2), (5, 7), (16, 16)])
def test_reference_adjoint_is_the_transpose(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(8, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randn(8, 3, H, W, generator=g, dtype=torch.float64)
    lhs, rhs = float((GP.apply(x, SUPPLIED) * y).sum()), float((x * GP.apply(y, SUPPLIED, adjoint=True)).sum())
    scale = float((GP.apply(x.abs(), SUPPLIED) * y.abs()).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale + 1e-300
    gx, = torch.autograd.grad((GP.apply(x, SUPPLIED) * y).sum(), x)
    assert torch.allclose(gx, GP.apply(y, SUPPLIED, adjoint=True), rtol=0, atol=1e-13)


def test_reflection_rule_is_np_pad_reflect():
    for N in (2, 3, 7):
        t = np.arange(-(N - 1), 2 * (N - 1) + 1)
        assert GP.valid(t, N).all() and not GP.valid(np.array([-N, 2 * N - 1]), N).any()
        assert np.array_equal(np.pad(np.arange(N), N - 1, mode="reflect"), GP.reflect(t, N))


# ------------------------------------------------------------------------------------------------------------ the case table
def test_case_table_reaches_what_the_gpu_tests_need():
    """On the reference alone: SUPPLIED at 36 x 36 has reflected taps on each of the four sides, taps beyond one period, output pixels
    without a coefficient, and adjoint elements of more than nine coefficients; the figures of the strongest minification (row 2),
    of row 5, and of row 5 at 2 x 5."""
    total = dict(left=0, right=0, top=0, bottom=0, beyond=0, empty=0)
    per_row = {}
    for b, row in enumerate(SUPPLIED):
        if G.is_identity(row):
            continue
        per_row[b] = c = GP.census(row, 36, 36)
        for k in total:
            total[k] += c[k]
    print({b: c for b, c in per_row.items()})
    assert all(total[k] > 0 for k in ("left", "right", "top", "bottom")), total
    assert total["beyond"] > 0 and total["empty"] > 0, total
    adj_n = [int(GP.tap_counts(SUPPLIED[b], 36, 36, True).max()) for b in range(8)]
    print("largest number of coefficients per adjoint element:", adj_n)
    assert max(adj_n) > 9
    c2 = per_row[2]
    assert (c2["reflected"], c2["nonzero"], c2["beyond"], c2["empty"]) == (2926, 5160, 24, 4), c2
    assert per_row[5]["reflected"] == 2872, per_row[5]
    assert max(adj_n[1], adj_n[7]) == 21, adj_n                            # the two magnifying rows
    small = GP.census(SUPPLIED[5], 2, 5)
    assert (small["beyond"], small["empty"]) == (16, 2), small


# ----------------------------------------------------------------------------------------------------------------- the surface
def test_constructor_keyword_and_its_rejection():
    assert small_dis().geom_padding == "zeros" and small_dis(diffaug_policy="scale,rotate,aniso").geom_padding == "zeros"
    dis = small_dis(diffaug_policy="scale,rotate,aniso", geom_padding="reflect")
    assert dis.geom_padding == "reflect"
    assert set(dis.state_dict()) == set(small_dis(diffaug_policy="scale,rotate,aniso").state_dict())           # no new key
    assert small_dis(diffaug_policy="color", geom_padding="reflect").geom_padding == "reflect"                 # accepted, inert
    assert small_dis(geom_padding="reflect").geom_padding == "reflect"
    for bad in ("reflection", "zero", "", None, "Reflect", 1, "wrap"):
        with pytest.raises(ValueError, match="geom_padding"):
            small_dis(diffaug_policy="scale,rotate,aniso", geom_padding=bad)
    from stylegan.pytorch_amd import functional as F
    from stylegan.pytorch_amd.GAN import Discriminator
    assert [a for a in vars(Discriminator) if a.endswith("_override")] == [h for s in F.AUG_STAGES for h in s.hooks]    # no new hook
    assert F.AdaGeomReflectFn.__name__ == "AdaGeomReflectFn" and F.AdaGeomReflectAdjFn.__name__ == "AdaGeomReflectAdjFn"
    assert not hasattr(F, "AdaGeomReflectLinFn")


def test_config_key_default_and_yaml_override(tmp_path):
    from stylegan.pytorch_amd.config import default_cfg
    cfg = default_cfg()
    assert cfg.model.dis.geom_padding == "zeros"
    y = tmp_path / "pad.yaml"
    y.write_text('model:\n  dis:\n    diffaug_policy: "scale,rotate,aniso"\n    geom_padding: "reflect"\n')
    cfg.merge_from_file(str(y))
    assert cfg.model.dis.geom_padding == "reflect" and cfg.model.dis.diffaug_policy == "scale,rotate,aniso"
    plain = tmp_path / "plain.yaml"
    plain.write_text("model:\n  dis:\n    use_wscale: true\n")
    cfg = default_cfg()
    cfg.merge_from_file(str(plain))
    assert cfg.model.dis.geom_padding == "zeros"


@pytest.fixture(scope="module")
def native():
    from stylegan.pytorch_amd import native as N
    N.build()
    return N


def test_header_binding_table_and_symbols_agree(native):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sgx.h")).read(), flags=re.S)
    I, P = ctypes.c_int, ctypes.c_void_p
    want = {"sgx_ada_geom_reflect": ("const float* x, float* y, const float* mat, int B, int H, int W, int adjoint, void* stream", [P, P, P, I, I, I, I, P]),
            "sgx_ada_geom_reflect_plan": ("int B, int H, int W, int adjoint, int aligned, int* out", [I, I, I, I, I, P])}
    lib = ctypes.CDLL(native.LIB_PATH)
    for name, (args, sig) in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m and " ".join(m.group(1).split()) == args, (name, m and m.group(1))
        assert native.SIGNATURES[name] == (I, sig), name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+SGX_ADA_GEOM_REFLECT_PLAN_INTS\s+%d\b" % PLAN_INTS, src)


def query(L, B, H, W, adjoint, aligned):
    out = (ctypes.c_int * PLAN_INTS)(*([7] * PLAN_INTS))
    rc = L.sgx_ada_geom_reflect_plan(B, H, W, int(adjoint), int(aligned), ctypes.addressof(out))
    return rc, list(out)


def restated_plan(B, H, W, adjoint, aligned):
    """[launches, kernel (0 px, 1 tile), ADJ, grid x, grid y, tiles per row of tiles]"""
    cdiv = lambda a, b: -(-a // b)
    if W % 4 == 0 and aligned:
        return [1, 1, int(bool(adjoint)), cdiv(H, 32) * cdiv(W, 32), B, cdiv(W, 32)]
    return [1, 0, int(bool(adjoint)), cdiv(H * W, 256), B, 0]


def test_plan_query_is_the_restated_plan(native):
    L = native.lib()
    n = 0
    for (H, W), B, aligned, adjoint in itertools.product(SIZES + ((2, 2), (2, 5), (1024, 1024)), (1, 5, 65535), (0, 1), (0, 1, 2)):
        rc, out = query(L, B, H, W, adjoint, aligned)
        assert rc == 0 and out == restated_plan(B, H, W, adjoint, aligned), (B, H, W, adjoint, aligned, rc, out)
        n += 1
    assert n >= 150
    assert query(L, 1, 33, 64, 0, 1)[1] == [1, 1, 0, 4, 1, 2] and query(L, 1, 96, 8, 1, 1)[1] == [1, 1, 1, 3, 1, 1]    # tiles per row: the WIDTH's
    assert query(L, 3, 33, 63, 1, 1)[1] == [1, 0, 1, 9, 3, 0] and query(L, 1, 32, 32, 0, 0)[1] == [1, 0, 0, 4, 1, 0]


def test_plan_query_rejections(native):
    L = native.lib()

    def rejected(code, words, *a):
        L.sgx_clear_error()
        rc, out = query(L, *a)
        msg = L.sgx_last_error().decode(errors="replace")
        L.sgx_clear_error()
        assert rc == code and words in msg and out == [0] * PLAN_INTS, (a, rc, msg, out)
    for H, W in ((1, 8), (8, 1), (1, 1)):
        rejected(EINVAL, "ada_geom_reflect: the reflection needs H, W >= 2", 1, H, W, 0, 1)
    for H, W in ((0, 8), (8, -1)):
        rejected(EINVAL, "ada_geom_reflect: bad arguments", 1, H, W, 0, 1)
    for B in (0, -1, 65536):
        rejected(EINVAL, f"ada_geom_reflect: bad arguments (B={B} 8x8)", B, 8, 8, 0, 1)
    rejected(EUNSUPPORTED, "ada_geom_reflect: image of 40000x40000 too large", 1, 40000, 40000, 0, 1)
    assert L.sgx_ada_geom_reflect_plan(1, 8, 8, 0, 1, None) == EINVAL and b"out is NULL" in L.sgx_last_error()
    L.sgx_clear_error()
    assert query(L, 65535, 2, 2, 1, 0) == (0, [1, 0, 1, 1, 65535, 0])
