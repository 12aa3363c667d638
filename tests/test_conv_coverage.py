"""CPU side of tests/test_gpu_conv_paths.py: (1) every hipLaunchKernelGGL site of the forward half of csrc/conv.hip, of its weight-packing
section and of csrc/conv2.hip is claimed by a row of conv_ref.CASES or excused by name with a reason, and every switch those launchers read
is set by a group or excused; (2) every conv_kernel / conv2_kernel instantiation the restated rules reach in the default environment over
a shape grid, at 256 and 304 CUs, is claimed by a default row, those reachable only under a group's switches by that group, and every split-K
instantiation by a row; (3) the
restated rules agree with the library's host-only answers and with the recorded tests/golden/conv_plan.json, and select for every row what
the row says; (4) the fp64 references agree with torch's fp64 convolutions and the oracle; (5) both criteria pass an fp32 emulation of the
operations and fail ten planted errors, each of which stays under the rel-L2 bars the tensor-level tests use."""
import collections
import ctypes
import itertools
import json
import os
import re

import pytest
import torch

import conv_ref as CR
import streaming_ref as SR
import test_conv_plan as TP
from oracle import stylegan_oracle as O
from test_streaming_coverage import CSRC, SITE, claims, unclaimed

F, H = torch.float32, torch.bfloat16
# Rows per environment group.  A row is a launch path someone decided to cover: dropping one has to be a decision made here too.
ROWS = {"default": 466, "conv2_0": 6, "conv2_31": 1, "nw4": 5, "nw8": 5, "small0": 2, "bpc1": 2, "regstore": 1, "nt3": 4, "bands0": 1, "deepk0_upa0": 28, "splitk0": 1,
        "splitk2": 1, "percu1": 2, "bigtile": 16, "smalltile": 5, "upblur_bpc2": 3, "fused0": 4}
FWD = ("sgx_conv3x3", "sgx_conv4x4s2_down", "sgx_conv4x4s2_up")

# ---------------------------------------------------------------------------------------------------------------- launch sites, switches
def sources():
    with open(os.path.join(CSRC, "conv.hip")) as f:
        src = f.read()
    a, b = src.index("// Weight gradients."), src.index("// Weight packing")
    assert 0 < a < b
    with open(os.path.join(CSRC, "conv2.hip")) as f:
        return src[:a], src[b:], f.read()


def sites():
    scan = lambda text: [(m.group(1), (m.group(2) or "").strip()) for m in SITE.finditer(text)]
    return [scan(t) for t in sources()]


def test_every_launch_site_is_claimed_or_excused():
    fwd, pack, c2 = sites()
    assert (len(fwd), len(pack), len(c2)) == (2, 4, 3), (fwd, pack, c2)      # the scan found the launchers
    every = fwd + pack + c2
    assert unclaimed(every, CR.CASES, CR.EXCLUDED_SITES) == []
    assert set(CR.EXCLUDED_SITES) <= {s[0] + s[1] for s in every}
    assert all(len(r) > 10 for r in list(CR.EXCLUDED_SITES.values()) + list(CR.EXCLUDED_PATHS.values()))
    for c in CR.CASES:
        assert c.why and c.group in ROWS, c.id
        for k in c.kernels + (c.args["k304"] or ()):                         # every kernel a row names is one of the three templates or launched by name
            assert re.match(r"conv_kernel<|conv2_kernel<|conv3_kernel<", k) or any(claims(s, k) for s in every), (c.id, k)
    # every switch the launchers read is set by a group or excused by name
    read = set(re.findall(r'SGX_SWITCH\(\s*\w+\s*,\s*"(SGX_[A-Z0-9_]*)"', "".join(sources())))
    assert read | {"SGX_TILE_BANDS", "SGX_NT_MIN_MB"} == set(CR.ENV0) | {"SGX_CONV_DBG", "SGX_CONV3_DBG"}
    assert read - {k for g in CR.GROUPS.values() for k in g} == {"SGX_CONV_DBG", "SGX_CONV3_DBG"} <= set(CR.EXCLUDED_PATHS)


def test_a_new_kernel_or_a_dropped_row_is_noticed():
    fwd, pack, c2 = sites()
    assert unclaimed(fwd + [("conv_splitk_finish2", "")], CR.CASES, CR.EXCLUDED_SITES) == ["conv_splitk_finish2"]
    assert unclaimed(fwd, [c for c in CR.CASES if CR.FIN not in c.kernels], CR.EXCLUDED_SITES) == [CR.FIN]
    assert unclaimed(pack, [c for c in CR.CASES if c.entry != "sgx_pack_weight_multi"], CR.EXCLUDED_SITES) == ["pack_weight_multi_kernel<float>", "pack_weight_multi_kernel<bf16_t>"]
    assert unclaimed(c2, [c for c in CR.CASES if c.entry != "sgx_pack_upblur"], CR.EXCLUDED_SITES) == ["pack_upblur_kernel"]
    assert dict(collections.Counter(c.group for c in CR.CASES)) == ROWS


# ---------------------------------------------------------------------------------------------------------------- instantiations
RAGGED = [(1, 1), (5, 7), (9, 13), (17, 19), (33, 35), (6, 10), (18, 26), (34, 38), (66, 70), (130, 134), (258, 262), (17, 32), (40, 64), (9, 32), (34, 64), (72, 96), (136, 128),
          (20, 32), (264, 256), (520, 512), (80, 128), (264, 512), (1032, 1024), (72, 64), (2, 2), (10, 14)]
CHANNELS = [(16, 16), (16, 32), (16, 48), (16, 64), (16, 96), (16, 128), (32, 16), (32, 32), (32, 64), (32, 128), (32, 256), (32, 512), (32, 1024), (32, 2048), (48, 96),
            (96, 48), (128, 16), (128, 32), (128, 64), (256, 32), (544, 32), (64, 64), (48, 16), (48, 32), (48, 64)]
BATCHES = (1, 2, 3, 5, 9, 17, 33)


def grid():
    """The grid of tests/test_conv_plan.py (W a multiple of 32) extended with ragged sizes, channel counts off the 32-channel chunk and odd
    batches; operands above 48 MB left out."""
    for s in TP.shapes():
        yield s
    for (Hh, W), (ci, co), B in itertools.product(RAGGED, CHANNELS, BATCHES):
        yield B, Hh, W, ci, co


def reach(env, ncus=(256, 304), limit=48 << 20):
    out = collections.defaultdict(list)
    for (B, Hh, W, ci, co) in grid():
        for dt in (H, F):
            for geo, e in enumerate(FWD):
                if (geo == 1 and (Hh % 2 or W % 2)) or CR.operand_bytes(geo, dt, B, Hh, W, ci, co) > limit:
                    continue
                for n in ncus:
                    p = CR.plan(e, dt, dict(B=B, H=Hh, W=W, Cin=ci, Cout=co), env, n)
                    if p.rc == 0:
                        out[p.kernels[0]].append((geo, dt, B, Hh, W, ci, co, n))
    return out


@pytest.fixture(scope="module")
def default_reach():
    return reach(CR.ENV0)


def claimed(group):
    return {k for c in CR.CASES if c.group == group for k in c.kernels + (c.args["k304"] or ())}


def test_every_reachable_instantiation_has_a_default_row(default_reach):
    missing = sorted(set(default_reach) - claimed("default"))
    assert not missing, f"{len(missing)} instantiations the default environment reaches have no default row: {missing[:6]}"
    assert len(default_reach) == 115 == len(CR.AUTO)
    # ... an integer row each, on a shape that selects it at both CU counts
    with_int = {k for c in CR.CASES if c.group == "default" and c.args["data"] == "int" and c.args["k304"] is None for k in c.kernels}
    assert set(default_reach) <= with_int
    for k, g, dt, B, Hh, W, ci, co in CR.AUTO:
        for n in (256, 304):
            assert CR.plan(CR.ENTRY[g], dt, dict(B=B, H=Hh, W=W, Cin=ci, Cout=co), CR.ENV0, n).kernels == (k,), (k, n)


def test_instantiations_reachable_only_under_a_switch_are_claimed(default_reach):
    """Every instantiation that a group's switches reach over the grid (operands up to 8 MB) and the default environment does not has a row in
    that group: no exclusions."""
    for group in ("conv2_0", "conv2_31", "small0", "deepk0_upa0", "bigtile", "smalltile"):
        only = set(reach(CR.group_env(group), limit=8 << 20)) - set(default_reach)
        assert not sorted(only - claimed(group)), (group, sorted(only - claimed(group))[:6])


SPLITK_CHANNELS = [(112, 16), (112, 32), (176, 32)]                  # 16-channel chunks with >= 4 of them


def test_every_reachable_splitk_instantiation_has_a_row():
    found = set()
    for (B, Hh, W, ci, co) in set(grid()) | {(B, Hh, W, ci, co) for (Hh, W), (ci, co), B in itertools.product(RAGGED, SPLITK_CHANNELS, BATCHES)}:
        if Hh % 2 == 0 and W % 2 == 0:
            for n in (256, 304):
                p = CR.plan("sgx_conv_splitk", H, dict(B=B, H=Hh, W=W, Cin=ci, Cout=co), CR.ENV0, n)
                if not p.rc:
                    found.add(p.kernels[0])
    rows = {c.kernels[0] for c in CR.CASES if c.entry == "sgx_conv_splitk" and c.kernels and c.group == "default" and c.args["data"] == "int"}
    assert found == rows and len(found) == 6, (sorted(found - rows), sorted(rows - found))


# ---------------------------------------------------------------------------------------------------------------- rules against the library
@pytest.fixture(scope="module")
def lib():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


def answers(L, dt, dtc, B, Hh, W, ci, co):
    """The library's host-only answers and the restated ones, side by side (256 CUs: what the library assumes without a device)."""
    got, want = [], []
    for geo in range(4):
        c5 = (ctypes.c_int * 5)()
        assert L.sgx_conv_config(geo, B, Hh, W, ci, co, dtc, ctypes.addressof(c5)) == 0
        got.append(list(c5))
        want.append(CR.conv_config(geo, dt, B, Hh, W, ci, co, CR.ENV0))
    got += [L.sgx_conv3x3_stats_nparts(B, Hh, W, ci, co, dtc), L.sgx_conv3x3_signbits_ok(B, Hh, W, ci, co, dtc), L.sgx_conv4x4s2_up_blur_ok(B, Hh, W, ci, co, dtc),
            L.sgx_conv_upblur_ok(B, Hh, W, ci, co, dtc)]
    want += [CR.stats_nparts(dt, B, Hh, W, ci, co, CR.ENV0, 256), CR.signbits_ok(dt, B, Hh, W, ci, co, CR.ENV0, 256), CR.up_blur_ok(dt, B, Hh, W, ci, co, CR.ENV0, 256),
             CR.upblur_ok(dt, B, Hh, W, ci, co, CR.ENV0)]
    if Hh % 2 == 0 and W % 2 == 0:
        got += [L.sgx_conv4x4s2_down_fade_ok(B, Hh, W, ci, co, dtc), L.sgx_conv_splitk_ws_bytes(1, B, Hh, W, ci, co, dtc)]
        want += [CR.down_fade_ok(dt, B, Hh, W, ci, co, CR.ENV0, 256), CR.splitk_ws_bytes(1, dt, B, Hh, W, ci, co, CR.ENV0, 256)]
    return got, want


def test_restated_rules_against_the_library(lib):
    wrong = []
    for s in sorted(set(grid())):
        for dt, dtc in ((H, 1), (F, 0)):
            got, want = answers(lib, dt, dtc, *s)
            if got != want:
                wrong.append((s, CR.dn(dt), got, want))
    assert not wrong, f"{len(wrong)} shapes: {wrong[:4]}"
    for geo in (0, 2):                                                                        # only the stride-2 geometry splits
        assert lib.sgx_conv_splitk_ws_bytes(geo, 1, 6, 10, 128, 32, 1) == 0 == CR.splitk_ws_bytes(geo, H, 1, 6, 10, 128, 32, CR.ENV0, 256)


def test_restated_rules_against_the_recorded_plan():
    with open(TP.FIXTURE) as f:
        rows = json.load(f)["rows"]
    col = {c: i for i, c in enumerate(TP.COLUMNS)}
    for s in TP.shapes():
        r, even = rows[TP.key(s)], s[1] % 2 == 0
        want = [CR.stats_nparts(H, *s, CR.ENV0, 256), CR.signbits_ok(H, *s, CR.ENV0, 256), CR.down_fade_ok(H, *s, CR.ENV0, 256) if even else None, CR.up_blur_ok(H, *s, CR.ENV0, 256),
                CR.upblur_ok(H, *s, CR.ENV0), CR.splitk_ws_bytes(1, H, *s, CR.ENV0, 256) if even else None] + [CR.conv_config(g, H, *s, CR.ENV0) for g in range(3)]
        assert r == want, (s, [c for c in col if r[col[c]] != want[col[c]]])


def test_case_table_shapes_select_what_they_say():
    by = CR.BY_ID
    for c in CR.CASES:
        a = c.args
        for n in (256, 304):
            p = CR.row_plan(c, n)
            assert (p.kernels, p.rc) == (tuple(CR.row_kernels(c, n)), a["rc"]), (n, c.id, p)
        if c.group != "default" and a["data"] in ("int", "sparse") and not a["rc"]:
            assert a["twin"], c.id                                    # every switched integer row has a default twin ...
        if a["twin"]:
            t = by[a["twin"]]
            assert t.args["data"] == a["data"] and a["data"] in ("int", "sparse") and t.group == "default" and t.dtype == c.dtype and not t.args["rc"], c.id
            assert all(t.args[k] == a[k] for k in ("B", "H", "W", "Cin", "Cout")), c.id       # ... of the same problem
        if a["rc"]:
            assert not c.kernels and a["rc"] in (CR.EINVAL, CR.EUNSUPPORTED, CR.EWORKSPACE), c.id
        if a["data"] in ("int", "sparse") and c.entry.startswith("sgx_conv"):                 # the integer rows' condition: every sum below 2^24
            assert 16 * a["Cin"] * 9 + 3 < 2 ** 24, c.id
    # the seams sit where the rows say
    E = CR.ENV0
    assert CR.conv2_pick(0, 3, 17, 32, 32, 2048, E, 256) == CR.Pick(8, False, False) and not CR.conv2_pick(0, 3, 17, 32, 32, 2112, E, 256).nw      # 33 channel blocks
    assert CR.conv2_pick(0, 3, 17, 32, 32, 2112 - 64, E, 256).nw                                                                              # ... 32 are taken
    g = CR.conv2_grid(0, CR.conv2_pick(0, 3, 17, 32, 64, 2048, E, 256), 3, 17, 32, 2048, E, 256)
    assert (g.ntiles, g.nslots, g.bands) == (6, 8, 0)                                                                                          # fewer tiles than slots
    g = CR.conv2_grid(0, CR.conv2_pick(0, 1, 64, 128, 32, 1024, E, 256), 1, 64, 128, 1024, E, 256)
    assert (g.ntiles, g.nslots) == (16, 16)                                                                                                    # one tile per slot
    for n, slots in ((256, 512), (304, 608)):                                                                                                 # the band order, per CU count
        pk = CR.conv2_pick(0, 10, 512, 512, 16, 16, E, n)
        g = CR.conv2_grid(0, pk, 10, 512, 512, 16, E, n)
        assert pk == CR.Pick(8, False, True) and (g.ntiles, g.nslots, g.bands) == (5120, slots, 1)
        g = CR.conv2_grid(0, CR.conv2_pick(0, 7, 512, 512, 16, 16, E, n), 7, 512, 512, 16, E, n)
        assert g.bands == 0 and g.ntiles == 3584 < 8 * 512                                                                                     # (B 8 is enough at 256 CUs, B 10 at 304)
    g = CR.conv2_grid(0, CR.conv2_pick(0, 10, 512, 512, 16, 16, CR.group_env("bands0"), 256), 10, 512, 512, 16, CR.group_env("bands0"), 256)
    assert g.bands == 0
    g1, g2 = (CR.conv2_grid(0, CR.Pick(4, False, True), 2, 264, 256, 16, CR.group_env(e), 256, epi=1).nslots for e in ("default", "bpc1"))
    assert (g1, g2) == (512, 256)
    # the overlap tiling of the blur epilogue: steps of 7 rows and 31 columns
    g = CR.conv2_grid(2, CR.Pick(4, False, False), 5, 9, 32, 1024, E, 256, epi=2)
    assert (g.tiles_y, g.tiles_x) == (2, 1) and CR.conv2_grid(2, CR.Pick(4, False, False), 1, 8, 33, 1024, E, 256, epi=2)[:2] == (2, 1)
    # split-K: the cap, nk / 2, the uneven range, one step outside
    assert [CR.conv_splitk_plan(1, H, 1, 6, 10, ci, 32, E, 256) for ci in (96, 128, 544)] == [0, 2, 8] and CR.conv_splitk_plan(1, H, 1, 6, 10, 544, 32, CR.group_env("splitk2"), 256) == 2
    assert CR.conv_splitk_plan(1, F, 1, 6, 10, 544, 32, E, 256) == 0 and CR.conv_splitk_plan(1, H, 1, 6, 10, 544, 32, CR.group_env("splitk0"), 256) == 0
    # deep-K on both sides of Cin % 128, the 8-wave / 4-wave / compact choice of sgx_conv_upblur
    assert CR.conv_deep_k(0, 1, 5, 7, 256, 32, E) and not CR.conv_deep_k(0, 1, 5, 7, 544, 32, E) and not CR.conv_deep_k(1, 1, 5, 7, 256, 32, E)
    assert CR.upblur_kernel(1, 512, 512, E, 256).endswith("<0, 8, 2, 2, 2, 0, 1>") and CR.upblur_kernel(1, 128, 128, E, 256).endswith("<0, 4, 2, 2, 2, 0, 1>")
    assert CR.upblur_kernel(1, 512, 512, dict(E, SGX_UPBLUR_BPC=2), 256).endswith("<0, 4, 2, 2, 2, 0, 2>")
    # every kernel family of the value rows has integer and rounding rows
    fam = collections.defaultdict(set)
    for c in CR.CASES:
        if c.kernels and c.group == "default" and c.entry in FWD + ("sgx_conv_variant", "sgx_conv_splitk"):
            k = c.kernels[0]
            fam[re.match(r"conv_kernel<\w+, \d+, \d|conv2_kernel<\d|conv3_kernel<\d", k).group(0) + (" splitk" if len(c.kernels) > 1 else "")].add("int" if c.args["data"] == "int" else "rounding")
    assert all(v >= {"int", "rounding"} for v in fam.values()), {k: v for k, v in fam.items() if not v >= {"int", "rounding"}}
    assert len(CR.GROUPS) - 1 == 17                                   # seventeen child processes, one after another
    # the rows the random fade rows lean on (tests/conv_runner.py: the lerp is held bit for bit to sgx_conv4x4s2_down + sgx_axpby): the stored activation
    # of the same operands against fp64
    for fade, down in (("fade-c2-D-mf2-randn", "c2-D-mf2-randn"), ("fade-c2-D-mf1-randn", "c2-D-mf1")):
        assert all(by[fade].args[k] == by[down].args[k] for k in ("B", "H", "W", "Cin", "Cout", "data", "bias", "act")) and by[down].entry == "sgx_conv4x4s2_down"


# ---------------------------------------------------------------------------------------------------------------- references against torch and the oracle
def _seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def test_references_against_torch_and_the_oracle():
    Fn = torch.nn.functional
    x = _seeded((2, 5, 7, 6), 1)                                      # NHWC, 6 input channels
    w9, w16 = _seeded((9, 4, 6), 2), _seeded((16, 4, 6), 3)
    k3 = w9.permute(1, 2, 0).reshape(4, 6, 3, 3)
    assert torch.allclose(CR.conv(x, w9, 0), nhwc(Fn.conv2d(nchw(x), k3, padding=1)), rtol=1e-12, atol=1e-12)
    x2 = _seeded((2, 6, 10, 6), 4)
    k4 = w16.permute(1, 2, 0).reshape(4, 6, 4, 4)
    assert torch.allclose(CR.conv(x2, w16, 1), nhwc(Fn.conv2d(nchw(x2), k4, stride=2, padding=1)), rtol=1e-12, atol=1e-12)
    assert torch.allclose(CR.conv(x, w16, 2), nhwc(Fn.conv_transpose2d(nchw(x), k4.permute(1, 0, 2, 3), stride=2, padding=1)), rtol=1e-12, atol=1e-12)
    assert tuple(CR.conv(x, w16, 2).shape) == (2, 10, 14, 4) and tuple(CR.conv(x2, w16, 1).shape) == (2, 3, 5, 4)
    # the packs: conv(x, pack_S(w)) is the oracle's equalized convolution; the adjoint pack is its data gradient; D / U / UF are its fused forms
    gain = 2 ** 0.5
    wp = _seeded((4, 6, 3, 3), 5)
    s = O.he_w_mul(6 * 9, gain)
    fwd, adj, Sf, Sa = CR.pack_weight(wp, 8, "S", s)
    assert tuple(fwd.shape) == (9, 4, 8) and tuple(adj.shape) == (9, 8, 4) and bool((fwd[:, :, 6:] == 0).all()) and bool((adj[:, 6:] == 0).all())
    assert bool((Sf >= fwd.abs() * (1 - 1e-12)).all()) and bool((Sa >= adj.abs() * (1 - 1e-12)).all())
    xr = nchw(x).requires_grad_(True)
    yo = O.eq_conv2d(xr, wp, None, gain)
    assert torch.allclose(CR.conv(x, fwd[:, :, :6].contiguous(), 0), nhwc(yo), rtol=1e-12, atol=1e-12)
    dy = _seeded(yo.shape, 6)
    gx, = torch.autograd.grad(yo, xr, dy)
    assert torch.allclose(CR.conv(nhwc(dy), adj[:, :6].contiguous(), 0), nhwc(gx), rtol=1e-12, atol=1e-12)
    xb = _seeded((1, 6, 128, 128), 7).requires_grad_(True)            # the oracle fuses the stride-2 forms from 128 / 64 pixels
    yd = O.eq_conv2d(xb, wp, None, gain, down=True)
    fD, aD, _, _ = CR.pack_weight(wp, 6, "D", s)
    assert torch.allclose(CR.conv(nhwc(xb.detach()), fD, 1), nhwc(yd), rtol=1e-11, atol=1e-12)
    dyd = _seeded(yd.shape, 8)
    gxd, = torch.autograd.grad(yd, xb, dyd)
    assert torch.allclose(CR.conv(nhwc(dyd), aD, 2), nhwc(gxd), rtol=1e-11, atol=1e-12)      # the adjoint of D runs as the transposed convolution
    for size, mode in ((64, "U"), (6, "UF")):
        xu = _seeded((1, 6, size, size), 9)
        fU, aU, _, _ = CR.pack_weight(wp, 6, mode, s)
        assert torch.allclose(CR.conv(nhwc(xu), fU, 2), nhwc(O.eq_conv2d(xu, wp, None, gain, up=True)), rtol=1e-11, atol=1e-12), mode
    # the blur: the oracle's blur3 is this filter / 16
    yb = _seeded((2, 6, 9, 5), 10)
    assert torch.allclose(CR.blur121(nhwc(yb))[0] / 16, nhwc(O.blur3(yb)), rtol=1e-12, atol=1e-12)
    # the 9 composite taps of sgx_pack_upblur: one 3x3 convolution of the zero-padded coarse grid to the four parity classes is blur o transposed
    # convolution away from the image border (where the 22 correction tiles take over), in both adjoint settings
    for mode, adjoint, shp in (("U", 0, (16, 32)), ("UF", 0, (16, 32)), ("D", 1, (32, 16))):
        wu = torch.randint(-3, 4, (*shp, 3, 3), generator=torch.Generator().manual_seed(14)).double()
        xu = _seeded((1, 7, 9, 32), 15)
        main = CR.pack_upblur_main(wu, mode, adjoint, 1 / 16)
        assert tuple(main.shape) == (9, 64, 32) and torch.equal(main.float().bfloat16().double(), main)
        y4 = CR.conv(xu, main, 0).view(1, 7, 9, 2, 2, 16)                       # [.., px, py, co] -> depth to space
        fine = y4.permute(0, 1, 4, 2, 3, 5).reshape(1, 14, 18, 16)
        ref = CR.conv_upblur(xu, wu, mode, adjoint, 1 / 16)[0]
        assert torch.allclose(fine[:, 2:-2, 2:-2], ref[:, 2:-2, 2:-2], rtol=1e-12, atol=1e-12) and not torch.allclose(fine, ref, rtol=1e-6, atol=1e-6), mode
    assert not torch.allclose(CR.pack_upblur_main(wu, "U", 0, 1 / 16), CR.pack_upblur_main(wu, "UF", 0, 1 / 16))
    # from_rgb in the store is sgx_rgb_in's reference
    pim, wr, rb = _seeded((2, 3, 5, 3), 11), _seeded((8, 3), 12), _seeded((8,), 13)
    r1, S1 = CR.rgb_resid(pim, wr, 0.5, rb, 2.0, 0.5)
    r2, S2 = SR.rgb_in(pim.reshape(-1, 3), wr.reshape(-1), 1, 3, 0.5, rb, 8)
    assert torch.allclose(r1.reshape(-1, 8), r2.reshape(-1, 8), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation, planted errors
def bf(t):
    return t.float().bfloat16().double()


def problem(geo, data, B=8, Hh=62, W=64, Cin=48, Cout=16, seed=40):
    """bf16-exact operands, eight images (the last an odd one of its block of two).  3x3 / transposed: 62x64 (two rows over the emulated tile); stride 2: 124x128 -> 62x64."""
    g = torch.Generator().manual_seed(seed)
    shx = (B, Hh * (2 if geo == 1 else 1), W * (2 if geo == 1 else 1), Cin)
    if data == "int":
        x, w = torch.randint(-3, 4, shx, generator=g).double(), torch.randint(-3, 4, (CR.TAPS[geo], Cout, Cin), generator=g).double()
        bias = torch.randint(-3, 4, (Cout,), generator=g).double()
    else:
        x, w = bf(torch.randn(shx, generator=g)), bf(torch.randn((CR.TAPS[geo], Cout, Cin), generator=g) * CR.weight_scale(geo, Cin))
        bias = (torch.randn((Cout,), generator=g) * 0.5).float().double()
    OH, OW = CR.out_hw(geo, *shx[1:3])
    mask = torch.randint(-3, 4, (B, OH, OW, Cout), generator=g).double()
    resid = torch.randint(-3, 4, (B, OH, OW, Cout), generator=g).double() if data == "int" else bf(torch.randn((B, OH, OW, Cout), generator=g))
    return x, w, bias, mask, resid


TILE = 4                                                              # tile rows of the emulated kernels
KC = 16                                                               # channels per K-chunk: Cin 48 -> 3 chunks, an odd count


def emulate(geo, x, w, bias, act, mask=None, fade=None, splits=1, ipb=1, plant=None):
    """The launch in fp32 as the kernels run it: the output in tiles of TILE rows, per tile the K-chunks in order, per chunk the taps in order,
    products chained in fp32; bias, LeakyReLU, one rounding to bf16, the mask on the rounded value; ``fade`` = (alpha, beta, resid): the lerp on
    the rounded activation and the sign bits; ``splits``: the chunks dealt to that many partial sums, added in order; ``ipb``: images per
    block (their halo comes from a staged patch that holds the block's images one after another).  ``plant``: one planted error."""
    B, Hh, W, Cin = x.shape
    Cout = w.shape[1]
    OH, OW = CR.out_hw(geo, Hh, W)
    x32, w32 = x.float(), w.float()
    nk = Cin // KC
    parts = [torch.zeros(B, OH, OW, Cout) for _ in range(splits)]
    for s in range(splits):
        chunks = list(range(s * nk // splits, (s + 1) * nk // splits))
        if plant == "drop_last_chunk" and splits == 1:
            chunks = chunks[:-1]
        for k in chunks:
            xs, ws = x32[..., k * KC:(k + 1) * KC], w32[:, :, k * KC:(k + 1) * KC]
            parts[s] = parts[s] + emulate_chunk(geo, xs, ws, OH, OW, ipb, plant)
    if plant == "drop_last_split" and splits > 1:
        parts = parts[:-1]
    acc = torch.zeros(B, OH, OW, Cout)
    for pz in parts:
        acc = acc + pz
    if plant == "stale_tile_row" and OH % TILE:
        r0 = OH // TILE * TILE
        acc[:, r0:] = acc[:, r0 - TILE:r0 - TILE + OH - r0]
    if plant == "swap_classes" and geo == 2:
        acc[:, OH - 1, 0::2], acc[:, OH - 1, 1::2] = acc[:, OH - 1, 1::2].clone(), acc[:, OH - 1, 0::2].clone()
    if bias is not None:
        b32 = bias.float()
        if plant == "bias_lane":
            j = torch.arange(Cout)
            b32 = b32[torch.where(j % 4 == 0, j, j - 1)]
        acc = acc + b32
    if act:
        acc = torch.where(acc > 0, acc, acc * torch.tensor(SR.LRELU, dtype=F))
    sl = None if mask is None else torch.where(mask > 0, 1.0, SR.LRELU).float()
    if plant == "mask_before_rounding" and sl is not None:
        y = (acc * sl).bfloat16()
    else:
        y = acc.bfloat16()
        if sl is not None:
            y = (y.float() * sl).bfloat16()
    if fade is None:
        return y, None
    alpha, beta, resid = fade
    a_in = acc if plant == "lerp_unrounded" else y.float()
    bits = SR.pack_bits(y > 0)
    if plant == "bit_order":
        bits = SR.pack_bits((y > 0).reshape(*y.shape[:-1], -1, 8).flip(-1).reshape(y.shape))
    return (alpha * a_in + beta * resid.float()).bfloat16(), bits


def emulate_chunk(geo, xs, ws, OH, OW, ipb, plant):
    """One K-chunk of every tile: the taps in order, one fp32 matrix product per tap added to the fp32 accumulator."""
    B, Hh, W, _ = xs.shape
    xp = torch.nn.functional.pad(xs, (0, 0, 1, 1, 1, 1))
    if plant == "top_halo":                                           # the halo row above the image: the image's own first row instead of zeros
        xp[:, 0, 1:-1] = xs[:, 0]
    if plant == "neighbour_halo" and ipb > 1:
        for b in range(B):
            if b % ipb:                                               # not the first image of its block
                xp[b, 0, 1:-1] = xs[b - 1, Hh - 1]
    if geo == 2:
        yp = torch.zeros(B, OH + 2, OW + 2, ws.shape[1])
        for t in range(16):
            yp[:, t // 4:t // 4 + 2 * Hh:2, t % 4:t % 4 + 2 * W:2] += xs @ ws[t].t()
        return yp[:, 1:-1, 1:-1]
    TK, IS = (3, 1) if geo == 0 else (4, 2)
    acc = torch.zeros(B, OH, OW, ws.shape[1])
    for t in range(TK * TK):
        acc = acc + xp[:, t // TK:t // TK + IS * OH:IS, t % TK:t % TK + IS * OW:IS] @ ws[t].t()
    return acc


WHOLE = ("mask_before_rounding", "lerp_unrounded", "bit_order")      # errors of a rounding's size, or in the sign bytes: everywhere


def confine(plant, clean, planted):
    """The planted error on ONE output pixel (all channels) of the last image -- the edge it belongs to: the top row for the halo plants, the
    last row otherwise -- and the clean emulation everywhere else: the size of error a tensor-level metric does not see."""
    if plant in WHOLE:
        return planted
    y = clean[0].clone()
    row = 0 if plant in ("top_halo", "neighbour_halo") else y.shape[1] - 1
    y[-1, row, -1] = planted[0][-1, row, -1]
    return y, clean[1]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# plant -> (what it is, geometry, epilogue keywords of the emulated launch)
PLANTS = {
    "top_halo": ("a wrong halo row on the top edge only", 0, {}),
    "stale_tile_row": ("the last ragged tile row taken from the previous tile", 0, {}),
    "drop_last_chunk": ("the last K-chunk of an odd count dropped", 0, {}),
    "swap_classes": ("two parity classes swapped on the last fine row", 2, {}),
    "bias_lane": ("the bias of lane j read at j - 1 within a 4-channel group", 0, {}),
    "mask_before_rounding": ("the mask applied before the rounding", 0, {"mask": True}),
    "bit_order": ("bit order reversed within a sign byte", 1, {"fade": True}),
    "lerp_unrounded": ("the lerp applied to the unrounded activation", 1, {"fade": True}),
    "drop_last_split": ("the last split of an uneven split-K dropped", 1, {"splits": 2}),
    "neighbour_halo": ("the neighbouring image's pixels in a multi-image block's halo", 0, {"ipb": 2}),
}
REL_L2_BF16 = 3e-3                                                    # the tightest bf16 bar of tests/test_gpu_kernels.py / test_gpu_fusions.py


def judge(geo, data, plant=None, mask=False, fade=False, splits=1, ipb=1, **shape):
    """-> (the worst err / bound or 0.0 for an exact row, rel-L2 of y against the reference)."""
    x, w, bias, m, resid = problem(geo, data, **shape)
    Cin = x.shape[3]
    alpha, beta = (CR.ALPHA_INT, CR.BETA_INT) if data == "int" else (CR.ALPHA_RND, CR.BETA_RND)
    args = (geo, x, w, bias, True, m if mask else None, (alpha, beta, resid) if fade else None, splits, ipb)
    y, bits = emulate(*args)
    if plant:
        y, bits = confine(plant, (y, bits), emulate(*args, plant))
    pre, S = CR.pre_activation(x, w, None, geo)
    if fade:
        a_r = CR.exact_store(pre, bias, CR.ACT_LRELU, None, H) if data == "int" else None
        if data == "int":
            want = (alpha * a_r.float() + beta * resid.float()).bfloat16()
            assert torch.equal(y.view(torch.int16), want.view(torch.int16)), f"y: {int((y != want).sum())} elements differ from the exact value"
            assert torch.equal(bits, SR.pack_bits(a_r > 0)), "sign bits differ from the exact sign"
            return 0.0, rel_l2(y, want)
        Lc = CR.chain(1, Cin)
        pre_b, S_b = pre + bias, S + bias.abs()
        a64, E = SR.act(pre_b, 1), (Lc + 2) * SR.U32 * S_b
        lo, hi = bf(a64 - E), bf(a64 + E)
        got = y.double()
        ar = bf(torch.minimum(torch.maximum((got - beta * resid) / alpha, lo), hi))      # the admissible rounded activation that explains y best
        near = pre_b.abs() <= E
        assert float(near.double().mean()) <= CR.BITS_CAP
        assert not bool(((SR.unpack_bits(bits, y.shape[-1]) != (pre_b > 0)) & ~near).any()), "sign bits differ from the fp64 pre-activation's sign"
        ref = alpha * ar + beta * resid
        return SR.assert_elementwise(y, ref, alpha * ar.abs() + beta * resid.abs(), 3, H, "y"), rel_l2(y, ref)
    if data == "int":
        want = CR.exact_store(pre, bias, CR.ACT_LRELU, m if mask else None, H)
        assert torch.equal(y.view(torch.int16), want.view(torch.int16)), f"y: {int((y != want).sum())} elements differ from the exact value"
        return 0.0, rel_l2(y, want)
    assert not mask
    ref, Sb = SR.act(pre + bias, 1), S + bias.abs()
    return SR.assert_elementwise(y, ref, Sb, CR.chain(geo, Cin, True, True, splits), H, "y"), rel_l2(y, ref)


def test_both_criteria_pass_the_fp32_emulation():
    for geo in (0, 1, 2):
        assert judge(geo, "int")[0] == 0.0
        r, l2 = judge(geo, "randn")
        assert 0.0 < r <= 1.0 and l2 < REL_L2_BF16, (geo, r, l2)
    assert judge(0, "int", mask=True)[0] == 0.0 and judge(1, "int", fade=True)[0] == 0.0 and judge(1, "int", splits=2)[0] == 0.0 and judge(0, "int", ipb=2)[0] == 0.0
    assert 0.0 < judge(1, "randn", fade=True)[0] <= 1.0 and 0.0 < judge(1, "randn", splits=2)[0] <= 1.0


@pytest.mark.parametrize("plant", list(PLANTS), ids=list(PLANTS))
def test_planted_errors_fail(plant):
    """Each planted error fails the integer row's bit equality or the randn row's bound -- at least one, most both -- while its rel-L2 against
    the clean tensor stays under the loosest bar the tensor-level tests hold bf16 convolutions to, 1e-2 (most under the tightest, 3e-3).  A
    plant may be a no-op on one kind of row by construction -- the unrounded lerp on integers -- which is why there are two kinds."""
    what, geo, kw = PLANTS[plant]
    failed, l2s = 0, []
    for data in ("int", "randn"):
        if kw.get("mask") and data == "randn":
            continue                                                  # (the mask is pinned on integer rows only)
        try:
            _, l2 = judge(geo, data, plant, **kw)
        except AssertionError:
            failed += 1
            continue
        l2s.append(l2)
    assert failed >= 1, f"{what}: no row fails"
    # what the old metric says about the same error: rel-L2 of the planted output against the clean emulation, on the randn problem
    x, w, bias, m, resid = problem(geo, "randn")
    fade = (CR.ALPHA_RND, CR.BETA_RND, resid) if kw.get("fade") else None
    args = (geo, x, w, bias, True, m if kw.get("mask") else None, fade, kw.get("splits", 1), kw.get("ipb", 1))
    clean = emulate(*args)
    planted = confine(plant, clean, emulate(*args, plant))
    if plant != "bit_order":                                          # (a sign byte is no tensor the old tests look at)
        l2 = rel_l2(planted[0], clean[0])
        assert l2 < 1e-2, f"{what}: rel-L2 {l2:.2e}"
        print(plant, f"rel-L2 {l2:.2e}")
