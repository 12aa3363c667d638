"""CPU side of tests/test_gpu_epilogue_paths.py and tests/test_gpu_optim_paths.py: (1) every hipLaunchKernelGGL site of csrc/gepi.hip and
csrc/optim.hip is claimed by a row of epilogue_ref or excused by name with a reason; (2) the launcher rules of gepi.hip, restated in
epilogue_ref, select for every row's own arguments exactly the kernels the row names; (3) the decoupled criterion passes an fp32 emulation of
the kernels' lane chains and fails planted errors of the kinds this family is prone to, which the suite's rel-L2 metric lets through."""
import collections
import os
import re

import pytest
import torch

import epilogue_ref as ER
import gpu_util
import streaming_ref as SR
from oracle import stylegan_oracle as O
from test_streaming_coverage import CSRC, claims, launch_sites, unclaimed

F, H = torch.float32, torch.bfloat16
OptimRow = collections.namedtuple("OptimRow", "id kernels")
OPTIM_ROWS = [OptimRow(e, k) for e, k in ER.OPTIM_KERNELS.items()]
# Rows per (entry point, environment group).  A row is a launch path someone decided to cover: dropping one has to be a decision made here too.
ROWS = {("sgx_gepi_fwd", "default"): 79, ("sgx_gepi_bwd", "default"): 64, ("sgx_gepi_stats", "default"): 8, ("sgx_blur3x3_stats", "default"): 4, ("sgx_conv3x3_stats", "default"): 1,
        ("sgx_gepi_fwd", "switch"): 10, ("sgx_gepi_bwd", "switch"): 36, ("sgx_gepi_bwd", "switch_nt"): 4, ("sgx_gepi_fwd", "nofold"): 8, ("sgx_gepi_bwd", "nofold"): 6}


def sites():
    return launch_sites(os.path.join(CSRC, "gepi.hip")), launch_sites(os.path.join(CSRC, "optim.hip"))


def test_every_launch_site_is_claimed_or_excused():
    ge, op = sites()
    assert len(ge) == 16 and len(op) == 4, (len(ge), len(op))        # the scan found the launchers: one site per kernel instantiation (dtype aside)
    assert len({s[0] + s[1] for s in ge}) == 16
    assert unclaimed(ge, ER.CASES, ER.EXCLUDED_SITES) == []
    assert unclaimed(op, OPTIM_ROWS, ER.EXCLUDED_SITES) == []
    assert any(k.startswith("blur_stats_kernel") for c in ER.CASES if c.entry == "sgx_blur3x3_stats" for k in c.kernels)
    assert set(ER.EXCLUDED_SITES) <= {s[0] + s[1] for s in ge + op}
    assert all(len(r) > 10 for r in list(ER.EXCLUDED_SITES.values()) + list(ER.EXCLUDED_PATHS.values()))
    for c in ER.CASES:                                               # every kernel a row names is launched somewhere in the file
        for k in c.kernels:
            assert any(claims(s, k) for s in ge), (c.id, k)
        assert c.why and c.group in ER.GROUPS and (c.entry, c.group) in ROWS, c.id
    assert len(ER.GROUPS) - 1 <= 3                                   # at most three child processes
    # every switch the launchers read is an SGX_SWITCH accessor, set by a group or excused by name (and planned by tests/test_gepi_plan.py)
    with open(os.path.join(CSRC, "gepi.hip")) as f:
        src = f.read()
    read = set(re.findall(r'SGX_SWITCH\(\s*\w+\s*,\s*"(SGX_[A-Z0-9_]*)"', src))
    assert read == {"SGX_GEPI_RPT", "SGX_GEPI_SMALL", "SGX_GEPI_APPLY1", "SGX_GEPI_BWD2S", "SGX_GEPI_FOLD"} and "getenv" not in src
    excused = " ".join(ER.EXCLUDED_PATHS)
    assert all(any(k in g for g in ER.GROUPS.values()) or k in excused for k in read), read


def test_a_new_kernel_or_a_dropped_row_is_noticed():
    ge, op = sites()
    assert unclaimed(ge + [("gepi_brand_new", "<T>")], ER.CASES, ER.EXCLUDED_SITES) == ["gepi_brand_new<T>"]
    assert unclaimed(ge + [("gepi_pass", "<T, 3>")], ER.CASES, ER.EXCLUDED_SITES) == ["gepi_pass<T, 3>"]
    assert unclaimed(op + [("lamb_multi_kernel", "")], OPTIM_ROWS, ER.EXCLUDED_SITES) == ["lamb_multi_kernel"]
    without = [c for c in ER.CASES if "gepi_rows_prereduce" not in c.kernels]
    assert unclaimed(ge, without, ER.EXCLUDED_SITES) == ["gepi_rows_prereduce"]
    no_nt = [c for c in ER.CASES if c.group != "switch_nt"]
    assert unclaimed(ge, no_nt, ER.EXCLUDED_SITES) == ["gepi_pass<T, 2, true>"]
    no_f32_apply1 = [c for c in ER.CASES if "gepi_apply1<float>" not in c.kernels]
    assert unclaimed(ge, no_f32_apply1, ER.EXCLUDED_SITES) == ["gepi_apply1<T> for ['float']"] * 1
    assert unclaimed(op, OPTIM_ROWS[1:], ER.EXCLUDED_SITES) == ["sumsq_stage1", "sumsq_stage2"]
    assert dict(collections.Counter((c.entry, c.group) for c in ER.CASES)) == ROWS


def selected(c):
    a, env = c.args, ER.group_env(c.group)
    if c.entry == "sgx_gepi_fwd":
        return ER.fwd_kernels(a["B"], a["HW"], a["C"], c.dtype, a["flags"], a.get("pre"), env)
    if c.entry == "sgx_gepi_bwd":
        return ER.bwd_kernels(a["B"], a["HW"], a["C"], c.dtype, env)
    if c.entry == "sgx_gepi_stats":
        return ER.stats_kernels(a["B"], a["HW"], a["C"], c.dtype, a["flags"], a.get("pre"))
    return ([f"blur_stats_kernel<{SR.tname(c.dtype)}>"] if c.entry == "sgx_blur3x3_stats" else []) + ER.fwd_kernels(a["B"], a["H"] * a["W"], a["C"], c.dtype, a["flags"], True, env)


def test_case_table_shapes_select_what_they_say():
    """gepi_geom, gepi_small_ok, GsPlan::pick, the two size thresholds and the pre-reduction condition, restated on the rows' own arguments."""
    for c in ER.CASES:
        assert tuple(selected(c)) == c.kernels, (c.id, selected(c))
        ve = 4 if c.dtype == F else 8
        assert c.args["C"] % ve == 0 and (256 % (c.args["C"] // ve) == 0 or (c.args["C"] // ve) % 256 == 0), c.id     # gepi_check takes it
        if "twin" in c.args:
            t = ER.BY_ID[c.args["twin"]]
            assert t.group == "default" and t.entry == c.entry and not t.kernels[0].startswith("gepi_small"), c.id
            assert all(t.args.get(k) == c.args.get(k) for k in ("B", "HW", "C", "flags", "bias", "data", "pre", "dbias")), c.id
    by = ER.BY_ID
    # the seams sit where the rows say
    assert ER.gs_plan(H, 256) == (1024, 0) and ER.gs_plan(H, 257) == (1024, 1) and ER.gs_plan(F, 128) == (512, 0) and ER.gs_plan(F, 129) == (512, 1)
    assert ER.gepi_small_ok(8, 1024, 512, H) and not ER.gepi_small_ok(9, 1024, 512, H) and 8 * 1024 * 512 * 2 == 8 << 20
    assert ER.gepi_small_ok(64, 16, 16, H) and not ER.gepi_small_ok(63, 16, 16, H)
    assert ER.gepi_geom(2, 1300, 32, 8) == ER.Geom(4, 64, 8, 512, 3) and ER.gepi_geom(6, 1 << 20, 16, 8) == ER.Geom(2, 128, 64, 8192, 128)
    assert ER.gepi_geom(1, 520, 2048, 4) == ER.Geom(256, 1, 8, 8, 65)
    assert ER.bwd2s_route(64, 4096, 16, H) == (8, 256) and ER.bwd2s_route(24, 1 << 20, 16, H) == (2048, 256) and ER.bwd2s_route(2, 626, 32, H) == (3, 0)
    # every cv of gepi_bwd2s in both dtypes, each with an integer row; every forward and backward path has an integer row
    for dt in (F, H):
        for cv in (1, 2, 4, 8, 16):
            rows = [c for c in ER.CASES if c.dtype == dt and f"gepi_bwd2s<{SR.tname(dt)}>" in c.kernels and c.args["C"] // (4 if dt == F else 8) == cv]
            assert len(rows) >= 3 and any(c.args["data"] == "int" for c in rows), (dt, cv)
    # every forward and backward path has an integer row, but for the ones excused by name with a reason (the conv_stats row runs the kernels of
    # the default pre-partials path, whose integer row is fwd-pre-int)
    paths = collections.defaultdict(set)
    for c in ER.CASES:
        paths[(c.group, tuple(k.replace("<float", "<T").replace("<bf16_t", "<T") for k in c.kernels))].add(c.args["data"])
    assert {k for k, v in paths.items() if "int" not in v} == set(ER.NO_INTEGER_ROW), sorted(k for k, v in paths.items() if "int" not in v)
    assert all(len(r) > 10 for r in ER.NO_INTEGER_ROW.values())
    for dt in (F, H):                                                                # ... in each dtype of its own
        for k in {(c.group, c.kernels) for c in ER.CASES if c.dtype == dt}:
            norm = (k[0], tuple(x.replace("<float", "<T").replace("<bf16_t", "<T") for x in k[1]))
            assert norm in ER.NO_INTEGER_ROW or any(c.args["data"] == "int" for c in ER.CASES if (c.group, c.kernels) == k), k
    # the default policy at the real thresholds
    assert 2 * 6 * (1 << 20) * 16 >= 192e6 > 2 * 5 * (1 << 20) * 16 and 2 * 24 * (1 << 20) * 16 >= 800e6 > 2 * 23 * (1 << 20) * 16
    assert "gepi_apply1<bf16_t>" in by["fwd-headline-B6-bf16"].kernels and "gepi_apply<bf16_t>" in by["fwd-headline-B5-bf16"].kernels
    assert "gepi_bwd2s<bf16_t>" in by["bwd-headline-B24-bf16"].kernels and "gepi_rows_prereduce" in by["bwd-headline-B24-bf16"].kernels
    # the fp32 chains the bounds use
    assert ER.chain_fwd(16, 256, 64, H, by["fwd-small-HW256-bf16"].kernels) == 2 and ER.chain_fwd(16, 1024, 64, H, by["fwd-small-HW1024-bf16"].kernels) == 4
    assert ER.chain_fwd(6, 1 << 20, 16, H, by["fwd-headline-B6-bf16"].kernels) == 64 and ER.chain_fwd(2, 300, 32, H, by["fwd-pre-7-bf16"].kernels) == 1
    assert ER.chain_bwd(2, 626, 32, H, by["bwd-bwd2s-cv4-3-blocks-bf16"].kernels) == (8, 6) and ER.chain_bwd(24, 1 << 20, 16, H, by["bwd-headline-B24-bf16"].kernels) == (64, 7)
    assert ER.blur_stats_geom(2, 20, 70, 32, 8) == (8, 6)


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation of the lane chains
def _seeded(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def lane_sums(v, L):
    """[B][HW][C] fp32 -> [B][C] fp64: lane r adds pixels r, r + R, .. (at most L of them) in fp32, the lanes are added in fp64."""
    B, HW, C = v.shape
    R = (HW + L - 1) // L
    pad = torch.zeros(B, R * L - HW, C)
    w = torch.cat([v, pad], 1).view(B, L, R, C)
    acc = torch.zeros(B, R, C)
    for i in range(L):
        acc = acc + w[:, i]
    assert acc.dtype == torch.float32
    return acc.double().sum(1)


def lrelu32(p):
    return torch.where(p > 0, p, torch.tensor(SR.LRELU) * p)


def emulate_fwd(x, bias, noise, nw, style, L, drop=None, noise_shift=0, swap=None):
    """The forward as the kernels compute it (fp32, the order of csrc/gepi.hip), with optional planted errors: ``drop`` pixels missing from the
    statistics, the noise of the last ``noise_shift`` pixels read one pixel on, the style of channel vectors ``swap`` exchanged in image 0."""
    B, HW, C = x.shape
    xf = x.float()
    a = lrelu32((xf + bias) + nw * noise.unsqueeze(-1))
    s = a if drop is None else torch.cat([a[:, :drop[0]], a[:, drop[1]:]], 1)
    m = lane_sums(s, L) / HW
    var = (lane_sums(s * s, L) / HW - m * m).clamp_min(0.0)
    mean, rstd = m.float(), (1.0 / torch.sqrt(var + ER.EPS)).float()
    nz = noise.clone()
    if noise_shift:
        nz[:, HW - noise_shift:HW - 1] = noise[:, HW - noise_shift + 1:]
    st = style.clone()
    if swap:
        (i, j), ve = swap, 8
        st[0, i * ve:(i + 1) * ve], st[0, j * ve:(j + 1) * ve] = style[0, j * ve:(j + 1) * ve], style[0, i * ve:(i + 1) * ve]
        st[0, C + i * ve:C + (i + 1) * ve], st[0, C + j * ve:C + (j + 1) * ve] = style[0, C + j * ve:C + (j + 1) * ve], style[0, C + i * ve:C + (i + 1) * ve]
    a2 = lrelu32((xf + bias) + nw * nz.unsqueeze(-1))
    y = ((a2 - mean.unsqueeze(1)) * rstd.unsqueeze(1)) * (st[:, :C] + 1.0).unsqueeze(1) + st[:, C:].unsqueeze(1)
    assert y.dtype == torch.float32
    return y.to(x.dtype), mean, rstd


HW_EMU = 16384


def fwd_operands(style_scale=0.5, offs=(0.0, 3.0, -1.5, 30.0)):
    B, HW, C = 2, HW_EMU, 64
    off = torch.tensor(offs)[torch.arange(C) % 4]
    x = (_seeded((B, HW, C), 1) + off).bfloat16()
    return x, _seeded((C,), 2, 0.1), _seeded((B, HW), 3), _seeded((C,), 4, 0.1), _seeded((B, 2 * C), 5, style_scale)


def judge_fwd(x, bias, noise, nw, style, y, mean, rstd, L):
    x64, b64, nz64, nw64 = x.double(), bias.double(), noise.double(), nw.double()
    (mr, rr), (dm, dr) = ER.gepi_stats(x64, b64, nz64, nw64, 3, L)
    r1, r2 = ER.assert_within(mean, mr, dm, "mean"), ER.assert_within(rstd, rr, dr, "rstd")
    ref, S = ER.gepi_fwd(x64, b64, nz64, nw64, style.double(), mean.double(), rstd.double(), 3)
    return r1, r2, SR.assert_elementwise(y, ref, S, ER.N_FWD, y.dtype, "y")


def true_y(x, bias, noise, nw, style):
    x64, b64, nz64, nw64 = x.double(), bias.double(), noise.double(), nw.double()
    (mr, rr), _ = ER.gepi_stats(x64, b64, nz64, nw64, 3, 1)
    return ER.gepi_fwd(x64, b64, nz64, nw64, style.double(), mr, rr, 3)[0]


def test_criterion_passes_the_fp32_emulation_of_the_lane_chains():
    ops = fwd_operands()
    for L in (2, 4, 64):
        r = judge_fwd(*ops, *emulate_fwd(*ops, L), L)
        assert max(r) <= 1.0, r
    # constant channels: a true variance of 0, the clamp, rstd = 1 / sqrt(eps); everything finite and inside the bounds
    x, bias, noise, nw, style = ops
    xc = ((_seeded((2, 1, 64), 6, 4.0)).round() / 4.0).expand(2, HW_EMU, 64).contiguous().bfloat16()
    y, mean, rstd = emulate_fwd(xc, bias, noise, torch.zeros(64), style, 64)
    judge_fwd(xc, bias, noise, torch.zeros(64), style, y, mean, rstd, 64)
    assert bool(torch.isfinite(y.float()).all()) and float(rstd.max()) <= 316.23
    # integer rows: 2^20 squares of integers |v| <= 3 add up exactly in fp32 in any order
    v = torch.randint(-3, 4, (1 << 20,), generator=torch.Generator().manual_seed(7)).float()
    sq = v * v
    assert float(sq.sum()) == float(sq.double().sum()) == float(sq.flip(0).cumsum(0)[-1]) < 1 << 24


def test_criterion_fails_planted_errors_the_rel_l2_metric_passes():
    """A wrong tail vector, a chunk missing from the statistics, the noise read one pixel off in the last row group, two channel vectors with
    each other's style: each passes rel-L2 at the suite's 3e-3 and fails here."""
    L = 64
    ops = fwd_operands()
    x, bias, noise, nw, style = ops
    want = true_y(*ops)
    good = emulate_fwd(*ops, L)
    gpu_util.assert_close(good[0].float(), want, 3e-3, "honest")
    # (1) the last 16-byte vector of image 1 holds the vector before it
    y = good[0].clone(); y[1, -1, -8:] = y[1, -1, -16:-8]
    gpu_util.assert_close(y.float(), want, 3e-3, "tail vector")
    with pytest.raises(AssertionError, match=r"y: \d of 2097152 elements.*\(1, 16383, 5\d\)"):
        judge_fwd(*ops, y, good[1], good[2], L)
    # (2) one chunk of 4 pixels missing from the statistics: y agrees with the kernel's own mean / rstd, the statistics do not with fp64
    ops2 = fwd_operands(offs=(0.0, 3.0, -1.5, 0.5))
    y, mean, rstd = emulate_fwd(*ops2, L, drop=(HW_EMU - 4, HW_EMU))
    gpu_util.assert_close(y.float(), true_y(*ops2), 3e-3, "dropped chunk")
    with pytest.raises(AssertionError, match="mean: .* values outside the bound"):
        judge_fwd(*ops2, y, mean, rstd, L)
    ref, S = ER.gepi_fwd(ops2[0].double(), bias.double(), noise.double(), nw.double(), style.double(), mean.double(), rstd.double(), 3)
    SR.assert_elementwise(y, ref, S, ER.N_FWD, y.dtype, "y on its own statistics")
    # (3) the noise of the last row group read one pixel on
    y, mean, rstd = emulate_fwd(*ops, L, noise_shift=3)
    gpu_util.assert_close(y.float(), want, 3e-3, "shifted noise")
    with pytest.raises(AssertionError, match=r"y: \d+ of 2097152 elements.*\(0, 16381, "):
        judge_fwd(*ops, y, mean, rstd, L)
    # (4) two channel vectors of image 0 with each other's style (styles near zero, as at initialisation)
    ops = fwd_operands(style_scale=0.002)
    want = true_y(*ops)
    y, mean, rstd = emulate_fwd(*ops, L, swap=(2, 5))
    gpu_util.assert_close(y.float(), want, 3e-3, "swapped styles")
    with pytest.raises(AssertionError, match=r"y: \d+ of 2097152 elements.*\(0, \d+, (1[6-9]|2[0-3])\)"):
        judge_fwd(*ops, y, mean, rstd, L)


def emulate_bwd(dy, x, bias, noise, nw, style, mean, rstd, L, skip_ror8=False):
    """sgx_gepi_bwd in fp32 in the kernels' order (gepi_pass<T, 1>, gepi_fin_bwd1, gepi_bwd2s with cv = 4).  skip_ror8: the first row-rotation
    sum left out -- lanes 8..15 of a 16-lane row never reach the lanes that write, modelled by pixel, not lane by lane: pixels p % 4 >= 2 are
    missing from dnw / dbias."""
    B, HW, C = x.shape
    xf, g = x.float(), dy.float()
    p = (xf + bias) + nw * noise.unsqueeze(-1)
    xh = (lrelu32(p) - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    s1, s0 = lane_sums(g, L), lane_sums(g * xh, L)
    sc = style[:, :C].double() + 1.0
    k1, k2 = (sc * s1 / HW).float().unsqueeze(1), (sc * s0 / HW).float().unsqueeze(1)
    ks = (style[:, :C] + 1.0).unsqueeze(1)
    da = rstd.unsqueeze(1) * ((g * ks - k1) - xh * k2)
    dp = da * torch.where(p > 0, 1.0, SR.LRELU)
    assert dp.dtype == torch.float32
    keep = dp if not skip_ror8 else dp * (torch.arange(HW) % 4 < 2).float().view(1, HW, 1)
    dnw = lane_sums(keep * noise.unsqueeze(-1), 6).sum(0).float()      # gepi_bwd2s with cv = 4: 4 vectors per thread + 2 row-rotation sums
    dbias = lane_sums(keep, 6).sum(0).float()
    return dp.to(x.dtype), torch.cat([s0, s1], 1).float(), dnw, dbias


def test_backward_criterion_on_the_emulation_and_an_omitted_row_rotation():
    """The honest backward passes; with one ror_add step of cv = 4 left out dx and dstyle are untouched (rel-L2 on them: 0 change) and d noise
    weight / d bias lose half their pixels: the reductions' own bound fails them.  (On those two outputs rel-L2 would object as well -- what hid
    such an error is that no test ran gepi_bwd2s against an independent reference.)"""
    B, HW, C, L = 2, 4096, 32, 8
    off = torch.tensor([0.0, 3.0, -1.5, 30.0])[torch.arange(C) % 4]
    x, dy = (_seeded((B, HW, C), 11) + off).bfloat16(), _seeded((B, HW, C), 12).bfloat16()
    bias, noise, nw, style = _seeded((C,), 13, 0.1), _seeded((B, HW), 14), _seeded((C,), 15, 0.3), _seeded((B, 2 * C), 16, 0.5)
    x64, b64, nz64, nw64 = x.double(), bias.double(), noise.double(), nw.double()
    (m64, r64), _ = ER.gepi_stats(x64, b64, nz64, nw64, 3, 0)
    mean, rstd = m64.float(), r64.float()
    b = ER.gepi_bwd(dy.double(), x64, b64, nz64, nw64, style.double(), mean.double(), rstd.double(), 3, L, 4 + 2)

    def judge(dx, dstyle, dnw, dbias):
        ref, nk = ER.choose_slope(dx, b)
        assert nk <= ER.kink_cap(dx.numel())
        out = [SR.assert_elementwise(dx, ref, b.S_dx, b.n_dx, dx.dtype, "dx"),
               SR.assert_elementwise(dstyle[:, :C], b.dstyle[:, :C], b.S_dstyle[:, :C], L + 7, F, "dstyle0"),
               SR.assert_elementwise(dstyle[:, C:], b.dstyle[:, C:], b.S_dstyle[:, C:], L, F, "dstyle1")]
        return out + [SR.assert_elementwise(dnw, b.dnw, b.S_dnw, b.n_dnw, F, "dnw"), SR.assert_elementwise(dbias, b.dbias, b.S_dbias, b.n_dbias, F, "dbias")]
    good = emulate_bwd(dy, x, bias, noise, nw, style, mean, rstd, L)
    assert max(judge(*good)) <= 1.0
    bad = emulate_bwd(dy, x, bias, noise, nw, style, mean, rstd, L, skip_ror8=True)
    assert torch.equal(bad[0], good[0]) and torch.equal(bad[1], good[1])
    with pytest.raises(AssertionError, match=r"dnw: \d+ of 32 elements"):
        judge(*bad)
    # the kink rule: an element at p = 0 may take either slope, no other may
    other = good[0].clone().float()
    i = (0, 5, 3)
    other[i] = float(b.dx_alt[i])
    with pytest.raises(AssertionError, match=r"dx: 1 of"):
        SR.assert_elementwise(other.bfloat16(), ER.choose_slope(other.bfloat16(), b)[0], b.S_dx, b.n_dx, H, "dx")


def test_references_against_the_oracle_and_autograd():
    x = _seeded((2, 9, 7, 16), 21).bfloat16().double()
    y, S = ER.blur3x3_stats(x, None, None, None, 0)
    assert torch.allclose(y, O.blur3(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1), rtol=1e-13, atol=1e-15) and bool((S >= y.abs()).all())
    # the epilogue and its backward against autograd of the same expression in fp64
    B, HW, C = 2, 37, 8
    xs, dy = _seeded((B, HW, C), 22).double().requires_grad_(True), _seeded((B, HW, C), 23).double()
    bias, nw, style = (_seeded((C,), 24).double().requires_grad_(True), _seeded((C,), 25).double().requires_grad_(True), _seeded((B, 2 * C), 26).double().requires_grad_(True))
    noise = _seeded((B, HW), 27).double()
    a = torch.nn.functional.leaky_relu(xs + bias + nw * noise.unsqueeze(-1), SR.LRELU)
    mean, var = a.mean(1), a.var(1, unbiased=False)
    yy = (a - mean.unsqueeze(1)) / torch.sqrt(var + ER.EPS).unsqueeze(1) * (style[:, :C] + 1).unsqueeze(1) + style[:, C:].unsqueeze(1)
    gx, gb, gn, gs = torch.autograd.grad((yy * dy).sum(), (xs, bias, nw, style))
    (m, r), _ = ER.gepi_stats(xs.detach(), bias.detach(), noise, nw.detach(), 3, 1)
    assert torch.allclose(m, mean.detach()) and torch.allclose(r, 1 / torch.sqrt(var.detach() + ER.EPS))
    assert torch.allclose(ER.gepi_fwd(xs.detach(), bias.detach(), noise, nw.detach(), style.detach(), m, r, 3)[0], yy.detach())
    b = ER.gepi_bwd(dy, xs.detach(), bias.detach(), noise, nw.detach(), style.detach(), m, r, 3, 1, 1)
    for got, want in ((b.dx, gx), (b.dbias, gb), (b.dnw, gn), (b.dstyle, gs)):
        assert torch.allclose(got, want, rtol=1e-10, atol=1e-12)
    assert bool((b.S_dx >= b.dx.abs() * (1 - 1e-12)).all())
    # producer partials add up to the whole, whatever the count
    for n in (1, 7, 17, 129):
        pt = ER.partials(xs.detach(), bias.detach(), noise, nw.detach(), 3, n) if n < HW else None
        if pt is not None:
            assert pt.shape == (B, n, C, 2) and torch.allclose(pt.sum(1)[..., 0], a.detach().sum(1)) and torch.allclose(pt.sum(1)[..., 1], (a * a).detach().sum(1))
    # Adam and the EMA against torch's own in fp64
    p0, g = _seeded((50,), 28).double(), _seeded((50,), 29).double()
    q = torch.nn.Parameter(p0.clone()); q.grad = g.clone()
    opt = torch.optim.Adam([q], lr=0.003, betas=(0.5, 0.75), eps=1e-8)
    opt.step()
    (rp, rm, rv), _ = ER.adam(p0, g, torch.zeros(50, dtype=torch.float64), torch.zeros(50, dtype=torch.float64), 0.5, 0.75, 1e-8, 0.003 / (1 - 0.5), (1 - 0.75) ** 0.5, 1.0)
    assert torch.allclose(rp, q.detach(), rtol=1e-12) and torch.allclose(rm, 0.5 * g) and torch.allclose(rv, 0.25 * g * g)
    assert torch.allclose(ER.ema(p0, g, 0.75)[0], 0.75 * p0 + 0.25 * g)


def test_workspace_query_takes_every_row_shape():
    """sgx_gepi_ws_bytes is host-only arithmetic over both vector widths.  fp32 with C = 4 has no bf16 vector: the query -- and with it every
    entry point, through gepi_check -- divided by zero (found by the rows *-fold-cv1-f32)."""
    from stylegan.pytorch_amd import native
    native.build()
    L = native.lib()
    for c in ER.CASES:
        a = c.args
        B, C, HW = a["B"], a["C"], a.get("HW") or a["H"] * a["W"]
        g = ER.gepi_geom(B, HW, C, 4 if c.dtype == F else 8)
        assert L.sgx_gepi_ws_bytes(B, HW, C) >= 2 * B * g.nchunk * C * 2 * 8 + B * C * 2 * 4, c.id
    assert L.sgx_gepi_ws_bytes(2, 2500, 4) > 0
