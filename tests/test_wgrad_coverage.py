"""CPU side of tests/test_gpu_wgrad_paths.py: (1) every hipLaunchKernelGGL site of csrc/wgrad2.hip and of the weight-gradient section of
csrc/conv.hip is claimed by a row of wgrad_ref.CASES or excused by name with a reason, and the wgrad_kernel instantiations the restated
wgrad_ch / wgrad_tile (wgrad_ref's, not the library's: tests/test_wgrad_plan.py holds the library's plan and its compiled kernels against
them) can return are exactly the ones the rows name; (2) the restated launcher rules select, for every row's own arguments,
the kernels and split counts the row says, at 256 and at 304 CUs; (3) the fp64 references agree with autograd of the oracle's convolution;
(4) both criteria pass an fp32 emulation of the kernels (per-split partials, then the finishing pass) and fail nine planted errors."""
import collections
import itertools
import os
import re

import pytest
import torch

import streaming_ref as SR
import wgrad_ref as WR
from oracle import stylegan_oracle as O
from test_streaming_coverage import CSRC, SITE, claims, unclaimed

F, H = torch.float32, torch.bfloat16
# Rows per environment group.  A row is a launch path someone decided to cover: dropping one has to be a decision made here too.
ROWS = {"default": 191, "w2_0": 3, "w2_3": 3, "w2_5": 3, "w2_6": 3, "tr0": 19, "pre0": 2, "pre4": 4, "maxsplit3": 3, "blocks": 2, "maxct1": 3}
# Sites that name no instantiation, by the text of the site
FUNCTION_POINTER = {"kern": "wgrad_kernel<T, GEO, TH, TW, BP, NSUB, KSUB, TR> through launch_wgrad's function pointer, one launch_wgrad per entry of WGRAD_TABLE: the instantiation scan below enumerates them"}


def sites():
    with open(os.path.join(CSRC, "conv.hip")) as f:
        src = f.read()
    a, b = src.index("// Weight gradients."), src.index("// Weight packing")
    assert 0 < a < b
    scan = lambda text: [(m.group(1), (m.group(2) or "").strip()) for m in SITE.finditer(text)]
    with open(os.path.join(CSRC, "wgrad2.hip")) as f:
        return scan(src[a:b]), scan(f.read())


def test_every_launch_site_is_claimed_or_excused():
    cv, w2 = sites()
    assert len(cv) == 6 and len(w2) == 4, (cv, w2)                    # the scan found the launchers
    assert unclaimed(cv + w2, WR.CASES, dict(WR.EXCLUDED_SITES, **FUNCTION_POINTER)) == []
    assert set(FUNCTION_POINTER) | set(WR.EXCLUDED_SITES) <= {s[0] + s[1] for s in cv + w2}
    assert all(len(r) > 10 for r in list(WR.EXCLUDED_SITES.values()) + list(WR.EXCLUDED_PATHS.values()) + list(FUNCTION_POINTER.values()))
    for c in WR.CASES:                                                # every kernel a row names is launched somewhere in the two files
        for k in c.kernels:
            assert k.startswith("wgrad_kernel<") or any(claims(s, k) for s in cv + w2), (c.id, k)
        assert c.why and c.group in ROWS, c.id
    # every switch the launchers read is set by a group or excused by name
    with open(os.path.join(CSRC, "conv.hip")) as f:
        src = f.read()
    with open(os.path.join(CSRC, "wgrad2.hip")) as f:
        read = set(re.findall(r'SGX_SWITCH\(\s*\w+\s*,\s*"(SGX_WGRAD[A-Z0-9_]*)"', src[src.index("// Weight gradients."):src.index("// Weight packing")] + f.read()))
    assert read == set(WR.ENV0) and read - {k for g in WR.GROUPS.values() for k in g} == set(WR.EXCLUDED_PATHS)


def test_a_new_kernel_or_a_dropped_row_is_noticed():
    cv, w2 = sites()
    ex = dict(WR.EXCLUDED_SITES, **FUNCTION_POINTER)
    assert unclaimed(w2 + [("wgrad2_s_kernel", "<16>")], WR.CASES, ex) == ["wgrad2_s_kernel<16>"]
    assert unclaimed(cv + [("wgrad_finish_kernel", "<32>")], WR.CASES, ex) == ["wgrad_finish_kernel<32>"]
    assert unclaimed(cv, [c for c in WR.CASES if WR.PRE not in c.kernels], ex) == [WR.PRE]
    assert unclaimed(w2, [c for c in WR.CASES if "wgrad2_d_kernel<1>" not in c.kernels], ex) == ["wgrad2_d_kernel<1>"]
    assert unclaimed(cv, [c for c in WR.CASES if "wgrad_finish_kernel<8>" not in c.kernels], ex) == ["wgrad_finish_kernel<8>"]
    assert dict(collections.Counter(c.group for c in WR.CASES)) == ROWS


def reachable():
    """Every wgrad_kernel instantiation wgrad_ref's wgrad_ch and wgrad_tile can return, by enumeration over the geometry, the dtype, SGX_WGRAD_TR, the
    parity classes of the channel counts (multiples of 16 that are / are not multiples of 32, and the 512-channel sizes of lowres_big) and
    the size classes of the n-side grid."""
    out = set()
    for geo, dt, tr, Cn, Ck, Hn, Wn, B in itertools.product((0, 1), (F, H), (0, 1), (16, 32, 48, 512), (16, 32, 48, 512), (4, 8, 12, 16, 40), (4, 8, 16, 24), (1, 40)):
        if dt == F and tr:
            continue
        NS, KS, _ = WR.wgrad_ch(geo, B, Hn, Wn, Ck, Cn)
        TH, TW, BP = WR.wgrad_tile(geo, Hn, Wn)
        out.add(WR.g1(dt, geo, TH, TW, NS, KS, bool(tr)))
    return out


def test_reachable_instantiations_equal_the_rows():
    named = {k for c in WR.CASES for k in c.kernels if k.startswith("wgrad_kernel<")}
    assert reachable() == named, (sorted(reachable() - named), sorted(named - reachable()))
    assert len(named) == 54                                           # 3 tiles x (4 + 2) channel pairs x (fp32, bf16 TR, bf16 plain)
    # each with an integer row of its own
    assert named == {k for c in WR.CASES if c.args["data"] == "int" for k in c.kernels if k.startswith("wgrad_kernel<")}


def test_case_table_shapes_select_what_they_say():
    for ncu in (256, 304):
        for c in WR.CASES:
            a, p = c.args, WR.row_plan(c, ncu)
            ns = WR.NS_AT_304.get(c.id, a["ns"]) if ncu == 304 else a["ns"]
            fns = ns if a["fns"] == a["ns"] else a["fns"]
            assert (p.kernels, p.nsplit, p.finish_ns, p.rc) == (c.kernels, ns, fns, a["rc"]), (ncu, c.id, p)
    assert {c.id for c in WR.CASES if WR.row_plan(c, 256).nsplit != WR.row_plan(c, 304).nsplit} == set(WR.NS_AT_304)
    by = WR.BY_ID
    for c in WR.CASES:
        a = c.args
        if a["data"] == "int":
            assert WR.exact_ok(c), c.id                               # the exactness condition of the integer rows
        if c.group != "default" and a["data"] == "int":
            assert a["twin"], c.id                                    # every switched integer row has a default twin ...
        if a["twin"]:
            t = by[a["twin"]]
            assert t.args["data"] == a["data"] == "int" and (t.group == "default") and t.dtype == c.dtype, c.id
            assert all(t.args[k] == a[k] for k in ("B", "H", "W", "Ck", "Cn", "mode", "adjoint", "O", "I", "acc", "bias")), c.id   # ... of the same problem
            assert (t.kernels, t.args["ns"], t.args["ws"]) != (c.kernels, a["ns"], a["ws"]) or c.group != t.group, c.id
    # the seams sit where the rows say
    assert WR.finish_epb(128, 64) == 64 and WR.finish_epb(112, 64) == 16 and WR.finish_epb(64, 32) == 16 and WR.finish_epb(48, 32) == 8 and WR.finish_epb(32, 32) == 8 and WR.finish_epb(48, 16) == 4
    assert WR.wgrad_ch(0, 4, 16, 16, 512, 512) == (2, 1, True) and WR.wgrad_ch(0, 1, 96, 88, 512, 512) == (2, 2, False) and WR.wgrad_ch(0, 1, 4, 4, 480, 480) == (2, 2, False)
    assert 1 * 96 * 88 > 64 * 128 >= 4 * 16 * 16
    assert WR.wgrad_nsplit(512, 64, 9 << 18, WR.ENV0) == 1 and WR.wgrad_nsplit(512, 65, 9 << 18, WR.ENV0) == 1 and WR.wgrad_nsplit(256, 65, 9 << 18, WR.ENV0) == 2
    assert WR.wgrad_nsplit(1, 5000, 9 * 256, WR.ENV0) == 1024 and WR.wgrad_nsplit(1, 5000, 16 * 32 * 32 + 1, WR.ENV0) == 512
    # the three regimes of sgx_wgrad2_plan, and where the CU count matters
    assert WR.wgrad2_plan(0, 9, 64, 64, 128, 128, WR.ENV0, 256)[0] == 64 and WR.wgrad2_plan(0, 9, 64, 64, 128, 128, WR.ENV0, 304)[0] == 72
    assert WR.wgrad2_plan(0, 4, 32, 32, 64, 64, WR.ENV0, 256)[0] == 8 and WR.wgrad2_plan(0, 3, 32, 32, 64, 64, WR.ENV0, 256)[0] == 0
    assert WR.wgrad2_plan(0, 16, 32, 32, 320, 512, WR.ENV0, 256)[0] == 8 and WR.wgrad2_plan(0, 15, 32, 32, 320, 512, WR.ENV0, 256)[0] == 0
    assert WR.wgrad2_plan(0, 2, 256, 512, 16, 16, WR.ENV0, 256)[0] == 256 == WR.wgrad2_plan(0, 2, 256, 512, 16, 16, WR.ENV0, 128)[0] and WR.wgrad2_plan(0, 2, 256, 512, 16, 16, WR.ENV0, 120)[0] == 240
    assert WR.wgrad2_plan(0, 2, 512, 1024, 16, 16, WR.ENV0, 256)[0] == 512 and WR.wgrad2_plan(0, 2, 512, 1024, 16, 16, WR.ENV0, 304)[0] == 608
    # every kernel family has integer, randn and |randn| rows
    fam = collections.defaultdict(set)
    for c in WR.CASES:
        if c.kernels:
            k = c.kernels[0]
            fam[("gen1 " + WR.tname(c.dtype)) if k.startswith("wgrad_kernel") else k, WR.PRE in c.kernels].add(c.args["data"])
    assert all(v == {"int", "randn", "abs"} for v in fam.values()), fam
    assert len(WR.GROUPS) - 1 == 10                                   # ten child processes, one after another


# ---------------------------------------------------------------------------------------------------------------- references against autograd
def _seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def test_references_against_the_oracle_and_autograd():
    gain = 2 ** 0.5
    # plain 3x3, with a bias, and I < Ip: the padded channels of x hold data the gradient must not see
    x, w, b = _seeded((2, 3, 7, 5), 1), _seeded((4, 3, 3, 3), 2).requires_grad_(True), _seeded((4,), 3).requires_grad_(True)
    y = O.eq_conv2d(x, w, b, gain)
    dy = _seeded(y.shape, 4)
    gw, gb = torch.autograd.grad((y * dy).sum(), (w, b))
    s = O.he_w_mul(3 * 9, gain)
    xp = torch.cat([x, _seeded((2, 2, 7, 5), 5)], 1)
    dW, S, db, Sb = WR.wgrad(nhwc(xp), nhwc(dy), "S", s, 3)
    assert dW.shape == gw.shape and torch.allclose(dW, gw, rtol=1e-12, atol=1e-13) and torch.allclose(db, gb, rtol=1e-12, atol=1e-13)
    assert bool((S >= dW.abs() * (1 - 1e-12)).all()) and bool((Sb >= db.abs() * (1 - 1e-12)).all())
    # the adjoint orientation (R1): the launch was the data-gradient convolution, x: O channels, dy: Ip channels
    x0 = _seeded((2, 3, 7, 5), 6).requires_grad_(True)
    g1 = _seeded((2, 4, 7, 5), 7)
    dx, = torch.autograd.grad(O.eq_conv2d(x0, w, None, gain), x0, g1, create_graph=True)
    g2 = _seeded((2, 5, 7, 5), 8)                                     # Ip = 5 > I = 3
    gw2, = torch.autograd.grad((dx * g2[:, :3]).sum(), w)
    dW2 = WR.wgrad(nhwc(g1), nhwc(g2), "S", s, 3, adjoint=1, want_db=False)[0]
    assert torch.allclose(dW2, gw2, rtol=1e-12, atol=1e-13)
    # accumulate: bit 0 adds to dW, bit 1 to db, each alone
    d0, b0 = _seeded(gw.shape, 9), _seeded((4,), 10)
    for acc in range(4):
        a = WR.wgrad(nhwc(x), nhwc(dy), "S", s, 3, 0, acc, d0, b0)
        assert torch.allclose(a[0], gw + (d0 if acc & 1 else 0), rtol=1e-12, atol=1e-13) and torch.allclose(a[2], gb + (b0 if acc & 2 else 0), rtol=1e-12, atol=1e-13)
    # fused down (the oracle fuses from 128 pixels): fine = x, coarse = dy
    x, w, b = _seeded((1, 2, 128, 128), 11), _seeded((3, 2, 3, 3), 12).requires_grad_(True), _seeded((3,), 13).requires_grad_(True)
    y = O.eq_conv2d(x, w, b, gain, down=True)
    assert y.shape == (1, 3, 64, 64)
    dy = _seeded(y.shape, 14)
    gw, gb = torch.autograd.grad((y * dy).sum(), (w, b))
    dW, _, db, _ = WR.wgrad(nhwc(x), nhwc(dy), "D", O.he_w_mul(2 * 9, gain), 2)
    assert torch.allclose(dW, gw, rtol=1e-11, atol=1e-12) and torch.allclose(db, gb, rtol=1e-11, atol=1e-12)
    # fused up (from 64 pixels): coarse = x, fine = dy, mode U; non-fused up (nearest-up then 3x3): mode UF
    for size, mode in ((64, "U"), (6, "UF")):
        x, w = _seeded((1, 2, size, size), 15), _seeded((3, 2, 3, 3), 16).requires_grad_(True)
        y = O.eq_conv2d(x, w, None, gain, up=True)
        assert y.shape == (1, 3, 2 * size, 2 * size)
        dy = _seeded(y.shape, 17)
        gw, = torch.autograd.grad((y * dy).sum(), w)
        dW = WR.wgrad(nhwc(dy), nhwc(x), mode, O.he_w_mul(2 * 9, gain), 2, want_db=False)[0]
        assert dW.shape == gw.shape and torch.allclose(dW, gw, rtol=1e-11, atol=1e-12), mode
        other = WR.wgrad(nhwc(dy), nhwc(x), "UF" if mode == "U" else "U", O.he_w_mul(2 * 9, gain), 2, want_db=False)[0]
        assert not torch.allclose(other, gw, rtol=1e-3, atol=1e-3)    # the flip is seen


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation, planted errors
def emulate(xk, xn, mode, scale, I, nsplit, rows_per_tile, acc=0, dW0=None, db0=None, adjoint=0, plant=None):
    """The launch in fp32 as the kernels run it: the n-side grid cut into tiles of ``rows_per_tile`` rows of one image, split s walks tiles s,
    s + nsplit, .. and keeps fp32 sums per tap (and the n side's column sums); the finishing pass adds the splits in order, folds the 4x4 taps,
    scales, re-lays-out, cuts at I and accumulates.  ``plant``: one of the errors of test_planted_errors_fail.  -> (dW [O][I][3][3] fp32 as a
    flat buffer with 9 spare floats behind it, db)."""
    geo = 0 if mode == "S" else 1
    B, Hn, Wn, Cn = xn.shape
    Ck = xk.shape[3]
    xk32, xn32 = xk.float(), xn.float()
    tiles = [(b, r) for b in range(B) for r in range(0, Hn, rows_per_tile)]
    NT = 9 if geo == 0 else 16
    part, bias = torch.zeros(nsplit, NT, Cn, Ck), torch.zeros(nsplit, Cn)
    for s in range(nsplit):
        mine = tiles[s::nsplit]
        if plant == "drop_tile" and s == 1:
            mine = mine[:-1]
        for (b, r) in mine:
            m = torch.zeros_like(xn32)
            m[b, r:r + rows_per_tile] = xn32[b, r:r + rows_per_tile]
            part[s] += WR.tap_partials(xk32, m, geo)
            bias[s] += xk32[b, (geo + 1) * r:(geo + 1) * (r + rows_per_tile)].sum((0, 1)) if plant == "db_from_k" else m.sum((0, 1, 2))
    assert part.dtype == torch.float32
    if plant == "bf16_partials":
        part = part.bfloat16().float()
    if plant == "swap_taps":
        part[:, 3, 5, 7], part[:, 4, 5, 7] = part[:, 4, 5, 7].clone(), part[:, 3, 5, 7].clone()
    order = list(range(nsplit)) + ([2] if plant == "split_twice" else [])
    tot, bsum = torch.zeros(9, Cn, Ck), torch.zeros(Cn)
    for s in order:
        P = part[s]
        if geo == 1:
            P4 = P.view(4, 4, Cn, Ck)
            P = ((P4[:3, :3] + P4[:3, 1:]) + (P4[1:, :3] + P4[1:, 1:])).reshape(9, Cn, Ck)
        tot, bsum = tot + P, bsum + bias[s]
    c = torch.tensor(scale, dtype=torch.float32) * (0.25 if mode == "D" and plant != "no_quarter" else 1.0)
    v = tot.flip(0) if (mode == "S" and adjoint) or (mode == "UF" and plant != "uf_noflip") else tot
    if adjoint or mode in ("U", "UF"):
        v = v.transpose(1, 2)
    v = (c * v).permute(1, 2, 0).contiguous()                          # [O][Ip][9]
    Oc = v.shape[0]
    out = torch.full((Oc * I * 9 + 9,), float("nan"))
    dw = out[:Oc * I * 9].view(Oc, I, 9)
    dw.copy_(v[:, :I] + dW0.float().view(Oc, I, 9) if acc & 1 else v[:, :I])
    if plant == "write_pad":
        for o in range(Oc):
            out[(o * I + I) * 9:(o * I + I) * 9 + 9] = v[o, I]        # the store of (o, i = I) in the [O][I][9] layout
    db = bsum + db0.float() if acc & 2 and plant != "ignore_acc_bit1" else bsum
    assert out.dtype == db.dtype == torch.float32
    return out, db


def judge(out, db, ref, S, rb, Sb, L, exact):
    dw = out[:ref.numel()].view(ref.shape)
    assert bool(torch.isnan(out[ref.numel():]).all()), "dW: written past its end"
    if exact:
        assert torch.equal(dw.view(torch.int32), ref.float().view(torch.int32)), f"dW: {int((dw != ref.float()).sum())} elements differ from the exact value"
        assert torch.equal(db.view(torch.int32), rb.float().view(torch.int32)), f"db: {int((db != rb.float()).sum())} elements differ from the exact value"
        return 0.0
    return max(SR.assert_elementwise(dw, ref, S, L, F, "dW"), SR.assert_elementwise(db, rb, Sb, L, F, "db"))


def problem(mode, data, seed=30):
    """B2, n side 16x24, 32 (n) x 32 (k) channels, bf16-exact operands, I = 17 of Ip = 32 for mode S."""
    g = torch.Generator().manual_seed(seed)
    geo = 0 if mode == "S" else 1
    shk, shn = (2, 16 * (geo + 1), 24 * (geo + 1), 32), (2, 16, 24, 32)
    if data == "int":
        xk, xn = torch.randint(-3, 4, shk, generator=g).double(), torch.randint(-3, 4, shn, generator=g).double()
    else:
        xk, xn = (torch.randn(shk, generator=g).abs().bfloat16().double(), torch.randn(shn, generator=g).abs().bfloat16().double())
    I = 17 if mode == "S" else 32
    dW0, db0 = (torch.randint(-3, 4, (32, I, 3, 3), generator=g) * 16).double(), (torch.randint(-3, 4, (32,), generator=g) * 16).double()
    scale = 0.5 if data == "int" else SR.f32(O.he_w_mul(32 * 9, 2 ** 0.5))
    return xk, xn, I, dW0, db0, scale


NSPLIT, ROWS_PER_TILE = 4, 4                                          # 8 tiles of 4 x 24 = 96 pixels
L_EMU = 2 * 96 + NSPLIT + 16
PLANTS = {"drop_tile": "one pixel tile dropped from one split", "split_twice": "one split added twice", "swap_taps": "two taps swapped for one channel pair",
          "no_quarter": "a missing 0.25 in mode D", "uf_noflip": "UF without the flip", "db_from_k": "db taken from the k side", "ignore_acc_bit1": "accumulate bit 1 ignored",
          "write_pad": "a padded channel written at i = I", "bf16_partials": "partials rounded to bf16"}
MODE_OF = {"no_quarter": "D", "uf_noflip": "UF"}


def run_emulation(mode, data, plant=None):
    xk, xn, I, dW0, db0, scale = problem(mode, data)
    db_ok = mode in ("S", "D")
    ref, S, rb, Sb = WR.wgrad(xk, xn, mode, scale, I, 0, 3, dW0, db0)
    out, db = emulate(xk, xn, mode, scale, I, NSPLIT, ROWS_PER_TILE, 3, dW0, db0, plant=plant)
    assert db_ok or plant not in ("db_from_k", "ignore_acc_bit1")
    return judge(out, db, ref, S, rb, Sb, L_EMU, data == "int")


def test_both_criteria_pass_the_fp32_emulation():
    for mode in ("S", "D", "U", "UF"):
        assert run_emulation(mode, "int") == 0.0
        r = run_emulation(mode, "abs")
        assert 0.0 < r <= 1.0, (mode, r)
    # the adjoint orientation
    xk, xn, I, dW0, db0, scale = problem("S", "int")
    ref, S, _, _ = WR.wgrad(xk, xn, "S", scale, 17, 1, 1, dW0, None, want_db=False)
    out, _ = emulate(xk, xn, "S", scale, 17, NSPLIT, ROWS_PER_TILE, 1, dW0, db0, adjoint=1)
    assert torch.equal(out[:ref.numel()].view(ref.shape), ref.float())


@pytest.mark.parametrize("plant", list(PLANTS), ids=list(PLANTS))
def test_planted_errors_fail(plant):
    """Each error fails the integer row's bit equality and the |randn| row's bound -- but for partials rounded to bf16, which the integer
    row cannot see (integers up to 256 are exact in bf16: with operands sparse enough that no partial exceeds that, the rounding changes
    nothing): that one is expected to pass the integer row and must fail the |randn| row, which is why every kernel family has rounding rows."""
    mode = MODE_OF.get(plant, "S")
    with pytest.raises(AssertionError, match="dW|db"):
        run_emulation(mode, "abs", plant)
    if plant == "bf16_partials":
        xk, xn, I, dW0, db0, scale = problem("S", "int")
        small = (torch.arange(xn.numel()).view(xn.shape) % 29 == 0)    # sparse operands: every sum an integer of at most 256, exact in bf16
        xn = torch.where(small, xn, torch.zeros_like(xn))
        ref, S, rb, Sb = WR.wgrad(xk, xn, "S", scale, I, 0, 0)
        out, db = emulate(xk, xn, "S", scale, I, NSPLIT, ROWS_PER_TILE, plant=plant)
        assert float(WR.tap_partials(xk.abs(), xn.abs(), 0).max()) <= 256 and float(xn.abs().sum((0, 1, 2)).max()) <= 256
        judge(out, db, ref, S, rb, Sb, L_EMU, True)                   # passes: the integer row does not see it
        return
    with pytest.raises(AssertionError, match="dW|db"):
        run_emulation(mode, "int", plant)
