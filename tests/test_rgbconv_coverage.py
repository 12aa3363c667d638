"""CPU side of tests/test_gpu_rgbconv_paths.py: (a) each of the seven hipLaunchKernelGGL sites of csrc/rgbconv.hip (one per kernel) is claimed by a row of
rgbconv_ref.CASES, every instantiation the launchers can reach is named by a row, every __global__ of the file is in the table; (b) the rows
reach what they are there for, computed from the restated launcher rules; (c) the references alone have the properties the GPU rows rely on,
and agree with autograd through the two layers; the contract rejections return before any launch; (d) the criteria pass a numpy fp32
emulation of the kernels' own arithmetic and fail six planted errors with the element named -- and what the checks that held this file before
(rel-L2 6e-3 / 8e-3 per tensor, 2 % of sign bits, exact integers at unit scales on 8 blocks) make of the same tensors is printed and pinned."""
import collections
import os
import re

import numpy as np
import pytest
import torch

import gpu_util
import rgbconv_ref as RR
import streaming_ref as SR
import test_streaming_coverage as TSC

RGB = os.path.join(TSC.CSRC, "rgbconv.hip")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
f4 = np.float32


@pytest.fixture(scope="module")
def lib():
    from stylegan.pytorch_amd import native
    native.build()
    return native.lib()


def source():
    with open(RGB) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------- (a) the scan
GENERIC = ("rgbconv_fwd_kernel", "<CB, EPI>")                # the one site that is generic in two template arguments: sgx_by_int<1, 2> around sgx_by_int<0, 1>


def unclaimed(sites, cases):
    """test_streaming_coverage.unclaimed (every value of the sgx_by_int list around a site), and for the generic site every pair of the two
    lists: the scan reads the innermost list only."""
    miss = TSC.unclaimed(sites, cases, {})
    named = {k for c in cases for k in c.kernels}
    if any(s[:2] == GENERIC for s in sites) and GENERIC[0] + GENERIC[1] not in miss:
        lack = [f"<{cb}, {epi}>" for cb in (1, 2) for epi in (0, 1) if RR.fwd_kernel(cb, epi) not in named]
        if lack:
            miss.append(f"{GENERIC[0]}{GENERIC[1]} for {lack}")
    return miss


def test_every_launch_site_of_rgbconv_hip_has_a_row():
    sites = TSC.launch_sites(RGB)
    # one site per kernel; the three <CB> kernels inside sgx_by_int<1, 2>, the LDS-tile forward inside that and sgx_by_int<0, 1>
    assert len(sites) == 7 and collections.Counter(s[0] for s in sites) == {k: 1 for k in RR.KERNELS}, sites
    by = {s[0]: s[1:] for s in sites}
    for k in ("rgbconv_fwdblur_kernel", "rgbconv_dgrad_kernel", "rgbconv_wgrad_kernel"):
        assert by[k] == ("<CB>", {"cb()": ["1", "2"], "CB": ["1", "2"]}), (k, by[k])
    assert by[GENERIC[0]] == (GENERIC[1], {"e()": ["0", "1"], "EPI": ["0", "1"]}), by[GENERIC[0]]
    assert all(by[k] == ("",) for k in (RR.PACK, RR.WFINISH, RR.CHAIN))
    assert unclaimed(sites, RR.CASES) == []
    kernels = set(re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+([A-Za-z_0-9]+)", source()))
    assert kernels == set(RR.KERNELS), kernels ^ set(RR.KERNELS)
    named = {k for c in RR.CASES for k in c.kernels}
    assert {k.split("<")[0] for k in named} == set(RR.KERNELS)
    for c in RR.CASES:
        assert c.why and c.entry in RR.ROWS, c.id
        for k in c.kernels:
            assert any(TSC.claims(s, k) for s in sites), (c.id, k)
    assert dict(collections.Counter(c.entry for c in RR.CASES)) == RR.ROWS
    assert len({r[0] for r in RR.REJECTIONS}) == len(RR.REJECTIONS)
    assert all(len(v) > 10 for v in RR.EXCLUDED_PATHS.values())


def test_a_new_site_or_a_dropped_row_is_noticed():
    sites = TSC.launch_sites(RGB)
    assert unclaimed(sites + [("rgbconv_fwdblur_kernel", "<4>")], RR.CASES) == ["rgbconv_fwdblur_kernel<4>"]
    assert unclaimed(sites + [("rgbconv_wgrad2_kernel", "")], RR.CASES) == ["rgbconv_wgrad2_kernel"]
    without = lambda k: [c for c in RR.CASES if k not in c.kernels]
    for k in ("rgbconv_fwdblur_kernel", "rgbconv_dgrad_kernel", "rgbconv_wgrad_kernel"):
        for cb in (1, 2):
            assert unclaimed(sites, without(f"{k}<{cb}>")) == [f"{k}<CB> for [{cb}]"]
    for cb in (1, 2):
        for epi in (0, 1):
            assert unclaimed(sites, without(RR.fwd_kernel(cb, epi))) == [f"rgbconv_fwd_kernel<CB, EPI> for ['<{cb}, {epi}>']"]
    assert unclaimed(sites, [c for c in RR.CASES if c.entry != "sgx_rgbconv_wgrad"]) == ["rgbconv_wgrad_kernel<CB>", "rgbconv_wfinish_kernel",
                                                                                         "rgbconv_chain_kernel"]


# ---------------------------------------------------------------------------------------------------------------- (b) rows reach their paths
def fwd_rows(variant=None, epi=1, special=False):
    return [c for c in RR.CASES if c.entry == "sgx_rgbconv_fwd" and c.args["epi"] == epi and (variant is None or c.args["variant"] == variant) and bool(c.args["special"]) == special]


def test_rows_reach_the_paths_they_are_there_for():
    for c in RR.CASES:
        r = RR.resolve(c)
        kernels, launches = RR.plan(r)
        assert tuple(kernels) == c.kernels and len(launches) == len(kernels), c.id
        a = r.args
        if a.get("B"):
            assert RR.shape_ok(a["B"], a["H"], a["W"], a["C"]), c.id
    assert not RR.shape_ok(1, 8, 64, 16) and not RR.shape_ok(1, 16, 32, 16) and not RR.shape_ok(1, 16, 64, 24) and not RR.shape_ok(1, 16, 64, 16, bf16=False)
    assert not RR.shape_ok(1, 24, 64, 16) and not RR.shape_ok(1, 16, 96, 16) and not RR.shape_ok(0, 16, 64, 16) and RR.shape_ok(1, 16, 64, 32)
    # the row-streaming forward: both walks, every row's last strip ragged, the listed last row blocks, both channel counts, NULL arguments
    v0 = fwd_rows(0)
    walks = {c.id: set(RR.fwdblur_walks(c.args["H"], c.args["W"], RR.fwdblur_geom(c.args["B"], c.args["H"], c.args["W"], c.args["nit"])).values()) for c in v0}
    assert walks["fwdblur-B2-16x64-C16-pos"] == {False} and walks["fwdblur-B1-48x128-C16-mix"] == {False, True}
    g = RR.fwdblur_geom(1, 48, 128)
    assert g.nit == 3 and g.nrb == 3 and [k for k, v in RR.fwdblur_walks(48, 128, g).items() if v] == [(sx, 1) for sx in range(1, 9)]
    assert all(c.args["W"] % RR.STRIP for c in v0) and 64 == 4 * 14 + 8
    assert {c.args["nit"]: RR.fwdblur_geom(1, 48, 128, c.args["nit"]).last for c in v0 if c.args["nit"]} == {1: 4, 2: 8, 4: 4, 6: 14, 8: 2}
    assert {c.args["C"] for c in v0} == {16, 32} and any(not c.args["bits"] for c in v0) and any(not c.args["b0"] for c in v0) and any(not c.args["ones"] for c in v0)
    assert {c.args["data"] for c in v0} == {"int", "pos", "mix", "real"}
    big = RR.BY_ID["fwdblur-B8-1024x1024-C16-nit"].args
    assert RR.fwdblur_geom(8, 1024, 1024).nit == 5 and 8 * 74 * 31 < 3 * 256 * 24 <= 8 * 74 * 37
    assert len({RR.fwdblur_geom(big["B"], big["H"], big["W"], n).grid for n in (3, 4, 5, 6)}) == 4
    assert RR.fwdblur_nit(32, 1024, 1024) == 6 and RR.fwdblur_nit(4, 1024, 1024) == 3
    # the LDS-tile forward: all four instantiations, both grid rules, LDS sizes as the structs give them
    assert {(c.args["variant"], c.args["C"]) for c in fwd_rows(1) + fwd_rows(2)} == {(1, 16), (1, 32), (2, 16), (2, 32)}
    assert {c.args["C"] for c in fwd_rows(epi=0)} == {16, 32} and {c.args["k"] for c in fwd_rows(epi=0)} == {0, -20, -120, 100, "zero", "tiles"}
    assert [RR.rc_fwd(cb, e).LDS for cb in (1, 2) for e in (0, 1)] == [9552, 10912 + 18 * 66 * 32, 9552, 6560 + 10 * 66 * 64]
    assert RR.rc_fwd(1, 1).TH == 16 and RR.rc_fwd(2, 1).TH == 8 and RR.rc_fwd(2, 0).TH == 16
    assert RR.plan(RR.BY_ID["fwd1-v2-B1-32x192-C32-pos"])[1][0][0] == (16, 1, 1) and RR.plan(RR.BY_ID["fwd1-v1-B1-32x192-C32-pos"])[1][0][0] is None
    # more tiles than blocks: whatever the occupancy query answers (2 .. 4 blocks per CU), the row's batch gives one-tile and two-tile blocks
    per_image = RR.fwd_ntiles(1, 256, 1024, 1, 1)
    assert per_image == RR.fwd_ntiles(1, 256, 1024, 1, 0) == 256
    for per_cu in (2, 3, 4):
        full = RR.ceil8(per_cu * RR.NCU_NOMINAL)
        nt = RR.persistent_batch(full, per_image) * per_image
        assert 1.1 * full <= nt <= 1.5 * full and {1, 2} <= set(RR.sched_counts(full, nt)), (per_cu, nt)
    assert len([c for c in RR.CASES if c.args.get("special") == "persistent"]) == 2
    # wgrad: zero partials, wfinish's second trip with a clamped tail, the tile loop's second trip, every acc bit, both ones, NULL outputs
    wg = [RR.resolve(c) for c in RR.CASES if c.entry == "sgx_rgbconv_wgrad"]
    nb = {c.id: (RR.wgrad_blocks(c.args["B"], c.args["H"], c.args["W"], RR.NCU_NOMINAL), RR.wgrad_ntiles(c.args["B"], c.args["H"], c.args["W"])) for c in wg}
    assert nb["wgrad-B2-16x64-C16-acc0"] == (8, 4) and nb["wgrad-B5-64x512-C16"] == (320, 320) and nb["wgrad-B3ncu-64x512-C16"] == (768, 832)
    assert RR.wfinish_trips(8) == (1, 7) and RR.wfinish_trips(320) == (2, 6) and RR.wfinish_trips(768) == (3, 0)
    assert set(RR.sched_counts(8, 4)) == {0, 1} and set(RR.sched_counts(320, 320)) == {1} and set(RR.sched_counts(768, 832)) == {1, 2}
    for ncu in (64, 80, 104, 228, 256, 304):                 # the tile-loop row takes its batch from the device
        r = RR.resolve(RR.BY_ID["wgrad-B3ncu-64x512-C16"], ncu).args
        nblk, nt = RR.wgrad_blocks(r["B"], 64, 512, ncu), RR.wgrad_ntiles(r["B"], 64, 512)
        assert nblk == RR.ceil8(3 * ncu) < nt and 2 in RR.sched_counts(nblk, nt), ncu
    assert {c.args["acc"] for c in wg} >= {0, 1, 2, 4, 8, 15} and {c.args["ones"] for c in wg} == {0, 1} and {c.args["C"] for c in wg} == {16, 32}
    assert {c.args["outs"] for c in wg} >= {"w0,b0,wr,br", "w0,wr", "w0", "w0,wr,br"}
    assert RR.wgrad_ws_bytes(8, 16) == 9 * 16 * 48 * 4 and [RR.wg_lds(1), RR.wg_lds(2)] == [32192, 48832]
    assert [RR.chain_blocks(16), RR.chain_blocks(32), RR.wfinish_grid(16), RR.wfinish_grid(32), RR.pack_grid(16), RR.pack_grid(32)] == [25, 68, 96, 192, 12, 24]
    assert [RR.dgrad_grid(2, 16, 64), RR.dgrad_grid(1, 48, 128), RR.dgrad_grid(1, 32, 192)] == [8, 8, 8] and RR.dgrad_grid(8, 1024, 1024) == RR.ceil8(8 * 74 * 32 // 4)
    # non-unit scales on at least half of the integer rows of every entry point
    for e in RR.ROWS:
        rows = [c for c in RR.CASES if c.entry == e and c.args["data"] != "real"]
        assert 2 * sum(bool(c.args["scaled"]) for c in rows) >= len(rows), (e, sum(bool(c.args["scaled"]) for c in rows), len(rows))
    assert RR.SCALED == (0.5, 0.25, 2.0)


def test_ws_bytes_and_ok_are_the_restated_rules(lib):
    """The two queries that launch nothing.  Without a device sgx_ncu answers 256, as NCU_NOMINAL."""
    if torch.cuda.is_available():
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
    else:
        ncu = RR.NCU_NOMINAL
    for B, H, W in ((2, 16, 64), (1, 32, 128), (5, 64, 512), (13, 64, 512), (32, 1024, 1024)):
        for C in (16, 32):
            assert lib.sgx_rgbconv_wgrad_ws_bytes(B, H, W, C) == RR.wgrad_ws_bytes(RR.wgrad_blocks(B, H, W, ncu), C), (B, H, W, C)
    assert lib.sgx_rgbconv_wgrad_ws_bytes(1, 16, 64, 24) == 0
    for B, H, W, C, dt in ((1, 16, 64, 16, 1), (1, 16, 64, 32, 1), (1, 8, 64, 16, 1), (1, 16, 32, 16, 1), (1, 24, 64, 16, 1), (1, 16, 96, 16, 1), (1, 16, 64, 24, 1), (1, 16, 64, 16, 0),
                           (0, 16, 64, 16, 1), (8, 1024, 1024, 16, 1)):
        assert lib.sgx_rgbconv_ok(B, H, W, C, dt) == int(RR.shape_ok(B, H, W, C, dt == 1)), (B, H, W, C, dt)


# ---------------------------------------------------------------------------------------------------------------- (c) references alone
def test_references_alone_have_what_the_gpu_rows_rely_on():
    shares = {}
    for c in RR.CASES:
        a = c.args
        if c.entry == "sgx_rgbconv_pack" and a["data"] != "real":
            RR.composed_of(a["C"], a["data"], a["scaled"], a["br"])          # asserts |W'|, |T| <= 2048 and exactness in both formats
        if c.entry == "sgx_rgbconv_fwd" and not a["special"]:
            if a["epi"] == 0:
                W4, _ = RR.composed_of(a["C"], "int", a["scaled"])
                _, S = RR.conv4(RR.with_ones(RR.image(a["B"], a["H"], a["W"], "int"), 0), W4)
                assert float(S.max()) * 8 < RR.EXACT, c.id
                if a["k"] == "tiles":
                    one = RR.one_scale_mask(RR.tile_exponents(a["H"], a["W"], "tiles"))
                    kmap = RR.tile_exponents(a["H"], a["W"], "tiles")
                    assert 0.5 < float(one.double().mean()) < 1.0 and len(kmap.unique()) == 6, c.id
                    d = [abs(float(kmap[y, x] - kmap[y2, x2])) for y, x, y2, x2 in ((0, 0, 0, 64), (0, 0, 16, 0), (0, 0, 16, 64), (16, 0, 0, 64))]
                    assert max(d) <= 12 and d == [6.0, 5.0, 11.0, 1.0]
                continue
            z, S = RR.forward_ref(a["B"], a["H"], a["W"], a["C"], a["data"], a["scaled"], a["ones"], a["b0"])      # asserts magnitudes, and pos > 0
            if a["data"] == "mix":
                shares[c.id] = float(RR.fwd_exact_mask(z).double().mean())
                assert 0.1 <= shares[c.id] <= 0.9, (c.id, shares[c.id])
            if a["data"] == "real":
                W4, S4 = RR.composed_of(a["C"], "real", False)
                dz = RR.operand_error(RR.with_ones(RR.image(a["B"], a["H"], a["W"], "real"), a["ones"]), W4, S4, a["C"], S)
                shares[c.id] = float((z.abs() <= dz).double().mean())
                assert shares[c.id] <= 0.02, (c.id, shares[c.id])
        if c.entry == "sgx_rgbconv_dgrad":
            assert float(RR.adjoint(RR.grad(a["B"], a["H"], a["W"], a["C"]), RR.composed_of(a["C"], "int", a["scaled"])[0]).abs().max()) * 8 < RR.EXACT
        if c.entry == "sgx_rgbconv_wgrad":
            a = RR.resolve(c).args
            d = RR.dwprime(RR.with_ones(RR.image(a["B"], a["H"], a["W"], "int"), a["ones"]), RR.grad(a["B"], a["H"], a["W"], a["C"]))
            assert float(d.abs().max()) * 2 * 2 * 9 * a["C"] < RR.EXACT, c.id
            if not a["ones"]:
                assert not bool(d[:, 3].any())
    print("shares (mix: outputs with an all-positive window; real: sign bits exempt): " + ", ".join(f"{k} {v:.4f}" for k, v in shares.items()))
    # the 8 x 1024^2 row and the two persistent rows draw the same kinds: their magnitudes are those of the rows above per pixel
    assert float(RR.params(16, "pos", True)["b0"].min()) == 1024 and float(RR.params(32, "mix", False)["b0"].max()) == 128


def test_references_are_the_derivatives_of_the_two_layers():
    """conv4 / adjoint / chain_rule against autograd through from_rgb (1x1) and conv0 (3x3, zero padding of from_rgb's OUTPUT) with the scales
    applied as EqualizedConv2d applies them, and against the unit-scale restatement tests/test_gpu_image_end.py holds the kernels to."""
    import test_gpu_image_end as TIE
    conv2d = torch.nn.functional.conv2d
    for C, data, scaled, ones in ((16, "int", True, 1), (32, "int", False, 1), (16, "real", False, 1), (16, "int", True, 0)):
        o = RR.params(C, data, scaled)
        B, H, W = 2, 16, 64
        img, gz = RR.image(B, H, W, data), RR.grad(B, H, W, C)
        P = {k: o[k].clone().requires_grad_(True) for k in ("w0", "b0", "wr", "br")}
        x = img.permute(0, 3, 1, 2).clone().requires_grad_(True)
        f = conv2d(x, (o["sr"] * P["wr"]).view(C, 3, 1, 1), o["bscale"] * P["br"] if ones else None)
        z = conv2d(f, o["s0"] * P["w0"], P["b0"] if ones else None, padding=1)
        grads = torch.autograd.grad((z * gz.permute(0, 3, 1, 2)).sum(), [x] + [P[k] for k in (("w0", "b0", "wr", "br") if ones else ("w0", "wr"))])
        W4, _ = RR.compose(o["w0"], o["wr"], o["br"] if ones else None, o["s0"], o["sr"], o["bscale"])
        z2, S = RR.conv4(RR.with_ones(img, ones), W4, o["b0"] if ones else None)
        tol = 0.0 if data != "real" else 1e-12
        assert float((z.detach().permute(0, 2, 3, 1) - z2).abs().max()) <= tol * float(S.max()) and bool((S >= z2.abs() - 1e-12).all())
        assert float((grads[0].permute(0, 2, 3, 1) - RR.adjoint(gz, W4)).abs().max()) <= tol * 1e3
        ch = RR.chain_rule(RR.dwprime(RR.with_ones(img, ones), gz), o["w0"], o["wr"], o["br"] if ones else None, o["s0"], o["sr"], o["bscale"])
        for k, g in zip(("w0", "b0", "wr", "br") if ones else ("w0", "wr"), grads[1:]):
            assert float((g - ch[k]).abs().max()) <= tol * 1e5, (C, data, k)
        if data == "int" and not scaled:
            p = TIE.int_params(C)
            assert all(torch.equal(p[k].reshape(o[k].shape), o[k]) for k in ("w0", "wr", "br"))
            assert torch.equal(TIE.composed(p), W4[:, :3])
            assert torch.equal(TIE.chain64(img.permute(0, 3, 1, 2), dict(p, b0=o["b0"]), True).permute(0, 2, 3, 1), z2)
    # the two pack layouts: k = kx * 4 + j and the flipped taps
    W4 = torch.arange(16 * 4 * 9, dtype=torch.float64).reshape(16, 4, 3, 3)
    wf, wd = RR.pack_wf(W4), RR.pack_wd(W4)
    assert wf[2, 5, 1 * 4 + 3] == W4[5, 3, 2, 1] and bool((wf[:, :, 12:] == 0).all()) and wf[0, 0, 0] == W4[0, 0, 0, 0]
    assert wd[0, 2 * 4 + 1, 7] == W4[7, 1, 2, 0] and bool((wd[:, 12:] == 0).all()) and bool((wd[:, 3::4] == 0).all())
    assert RR.dwp_layout(W4)[(5 * 3 + 2) * 16 + 1 * 4 + 3] == W4[5, 3, 2, 1]
    # blur and bits are streaming_ref's, whose own coverage test holds them to the oracle
    zz = RR.ints((1, 4, 4, 8), 1, -3, 3)
    assert torch.equal(SR.unpack_bits(SR.pack_bits(zz > 0), 8), zz > 0)


# ---------------------------------------------------------------------------------------------------------------- rejections
FAKE = 0x10000                                               # a device pointer that is never followed


def reject(L, id):
    P, st, BIG = FAKE, None, 1 << 30
    fwd = lambda img=P, y=P, H=16, W=64, C=16, dt=1, epi=1, ones=1: L.sgx_rgbconv_fwd(img, P, P, y, P, 1, H, W, C, epi, ones, dt, st)
    dg = lambda gi=P, H=16, W=64, C=16, dt=1: L.sgx_rgbconv_dgrad(P, P, gi, 1, H, W, C, dt, st)
    wg = lambda wr=P, ws=P, wsb=BIG, H=16, W=64, C=16, dt=1, ones=1, db0=P: L.sgx_rgbconv_wgrad(P, P, ones, P, 1.0, wr, 1.0, P, 1.0, P, db0, P, None if not ones else P, 0, ws, wsb, 1, H, W,
                                                                                              C, dt, st)
    calls = {
        "pack-w0-null": lambda: L.sgx_rgbconv_pack(None, 1.0, P, 1.0, P, 1.0, P, P, 16, st),
        "pack-wd-null": lambda: L.sgx_rgbconv_pack(P, 1.0, P, 1.0, P, 1.0, P, None, 16, st),
        "pack-C24": lambda: L.sgx_rgbconv_pack(P, 1.0, P, 1.0, P, 1.0, P, P, 24, st),
        "fwd-img-null": lambda: fwd(img=None), "fwd-y-null": lambda: fwd(y=None), "fwd-H8": lambda: fwd(H=8), "fwd-W32": lambda: fwd(W=32), "fwd-C24": lambda: fwd(C=24),
        "fwd-fp32": lambda: fwd(dt=0), "fwd-epi2": lambda: fwd(epi=2), "fwd-epi0-ones": lambda: fwd(epi=0, ones=1),
        "dgrad-gi-null": lambda: dg(gi=None), "dgrad-H8": lambda: dg(H=8), "dgrad-W32": lambda: dg(W=32), "dgrad-C24": lambda: dg(C=24), "dgrad-fp32": lambda: dg(dt=0),
        "wgrad-ws-null": lambda: wg(ws=None), "wgrad-wr-null": lambda: wg(wr=None), "wgrad-H8": lambda: wg(H=8), "wgrad-W32": lambda: wg(W=32), "wgrad-C24": lambda: wg(C=24),
        "wgrad-fp32": lambda: wg(dt=0), "wgrad-noones-db0": lambda: wg(ones=0, db0=P),
        "wgrad-ws-short": lambda: wg(wsb=L.sgx_rgbconv_wgrad_ws_bytes(1, 16, 64, 16) - 4),
        "tune-variant3": lambda: L.sgx_rgbconv_tune(3, 0, 0), "tune-nit9": lambda: L.sgx_rgbconv_tune(0, 9, 0), "tune-dbg1": lambda: L.sgx_rgbconv_tune(0, 0, 1),
    }
    return calls[id]()


@pytest.mark.parametrize("id,entry,code,words,why", RR.REJECTIONS, ids=[r[0] for r in RR.REJECTIONS])
def test_contract_rejections_return_before_any_launch(lib, id, entry, code, words, why):
    lib.sgx_clear_error()
    try:
        rc = reject(lib, id)
        msg = lib.sgx_last_error().decode(errors="replace")
    finally:
        lib.sgx_clear_error()
        assert lib.sgx_rgbconv_tune(-1, 0, 0) == 0           # (a rejected sgx_rgbconv_tune leaves the state alone; this is the default)
    assert rc == code and words in msg, (id, rc, msg, why)


def test_rejection_table_covers_every_entry_point():
    per = collections.Counter(r[1] for r in RR.REJECTIONS)
    assert per == {"sgx_rgbconv_pack": 3, "sgx_rgbconv_fwd": 8, "sgx_rgbconv_dgrad": 5, "sgx_rgbconv_wgrad": 8, "sgx_rgbconv_tune": 3}, per


# ---------------------------------------------------------------------------------------------------------------- (d) the criteria on emulations
def pair_sums(a, axis):
    """The [1, 2, 1] taps as the kernel adds them, zero beyond the ends: (a[i - 1] + a[i]) + (a[i] + a[i + 1]) in fp32."""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (1, 1)
    ap = np.pad(a, pad)
    n = a.shape[axis]
    t = np.take(ap, range(1, n + 2), axis) + np.take(ap, range(0, n + 1), axis)
    return np.take(t, range(0, n), axis) + np.take(t, range(1, n + 1), axis)


def emu_fwdblur(img, W4, b0, ones, geom=None, halo_ones=False, img_bf16=False, zero_carry=False, drop_last_block=False):
    """rgbconv_fwdblur_kernel in numpy fp32: fp16 operands (image, W', T; the bias channel 1 inside the image), the accumulator started at b0
    and the 36 products added one at a time (one admissible order of the MFMAs' sums), max(x / 16, x (0.2f / 16)), the pair sums along the
    row and down the column, one bf16 rounding; the sign byte of a row is that of its activation.  img fp64 [B][H][W][3] -> (y bf16, bits).
    The planted errors: halo_ones -- the bias channel is 1 outside the image too; img_bf16 -- the image rounded to bf16; zero_carry -- the
    first stored row of every row block but the first takes its sign byte from the zero-initialised carry; drop_last_block -- the rows of a
    ragged last row block are not stored (the Guarded prefill stays)."""
    B, H, W, _ = img.shape
    C = W4.shape[0]
    x = (img.float().bfloat16() if img_bf16 else img.float().half()).float().numpy()
    w = W4.to(F16).float().numpy()
    x4 = np.zeros((B, H + 2, W + 2, 4), f4)
    x4[:, 1:-1, 1:-1, :3] = x
    x4[:, 1:-1, 1:-1, 3] = f4(ones)
    if halo_ones:
        x4[..., 3] = f4(ones)
    acc = np.zeros((B, H, W, C), f4) + (0 if b0 is None else b0.float().numpy())
    for ky in range(3):
        for kx in range(3):
            for j in range(4):
                acc = acc + x4[:, ky:ky + H, kx:kx + W, j:j + 1] * w[:, j, ky, kx]
    a = np.maximum(acc * f4(0.0625), acc * (f4(0.2) * f4(0.0625)))
    o = pair_sums(pair_sums(a, 2), 1)
    y = torch.from_numpy(o).bfloat16()
    bits = SR.pack_bits(torch.from_numpy(a > 0))
    if geom is not None and zero_carry:
        for k in range(1, geom.nrb):
            bits[:, k * geom.rb] = 0
    if geom is not None and drop_last_block and geom.last < geom.rb:
        y.view(torch.int16)[:, (geom.nrb - 1) * geom.rb:] = -1              # 0xFFFF: the prefill
    return y, bits


def emu_pack(o, C, with_br=True, s0_only=False):
    """rgbconv_pack_kernel in numpy fp32: the sum over i in order, then one multiply by s0 * sr (j < 3) or s0 (the bias channel).  The planted
    error: s0 in place of s0 * sr.  -> W4 in fp32 (the kernel rounds it to fp16 for wf and to bf16 for wd)."""
    w0, wr, br = o["w0"].float().numpy(), o["wr"].float().numpy(), o["br"].float().numpy() * f4(o["bscale"])
    W4 = np.zeros((C, 4, 3, 3), f4)
    for j in range(4):
        if j == 3 and not with_br:
            continue
        v = np.zeros((C, 3, 3), f4)
        for i in range(C):
            v = v + w0[:, i] * (wr[i, j] if j < 3 else br[i])
        W4[:, j] = v * (f4(o["s0"]) * (f4(o["sr"]) if (j < 3 and not s0_only) else f4(1.0)))
    return torch.from_numpy(W4)


def tile_partials(x4, gz, nblk):
    """rgbconv_wgrad_kernel's workspace: per 8 x 64 tile the exact dW', added per block as rc_sched walks the tiles -> [nblk][C * 48] fp32."""
    B, H, W, C = gz.shape
    xp = torch.nn.functional.pad(x4, (0, 0, 1, 1, 1, 1))
    tx_n, ty_n = W // 64, H // 8
    part = torch.zeros(nblk, C * 48, dtype=torch.float64)
    for blk in range(nblk):
        for t in RR.rc_sched(blk, nblk, B * tx_n * ty_n):
            tx, ty, b = t % tx_n, t // tx_n % ty_n, t // tx_n // ty_n
            g = gz[b, ty * 8:ty * 8 + 8, tx * 64:tx * 64 + 64].reshape(-1, C)
            d = torch.zeros(C, 4, 3, 3, dtype=torch.float64)
            for ky in range(3):
                for kx in range(3):
                    d[:, :, ky, kx] = g.t() @ xp[b, ty * 8 + ky:ty * 8 + ky + 8, tx * 64 + kx:tx * 64 + kx + 64].reshape(-1, 4)
            part[blk] += RR.dwp_layout(d)
    return part.float()


def emu_wfinish(part, first_trip_only=False):
    """rgbconv_wfinish_kernel in numpy fp32: slice sl of 32 adds its terms k = sl, sl + 32, ... in order, eight of them per trip of the loop
    k0 += 256; the 32 slices are added in order.  The planted error: the loop runs one trip."""
    p = part.numpy()
    nblk = p.shape[0]
    s = np.zeros((32, p.shape[1]), f4)
    for sl in range(32):
        for k in range(sl, min(nblk, 256) if first_trip_only else nblk, 32):
            s[sl] = s[sl] + p[k]
    out = np.zeros(p.shape[1], f4)
    for sl in range(32):
        out = out + s[sl]
    return torch.from_numpy(out)


def _old(name, passes, how):
    print(f"planted {name}: the older check ({how}) {'passes it' if passes else 'fails it'}")
    return bool(passes)


def old_forward_checks(y, bits, z, xb):
    """What tests/test_gpu_rgbconv.py asks of the forward: rel-L2 <= 6e-3 of the tensor, every sign bit with |z| above 2 % of the mean right,
    fewer than 2 % of all bits wrong."""
    gb = SR.unpack_bits(bits, z.shape[-1])
    sure = z.abs() > 2e-2 * z.abs().mean()
    rel = gpu_util.rel_err(y.float().nan_to_num(0.0), xb)
    return rel, bool(rel <= 6e-3 and bool((gb[sure] == (z > 0)[sure]).all()) and float((gb != (z > 0)).double().mean()) < 2e-2)


def test_criteria_pass_the_emulations_and_fail_the_six_planted_errors():
    """The honest fp32 emulation meets each criterion; each planted error fails it with the element in the message.  What the older checks make
    of the same tensors is printed and pinned: the record of what the gap was."""
    old = {}
    # ---- the forward on integers: (1, 48, 128, C16), mix, the heuristic's three row blocks of 16 and nit 8 (46 + 2 rows)
    B, H, W, C = RR.SB
    o, img = RR.params(C, "mix", False), RR.image(B, H, W, "mix")
    W4, _ = RR.composed_of(C, "mix", False)
    z, _ = RR.forward_ref(B, H, W, C, "mix", False)
    y, bits = emu_fwdblur(img, W4, o["b0"], 1)
    r = RR.check_fwd_int(y, bits, z, 0, "emulation")
    assert 0.0 < r <= 1.0, r
    print(f"emulated fwdblur, mix: worst err/bound of the elements with a negative pre-activation in the window {r:.3f}")
    xb = RR.blur(RR.lrelu(z))
    assert old_forward_checks(y, bits, z, xb)[1]
    # (1) from_rgb's bias channel 1 in the halo: T applied through taps outside the image
    yb, bb = emu_fwdblur(img, W4, o["b0"], 1, halo_ones=True)
    with pytest.raises(AssertionError, match=r"elements differ from the exact value's bf16; first at flat index \d+ \(0, 0, 0, \d+\)"):
        RR.check_fwd_int(yb, bb, z, 0, "bias channel set in the halo")
    zs, _ = RR.forward_ref(*RR.SA, "pos", True)
    ys, bs = emu_fwdblur(RR.image(*RR.SA[:3], "pos"), RR.composed_of(16, "pos", True)[0], RR.params(16, "pos", True)["b0"], 1, halo_ones=True)
    with pytest.raises(AssertionError, match=r"first at flat index \d+ \(0, 0, 0, \d+\)"):
        RR.check_fwd_int(ys, bs, zs, 0, "bias channel set in the halo, pos row")
    # (3) the first stored row of a second row block with the sign byte of the zero-initialised carry
    g3 = RR.fwdblur_geom(B, H, W)
    yc, bc = emu_fwdblur(img, W4, o["b0"], 1, geom=g3, zero_carry=True)
    with pytest.raises(AssertionError, match=r"sign bits differ from z > 0; first at \(b, y, x, channel\) = \(0, 16, 0, \d+\)"):
        RR.check_fwd_int(yc, bc, z, 0, "sign byte from the zeroed carry")
    old["carry"] = _old("sign byte of a row block's first row from the zeroed carry", old_forward_checks(yc, bc, z, xb)[1], "every sure bit right, < 2 % wrong")
    # (4) the ragged last row block (2 rows at nit 8) not stored
    g8 = RR.fwdblur_geom(B, H, W, 8)
    yd, bd = emu_fwdblur(img, W4, o["b0"], 1, geom=g8, drop_last_block=True)
    with pytest.raises(AssertionError, match=r"first at flat index \d+ \(0, 46, 0, 0\)"):
        RR.check_fwd_int(yd, bd, z, 0, "last row block not stored")
    rel, ok = old_forward_checks(yd, bd, z, xb)
    old["ragged"] = _old(f"ragged last row block not stored (rel-L2 {rel:.2e} with the missing rows read as 0)", ok, "equal bits across nit 6 / 4 / 1 and rel-L2 6e-3, at "
                         "heights 16, 32, 48, 160 whose row blocks of 16, 34, 22 and 4 rows are ragged at H = 48 and 160")
    # ---- the forward on randn: (2, 16, 64, C16)
    B, H, W, C = RR.SA
    o, img = RR.params(C, "real", False), RR.image(B, H, W, "real")
    W4, S4 = RR.composed_of(C, "real", False)
    z, S = RR.forward_ref(B, H, W, C, "real", False)
    dz = RR.operand_error(RR.with_ones(img, 1), W4, S4, C, S)
    y, bits = emu_fwdblur(img, W4, o["b0"], 1)
    r = RR.check_fwd_real(y, bits, z, dz, 0, "emulation, randn")
    assert 0.0 < r <= 1.0, r
    print(f"emulated fwdblur, randn: worst err/bound {r:.3f}")
    xb = RR.blur(RR.lrelu(z))
    assert old_forward_checks(y, bits, z, xb)[1]
    yb, bb = emu_fwdblur(img, W4, o["b0"], 1, halo_ones=True)
    with pytest.raises(AssertionError, match=r"values outside the bound; first at \(0, 0, 0, \d+\)"):
        RR.check_fwd_real(yb, bb, z, dz, 0, "bias channel set in the halo, randn")
    rel, ok = old_forward_checks(yb, bb, z, xb)
    old["halo"] = _old(f"bias channel set in the halo (rel-L2 {rel:.2e} at 16 x 64)", ok, "rel-L2 6e-3, 2 % of bits")
    # (2) the image rounded to bf16 instead of fp16
    y2, b2 = emu_fwdblur(img, W4, o["b0"], 1, img_bf16=True)
    rel, ok = old_forward_checks(y2, b2, z, xb)
    old["bf16-image"] = _old(f"image rounded to bf16 (rel-L2 {rel:.2e})", ok, "rel-L2 6e-3, 2 % of bits")
    r2 = RR.check_fwd_real(y2, b2, z, dz, 0, "image rounded to bf16")          # the worst-case operand bound cannot see it ...
    wfq = RR.pack_wf(W4).to(F16).double()
    rq, exempt = RR.check_fwd_operands(y, bits, img, wfq, o["b0"], 1, 0, "emulation, randn")
    assert 0.0 < rq <= 1.0 and exempt < 1e-4, (rq, exempt)
    print(f"emulated fwdblur, randn, against its own operands: worst err/bound {rq:.3f}, {exempt:.1e} of the sign bits exempt; with the bf16 image the operand bound is used to {r2:.3f}")
    with pytest.raises(AssertionError, match=r"\(own operands\): \d+ (of \d+ values outside the bound; first at \(\d+, \d+, \d+, \d+\)|sign bits differ from z > 0; first at \(b, y, x, channel\) = \(\d+, \d+, \d+, \d+\))"):
        RR.check_fwd_operands(y2, b2, img, wfq, o["b0"], 1, 0, "image rounded to bf16")          # ... the kernel's own operands do
    # ---- (5) the pack with s0 in place of s0 * sr for j < 3, on the scaled integers and on randn
    for C in (16, 32):
        o = RR.params(C, "int", True)
        W4, _ = RR.composed_of(C, "int", True)
        assert torch.equal(emu_pack(o, C).double(), W4)
        bad = RR.pack_wd(emu_pack(o, C, s0_only=True).double())
        with pytest.raises(AssertionError, match=r"elements differ from the exact value's bf16; first at flat index \d+ \(0, 0, \d+\)"):
            RR.assert_bf16_bits(bad.bfloat16(), RR.pack_wd(W4), "s0 in place of s0 sr")
    o = RR.params(16, "real", False)
    W4, S4 = RR.compose(o["w0"], o["wr"], o["br"], o["s0"], o["sr"], o["bscale"])
    rf, good, bad = RR.pack_wf(W4), RR.pack_wf(emu_pack(o, 16).double()).to(F16), RR.pack_wf(emu_pack(o, 16, s0_only=True).double()).to(F16)
    bound = RR.pack_bound(rf, RR.pack_wf(S4), 16, RR.R_F16, RR.TINY_F16)
    r = RR.ER.assert_within(good, rf, bound, "emulated pack")
    assert 0.0 < r <= 1.0, r
    print(f"emulated pack, randn: worst err/bound {r:.3f}")
    with pytest.raises(AssertionError, match=r"values outside the bound; first at \(0, 0, 0\)"):
        RR.ER.assert_within(bad, rf, bound, "s0 in place of s0 sr")
    unit = RR.params(16, "int", False)
    old["pack-scale"] = _old("s0 in place of s0 sr in the pack", torch.equal(emu_pack(unit, 16), emu_pack(unit, 16, s0_only=True)), "exact integers with every scale 1.0")
    # ---- (6) wfinish dropping the terms k >= 256: (5, 64, 512, C16), 320 blocks
    B, H, W, C = 5, 64, 512, 16
    x4, gz = RR.with_ones(RR.image(B, H, W, "int"), 1), RR.grad(B, H, W, C)
    used = RR.DWP_USED.repeat(C)
    want = RR.dwp_layout(RR.dwprime(x4, gz))
    part = tile_partials(x4, gz, 320)
    assert RR.assert_bits(emu_wfinish(part)[used], want[used], "emulated wfinish") == 0.0
    with pytest.raises(AssertionError, match=r"elements differ from the exact value; first at flat index 0 "):
        RR.assert_bits(emu_wfinish(part, first_trip_only=True)[used], want[used], "wfinish without its second trip")
    p8 = tile_partials(RR.with_ones(RR.image(2, 16, 64, "int"), 1), RR.grad(2, 16, 64, 16), 8)
    old["wfinish-tail"] = _old("wfinish dropping the terms k >= 256", torch.equal(emu_wfinish(p8), emu_wfinish(p8, first_trip_only=True)), "exact integers on 8 blocks; rel-L2 8e-3 on "
                               "at most 5 x 8 x 4 = 160 blocks")
    # ---- an unwritten element (the Guarded prefill) fails each kind of check
    nan = torch.full((1, 1, 1, 8), float("nan")).bfloat16()
    one = torch.ones(1, 1, 1, 8, dtype=torch.float64)
    with pytest.raises(AssertionError, match="8 of 8 elements differ"):
        RR.assert_bf16_bits(nan, one, "sentinel")
    with pytest.raises(AssertionError, match="8 of 8 values outside"):
        RR.ER.assert_within(nan, one, 1e30 * one, "sentinel")
    assert old == {"carry": False, "ragged": False, "halo": False, "bf16-image": True, "pack-scale": True, "wfinish-tail": True}, old
