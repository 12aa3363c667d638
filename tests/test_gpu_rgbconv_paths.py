"""-m gpu: every launch path of the discriminator's composed first layer (csrc/rgbconv.hip) at the C ABI, one test per row of
rgbconv_ref.CASES.  tests/test_gpu_rgbconv.py and tests/test_gpu_image_end.py hold the same kernels by rel-L2 per tensor and by exact
integers at unit scales; this file holds them per element.

Each row is one call through native.lib() under the library's profiler (epilogue_runner.profiled): the return code is 0, the kernels that
ran and their grids, blocks and dynamic LDS sizes are what rgbconv_ref.plan restates from the row's arguments (the persistent grid of
rgbconv_fwd_kernel, sized by an occupancy query, by its properties) and, every one by value, what sgx_rgbconv_plan reported for the call
(tests/test_rgbconv_plan.py holds the query to the restated rules without a device), every output -- the two packs, y, the sign bits, gi, the four parameter
gradients and the whole wgrad workspace -- is a streaming_ref.Guarded view pre-filled with NaN bytes whose bands come back untouched, and
the values meet rgbconv_ref's criteria: bit for bit on the integer rows, the per-element bounds against the fp64 restatement otherwise.
sgx_rgbconv_tune's state is process-wide: every test leaves (-1, 0, 0) behind (the autouse fixture), whatever it raised."""
import json
import os

import pytest
import torch

import epilogue_ref as ER
import epilogue_runner as ERUN
import rgbconv_ref as RR
import streaming_ref as SR
import test_rgbconv_plan as TRP
from epilogue_runner import DEV, native, p

pytestmark = pytest.mark.gpu
F32, BF16, F16, U8 = torch.float32, torch.bfloat16, torch.float16, torch.uint8
NAMES = ("w0", "b0", "wr", "br")
WORST = {}                          # entry point -> {output: (worst err / bound, row)}: printed per row, kept by a measuring run (SGX_RGBCONV_REPORT)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()
    rep = os.environ.get("SGX_RGBCONV_REPORT")
    if rep:
        with open(rep, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


@pytest.fixture(autouse=True)
def _tune_restored():
    yield
    N = native()
    N.check(N.lib().sgx_rgbconv_tune(-1, 0, 0), "sgx_rgbconv_tune")


def note(c, what, ratio):
    w = WORST.setdefault(c.entry, {})
    if ratio >= w.get(what, (-1.0, ""))[0]:
        w[what] = (ratio, c.id)
    print(f"{c.id} {what}: err/bound {ratio:.3f}")


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev(t, dtype=F32):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def G(shape, dtype=F32):
    return SR.Guarded(shape, dtype, DEV)


def launch(c, call, B=None):
    """The call under the profiler: rc 0 (profiled checks it), the row's kernels in order, the restated geometry, and kernels and geometry
    as the library's own query reports them under the tune state of the call (B: the batch size where the row leaves it to the device)
    -> the grids."""
    a = c.args
    q = TRP.lib_plan(native().lib(), TRP.ENTRY[c.entry], B or a.get("B") or 0, a.get("H") or 0, a.get("W") or 0, a["C"], a.get("epi", 0))
    ran = ERUN.profiled(c.id, c.entry, call)
    kernels, launches = RR.plan(c, ncu())
    assert tuple(ran) == tuple(c.kernels) == tuple(kernels), f"{c.id}: launched {ran}, the row says {c.kernels}, the rules {kernels} ({c.why})"
    got = [(tuple(g), tuple(b), int(lds)) for g, b, lds in native().prof_launches()]
    assert len(got) == len(launches), (c.id, got)
    for (g, b, lds), (wg, wb, wl) in zip(got, launches):
        assert (b, lds) == (wb, wl) and g[1:] == (1, 1) and (wg is None or g == wg), f"{c.id}: launch geometry {got}, restated {launches}"
    assert (tuple(ran), got) == TRP.launches_of(q), f"{c.id}: launched {ran} as {got}, sgx_rgbconv_plan reported {q}"
    return [g[0] for g, _, _ in got]


def packs(L, N, C, data, scaled, with_br=True):
    """The two operand packs of a row, made by the library (held by the pack rows) -> (wf, wd) Guarded."""
    o = RR.params(C, data, scaled)
    wf, wd = G((3, C, 16), BF16), G((3, 16, C), BF16)
    w0, wr, br = dev(o["w0"]), dev(o["wr"]), dev(o["br"]) if with_br else None
    with ERUN.sticky("sgx_rgbconv_pack"):
        N.check(L.sgx_rgbconv_pack(p(w0), o["s0"], p(wr), o["sr"], p(br), o["bscale"], p(wf.t), p(wd.t), C, N.stream()), "sgx_rgbconv_pack")
        torch.cuda.synchronize()
    return wf, wd


# ---------------------------------------------------------------------------------------------------------------- pack
def run_pack(L, N, c):
    a = c.args
    C = a["C"]
    o = RR.params(C, a["data"], a["scaled"])
    wf, wd = G((3, C, 16), BF16), G((3, 16, C), BF16)
    w0, wr, br = dev(o["w0"]), dev(o["wr"]), dev(o["br"]) if a["br"] else None
    launch(c, lambda: L.sgx_rgbconv_pack(p(w0), o["s0"], p(wr), o["sr"], p(br), o["bscale"], p(wf.t), p(wd.t), C, N.stream()))
    wf.assert_intact(f"{c.id} wf"); wd.assert_intact(f"{c.id} wd")
    W4, S4 = RR.compose(w0.double().cpu(), wr.double().cpu(), None if br is None else br.double().cpu(), o["s0"], o["sr"], o["bscale"])
    rf, rd, gf, gd = RR.pack_wf(W4), RR.pack_wd(W4), wf.t.cpu().view(F16), wd.t.cpu()
    zf, zd = RR.pack_wf(torch.ones_like(W4)) == 0, RR.pack_wd(torch.ones_like(W4)) == 0       # the slots that hold no weight
    if br is None:
        zf = zf | (RR.pack_wf(torch.cat([torch.zeros_like(W4[:, :3]), torch.ones_like(W4[:, 3:])], 1)) != 0)
    assert bool((gf.view(torch.int16)[zf] == 0).all()) and bool((gd.view(torch.int16)[zd] == 0).all()), f"{c.id}: a padding or bias slot is not +0"
    if a["data"] == "int":
        ne = gf.view(torch.int16) != rf.to(F16).view(torch.int16)
        assert not bool(ne.any()), f"{c.id} wf: {int(ne.sum())} of {ne.numel()} fp16 values differ from the exact ones; first at [ky][o][k] = {tuple(int(v) for v in ne.nonzero()[0])}"
        RR.assert_bf16_bits(gd, rd, f"{c.id} wd")
        note(c, "wf", 0.0); note(c, "wd", 0.0)
    else:
        note(c, "wf", ER.assert_within(gf, rf, RR.pack_bound(rf, RR.pack_wf(S4), C, RR.R_F16, RR.TINY_F16), f"{c.id} wf"))
        note(c, "wd", ER.assert_within(gd, rd, RR.pack_bound(rd, RR.pack_wd(S4), C, SR.R_BF16, 0.0), f"{c.id} wd"))


# ---------------------------------------------------------------------------------------------------------------- forward
def fwd_call(L, N, img, wf, b0, y, bits, a, B):
    return lambda: L.sgx_rgbconv_fwd(p(img), p(wf.t), p(b0), p(y.t), p(bits.t) if bits is not None else None, B, a["H"], a["W"], a["C"], a["epi"], a["ones"], N.BF16, N.stream())


def run_fwd(L, N, c):
    a = c.args
    if a["special"] == "big":
        return run_fwd_big(L, N, c)
    if a["special"] == "persistent":
        return run_fwd_persistent(L, N, c)
    B, H, W, C, epi, v = a["B"], a["H"], a["W"], a["C"], a["epi"], a["variant"]
    o = RR.params(C, a["data"], a["scaled"])
    wf, _ = packs(L, N, C, a["data"], a["scaled"])
    img64 = RR.image(B, H, W, a["data"])
    kmap = None
    if epi == 0:
        kmap = RR.tile_exponents(H, W, 0 if a["k"] == "zero" else a["k"])
        img64 = img64 * (0.0 if a["k"] == "zero" else torch.exp2(kmap).view(1, H, W, 1))
        assert torch.equal(img64.float().double(), img64)
    img, b0 = dev(img64), dev(o["b0"]) if a["b0"] else None
    y, bits = G((B, H, W, C), BF16), G((B, H, W, C // 8), U8) if (a["bits"] and epi) else None
    N.check(L.sgx_rgbconv_tune(v, a["nit"], 0), "sgx_rgbconv_tune")
    grids = launch(c, fwd_call(L, N, img, wf, b0, y, bits, a, B))
    y.assert_intact(f"{c.id} y")
    if bits is not None:
        bits.assert_intact(f"{c.id} bits")
    if RR.plan(c)[1][0][0] is None:
        RR.check_rc_grid(grids[0], RR.fwd_ntiles(B, H, W, C // 16, epi), ncu())
    gy, gb = y.t.cpu(), None if bits is None else bits.t.cpu()
    if epi == 0:
        W4, _ = RR.composed_of(C, a["data"], a["scaled"])
        ref, S = RR.conv4(RR.with_ones(img64, 0), W4)
        if a["k"] == "zero":
            assert bool((gy.view(torch.int16) == 0).all()), f"{c.id}: {int((gy.view(torch.int16) != 0).sum())} outputs of an all-zero image are not +0"
            return note(c, "y epi 0", 0.0)
        one = RR.one_scale_mask(kmap).view(1, H, W, 1).expand(B, H, W, C)
        RR.assert_bf16_bits(gy, ref, f"{c.id} y (windows in one tile's scale)", one)
        return note(c, "y epi 0", 0.0 if bool(one.all()) else SR.assert_elementwise(gy, ref, S, RR.N_CONV, BF16, f"{c.id} y"))
    z, S = RR.forward_ref(B, H, W, C, a["data"], a["scaled"], a["ones"], a["b0"])
    what = f"y variant {min(v, 1)} {'real' if a['data'] == 'real' else 'int'}"
    if a["data"] == "real":
        W4, S4 = RR.composed_of(C, "real", False)
        dz = RR.operand_error(RR.with_ones(img64, a["ones"]), W4, S4, C, S)
        note(c, what, RR.check_fwd_real(gy, gb, z, dz, v, c.id))
        rq, exempt = RR.check_fwd_operands(gy, gb, img64, wf.t.cpu().view(F16).double(), o["b0"] if a["b0"] else None, a["ones"], v, c.id)
        assert exempt < 1e-3, (c.id, exempt)
        return note(c, what + ", own operands", rq)
    note(c, what, RR.check_fwd_int(gy, gb, z, v, c.id))


def run_fwd_big(L, N, c):
    """8 x 1024^2 on integers made on the device, no CPU reference: the grid shows the heuristic's nit 5, and the overrides 3 and 6 -- row
    blocks of 16 and 34 rows against 28 -- give the same bits."""
    a = c.args
    B, H, W, C = a["B"], a["H"], a["W"], a["C"]
    o = RR.params(C, a["data"], a["scaled"])
    wf, _ = packs(L, N, C, a["data"], a["scaled"])
    g = torch.Generator(device=DEV).manual_seed(41)
    img = torch.randint(-3, 4, (B, H, W, 3), generator=g, device=DEV).float()
    b0 = dev(o["b0"])
    geo = RR.fwdblur_geom(B, H, W)
    assert geo.nit == 5 and len({RR.fwdblur_geom(B, H, W, n).grid for n in (4, 5, 6)}) == 3
    outs = []
    for nit in (0, 3, 6):
        y, bits = G((B, H, W, C), BF16), G((B, H, W, C // 8), U8)
        N.check(L.sgx_rgbconv_tune(-1, nit, 0), "sgx_rgbconv_tune")
        grids = launch(c._replace(args=dict(a, nit=nit)), fwd_call(L, N, img, wf, b0, y, bits, a, B))
        assert grids[0] == RR.fwdblur_geom(B, H, W, nit or 5).grid
        y.assert_intact(f"{c.id} y nit {nit}"); bits.assert_intact(f"{c.id} bits nit {nit}")
        outs.append((y, bits))
    for (y, bits), nit in zip(outs[1:], (3, 6)):
        assert torch.equal(y.t.view(torch.int16), outs[0][0].t.view(torch.int16)), f"{c.id}: y differs between the heuristic's row blocks and nit {nit}"
        assert torch.equal(bits.t, outs[0][1].t), f"{c.id}: the sign bits differ between the heuristic's row blocks and nit {nit}"
    assert not bool(outs[0][0].t.isnan().any())


def run_fwd_persistent(L, N, c):
    """More tiles than blocks.  A first launch with at least 4 tiles per CU shows the full persistent grid; the batch size of the row is the
    smallest with 1.1 times as many tiles, and rc_sched then gives some blocks two tiles and some one.  Integer data, the fp64 reference on
    the device one image at a time, every output bit for bit."""
    a = c.args
    H, W, C, epi = a["H"], a["W"], a["C"], a["epi"]
    o = RR.params(C, a["data"], a["scaled"])
    wf, _ = packs(L, N, C, a["data"], a["scaled"])
    per_image = RR.fwd_ntiles(1, H, W, C // 16, epi)
    B0 = RR.cdiv(4 * ncu(), per_image)
    N.check(L.sgx_rgbconv_tune(a["variant"], 0, 0), "sgx_rgbconv_tune")
    b0 = dev(o["b0"]) if epi else None
    probe, y0 = dev(RR.image(B0, H, W, "int")), G((B0, H, W, C), BF16)
    full = launch(c, fwd_call(L, N, probe, wf, b0, y0, None, a, B0), B0)[0]
    RR.check_rc_grid(full, B0 * per_image, ncu())
    del y0, probe
    B = RR.persistent_batch(full, per_image)
    ntiles = B * per_image
    assert 1.1 * full <= ntiles <= 1.5 * full, (full, ntiles)
    img64 = RR.image(B, H, W, "int")
    img = dev(img64)
    y, bits = G((B, H, W, C), BF16), G((B, H, W, C // 8), U8) if epi else None
    grid = launch(c, fwd_call(L, N, img, wf, b0, y, bits, a, B), B)[0]
    counts = RR.sched_counts(grid, ntiles)
    assert grid == full < ntiles and 1 in counts and 2 in counts, (grid, full, ntiles, sorted(set(counts)))
    y.assert_intact(f"{c.id} y")
    W4 = RR.composed_of(C, a["data"], a["scaled"])[0].to(DEV)
    for b in range(B):
        x4 = RR.with_ones(img[b:b + 1].double(), a["ones"])
        z, S = RR.conv4(x4, W4, o["b0"].to(DEV) if epi else None)
        assert float(S.max()) * 8 < RR.EXACT
        if epi:
            assert float(z.min()) > 0
            RR.assert_bf16_bits(y.t[b:b + 1], RR.blur(RR.tile_act(z)), f"{c.id} y image {b}")
            RR.assert_sign_bits(bits.t[b:b + 1], z, f"{c.id} image {b}")
        else:
            RR.assert_bf16_bits(y.t[b:b + 1], z, f"{c.id} y image {b}")
    if bits is not None:
        bits.assert_intact(f"{c.id} bits")
    note(c, f"y persistent epi {epi}", 0.0)


# ---------------------------------------------------------------------------------------------------------------- image gradient
def run_dgrad(L, N, c):
    a = c.args
    B, H, W, C = a["B"], a["H"], a["W"], a["C"]
    _, wd = packs(L, N, C, a["data"], a["scaled"])
    gz64 = RR.grad(B, H, W, C)
    gz, gi = dev(gz64, BF16), G((B, H, W, 3))
    launch(c, lambda: L.sgx_rgbconv_dgrad(p(gz), p(wd.t), p(gi.t), B, H, W, C, N.BF16, N.stream()))
    gi.assert_intact(f"{c.id} gi")
    ref = RR.adjoint(gz64, RR.composed_of(C, a["data"], a["scaled"])[0])
    assert float(ref.abs().max()) * 8 < RR.EXACT
    note(c, "gi", RR.assert_bits(gi.t, ref, f"{c.id} gi"))


# ---------------------------------------------------------------------------------------------------------------- parameter gradients
def run_wgrad(L, N, c):
    c = RR.resolve(c, ncu())
    a = c.args
    B, H, W, C, acc, ones = a["B"], a["H"], a["W"], a["C"], a["acc"], a["ones"]
    o = RR.params(C, "int", a["scaled"])
    img64, gz64 = RR.image(B, H, W, "int"), RR.grad(B, H, W, C)
    img, gz = dev(img64), dev(gz64, BF16)
    w0, wr, br = dev(o["w0"]), dev(o["wr"]), dev(o["br"]) if a["br"] else None
    given = a["outs"].split(",")
    shapes = {"w0": (C, C, 3, 3), "b0": (C,), "wr": (C, 3), "br": (C,)}
    pre = {k: RR.ints(shapes[k], 50 + i, -5, 5) for i, k in enumerate(NAMES)}
    outs = {k: G(shapes[k]) for k in given}
    for i, k in enumerate(NAMES):
        if k in outs and acc >> i & 1:
            outs[k].t.copy_(pre[k].float())
    nblk, nout = RR.wgrad_blocks(B, H, W, ncu()), C * 48
    ntiles = RR.wgrad_ntiles(B, H, W)
    wsb = L.sgx_rgbconv_wgrad_ws_bytes(B, H, W, C)
    assert wsb == RR.wgrad_ws_bytes(nblk, C), (wsb, nblk)
    ws = G((wsb // 4,))
    op = lambda k: p(outs[k].t) if k in outs else None
    grids = launch(c, lambda: L.sgx_rgbconv_wgrad(p(img), p(gz), ones, p(w0), o["s0"], p(wr), o["sr"], p(br), o["bscale"], op("w0"), op("b0"), op("wr"), op("br"), acc,
                                                  p(ws.t), wsb, B, H, W, C, N.BF16, N.stream()))
    RR.check_rc_grid(grids[0], ntiles, ncu(), per_cu=3)
    counts = RR.sched_counts(nblk, ntiles)
    if "3ncu" in c.id:
        assert nblk < ntiles and 2 in counts and 1 in counts, (nblk, ntiles)
    ws.assert_intact(f"{c.id} workspace")
    for k in outs:
        outs[k].assert_intact(f"{c.id} d{k}")
    # the workspace: every partial and dW' written, every block's partial an exact integer, their sum and dW' the exact value
    d = RR.dwprime(RR.with_ones(img64, ones), gz64)
    assert float(d.abs().max()) * 2 * 2 * 9 * C < RR.EXACT                   # |W0|, |Wr|, |br| bscale <= 2 * 2: no partial sum of the chain rule leaves the exact range
    wst = ws.t.cpu()
    assert not bool(wst.isnan().any()), f"{c.id}: {int(wst.isnan().sum())} workspace floats unwritten, first at {int(wst.isnan().nonzero()[0])} of {wst.numel()}"
    part, dwp = wst[:nblk * nout].view(nblk, nout).double(), wst[nblk * nout:]
    assert torch.equal(part, part.round()), f"{c.id}: a block partial is no integer"
    used = RR.DWP_USED.repeat(C)
    want = RR.dwp_layout(d)
    RR.assert_bits(part.sum(0)[used].float(), want[used], f"{c.id} sum of the block partials")
    RR.assert_bits(dwp[used], want[used], f"{c.id} dW' in the workspace")
    if ntiles <= 16:                                         # each block's partial against the tiles rc_sched gives it
        for blk in range(nblk):
            gt = torch.zeros_like(gz64)
            for t in RR.rc_sched(blk, nblk, ntiles):
                tx, ty, b = t % (W // 64), t // (W // 64) % (H // 8), t // (W // 64) // (H // 8)
                gt[b, ty * 8:ty * 8 + 8, tx * 64:tx * 64 + 64] = gz64[b, ty * 8:ty * 8 + 8, tx * 64:tx * 64 + 64]
            RR.assert_bits(part[blk][used].float(), RR.dwp_layout(RR.dwprime(RR.with_ones(img64, ones), gt))[used], f"{c.id} partial of block {blk}")
    ch = RR.chain_rule(d, o["w0"], o["wr"], o["br"] if a["br"] else None, o["s0"], o["sr"], o["bscale"])
    for i, k in enumerate(NAMES):
        if k in outs:
            ref = ch[k] + pre[k] if acc >> i & 1 else ch[k]
            note(c, f"d{k}", RR.assert_bits(outs[k].t, ref.reshape(shapes[k]), f"{c.id} d{k}"))


RUN = {"sgx_rgbconv_pack": run_pack, "sgx_rgbconv_fwd": run_fwd, "sgx_rgbconv_dgrad": run_dgrad, "sgx_rgbconv_wgrad": run_wgrad}


@pytest.mark.parametrize("cid", [c.id for c in RR.CASES])
def test_row(cid):
    N = native()
    L = N.lib()
    assert torch.cuda.is_available()
    c = RR.BY_ID[cid]
    with ERUN.sticky(cid):                                   # after a HIP error nothing more is started on the device from this process
        RUN[c.entry](L, N, c)
