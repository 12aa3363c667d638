"""Runs rows of conv_ref.CASES through native.lib() on the GPU: in-process for tests/test_gpu_conv_paths.py, and as a fresh child process for
the rows that need process-wide switches (``python conv_runner.py GROUP`` with the group's environment: one JSON line per row, the process
stops at the first HIP error).  Each row: the library's profiler brackets the call; the kernels and launch notes must be exactly what the
restated rules give at this device's CU count and what the row says; y, sign bits, statistics partials and the split-K workspace sit in
streaming_ref.Guarded buffers (the workspace exactly as large as the query says); a call that returns an error has written nothing; the
host queries agree with what the launch shows; and the values meet conv_ref's criteria: bit equality on integer rows, the chain bound on
the others."""
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import conv_ref as CR  # noqa: E402
import epilogue_ref as ER  # noqa: E402
import epilogue_runner as ERUN  # noqa: E402
import streaming_ref as SR  # noqa: E402
from epilogue_runner import DEV, digest, ints, native, p, rnd, sticky  # noqa: E402
from wgrad_runner import profiled  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
RESULTS = {}                        # row id -> what run_case returned (ratios, hash): rows run once per process
U32 = SR.U32


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def operand(shape, dtype, seed, data, scale=1.0, dense=False):
    """int: integers in [-3, 3]; sparse: -1 / 0 / 1 with a share SPARSE of non-zeros (dense: no thinning -- the weights); randn / abs."""
    if data == "int":
        return ints(shape, dtype, seed)
    if data == "sparse":
        g = ERUN._gen(seed)
        v = torch.randint(-1, 2, tuple(shape), generator=g, device=DEV)
        if not dense:
            v = v * (torch.rand(tuple(shape), generator=g, device=DEV) < CR.SPARSE)
        return v.to(dtype)
    t = rnd(shape, F32, seed, scale)
    return (t.abs() if data == "abs" else t).to(dtype)


def mask_like(shape, dtype, seed):
    """An integer mask tensor with zeros of both signs: mask > 0 is false for +0 and -0."""
    m = ints(shape, dtype, seed)
    m.view(-1)[::7] = -0.0
    return m


def bits_eq(a, b):
    it = torch.int16 if a.dtype == BF16 else (torch.int32 if a.dtype == F32 else torch.uint8)
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def assert_bits(got, want, what):
    if not bits_eq(got, want):
        diff = (got.float() != want.float()) | (torch.signbit(got.float()) != torch.signbit(want.float()))
        first = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} of {got.numel()} elements differ from the exact value; first at {first}: got {float(got[first])!r}, exact {float(want[first])!r}")


def unwritten(g):
    return g is None or bool((g.buf == SR.SENTINEL).all())


def family(kernels):
    if not kernels:
        return "none"
    k = kernels[0]
    if k.startswith("pack_upblur"):
        return "pack_upblur"
    m = re.match(r"(conv_kernel<(\w+), (\d+), (\d)|conv2_kernel<(\d), \d, (\d), (\d+), \w+, (\d)|conv3_kernel<(\d)|pack_weight\w*<(\w+))", k)
    if k.startswith("conv_kernel"):
        return f"g1 {m.group(2)} kc{m.group(3)} geo{m.group(4)}" + (" splitk" if len(kernels) > 1 else "")
    if k.startswith("conv2_kernel"):
        return f"c2 geo{m.group(5)} mf{m.group(6)} kc{m.group(7)} epi{m.group(8)}"
    if k.startswith("conv3_kernel"):
        return f"c3 geo{m.group(9)}"
    return f"pack {m.group(10)}"


def check_launch(c, rc, recs, pl, cus):
    L = native().lib()
    ran, notes = tuple(k for k, _ in recs), tuple(d for _, d in recs)
    assert rc == pl.rc == c.args["rc"], f"{c.id}: returned {rc} ({L.sgx_last_error().decode(errors='replace')}), the restated rules give {pl.rc}, the row {c.args['rc']}"
    assert ran == pl.kernels, f"{c.id}: launched {ran}, the restated rules give {pl.kernels} at {cus} CUs ({c.why})"
    assert ran == tuple(CR.row_kernels(c, cus)), f"{c.id}: launched {ran}, the row expects {CR.row_kernels(c, cus)} ({c.why})"
    assert all(w is None or n == w for n, w in zip(notes, pl.notes)), f"{c.id}: the launch notes are {notes}, expected {pl.notes}"
    if rc:
        L.sgx_clear_error()


def check_config(L, c, geo, ran):
    """sgx_conv_config against the conv_kernel instantiation that ran: {KC, TH, TW, BP, CT}, in every group (the query reads the same switches
    as the launch).  The transposed convolution is asked as geo 3, `as launched`: the all-class kernel's configuration where that runs (its
    template geometry prints as 3), the per-class kernel's -- geo 2's answer -- everywhere else."""
    if not ran or not ran[0].startswith("conv_kernel<"):
        return
    a = c.args
    t = [int(v) for v in re.findall(r"-?\d+", ran[0].split("<")[1].replace("bf16_t", "").replace("float", ""))]
    ask = [3] if geo == 2 else [geo]
    if geo == 2 and t[1] == 2:
        ask.append(2)
    for g in ask:
        c5 = (ctypes.c_int * 5)()
        assert L.sgx_conv_config(g, a["B"], a["H"], a["W"], a["Cin"], a["Cout"], dtc(c), ctypes.addressof(c5)) == 0
        assert list(c5) == [t[0]] + t[2:6], f"{c.id}: sgx_conv_config(geo {g}) says {list(c5)}, the launch ran {ran[0]}"
        want = CR.conv_config(g, c.dtype, a["B"], a["H"], a["W"], a["Cin"], a["Cout"], CR.group_env(c.group))
        assert list(c5) == want, f"{c.id}: sgx_conv_config(geo {g}) says {list(c5)}, restated {want}"


def dtc(c):
    return 0 if c.dtype == F32 else 1


def run_conv(L, N, c):
    """Every convolution entry point.  x, w, bias, mask from fixed seeds: rows of the same problem share their operands, which is what
    makes the twin hashes comparable."""
    a, dt, cus = c.args, c.dtype, ncu()
    B, Hh, W, Cin, Cout, data = a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["data"]
    geo = CR.geo_of(c)
    env = CR.group_env(c.group)
    pl = CR.row_plan(c, cus)
    e = c.entry
    OH, OW = CR.out_hw(geo, Hh, W)
    exact = data in ("int", "sparse")
    st = N.stream()
    x = operand((B, Hh, W, Cin), dt, 300, data)
    w = operand((CR.TAPS[geo], Cout, Cin), dt, 301, data, CR.weight_scale(geo, Cin), dense=True)
    bias = (ints((Cout,), F32, 302) if exact else rnd((Cout,), F32, 302, 0.5)) if a["bias"] else None
    act = a["act"]
    mask = mask_like((B, OH, OW, Cout), dt, 303) if a["mask"] else None
    y = SR.Guarded((B, OH, OW, Cout), dt, DEV)
    bits = part = ws = None
    res = {}
    shape = (B, Hh, W, Cin, Cout)
    # ---- the call
    if e == "sgx_conv3x3":
        call = lambda: L.sgx_conv3x3(p(x), p(w), p(bias), p(y.t), *shape, act, p(mask), dtc(c), st)
    elif e == "sgx_conv4x4s2_down":
        call = lambda: L.sgx_conv4x4s2_down(p(x), p(w), p(bias), p(y.t), *shape, act, dtc(c), st)
    elif e == "sgx_conv4x4s2_up":
        call = lambda: L.sgx_conv4x4s2_up(p(x), p(w), p(y.t), *shape, dtc(c), st)
    elif e == "sgx_conv_variant":
        call = lambda: L.sgx_conv_variant(geo, p(x), p(w), p(bias), p(y.t), *shape, act, dtc(c), a["variant"], st)
    elif e == "sgx_conv_splitk":
        q = L.sgx_conv_splitk_ws_bytes(geo, *shape, dtc(c))
        want = CR.splitk_ws_bytes(geo, dt, *shape, env, cus)
        assert q == want, f"{c.id}: sgx_conv_splitk_ws_bytes returns {q}, restated {want}"
        wsb = (q - 1 if a.get("ws") == "short" else q)
        ws = SR.Guarded((max(wsb, 1),), torch.uint8, DEV)
        call = lambda: L.sgx_conv_splitk(geo, p(x), p(w), p(bias), p(y.t), None, *shape, act, dtc(c), p(ws.t), wsb, st)
    elif e == "sgx_conv3x3_signbits":
        ok = L.sgx_conv3x3_signbits_ok(*shape, dtc(c))
        assert ok == CR.signbits_ok(dt, *shape, env, cus), f"{c.id}: sgx_conv3x3_signbits_ok = {ok}"
        bits = SR.Guarded((B, OH, OW, Cout // 8), torch.uint8, DEV)
        call = lambda: L.sgx_conv3x3_signbits(p(x), p(w), p(bias), p(y.t), p(bits.t), *shape, act, p(mask), dtc(c), st)
    elif e == "sgx_conv3x3_stats":
        npart = L.sgx_conv3x3_stats_nparts(*shape, dtc(c))
        assert npart == CR.stats_nparts(dt, *shape, env, cus), f"{c.id}: sgx_conv3x3_stats_nparts = {npart}, restated {CR.stats_nparts(dt, *shape, env, cus)}"
        noise, nw = rnd((B, OH * OW), F32, 304), rnd((Cout,), F32, 305, 0.3)
        part = SR.Guarded((B, max(npart, 1), Cout, 2), torch.float64, DEV)
        pb = part.nbytes - (1 if a.get("part") == "short" else 0)
        call = lambda: L.sgx_conv3x3_stats(p(x), p(w), p(y.t), p(bias), p(noise), p(nw), p(part.t), pb, *shape, dtc(c), st)
    elif e in ("sgx_conv4x4s2_up_blur", "sgx_conv4x4s2_up_blur_bits"):
        ok = L.sgx_conv4x4s2_up_blur_ok(*shape, dtc(c))
        assert ok == CR.up_blur_ok(dt, *shape, env, cus), f"{c.id}: sgx_conv4x4s2_up_blur_ok = {ok}"
        if e.endswith("bits"):
            mask = mask_like((B, OH, OW, Cout), dt, 303)                                      # the mask the bits come from
            mbits = SR.pack_bits(mask > 0).contiguous()
            call = lambda: L.sgx_conv4x4s2_up_blur_bits(p(x), p(w), p(y.t), p(mbits), *shape, dtc(c), st)
        else:
            call = lambda: L.sgx_conv4x4s2_up_blur(p(x), p(w), p(y.t), p(mask), *shape, dtc(c), st)
    elif e in ("sgx_conv4x4s2_down_fade", "sgx_conv4x4s2_down_fade_rgb"):
        ok = L.sgx_conv4x4s2_down_fade_ok(*shape, dtc(c))
        assert ok == CR.down_fade_ok(dt, *shape, env, cus), f"{c.id}: sgx_conv4x4s2_down_fade_ok = {ok}"
        alpha, beta = (CR.ALPHA_INT, CR.BETA_INT) if exact else (CR.ALPHA_RND, CR.BETA_RND)
        ab = torch.tensor([alpha, beta], dtype=F32, device=DEV) if a.get("ab_dev") else None
        ha, hb = (0.0, 0.0) if ab is not None else (alpha, beta)
        bits = SR.Guarded((B, OH, OW, max(Cout // 8, 1)), torch.uint8, DEV)
        if e.endswith("rgb"):
            pimg, wr = operand((B, OH, OW, 3), F32, 306, data), operand((Cout, 3), F32, 307, data)
            rb = (ints((Cout,), F32, 308) if exact else rnd((Cout,), F32, 308)) if a["rb"] else None
            wsc, bs1, bs2 = 0.5, 2.0, 0.5                                                      # (powers of two: (rb bs1) bs2 is exact however it is fused)
            call = lambda: L.sgx_conv4x4s2_down_fade_rgb(p(x), p(w), p(bias), p(pimg), p(wr), wsc, p(rb), bs1, bs2, ha, hb, p(ab), p(y.t), p(bits.t), *shape, dtc(c), st)
        else:
            resid = operand((B, OH, OW, Cout), dt, 309, data)
            call = lambda: L.sgx_conv4x4s2_down_fade(p(x), p(w), p(bias), p(resid), ha, hb, p(ab), p(y.t), p(bits.t), *shape, dtc(c), st)
    else:
        raise KeyError(e)
    rc, recs = profiled(c.id, call)
    check_launch(c, rc, recs, pl, cus)
    guards = [(y, "y"), (bits, "sign bits"), (part, "partials"), (ws, "workspace")]
    for g, what in guards:
        if g is not None:
            g.assert_intact(f"{c.id} {what}")
    res["family"] = family(pl.kernels)
    if rc:                                                                                    # an error return: nothing launched, nothing written
        for g, what in guards:
            assert unwritten(g), f"{c.id}: {what} was written by a call that returned {rc}"
        return res
    ran = tuple(k for k, _ in recs)
    check_config(L, c, geo, ran)
    if e == "sgx_conv_splitk":                                                                # the query / (pixels x Cout x 4) is the /k<N> of the launch note
        ks = int(re.search(r"/k(\d+) ", recs[0][1]).group(1))
        assert q == ks * B * OH * OW * Cout * 4 and ks == pl.ksplit, f"{c.id}: the workspace query {q} against the launch note {recs[0][1]}"
    # ---- the values
    x64, w64, b64 = x.double(), w.double(), (bias.double() if bias is not None else None)
    pre, S = CR.pre_activation(x64, w64, None, geo)                                            # without the bias: exact_store adds it in fp32
    if e in ("sgx_conv4x4s2_up_blur", "sgx_conv4x4s2_up_blur_bits"):
        assert exact, "the blur epilogue has integer rows only (conv_ref.EXCLUDED_PATHS)"
        blur, vert = CR.blur121(pre)
        for t, what in ((pre, "the transposed convolution"), (vert, "the vertical pass"), (blur, "the blurred value")):      # bf16-exact, so the kernel's intermediate roundings change nothing
            assert torch.equal(t.float().bfloat16().double(), t), f"{c.id}: {what} of the reference is not exact in bf16: choose sparser operands"
        want = blur.float().to(dt)
        if mask is not None:
            want = (want.float() * torch.where(mask.float() > 0, 1.0, SR.LRELU).float()).to(dt)
        assert_bits(y.t, want, f"{c.id} y")
        res["hash"] = digest(y.t)
    elif e in ("sgx_conv4x4s2_down_fade", "sgx_conv4x4s2_down_fade_rgb"):
        if e.endswith("rgb"):                                                                  # the residual through sgx_rgb_in: the same arithmetic, bit for bit
            resid = torch.empty((B, OH, OW, Cout), dtype=dt, device=DEV)
            rbe = None if rb is None else (rb * bs1) * bs2
            N.check(L.sgx_rgb_in(p(pimg), p(wr), 1, 3, wsc, p(rbe), p(resid), B * OH * OW, Cout, dtc(c), st), "sgx_rgb_in")
            if exact:
                rr, _ = CR.rgb_resid(pimg.double(), wr.double(), wsc, None if rb is None else rb.double(), bs1, bs2)
                assert_bits(resid, rr.float().to(dt), f"{c.id} the residual of an integer row")
        # the promise of sgx.h: the lerp on the bf16-ROUNDED activation, exactly as sgx_axpby on the tensor sgx_conv4x4s2_down stores -- on every row
        # (this is what pins the random fade rows: the activation itself is held to fp64 by the same-seed rows c2-D-mf2-randn / -abs and c2-D-mf1 of
        # sgx_conv4x4s2_down, sgx_axpby by tests/test_gpu_streaming_kernels.py; tests/test_conv_coverage.py asserts that those rows exist)
        act_t, lerp = torch.empty((B, OH, OW, Cout), dtype=dt, device=DEV), torch.empty((B, OH, OW, Cout), dtype=dt, device=DEV)
        N.check(L.sgx_conv4x4s2_down(p(x), p(w), p(bias), p(act_t), *shape, CR.ACT_LRELU, dtc(c), st), "sgx_conv4x4s2_down")
        N.check(L.sgx_axpby(p(act_t), p(resid), p(lerp), alpha, beta, act_t.numel(), dtc(c), st), "sgx_axpby")
        torch.cuda.synchronize()
        assert_bits(y.t, lerp, f"{c.id} y against sgx_conv4x4s2_down + sgx_axpby")
        a_r = CR.exact_store(pre, bias, CR.ACT_LRELU, None, dt) if exact else None
        if exact:
            assert_bits(act_t, a_r, f"{c.id} the activation")
            assert_bits(y.t, (alpha * a_r.float() + beta * resid.float()).to(dt), f"{c.id} y")
            assert torch.equal(bits.t, SR.pack_bits(a_r > 0)), f"{c.id}: the sign bits differ from the exact sign in {int((bits.t != SR.pack_bits(a_r > 0)).sum())} bytes"
            res["zeros"] = int((a_r == 0).sum())
            assert res["zeros"] > 0 and bool((a_r < 0).any()), f"{c.id}: no activation of this integer row is exactly zero"
        else:
            # L: 16 taps x Cin + bias + LeakyReLU (chain); the activation is then ROUNDED to bf16 (restated: where the fp64 activation is within
            # its own bound E of a rounding boundary every bf16 value of [a - E, a + E] is admissible), and the lerp adds two products and a sum
            Lc = CR.chain(1, Cin, bias is not None, True)
            pre_b, S_b = pre + b64, S + b64.abs()
            a64 = SR.act(pre_b, 1)
            E = (Lc + 2) * U32 * S_b
            lo, hi = (a64 - E).float().bfloat16().double(), (a64 + E).float().bfloat16().double()
            r64 = resid.double()
            got = y.t.double()
            ar = torch.minimum(torch.maximum((got - beta * r64) / alpha, lo), hi).float().bfloat16().double()      # the admissible rounded activation that explains y best
            res["ambiguous"] = float((lo != hi).double().mean())
            res["y"] = SR.assert_elementwise(y.t, alpha * ar + beta * r64, alpha * ar.abs() + beta * r64.abs(), 3, dt, f"{c.id} y")
            near = pre_b.abs() <= E                                                            # the sign of these is not pinned by the reference
            res["bits_left_out"] = float(near.double().mean())
            assert res["bits_left_out"] <= CR.BITS_CAP, f"{c.id}: {res['bits_left_out']:.4%} of the pre-activations are within their own bound: the inputs do not keep the cap"
            wrong = (SR.unpack_bits(bits.t, Cout) != (pre_b > 0)) & ~near
            assert not bool(wrong.any()), f"{c.id}: {int(wrong.sum())} sign bits differ from the fp64 pre-activation's sign, first at {tuple(int(v) for v in wrong.nonzero()[0])}"
        assert torch.equal(bits.t, SR.pack_bits(act_t > 0)), f"{c.id}: the sign bits are not those of the activation sgx_conv4x4s2_down stores"
        res["hash"] = digest(y.t, bits.t)
    else:
        splits = pl.ksplit if e == "sgx_conv_splitk" else 1
        if part is not None:                                                                   # sgx_conv3x3_stats: y has no bias and no activation, `bias` is the epilogue's
            eb64, bias, b64, act = b64, None, None, CR.ACT_NONE
        if exact:
            assert_bits(y.t, CR.exact_store(pre, bias, act, mask, dt), f"{c.id} y")
            res["hash"] = digest(y.t)
            if bits is not None or (mask is not None and y.t.numel() >= 1 << 16):              # the row pins > 0 at zero: the reference alone says it holds exact zeros and negatives (mask rows of a few hundred outputs may hold none)
                pz = pre + b64 if b64 is not None else pre
                res["zeros"] = int((pz == 0).sum())
                assert res["zeros"] > 0 and bool((pz < 0).any()), f"{c.id}: no pre-activation of this integer row is exactly zero"
        else:
            assert mask is None
            # L: the taps that meet in one output x Cin products in fp32, any order, + the bias + the LeakyReLU product (+ the sum of the splits)
            ref, Sb = (pre + b64, S + b64.abs()) if b64 is not None else (pre, S)
            res["y"] = SR.assert_elementwise(y.t, SR.act(ref, act), Sb, CR.chain(geo, Cin, bias is not None, act != 0, splits), dt, f"{c.id} y")
        if bits is not None:                                                                   # the stored activation is there: no exclusions
            assert torch.equal(bits.t, SR.pack_bits(y.t > 0)), f"{c.id}: the sign bits differ from pack_bits(y > 0) in {int((bits.t != SR.pack_bits(y.t > 0)).sum())} bytes"
        if part is not None:
            HW = OH * OW
            Lc = ER.conv_stats_chain(Hh, W, Cout, npart)
            y64 = y.t.double().reshape(B, HW, Cout)
            sums, Ss = ER.activation_sums(y64, eb64, noise.double(), nw.double(), True)
            got = part.t.sum(1)
            res["sum_a"] = SR.assert_elementwise(got[..., 0], sums[..., 0], Ss[..., 0], Lc + 4, torch.float64, f"{c.id} sum a")
            res["sum_a2"] = SR.assert_elementwise(got[..., 1], sums[..., 1], Ss[..., 1], Lc + 9, torch.float64, f"{c.id} sum a^2")
    return res


def pack_problem(dt, mode, kind, data, seed):
    O, I, Ip, _ = CR.PACK_SHAPES[kind]
    w = operand((O, I, 3, 3), F32, seed, data)
    scale = 0.5 if data == "int" else SR.f32(0.0371)
    taps = 9 if mode == "S" else 16
    return w, scale, O, I, Ip, SR.Guarded((taps, O, Ip), dt, DEV), SR.Guarded((taps, Ip, O), dt, DEV)


def check_pack(c, dt, mode, data, w, scale, Ip, fwd, adj, res):
    rf, ra, Sf, Sa = CR.pack_weight(w.double(), Ip, mode, scale)
    for g, ref, S, what in ((fwd, rf, Sf, "fwd"), (adj, ra, Sa, "adj")):
        g.assert_intact(f"{c.id} {what}")
        if data == "int":                                                                      # sums of at most four integers times 0.5 (x 0.25): exact in fp32 and in bf16
            assert torch.equal(ref.float().to(dt).double(), ref), c.id
            assert_bits(g.t, ref.float().to(dt), f"{c.id} {what}")
        else:                                                                                  # L: three sums of the 3x3 -> 4x4 synthesis and two products
            res[what] = max(res.get(what, 0.0), SR.assert_elementwise(g.t, ref, S, 5, dt, f"{c.id} {what}"))


def run_pack(L, N, c):
    a, dt, cus = c.args, c.dtype, ncu()
    pl = CR.row_plan(c, cus)
    st = N.stream()
    res = {"family": family(pl.kernels)}
    if c.entry == "sgx_pack_weight":
        w, scale, O, I, Ip, fwd, adj = pack_problem(dt, a["mode"], [k for k, v in CR.PACK_SHAPES.items() if v[:3] == (a["O"], a["I"], a["Ipad"])][0], a["data"], 310)
        rc, recs = profiled(c.id, lambda: L.sgx_pack_weight(p(w), p(fwd.t), p(adj.t), O, I, Ip, CR.MODES[a["mode"]], scale, dtc(c), st))
        check_launch(c, rc, recs, pl, cus)
        check_pack(c, dt, a["mode"], a["data"], w, scale, Ip, fwd, adj, res)
        res["hash"] = digest(fwd.t, adj.t)
        return res
    probs, rows, first = [], [], 0
    for i, (mode, kind) in enumerate(a["params"]):
        w, scale, O, I, Ip, fwd, adj = pack_problem(dt, mode, kind, "int" if i % 2 == 0 else "randn", 320 + i)
        nb = L.sgx_pack_weight_blocks(O, Ip)
        assert nb == CR.cdiv(O, 32) * CR.cdiv(Ip, 32)
        sbits = ctypes.c_uint32.from_buffer(ctypes.c_float(scale)).value
        rows.append([p(w), p(fwd.t), p(adj.t), O, I, Ip, CR.MODES[mode], sbits, first, nb])
        probs.append((mode, "int" if i % 2 == 0 else "randn", w, scale, O, I, Ip, fwd, adj))
        first += nb
    table = torch.tensor(rows, dtype=torch.int64, device=DEV)
    rc, recs = profiled(c.id, lambda: L.sgx_pack_weight_multi(p(table), len(rows), first, dtc(c), st))
    check_launch(c, rc, recs, pl, cus)
    for mode, data, w, scale, O, I, Ip, fwd, adj in probs:
        check_pack(c, dt, mode, data, w, scale, Ip, fwd, adj, res)
        f1, a1 = torch.empty_like(fwd.t), torch.empty_like(adj.t)                             # bit-equal to the single-parameter launch
        N.check(L.sgx_pack_weight(p(w), p(f1), p(a1), O, I, Ip, CR.MODES[mode], scale, dtc(c), st), "sgx_pack_weight")
        torch.cuda.synchronize()
        assert bits_eq(fwd.t, f1) and bits_eq(adj.t, a1), f"{c.id}: parameter {mode} {O}x{I} differs from its single launch"
    return res


def upblur_problem(c):
    """The parameter of the layer (mode U / UF: [16][32][3][3]; mode D, adjoint: [32][16][3][3]), integers in [-3, 3], and the scale w_mul / 16
    with w_mul = 1: every composite tap and correction tile is an integer of at most 192 times 2^-4 (2^-6 in mode D), exact in bf16."""
    a = c.args
    O, I = (32, 16) if a["adjoint"] else (16, 32)
    return ints((O, I, 3, 3), F32, 330), O, I, 1.0 / 16


def run_upblur(L, N, c):
    a, cus = c.args, ncu()
    st = N.stream()
    pl = CR.row_plan(c, cus)
    w, O, I, scale = upblur_problem(c)
    res = {"family": family(pl.kernels)}
    wc = SR.Guarded((80 * 16 * 32,), BF16, DEV)                                                # [9][4 N][K] + [22][2 N][K], N K = 512
    pack = lambda: L.sgx_pack_upblur(p(w), p(wc.t), O, I, CR.MODES[a["mode"]], a["adjoint"], scale, st)
    if c.entry == "sgx_pack_upblur":
        rc, recs = profiled(c.id, pack)
        check_launch(c, rc, recs, pl, cus)
        wc.assert_intact(f"{c.id} wc")
        main = CR.pack_upblur_main(w.double(), a["mode"], a["adjoint"], scale)
        assert torch.equal(main.float().bfloat16().double(), main), f"{c.id}: a composite tap of the reference is not exact in bf16"
        assert_bits(wc.t[:main.numel()].view(main.shape), main.float().bfloat16(), f"{c.id} composite taps")
        assert torch.equal(wc.t.float().bfloat16(), wc.t) and not bool(torch.isnan(wc.t.float()).any()), f"{c.id}: a correction tile was not written"
        res["hash"] = digest(wc.t)
        return res
    B, Hh, W, Cin, Cout = a["B"], a["H"], a["W"], a["Cin"], a["Cout"]
    shape = (B, Hh, W, Cin, Cout)
    ok = L.sgx_conv_upblur_ok(*shape, 1)
    assert ok == CR.upblur_ok(BF16, *shape, CR.group_env(c.group)), f"{c.id}: sgx_conv_upblur_ok = {ok}"
    if not a["rc"]:
        N.check(pack(), "sgx_pack_upblur")
    x = ints((B, Hh, W, Cin), BF16, 331)
    y = SR.Guarded((B, 2 * Hh, 2 * W, Cout), BF16, DEV)
    m = mask_like((B, 2 * Hh, 2 * W, Cout), BF16, 332) if a["bits"] else None
    mbits = SR.pack_bits(m > 0).contiguous() if m is not None else None
    rc, recs = profiled(c.id, lambda: L.sgx_conv_upblur(p(x), p(wc.t), p(y.t), p(mbits), *shape, 1, st))
    check_launch(c, rc, recs, pl, cus)
    y.assert_intact(f"{c.id} y")
    wc.assert_intact(f"{c.id} wc")
    if rc:
        assert unwritten(y), f"{c.id}: y was written by a call that returned {rc}"
        return res
    ref, ct, vert = CR.conv_upblur(x.double(), w.double(), a["mode"], a["adjoint"], scale)
    v = ref.float()
    assert torch.equal(v.double(), ref), f"{c.id}: the sums of an integer row are exact in fp32"
    if m is not None:                                                                          # the slope multiplies in fp32 before the one rounding
        v = v * torch.where(m.float() > 0, 1.0, SR.LRELU).float()
    assert_bits(y.t, v.bfloat16(), f"{c.id} y")
    res["hash"] = digest(y.t)
    return res


def run(L, N, c):
    res = run_upblur(L, N, c) if c.entry in ("sgx_conv_upblur", "sgx_pack_upblur") else (run_pack(L, N, c) if c.entry.startswith("sgx_pack") else run_conv(L, N, c))
    twin = c.args["twin"]
    if twin and CR.BY_ID[twin].group == c.group:                                              # (the parent compares across processes)
        assert res["hash"] == run_case(CR.BY_ID[twin])["hash"], f"{c.id}: the bits differ from the row {twin}"
    return res


def run_case(c):
    """Run a row once in this process (whose environment must be the row's group) -> its figures."""
    if c.id not in RESULTS:
        N = native()
        with sticky(c.id):                                   # the operands, the call and the fp64 references alike
            res = run(N.lib(), N, c)
        RESULTS[c.id] = res
        rep = os.environ.get("SGX_CONV_REPORT")              # a measuring run keeps every figure
        if rep:
            with open(rep, "a") as f:
                f.write(json.dumps({"id": c.id, **res}) + "\n")
    return RESULTS[c.id]


def main(group):
    for k in {k for g in CR.GROUPS.values() for k in g}:
        assert os.environ.get(k) == CR.GROUPS[group].get(k), f"{k} must be {CR.GROUPS[group].get(k)} for group {group}"
    for c in [c for c in CR.CASES if c.group == group]:
        try:
            print(json.dumps({"id": c.id, "ok": True, **run_case(c)}), flush=True)
        except AssertionError as e:
            print(json.dumps({"id": c.id, "ok": False, "error": str(e)[:600]}), flush=True)
            if ERUN._FAULT is not None:
                return 3
        except RuntimeError as e:                            # a HIP error: stop here
            print(json.dumps({"id": c.id, "ok": False, "error": "HIP: " + str(e)[:600]}), flush=True)
            return 3
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
