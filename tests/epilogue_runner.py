"""Runs rows of epilogue_ref.CASES through native.lib() on the GPU: in-process for tests/test_gpu_epilogue_paths.py, and as a fresh child process
for the rows that need process-wide switches (``python epilogue_runner.py GROUP`` with the group's environment: one JSON line per row, the
process stops at the first HIP error).  Each row: the library's profiler brackets the call, the kernels that ran must be exactly the row's,
every output sits in a streaming_ref.Guarded buffer, and the values meet the decoupled criterion of epilogue_ref."""
import contextlib
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import epilogue_ref as ER  # noqa: E402
import streaming_ref as SR  # noqa: E402

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
_FAULT = None
RESULTS = {}                        # row id -> what run_case returned (ratios, hashes): rows run once per process


def native():
    from stylegan.pytorch_amd import native as N
    return N


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rnd(shape, dtype, seed, scale=1.0):
    return (scale * torch.randn(tuple(shape), generator=_gen(seed), device=DEV, dtype=torch.float32)).to(dtype)


def ints(shape, dtype, seed):
    return torch.randint(-3, 4, tuple(shape), generator=_gen(seed), device=DEV).to(dtype)


def p(t):
    return None if t is None else t.data_ptr()


def d(t):
    return None if t is None else t.double()


def G(shape, dtype):
    return SR.Guarded(shape, dtype, DEV)


@contextlib.contextmanager
def sticky(what):
    """The sticky-fault rule around everything that touches the device: a HIP error (torch and the library's own check raise a RuntimeError
    for one) is remembered, and after one nothing more is started on the device from this process."""
    global _FAULT
    assert _FAULT is None, f"not run: the GPU reported an error in an earlier case ({_FAULT})"
    try:
        yield
    except RuntimeError as e:
        _FAULT = f"{what}: {e}"
        raise


def profiled(what, entry, call):
    """One (or a sequence of) C ABI calls under the library's profiler -> kernel_id() of every launch, in order."""
    N = native()
    with sticky(what):
        N.prof_start(1)
        try:
            rc = call()
            torch.cuda.synchronize()
        finally:
            N.prof_start(0)
        N.check(rc, entry)
        return [SR.kernel_id(r[0]) for r in N.prof_records()]


def launch(c, call, kernels=None):
    ran = profiled(c.id, c.entry, call)
    want = list(c.kernels if kernels is None else kernels)
    assert ran == want, f"{c.id}: launched {ran}, expected {want} ({c.why})"


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def elementwise(c, g, ref, S, n, what):
    r = SR.assert_elementwise(g.t, ref.reshape(g.t.shape), S.reshape(g.t.shape), n, g.t.dtype, f"{c.id} {what}")
    g.assert_intact(f"{c.id} {what}")
    return r


def within(c, g, ref, bound, what):
    r = ER.assert_within(g.t, ref, bound, f"{c.id} {what}")
    g.assert_intact(f"{c.id} {what}")
    return r


def operands(c, HW=None):
    a = c.args; B, C = a["B"], a["C"]; HW = HW or a["HW"]
    noise, style = rnd((B, HW), F32, 102), rnd((B, 2 * C), F32, 104, 0.5)
    bias = rnd((C,), F32, 101, 0.1) if a["bias"] else None
    if a["data"] == "int":                                   # small integers: bf16-exact, every sum exact in fp32 whatever the order
        return ints((B, HW, C), c.dtype, 100), None, noise, torch.zeros(C, device=DEV), style
    if a["data"] == "const":                                 # one value per (image, channel), quarters: the true variance is 0
        q = (rnd((B, 1, C), F32, 100, 4.0)).round() / 4.0
        return q.expand(B, HW, C).contiguous().to(c.dtype), bias, noise, torch.zeros(C, device=DEV), style
    off = torch.tensor([0.0, 0.5, -1.5, 3.0], device=DEV)[torch.arange(C, device=DEV) % 4]
    return (rnd((B, HW, C), F32, 100) + off).to(c.dtype), bias, noise, rnd((C,), F32, 103, 0.3), style


def dtc(c):
    return 0 if c.dtype == F32 else 1


def ulp_apart(a, b):
    """Largest distance in fp32 ulps between two positive fp32 tensors."""
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


def check_stats(c, res, mean, rstd, x64, b64, nz64, nw64, flags, L):
    (mr, rr), (dm, dr) = ER.gepi_stats(x64, b64, nz64, nw64, flags, L)
    res["mean"], res["rstd"] = within(c, mean, mr, dm, "mean"), within(c, rstd, rr, dr, "rstd")
    if c.args["data"] == "int" and flags & ER.EPI_NORM:
        HW = x64.shape[1]
        want = (x64.sum(1) / HW).float()                     # the sum is exact, HW <= 2^24: one rounding to fp64 (none for a power of two), one to fp32
        assert torch.equal(mean.t.view(torch.int32), want.view(torch.int32)), f"{c.id}: mean of an integer row differs from the exact value in {int((mean.t != want).sum())} places"
        assert ulp_apart(rstd.t, rr.float()) <= 1, f"{c.id}: rstd of an integer row {ulp_apart(rstd.t, rr.float())} ulps off"
    if c.args["data"] == "const":
        assert bool(torch.isfinite(rstd.t).all()) and float(rstd.t.max()) <= 1.0 / ER.EPS ** 0.5 * (1 + 1e-6), f"{c.id}: rstd past 1 / sqrt(eps)"


def make_pre(c, x64, b64, nz64, nw64, flags):
    npart = c.args.get("pre")
    if not npart:
        return None, 0
    return ER.partials(x64, b64, nz64, nw64, flags, npart).contiguous(), npart


def run_fwd(L, N, c):
    a = c.args; B, HW, C, flags = a["B"], a["HW"], a["C"], a["flags"]
    x, bias, noise, nw, style = operands(c)
    x64, b64, nz64, nw64 = x.double(), d(bias), noise.double(), nw.double()
    pre, npart = make_pre(c, x64, b64, nz64, nw64, flags)
    y, mean, rstd = G((B, HW, C), c.dtype), G((B, C), F32), G((B, C), F32)
    wsb = L.sgx_gepi_ws_bytes(B, HW, C)
    ws = N.workspace(wsb, DEV)
    launch(c, lambda: L.sgx_gepi_fwd(p(x), p(bias), p(noise), p(nw), p(style), p(y.t), p(mean.t), p(rstd.t), p(ws), wsb, p(pre), npart, B, HW, C, flags, dtc(c), N.stream()))
    res = {}
    check_stats(c, res, mean, rstd, x64, b64, nz64, nw64, flags, ER.chain_fwd(B, HW, C, c.dtype, c.kernels))
    del pre
    ref, S = ER.gepi_fwd(x64, b64, nz64, nw64, style.double(), mean.t.double(), rstd.t.double(), flags)
    res["y"] = elementwise(c, y, ref, S, ER.N_FWD, "y")
    if y.t.numel() <= 1 << 23:
        res["hash"] = digest(y.t)
    return res


def run_stats(L, N, c):
    a = c.args; B, HW, C, flags = a["B"], a["HW"], a["C"], a["flags"]
    x, bias, noise, nw, _ = operands(c)
    x64, b64, nz64, nw64 = x.double(), d(bias), noise.double(), nw.double()
    pre, npart = make_pre(c, x64, b64, nz64, nw64, flags)
    mean, rstd = G((B, C), F32), G((B, C), F32)
    wsb = L.sgx_gepi_ws_bytes(B, HW, C)
    ws = N.workspace(wsb, DEV)
    launch(c, lambda: L.sgx_gepi_stats(p(x), p(bias), p(noise), p(nw), p(mean.t), p(rstd.t), p(ws), wsb, p(pre), npart, B, HW, C, flags, dtc(c), N.stream()))
    res = {}
    check_stats(c, res, mean, rstd, x64, b64, nz64, nw64, flags, ER.chain_fwd(B, HW, C, c.dtype, c.kernels))
    return res


def run_blur_stats(L, N, c):
    a = c.args; B, Hh, W, C, flags = a["B"], a["H"], a["W"], a["C"], a["flags"]
    HW, on = Hh * W, flags & ER.EPI_ACT
    _, bias, noise, nw, style = operands(c, HW)
    x = rnd((B, Hh, W, C), c.dtype, 105)
    rt, npart = ER.blur_stats_geom(B, Hh, W, C, 4 if c.dtype == F32 else 8)
    assert L.sgx_blur3x3_stats_nparts(B, Hh, W, C, dtc(c)) == npart, f"{c.id}: the strip geometry restated in epilogue_ref"
    yb, part = G((B, Hh, W, C), c.dtype), G((B, npart, C, 2), torch.float64)
    y, mean, rstd = G((B, HW, C), c.dtype), G((B, C), F32), G((B, C), F32)
    wsb = L.sgx_gepi_ws_bytes(B, HW, C)
    ws = N.workspace(wsb, DEV)

    def call():
        rc = L.sgx_blur3x3_stats(p(x), p(yb.t), p(bias), p(noise), p(nw), p(part.t), part.nbytes, B, Hh, W, C, 1 if on else 0, dtc(c), N.stream())
        return rc or L.sgx_gepi_fwd(p(yb.t), p(bias), p(noise), p(nw), p(style), p(y.t), p(mean.t), p(rstd.t), p(ws), wsb, p(part.t), npart, B, HW, C, flags, dtc(c), N.stream())
    launch(c, call)
    res = {}
    ref, S = ER.blur3x3_stats(x.double(), d(bias), noise.double(), nw.double(), on)
    res["blur"] = elementwise(c, yb, ref, S, 9, "blur")
    y64, b64, nz64, nw64 = yb.t.double().reshape(B, HW, C), d(bias), noise.double(), nw.double()
    sums, Ss = ER.activation_sums(y64, b64, nz64, nw64, on)
    got = part.t.sum(1)
    part.assert_intact(f"{c.id} partials")
    res["sum_a"] = SR.assert_elementwise(got[..., 0], sums[..., 0], Ss[..., 0], rt + 4, torch.float64, f"{c.id} sum a")
    res["sum_a2"] = SR.assert_elementwise(got[..., 1], sums[..., 1], Ss[..., 1], rt + 9, torch.float64, f"{c.id} sum a^2")
    check_stats(c, res, mean, rstd, y64, b64, nz64, nw64, flags, rt)
    ref, S = ER.gepi_fwd(y64, b64, nz64, nw64, style.double(), mean.t.double(), rstd.t.double(), flags)
    res["y"] = elementwise(c, y, ref, S, ER.N_FWD, "y")
    return res


def run_bwd(L, N, c):
    a = c.args; B, HW, C, flags = a["B"], a["HW"], a["C"], a["flags"]
    x, bias, noise, nw, style = operands(c)
    dy = ints((B, HW, C), c.dtype, 110) if a["data"] == "int" else rnd((B, HW, C), c.dtype, 110)
    x64, b64, nz64, nw64 = x.double(), d(bias), noise.double(), nw.double()
    (m64, r64), _ = ER.gepi_stats(x64, b64, nz64, nw64, flags, 0)
    mean, rstd = m64.float(), r64.float()                    # the backward's inputs: the fp64 statistics rounded once
    dx, dstyle, dnw = G((B, HW, C), c.dtype), G((B, 2 * C), F32), G((C,), F32)
    dbias = G((C,), F32) if a.get("dbias", True) else None
    wsb = L.sgx_gepi_ws_bytes(B, HW, C)
    ws = N.workspace(wsb, DEV)
    launch(c, lambda: L.sgx_gepi_bwd(p(dy), p(x), p(bias), p(noise), p(nw), p(style), p(mean), p(rstd), p(dx.t), p(dstyle.t), p(dnw.t), p(dbias.t if dbias else None),
                                     p(ws), wsb, B, HW, C, flags, dtc(c), N.stream()))
    L1, L2 = ER.chain_bwd(B, HW, C, c.dtype, c.kernels)
    dy64 = dy.double()
    b = ER.gepi_bwd(dy64, x64, b64, nz64, nw64, style.double(), mean.double(), rstd.double(), flags, L1, L2)
    del x64
    res = {}
    ref, nk = ER.choose_slope(dx.t, b)
    assert nk <= ER.kink_cap(dx.t.numel()), f"{c.id}: {nk} pre-activations within {ER.KINK} u of zero in the reference: the inputs do not keep the cap"
    res["kink"] = nk
    res["dx"] = elementwise(c, dx, ref, b.S_dx, b.n_dx, "dx")
    ds = dstyle.t.double()
    res["dstyle0"] = SR.assert_elementwise(ds[:, :C], b.dstyle[:, :C], b.S_dstyle[:, :C], L1 + 7, F32, f"{c.id} dstyle[:, :C]")
    res["dstyle1"] = SR.assert_elementwise(ds[:, C:], b.dstyle[:, C:], b.S_dstyle[:, C:], L1, F32, f"{c.id} dstyle[:, C:]")
    dstyle.assert_intact(f"{c.id} dstyle")
    res["dnw"] = elementwise(c, dnw, b.dnw, b.S_dnw, b.n_dnw, "dnw")
    if dbias:
        res["dbias"] = elementwise(c, dbias, b.dbias, b.S_dbias, b.n_dbias, "dbias")
    if a["data"] == "int":
        want = dy64.sum(1).float()
        assert torch.equal(dstyle.t[:, C:].view(torch.int32), want.view(torch.int32)), f"{c.id}: sum dy of an integer row differs from the exact value in {int((dstyle.t[:, C:] != want).sum())} places"
    if dx.t.numel() <= 1 << 23:
        res["hash"] = digest(dx.t)                          # (d noise weight / d bias are summed in another order by gepi_bwd2s: no promise of bits)
    return res


def run_conv_stats(L, N, c):
    """The producer runs through the package's own convolution call (it owns the weight pack; tests/test_gpu_fusions.py checks y against the
    plain convolution); here: its partials against fp64 sums of the stored y, then the epilogue on them."""
    from oracle import stylegan_oracle as O
    from stylegan.pytorch_amd import functional as Fn
    a = c.args; B, Hh, W, C, flags = a["B"], a["H"], a["W"], a["C"], a["flags"]
    HW = Hh * W
    _, bias, noise, nw, style = operands(c, HW)
    x, w = rnd((B, Hh, W, C), BF16, 105), rnd((C, C, 3, 3), F32, 106)
    assert Fn.conv_stats_nparts(x, C) > 0, "shape expected to have a fused kernel"
    with sticky(c.id + " (the convolution)"):
        yb, part = Fn.ConvFn.apply(x, w, None, "S", O.he_w_mul(C * 9, 2 ** 0.5), C, False, 0, None, False, False, (bias, noise.view(B, 1, Hh, W), nw))
        torch.cuda.synchronize()
    npart = part.shape[1]
    assert part.dtype == torch.float64 and tuple(part.shape) == (B, npart, C, 2) and part.is_contiguous()
    Lc = ER.conv_stats_chain(Hh, W, C, npart)
    y, mean, rstd = G((B, HW, C), c.dtype), G((B, C), F32), G((B, C), F32)
    wsb = L.sgx_gepi_ws_bytes(B, HW, C)
    ws = N.workspace(wsb, DEV)
    launch(c, lambda: L.sgx_gepi_fwd(p(yb), p(bias), p(noise), p(nw), p(style), p(y.t), p(mean.t), p(rstd.t), p(ws), wsb, p(part), npart, B, HW, C, flags, dtc(c), N.stream()))
    res = {}
    y64, b64, nz64, nw64 = yb.double().reshape(B, HW, C), d(bias), noise.double(), nw.double()
    sums, Ss = ER.activation_sums(y64, b64, nz64, nw64, True)
    got = part.sum(1)
    res["sum_a"] = SR.assert_elementwise(got[..., 0], sums[..., 0], Ss[..., 0], Lc + 4, torch.float64, f"{c.id} sum a")
    res["sum_a2"] = SR.assert_elementwise(got[..., 1], sums[..., 1], Ss[..., 1], Lc + 9, torch.float64, f"{c.id} sum a^2")
    check_stats(c, res, mean, rstd, y64, b64, nz64, nw64, flags, Lc)
    ref, S = ER.gepi_fwd(y64, b64, nz64, nw64, style.double(), mean.t.double(), rstd.t.double(), flags)
    res["y"] = elementwise(c, y, ref, S, ER.N_FWD, "y")
    return res


RUNNERS = {"sgx_conv3x3_stats": run_conv_stats, "sgx_gepi_fwd": run_fwd, "sgx_gepi_bwd": run_bwd, "sgx_gepi_stats": run_stats, "sgx_blur3x3_stats": run_blur_stats}


def run_case(c):
    """Run a row once in this process (whose environment must be the row's group) -> its figures."""
    if c.id not in RESULTS:
        N = native()
        with sticky(c.id):                                   # the operands, the call and the fp64 references alike
            res = RUNNERS[c.entry](N.lib(), N, c)
        RESULTS[c.id] = res
        rep = os.environ.get("SGX_EPILOGUE_REPORT")          # a measuring run keeps every figure
        if rep:
            with open(rep, "a") as f:
                f.write(json.dumps({"id": c.id, "entry": c.entry, **res}) + "\n")
    return RESULTS[c.id]


def main(group):
    for k, v in ER.GROUPS[group].items():
        assert os.environ.get(k) == v, f"{k} must be {v} for group {group}"
    for c in [c for c in ER.CASES if c.group == group]:
        try:
            print(json.dumps({"id": c.id, "ok": True, **run_case(c)}), flush=True)
        except AssertionError as e:
            print(json.dumps({"id": c.id, "ok": False, "error": str(e)[:600]}), flush=True)
            if _FAULT is not None:
                return 3
        except RuntimeError as e:                            # a HIP error: stop here
            print(json.dumps({"id": c.id, "ok": False, "error": "HIP: " + str(e)[:600]}), flush=True)
            return 3
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
