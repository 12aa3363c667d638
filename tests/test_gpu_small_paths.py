"""-m gpu: every launch path of the fp32 GEMM with its EqualizedLinear fusions, the grouped style affines, minibatch stddev and the logistic loss
head (csrc/small.hip) at the C ABI, one test per row of small_ref.CASES, in this process (small.hip has no process-wide switches).

Each row is one call through native.lib() under the library's profiler (epilogue_runner.profiled): the return code is 0, the kernels that
ran and their grids, blocks and dynamic LDS sizes are exactly what small_ref.plan restates from the row's arguments, every output -- C, the
split-K workspace, y, gx, dw, db, glm, dx, ddy, loss, g_fake, g_real -- is a streaming_ref.Guarded view pre-filled with NaN bytes whose bands
come back untouched, and the values meet small_ref's criteria: the exact value bit for bit on the integer rows, the per-element chain bound
against the fp64 restatement otherwise.  A row with an operand 4 bytes off must also give the aligned call's bits."""
import json
import os

import pytest
import torch

import epilogue_ref as ER
import epilogue_runner as ERUN
import small_ref as SM
import streaming_ref as SR
from epilogue_runner import DEV, native, p

pytestmark = pytest.mark.gpu
F32 = torch.float32
WORST = {}                          # entry point -> {output: worst err / bound}: printed per row, kept by a measuring run (SGX_SMALL_REPORT)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()
    rep = os.environ.get("SGX_SMALL_REPORT")
    if rep:
        with open(rep, "w") as f:
            json.dump(WORST, f, indent=1, sort_keys=True)


def note(c, what, ratio):
    w = WORST.setdefault(c.entry, {})
    what = f"{what} {'bf16' if c.dtype == torch.bfloat16 else 'fp32'}"
    if ratio >= w.get(what, (-1.0, ""))[0]:
        w[what] = (ratio, c.id)
    print(f"{c.id} {what}: err/bound {ratio:.3f}")


def put(t, shift=0):
    """An operand on the device; ``shift`` bytes off its 16-byte alignment when asked (a Guarded view is the shifted buffer)."""
    if t is None:
        return None
    g = SR.Guarded(t.shape, t.dtype, DEV, shift)
    g.t.copy_(t)
    assert g.t.data_ptr() % 16 == shift % 16
    return g.t


def G(shape, dtype=F32):
    return SR.Guarded(shape, dtype, DEV)


def launch(c, call, want=None):
    """The call under the profiler: rc 0 (profiled checks it), the row's kernels in order, the restated geometry."""
    ran = ERUN.profiled(c.id, c.entry, call)
    kernels, launches = want or SM.plan(c)
    assert tuple(ran) == tuple(c.kernels) == tuple(kernels), f"{c.id}: launched {ran}, the row says {c.kernels}, the rules {kernels} ({c.why})"
    got = [(tuple(g), tuple(b), int(lds)) for g, b, lds in native().prof_launches()]
    assert got == launches, f"{c.id}: launch geometry {got}, restated {launches}"


def d(t):
    return None if t is None else t.double()


def value(c, g, ref, S, n, what, act=0):
    """One output against its reference: bits on an integer row, the chain bound otherwise; then its guard bands."""
    ref = ref.reshape(g.t.shape)
    if c.args.get("data") == "int":
        r = SM.assert_bits(g.t, SR.act(ref, act) if act else ref, f"{c.id} {what}", rounded=bool(act))
    else:
        r = SM.check_act(g.t, ref, S.reshape(g.t.shape), n, act, f"{c.id} {what}")
    g.assert_intact(f"{c.id} {what}")
    note(c, what, r)


# ---------------------------------------------------------------------------------------------------------------- GEMM family
def run_gemm(L, N, c):
    a = c.args
    M, Nn, K, ta, tb = a["M"], a["N"], a["K"], a["ta"], a["tb"]
    o, pl = SM.gemm_operands(c), SM.gemm_plan_of(c)
    wsb = SM.gemm_ws_bytes(M, Nn, K)
    assert L.sgx_gemm_ws_bytes(M, Nn, K) == wsb
    given = {"full": wsb, "null": 0, "short": wsb - 4}[a["ws"]]
    ws = G((max(given, 16) // 4,)) if a["ws"] != "null" else None
    C = G((M, Nn))

    def call(A, B, out):
        return lambda: L.sgx_gemm_f32(p(A), p(B), p(out.t), M, Nn, K, ta, tb, o["alpha"], p(ws.t) if ws else None, given, N.stream())

    A, B = put(o["A"], 4 if "A" in a["shift"] else 0), put(o["B"], 4 if "B" in a["shift"] else 0)
    launch(c, call(A, B, C))
    ref, S = SM.gemm(A.double(), B.double(), ta, tb, o["alpha"])
    value(c, C, ref, S, SM.gemm_chain(pl), "C")
    if ws is not None:
        ws.assert_intact(f"{c.id} workspace")
        if pl.splits == 1:                                   # an unsplit launch does not touch the workspace it was offered
            assert bool((ws.buf == SR.SENTINEL).all()), f"{c.id}: the workspace was written by an unsplit launch"
        else:                                                # every partial written; on integers each is the exact sum over its split's k
            part = ws.t[:pl.splits * M * Nn].view(pl.splits, M, Nn)
            assert not bool(part.isnan().any()), f"{c.id}: {int(part.isnan().sum())} workspace partials unwritten"
            if a["data"] == "int":
                a64, b64 = (A.double().t() if ta else A.double()), (B.double().t() if tb else B.double())
                for z, sl in enumerate(SM.gemm_slices(K, pl.splits)):
                    k0, k1 = sl[0][0], max(sl[0][0], max(ke for _, ke in sl))
                    SM.assert_bits(part[z], a64[:, k0:k1] @ b64[k0:k1], f"{c.id} workspace partial {z} (k {k0}..{k1})")
    if a["shift"]:                                           # the aligned call: other kernel or other body, the same bits
        C2 = G((M, Nn))
        ERUN.profiled(c.id, c.entry, call(put(o["A"]), put(o["B"]), C2))
        assert torch.equal(C.t.view(torch.int32), C2.t.view(torch.int32)), f"{c.id}: the bits differ from the aligned call's"


def run_linear_fwd(L, N, c):
    a = c.args
    B, Nn, K = a["B"], a["N"], a["K"]
    o, pl = SM.gemm_operands(c), SM.gemm_plan_of(c)
    w, bias = put(o["w"]), put(o["bias"])
    call = lambda x, out: (lambda: L.sgx_linear_fwd(p(x), p(w), p(bias), p(out.t), B, Nn, K, o["w_mul"], o["b_mul"], a["act"], N.stream()))
    x, y = put(o["x"], 4 if a["shift"] else 0), G((B, Nn))
    launch(c, call(x, y))
    pre, S = SM.linear_fwd(x.double(), w.double(), d(bias), o["w_mul"], o["b_mul"])
    value(c, y, pre, S, SM.gemm_chain(pl, bias=a["bias"], act=a["act"]), "y", a["act"])
    if a["shift"]:
        y2 = G((B, Nn))
        ERUN.profiled(c.id, c.entry, call(put(o["x"]), y2))
        assert torch.equal(y.t.view(torch.int32), y2.t.view(torch.int32)), f"{c.id}: the bits differ from the aligned call's"


def run_linear_bwd_data(L, N, c):
    a = c.args
    B, Nn, K = a["B"], a["N"], a["K"]
    o, pl = SM.gemm_operands(c), SM.gemm_plan_of(c)
    gy, w = put(o["gy"]), put(o["w"])
    call = lambda m, out: (lambda: L.sgx_linear_bwd_data(p(gy), p(m), p(w), p(out.t), B, Nn, K, o["w_mul"], N.stream()))
    m, gx = put(o["y_act"], 4 if a["shift"] else 0), G((B, K))
    launch(c, call(m, gx))
    ref, S = SM.linear_bwd_data(gy.double(), d(m), w.double(), o["w_mul"])
    value(c, gx, ref, S, SM.gemm_chain(pl, mask=a["mask"]), "gx")
    if a["shift"]:
        g2 = G((B, K))
        ERUN.profiled(c.id, c.entry, call(put(o["y_act"]), g2))
        assert torch.equal(gx.t.view(torch.int32), g2.t.view(torch.int32)), f"{c.id}: the bits differ from the aligned call's"


def run_linear_bwd_param(L, N, c):
    a = c.args
    B, Nn, K = a["B"], a["N"], a["K"]
    o, pl = SM.gemm_operands(c), SM.gemm_plan_of(c)
    gy, m, x = put(o["gy"]), put(o["y_act"]), put(o["x"])
    dw, db = G((Nn, K)), (G((Nn,)) if a["db"] else None)
    launch(c, lambda: L.sgx_linear_bwd_param(p(gy), p(m), p(x), p(dw.t), p(db.t) if db else None, B, Nn, K, o["w_mul"], o["b_mul"], N.stream()))
    rw, Sw, rb, Sb = SM.linear_bwd_param(gy.double(), d(m), x.double(), o["w_mul"], o["b_mul"])
    value(c, dw, rw, Sw, SM.gemm_chain(pl, mask=a["mask"]), "dw")
    if db is not None:                                       # colsum: a sequential chain of the GEMM's K = B, the mask's rounding, cscale
        value(c, db, rb, Sb, B + 2, "db")


# ---------------------------------------------------------------------------------------------------------------- style affines
def run_style(L, N, c):
    a = c.args
    B, D, Ns, layers, Ln = a["B"], a["D"], a["Ns"], a["layers"], a["L"]
    Gn = len(Ns)
    o = SM.style_operands(c)
    lm, Ws, bs, gys = put(o["lm"]), [put(w) for w in o["Ws"]], [put(b) for b in o["biases"]], [put(g) for g in o["gys"]]
    yo, ti, no, tiles = SM.style_layout(Ns, B)
    bits = lambda v: int(torch.tensor(v, dtype=torch.float32).view(torch.int32))
    rows = [[Ws[g].data_ptr(), bs[g].data_ptr() if bs[g] is not None else 0, Ns[g], yo[g], ti[g], bits(o["w_muls"][g]), bits(o["b_muls"][g]), layers[g]] for g in range(Gn)]
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    gy = torch.cat([g.reshape(-1) for g in gys])
    ntot = sum(Ns)
    if c.entry == "sgx_style_fwd":
        y = G((B * ntot,))
        launch(c, lambda: L.sgx_style_fwd(p(lm), p(table), p(y.t), Gn, B, D, tiles, N.stream()))
        ref = torch.empty(B * ntot, dtype=torch.float64, device=DEV)
        S = torch.empty_like(ref)
        for g in range(Gn):
            r, s = SM.style_fwd(lm[layers[g]].double(), Ws[g].double(), d(bs[g]), o["w_muls"][g], o["b_muls"][g])
            ref[yo[g]:yo[g] + B * Ns[g]], S[yo[g]:yo[g] + B * Ns[g]] = r.reshape(-1), s.reshape(-1)
        value(c, y, ref, S, SM.style_chain(c.entry, B, D, max(Ns)), "y")
    elif c.entry == "sgx_style_bwd_data":
        glm = G((Ln, B, D))
        launch(c, lambda: L.sgx_style_bwd_data(p(gy), p(table), p(glm.t), Gn, B, D, max(Ns), N.stream()))
        glm.assert_intact(f"{c.id} glm")
        worst = 0.0
        for g in range(Gn):
            r, s = SM.style_bwd_data(gys[g].double(), Ws[g].double(), o["w_muls"][g])
            what = f"{c.id} glm[{layers[g]}] (group {g}, N = {Ns[g]})"
            if a["data"] == "int":
                SM.assert_bits(glm.t[layers[g]], r, what)
            else:
                worst = max(worst, SR.assert_elementwise(glm.t[layers[g]], r, s, SM.style_chain(c.entry, B, D, Ns[g]), F32, what))
        for l in set(range(Ln)) - set(layers):               # a layer without a group keeps its prior contents
            assert bool((glm.t[l].contiguous().view(torch.uint8) == SR.SENTINEL).all()), f"{c.id}: glm[{l}] has no group and was written"
        note(c, "glm", worst)
    else:
        dw, db = G((ntot, D)), (G((ntot,)) if a["db"] else None)
        launch(c, lambda: L.sgx_style_bwd_param(p(gy), p(lm), p(table), p(dw.t), p(db.t) if db else None, Gn, B, D, tiles, N.stream()))
        rw, Sw, rb, Sb = (torch.cat(t) for t in zip(*[SM.style_bwd_param(gys[g].double(), lm[layers[g]].double(), o["w_muls"][g], o["b_muls"][g]) for g in range(Gn)]))
        value(c, dw, rw, Sw, SM.style_chain(c.entry, B, D, 0), "dw")
        if db is not None:
            value(c, db, rb, Sb, B + 1, "db")


# ---------------------------------------------------------------------------------------------------------------- minibatch stddev
def run_mbstd(L, N, c):
    a = c.args
    B, HW, C, Cpad, dt = a["B"], a["HW"], a["C"], a["Cpad"], c.dtype
    o = SM.mbstd_operands(c)
    x, dy, ggx = put(o["x"]), put(o["dy"]), put(o["ggx"])
    dtc = 0 if dt == F32 else 1
    if c.entry == "sgx_mbstd_fwd":
        y = G((B, HW, Cpad), dt)
        launch(c, lambda: L.sgx_mbstd_fwd(p(x), p(y.t), B, HW, C, Cpad, dtc, N.stream()))
        st = SM.mbstd_stats(x.double())
        note(c, "stat", SM.check_padded(y.t, x, C, st.stat, st.dstat, B, C, f"{c.id} y"))
        y.assert_intact(f"{c.id} y")
    elif c.entry == "sgx_mbstd_bwd":
        dx = G((B, HW, C), dt)
        launch(c, lambda: L.sgx_mbstd_bwd(p(dy), p(x), p(dx.t), B, HW, C, Cpad, dtc, N.stream()))
        ref, bound = SM.mbstd_bwd(dy.double(), x.double(), C)
        note(c, "dx", ER.assert_within(dx.t, ref, SM.with_store(ref, bound, dt), f"{c.id} dx"))
        dx.assert_intact(f"{c.id} dx")
    else:
        ddy, gx = G((B, HW, Cpad), dt), G((B, HW, C), dt)
        launch(c, lambda: L.sgx_mbstd_bwd2(p(ggx), p(dy), p(x), p(ddy.t), p(gx.t), B, HW, C, Cpad, dtc, N.stream()))
        dstat, dstat_b, rg, bg = SM.mbstd_bwd2(ggx.double(), dy.double(), x.double(), C)
        note(c, "ddy", SM.check_padded(ddy.t, ggx, C, dstat, dstat_b, B, C, f"{c.id} ddy"))
        note(c, "gx", ER.assert_within(gx.t, rg, SM.with_store(rg, bg, dt), f"{c.id} gx"))
        ddy.assert_intact(f"{c.id} ddy")
        gx.assert_intact(f"{c.id} gx")


# ---------------------------------------------------------------------------------------------------------------- logistic head
def run_logistic(L, N, c):
    """Per element against fp64 softplus / sigmoid under small_ref.logistic's bound (expf 3 ulp, log1pf 2 ulp: an assumption, the HIP math
    documentation is not shipped with the ROCm tree).  Measured on the MI355X, worst err / bound over the nine rows: loss 0.075, g_fake 0.179,
    g_real 0.170."""
    a = c.args
    o = SM.logistic_operands(c)
    fake, real = put(o["fake"]), put(o["real"])
    nf, nr, scale = fake.numel(), (real.numel() if real is not None else 0), SR.f32(0.5)
    loss, gf, gr = G((1,)), G((nf,)), (G((nr,)) if nr else None)
    launch(c, lambda: L.sgx_logistic_loss(p(fake), nf, p(real), nr, scale, a["gen"], p(loss.t), p(gf.t), p(gr.t) if gr else None, N.stream()))
    rl, bl, rf, bf, rr, br = SM.logistic(fake.double(), d(real), scale, a["gen"])
    for g, ref, bound, what in ((loss, rl, bl, "loss"), (gf, rf, bf, "g_fake"), (gr, rr, br, "g_real")):
        if g is not None:
            assert bool(torch.isfinite(g.t).all()), f"{c.id} {what}: NaN or Inf"
            note(c, what, ER.assert_within(g.t, ref, bound, f"{c.id} {what}"))
            g.assert_intact(f"{c.id} {what}")


RUNNERS = {"sgx_gemm_f32": run_gemm, "sgx_linear_fwd": run_linear_fwd, "sgx_linear_bwd_data": run_linear_bwd_data, "sgx_linear_bwd_param": run_linear_bwd_param,
           "sgx_style_fwd": run_style, "sgx_style_bwd_data": run_style, "sgx_style_bwd_param": run_style, "sgx_mbstd_fwd": run_mbstd, "sgx_mbstd_bwd": run_mbstd,
           "sgx_mbstd_bwd2": run_mbstd, "sgx_logistic_loss": run_logistic}


@pytest.mark.parametrize("case", SM.CASES, ids=[c.id for c in SM.CASES])
def test_small_case(case):
    N = native()
    with ERUN.sticky(case.id):                              # the operands, the call and the fp64 references alike
        RUNNERS[case.entry](N.lib(), N, case)


# ---------------------------------------------------------------------------------------------------------------- the functional layer
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_matmul_fn_first_order_gradients(ta, tb):
    """MatMulFn.backward's transposition table at a ragged shape: gA = alpha gC op(B)^T and gB = alpha op(A)^T gC, each in the layout of its
    operand, per element against fp64.  Chains: the GEMM's, with the inner dimension N for gA and M for gB."""
    from stylegan.pytorch_amd import functional as Fn
    M, Nn, K, alpha = 19, 37, 45, SR.f32(0.37)
    with ERUN.sticky(f"matmul-t{ta}{tb}"):
        A = SM.rnd((K, M) if ta else (M, K), 71).to(DEV).requires_grad_(True)
        B = SM.rnd((Nn, K) if tb else (K, Nn), 72).to(DEV).requires_grad_(True)
        gC = SM.rnd((M, Nn), 73).to(DEV)
        C = Fn.MatMulFn.apply(A, B, ta, tb, alpha)
        gA, gB = torch.autograd.grad(C, (A, B), gC)
        a64, b64, g64 = A.detach().double(), B.detach().double(), gC.double()
        opA, opB = (a64.t() if ta else a64), (b64.t() if tb else b64)
        ref, S = SM.gemm(a64, b64, ta, tb, alpha)
        SR.assert_elementwise(C.detach(), ref, S, SM.gemm_chain(SM.gemm_plan(M, Nn, K, ta, tb)), F32, f"t{ta}{tb} C")
        rA, SA = alpha * (g64 @ opB.t()), alpha * (g64.abs() @ opB.abs().t())                  # [M][K]: d/d op(A)
        rB, SB = alpha * (opA.t() @ g64), alpha * (opA.abs().t() @ g64.abs())                  # [K][N]: d/d op(B)
        if ta:
            rA, SA = rA.t(), SA.t()
        if tb:
            rB, SB = rB.t(), SB.t()
        assert gA.shape == A.shape and gB.shape == B.shape
        SR.assert_elementwise(gA, rA, SA, SM.gemm_chain(SM.gemm_plan(M, K, Nn, 0, 0)), F32, f"t{ta}{tb} gA")
        SR.assert_elementwise(gB, rB, SB, SM.gemm_chain(SM.gemm_plan(K, Nn, M, 0, 0)), F32, f"t{ta}{tb} gB")
