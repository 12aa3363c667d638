"""-m gpu: the multi-tensor optimizer kernels (csrc/optim.hip) at the C ABI: sgx_gradnorm_clip_coef on integer-valued gradients, whose sum of
squares is exact in every order, at every loop of sumsq_stage1; sgx_adam_multi / sgx_ema_multi per element against fp64 for the parameter and
both moments, past the first grid-stride trip.  Outputs sit in guard-banded buffers; the library's profiler names the kernels that ran."""
import numpy as np
import pytest
import torch

import epilogue_ref as ER
import epilogue_runner as RUN
import streaming_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32


def _native():
    from stylegan.pytorch_amd import native
    return native


def table(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def sizes_of(ts):
    return torch.tensor([t.numel() for t in ts], dtype=torch.int64, device=DEV)


def profiled(N, entry, call):
    ran = tuple(RUN.profiled(entry, entry, call))
    assert ran == ER.OPTIM_KERNELS[entry], (entry, ran)


def int_grad(n, shift, seed):
    """Integers in [-2, 2] as fp32, optionally starting 4 bytes into a 16-byte aligned buffer (a bucket view)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = torch.zeros(n + 4, dtype=F32, device=DEV)
    v = buf[shift:shift + n]
    v.copy_(torch.randint(-2, 3, (n,), generator=g, device=DEV).float())
    v[:1].copy_(torch.where(v[:1] == 0, 1.0, v[:1]))         # never all zero: the norm is at least 1
    assert v.data_ptr() % 16 == 4 * shift
    return v


def gradnorm(N, grads, max_norm):
    L = N.lib()
    out = SR.Guarded((2,), F32, DEV)
    partial = SR.Guarded((len(grads) * 32,), torch.float64, DEV)
    ptrs, sizes = table(grads), sizes_of(grads)
    profiled(N, "sgx_gradnorm_clip_coef", lambda: L.sgx_gradnorm_clip_coef(ptrs.data_ptr(), sizes.data_ptr(), len(grads), max_norm, partial.t.data_ptr(), out.t.data_ptr(), N.stream()))
    out.assert_intact("out"); partial.assert_intact("partial")
    return out.t


def check_norm(out, grads, max_norm, what):
    exact = sum(int((g.double() ** 2).sum().item()) for g in grads)
    assert exact < 1 << 24, "the total stays exact in fp32"
    assert float(out[0]) == float(exact), f"{what}: sum of squares {float(out[0])!r}, exact {exact}"
    # out[1] = min(1, max_norm / (sqrt(total) + 1e-6)) in fp32: the root (rounded from fp64), the sum, the division
    coef = SR.f32(max_norm) / (float(exact) ** 0.5 + SR.f32(1e-6))
    want = min(1.0, coef)
    assert abs(float(out[1]) - want) <= 5 * SR.U32 * want, f"{what}: clip coefficient {float(out[1])!r}, expected {want!r}"
    if coef >= 1.0 + 1e-5:
        assert float(out[1]) == 1.0, what
    return exact ** 0.5


@pytest.mark.parametrize("n,shift,why", ER.GRADNORM_SIZES, ids=[f"n{n}{'-misaligned' if s else ''}" for n, s, _ in ER.GRADNORM_SIZES])
def test_gradnorm_one_tensor_is_exact(n, shift, why):
    N = _native()
    with RUN.sticky(f"gradnorm n = {n}"):
        g = [int_grad(n, shift, 7 + n % 97)]
        norm = float((g[0].double() ** 2).sum().item()) ** 0.5
        assert norm >= 1.0
        for factor in (0.5, 2.0):                           # max_norm relative to the exact norm: the norm above it (out[1] = 1 / 2) and below (1)
            out = gradnorm(N, g, factor * norm)
            check_norm(out, g, factor * norm, f"n = {n} ({why}), max_norm {factor} x the norm")
            assert (float(out[1]) < 0.6) if factor < 1 else (float(out[1]) == 1.0), (n, factor, float(out[1]))


def test_gradnorm_many_tensors_is_exact():
    """All the sizes at once, and 13 tensors: 416 partials, so stage 2's 256 threads take a second trip."""
    N = _native()
    with RUN.sticky("gradnorm, 13 tensors"):
        gs = [int_grad(n, s, 11 + i) for i, (n, s, _) in enumerate(ER.GRADNORM_SIZES)] + [int_grad(n, 0, 40 + n) for n in (5, 260, 70001)]
        assert len(gs) * 32 > 256
        for max_norm in (1.0, 1e6):
            check_norm(gradnorm(N, gs, max_norm), gs, max_norm, f"{len(gs)} tensors, max_norm {max_norm}")
        assert float(gradnorm(N, gs, 1.0)[1]) < 1.0


def filled(vals):
    """Guard-banded in-place operands holding ``vals``."""
    out = []
    for v in vals:
        g = SR.Guarded(v.shape, F32, DEV)
        g.t.copy_(v)
        out.append(g)
    return out


def rnd(n, seed, scale=1.0):
    return scale * torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


@pytest.mark.parametrize("beta1", [0.0, 0.9])
@pytest.mark.parametrize("scaled", [False, True], ids=["grad_scale-null", "grad_scale"])
def test_adam_multi_per_element(beta1, scaled):
    """One tensor of one element, the last size of a single grid-stride trip (65 536), the first of two, and a 512 x 512 x 3 x 3 weight;
    non-zero moments, a step size and bias correction of its own per tensor."""
    with RUN.sticky(f"adam beta1 = {beta1}"):
        _adam(beta1, scaled)


def _adam(beta1, scaled):
    N = _native(); L = N.lib()
    ns = ER.ADAM_SIZES
    p0 = [rnd(n, 200 + i) for i, n in enumerate(ns)]
    g = [rnd(n, 210 + i, 20.0) for i, n in enumerate(ns)]
    m0 = [rnd(n, 220 + i, 3.0) for i, n in enumerate(ns)]
    v0 = [rnd(n, 230 + i, 5.0) ** 2 for i, n in enumerate(ns)]
    beta2, eps = 0.99, 1e-8
    steps = np.float32([0.003 / (1 - 0.9 ** (i + 1)) for i in range(len(ns))])
    bc2 = np.float32([(1 - 0.99 ** (i + 1)) ** 0.5 for i in range(len(ns))])
    gscale = torch.tensor([0.37], device=DEV) if scaled else None
    P, M, V = filled(p0), filled(m0), filled(v0)
    tp, tg, tm, tv, sz = table([x.t for x in P]), table(g), table([x.t for x in M]), table([x.t for x in V]), sizes_of(g)
    sd, bd = torch.tensor(steps, device=DEV), torch.tensor(bc2, device=DEV)
    profiled(N, "sgx_adam_multi", lambda: L.sgx_adam_multi(tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(), sz.data_ptr(), len(ns), beta1, beta2, eps,
                                                           sd.data_ptr(), bd.data_ptr(), None if gscale is None else gscale.data_ptr(), N.stream()))
    gs = float(gscale.double().item()) if scaled else 1.0
    for i, n in enumerate(ns):
        (rp, rm, rv), (Sp, Sm, Sv) = ER.adam(p0[i].double(), g[i].double(), m0[i].double(), v0[i].double(), beta1, beta2, SR.f32(eps), float(steps[i]), float(bc2[i]), gs)
        for what, got, ref, S, nt in (("exp_avg", M[i], rm, Sm, ER.N_ADAM_M), ("exp_avg_sq", V[i], rv, Sv, ER.N_ADAM_V), ("p", P[i], rp, Sp, ER.N_ADAM_P)):
            r = SR.assert_elementwise(got.t, ref, S, nt, F32, f"adam tensor {i} (n = {n}) {what}")
            got.assert_intact(f"adam tensor {i} {what}")
            print(f"adam beta1={beta1} n={n} {what}: worst err/bound {r:.3f}")
        assert not torch.equal(P[i].t, p0[i]), "the step moved the parameter"


def test_ema_multi_per_element():
    with RUN.sticky("ema"):
        _ema()


def _ema():
    N = _native(); L = N.lib()
    ns = ER.ADAM_SIZES
    a0, b = [rnd(n, 300 + i) for i, n in enumerate(ns)], [rnd(n, 310 + i) for i, n in enumerate(ns)]
    A = filled(a0)
    ta, tb, sz = table([x.t for x in A]), table(b), sizes_of(b)
    beta = 0.999
    profiled(N, "sgx_ema_multi", lambda: L.sgx_ema_multi(ta.data_ptr(), tb.data_ptr(), sz.data_ptr(), len(ns), beta, N.stream()))
    for i, n in enumerate(ns):
        ref, S = ER.ema(a0[i].double(), b[i].double(), beta)
        r = SR.assert_elementwise(A[i].t, ref, S, ER.N_EMA, F32, f"ema tensor {i} (n = {n})")
        A[i].assert_intact(f"ema tensor {i}")
        print(f"ema n={n}: worst err/bound {r:.3f}")
