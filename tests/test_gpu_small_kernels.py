"""-m gpu: the launch paths that the small-problem work added to csrc/small.hip and csrc/conv.hip, against fp64 on seeded inputs.

The changed kernels keep the arithmetic per output element they had (tools/small_probe.py compares two builds bit for bit), so
the bar here is the one tests/test_gpu_kernels.py holds the fp32 MFMA GEMM to (TIGHT = 2e-5 rel-L2: an exact fma chain in fp32
against fp64); the cases are the ones the new code decides on: K <= 4 (outer-product kernel, every ta, N a multiple of 4 or not),
K tails and row / column remainders of the 16x16-tile kernel in both of its instantiations (a wave's K slice below / at 128),
minibatch-stddev shapes whose loops end inside a batch of MBSTD_U elements, and weight tiles whose last rows lie beyond O."""
import pytest
import torch

import golden_util as gu
from gpu_util import DEV, assert_close
from oracle import stylegan_oracle as O

pytestmark = pytest.mark.gpu
TIGHT = 2e-5


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from stylegan.pytorch_amd import native
    assert torch.cuda.is_available()
    native.lib()


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


GEMM_CASES = [
    # (M, N, K, ta, tb)
    (4, 512, 1, 0, 0), (512, 8192, 4, 1, 0), (1, 512, 4, 1, 0), (33, 64, 3, 1, 0), (33, 64, 2, 0, 0), (7, 20, 4, 0, 0),   # outer products
    (5, 30, 3, 1, 0), (5, 30, 4, 0, 1), (19, 36, 4, 1, 1),                       # K <= 4 that stay on the tile kernel (N % 4, tb)
    (37, 50, 77, 0, 0), (37, 50, 77, 1, 1), (20, 33, 100, 1, 0), (20, 33, 100, 0, 1), (8, 48, 8, 1, 0),   # tails, remainders
    (4, 40, 512, 0, 0), (4, 40, 512, 0, 1), (9, 24, 520, 1, 0), (9, 24, 1030, 1, 1),   # slices of 128 and more (+ a tail)
    (4, 512, 8192, 0, 1), (4, 8192, 512, 0, 0),                                  # the discriminator's dense layer at batch 4
]


@pytest.mark.parametrize("M,N,K,ta,tb", GEMM_CASES)
def test_gemm_paths_match_fp64(M, N, K, ta, tb):
    from stylegan.pytorch_amd import functional as F
    A = gu.seeded((K, M) if ta else (M, K), 11).to(DEV)
    B = gu.seeded((N, K) if tb else (K, N), 12).to(DEV)
    C = F.MatMulFn.apply(A, B, ta, tb, 0.37)
    ref = 0.37 * (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    assert C.shape == ref.shape
    assert rel_l2(C, ref) <= TIGHT, (M, N, K, ta, tb, rel_l2(C, ref))


def test_outer_product_is_the_mfma_sum_bit_for_bit():
    """K <= 4: the outer-product kernel forms fma(a_k, b_k, acc) in k order from zero, which is what v_mfma_f32_16x16x4_f32 does with
    the other three k slots zero.  N = 30 keeps the same operands on the tile kernel: the common columns must be identical bits."""
    from stylegan.pytorch_amd import functional as F
    for K in (1, 2, 3, 4):
        A = gu.seeded((K, 45), 21).to(DEV)
        B32 = gu.seeded((K, 32), 22).to(DEV)
        B30 = B32[:, :30].contiguous()
        c32 = F.MatMulFn.apply(A, B32, 1, 0, 1.7)
        c30 = F.MatMulFn.apply(A, B30, 1, 0, 1.7)
        assert torch.equal(c32[:, :30], c30), K


@pytest.mark.parametrize("B,H,C", [(4, 4, 512), (8, 4, 24), (2, 4, 16), (4, 4, 2600), (16, 2, 72)])
def test_minibatch_stddev_fp32_forward_and_both_backwards(B, H, C):
    """As test_gpu_kernels.test_minibatch_stddev (same bars), at the batch-4 shape of the 1024x1024 discriminator and at shapes whose
    loops end inside a batch of MBSTD_U elements or run several of them."""
    from stylegan.pytorch_amd.CustomLayers import StddevLayer
    x = gu.seeded((B, C, H, H), 31)
    xg = x.to(DEV).requires_grad_(True)
    y = StddevLayer(4, 1)(xg)
    x64 = x.double().requires_grad_(True)
    y64 = O.minibatch_stddev(x64)
    assert_close(y, y64, 1e-6, "y")
    w = gu.seeded(y64.shape, 32)
    (g1,) = torch.autograd.grad((y * w.to(DEV)).sum(), xg, create_graph=True)
    (g64,) = torch.autograd.grad((y64 * w.double()).sum(), x64, create_graph=True)
    assert_close(g1, g64, 1e-5, "dx")
    if B == 2:
        # group of 2: d0 = -d1 and the statistic is |d|, whose second derivative is zero; what the fp64 reference holds is the residue of
        # the 1e-8 under the root (|ref| ~ 1e-3 against terms of order 1), which no fp32 evaluation follows to a relative bar.  The
        # existing suite keeps its one such case; here the group of 2 checks the loops' remainders on y and dx only.
        return
    (g1 * g1).sum().backward(); (g64 * g64).sum().backward()
    assert_close(xg.grad, x64.grad, 1e-4, "second order")


@pytest.mark.parametrize("B,H,C", [(4, 4, 512), (8, 4, 24)])
def test_minibatch_stddev_bf16(B, H, C):
    """bf16 storage: the inputs are bf16 values, so the only error of y is the rounding of each output (2^-9 relative per element);
    dx carries the rounding of the incoming gradient and of the result, and its statistic term is formed from the rounded
    gradient: three roundings of 2^-9, bar 2^-7."""
    from stylegan.pytorch_amd.CustomLayers import StddevLayer
    x = gu.seeded((B, C, H, H), 31).to(torch.bfloat16)
    xg = x.to(DEV).requires_grad_(True)
    y = StddevLayer(4, 1)(xg)
    x64 = x.double().requires_grad_(True)
    y64 = O.minibatch_stddev(x64)
    assert_close(y.float(), y64, 2.0 ** -8, "y")
    w = gu.seeded(y64.shape, 32)
    (g1,) = torch.autograd.grad((y.float() * w.to(DEV)).sum(), xg)
    (g64,) = torch.autograd.grad((y64 * w.double()).sum(), x64)
    assert_close(g1.float(), g64, 2.0 ** -7, "dx")


@pytest.mark.parametrize("O_,I_,mode", [(32, 32, 0), (48, 32, 0), (40, 64, 0), (16, 32, 1), (80, 32, 2)])
def test_pack_weight_tiles_with_rows_beyond_O(O_, I_, mode):
    """The 16-byte tile loads clamp the row and zero the value: forward pack of the 3x3 / folded 4x4 taps against the formula."""
    from stylegan.pytorch_amd import native as N
    w = gu.seeded((O_, I_, 3, 3), 41).to(DEV)
    taps = 9 if mode == N.PACK_S else 16
    fwd = torch.full((taps, O_, I_), float("nan"), device=DEV)
    adj = torch.full((taps, I_, O_), float("nan"), device=DEV)
    N.check(N.lib().sgx_pack_weight(N.ptr(w), N.ptr(fwd), N.ptr(adj), O_, I_, I_, mode, 0.5, N.F32, N.stream()), "sgx_pack_weight")
    w64 = w.double().cpu()
    if mode == N.PACK_S:
        ref = 0.5 * w64.permute(2, 3, 0, 1).reshape(9, O_, I_)
        ref_adj = ref.flip(0).transpose(1, 2)
    else:
        pad = torch.nn.functional.pad(w64, (1, 1, 1, 1))
        k4 = pad[:, :, 1:, 1:] + pad[:, :, :-1, 1:] + pad[:, :, 1:, :-1] + pad[:, :, :-1, :-1]      # [O][I][4][4]
        ref = 0.5 * (0.25 if mode == N.PACK_D else 1.0) * k4.permute(2, 3, 0, 1).reshape(16, O_, I_)
        ref_adj = ref.transpose(1, 2)
    assert rel_l2(fwd, ref) <= 1e-6
    assert rel_l2(adj, ref_adj) <= 1e-6
