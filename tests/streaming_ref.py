"""fp64 restatements of the streaming (bandwidth-class) entry points of libsgx_hip.so -- csrc/pointwise.hip and the R1 head / PixelNorm
pieces of csrc/small.hip -- written from their definitions in include/sgx.h, the per-element error criterion they are held to, guard-banded
output buffers, and the table of cases that walks every launch path of their C++ launchers.  Test-side only: the product never imports this,
and nothing here calls the library under test.

Layout conventions are the library's: activations NHWC, RGB images fp32 [.., 3], parameters fp32.  Every reference takes fp64 tensors (on any
device; the big cases run them on the GPU with torch's own fp64 ops) and returns ``(ref, S)``: the value, and the same expression evaluated
on the absolute values of inputs and coefficients.  ``S`` is the per-element scale of the fp32 arithmetic error: a kernel that evaluates the
expression in fp32 with a longest chain of ``n`` operations is within ``n * 2^-24 * S`` of ``ref`` to first order (each rounding is
relative to a partial result that is bounded by the same partial expression on absolute values).  Coefficients are given as the fp32
values the C ABI receives (``f32()``)."""
import json
import math
import os
from collections import namedtuple

import numpy as np
import torch

U32 = 2.0 ** -24                    # unit roundoff of fp32 (round to nearest)
R_BF16 = 2.0 ** -8                  # half a bf16 ulp relative to the value, at most: ulp = 2^(e-7) for |v| in [2^e, 2^(e+1))
LRELU = float(np.float32(0.2))      # the slope as the kernels hold it
GUARD = 256                         # bytes of sentinel on each side of an output
SENTINEL = 0xFF                     # every byte: fp32 0xFFFFFFFF and bf16 0xFFFF are NaNs, so an unwritten element fails the value check


def f32(v):
    """A Python float rounded to fp32, as a c_float argument arrives in the library."""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------- the criterion
def assert_elementwise(got, ref, S, nterms, out_dtype, what=""):
    """Every element: |got - ref| <= r |ref| + (nterms + 2) 2^-24 S.

    The kernels compute in fp32 and round once on the store.  The fp32 value is within nterms * 2^-24 * S of ref (first order, see the module
    docstring; the + 2 covers the second-order terms (1 + u)^n - 1 - n u for every n used here, n u << 1, and the one rounding of an fp32
    store of a value that was accumulated in fp64).  A bf16 store then moves it by at most half a bf16 ulp, r = 2^-8 of the value; fp32
    outputs have r = 0.  Written as ``not (err <= bound).all()``: a NaN (an unwritten sentinel, a poisoned lane) fails."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(S.shape), (what, tuple(got.shape), tuple(ref.shape), tuple(S.shape))
    r = R_BF16 if out_dtype == torch.bfloat16 else 0.0
    g = got.detach().to(torch.float64)
    ref = ref.to(g.device)
    err = (g - ref).abs_()
    bound = ref.abs().mul_(r).add_(S.to(g.device), alpha=(nterms + 2) * U32)
    ok = err <= bound
    if not bool(ok.all()):
        bad = (~ok).flatten().nonzero().flatten()
        first = int(bad[0])
        coords = tuple(int(v) for v in np.unravel_index(first, tuple(got.shape))) if got.dim() else ()
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements outside the bound; first at flat index {first} {coords}: got "
                             f"{float(g.flatten()[first])!r}, ref {float(ref.flatten()[first])!r}, err {float(err.flatten()[first]):.3e} > "
                             f"bound {float(bound.flatten()[first]):.3e}")
    return float((err / bound.clamp_min(1e-300)).max()) if got.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------- guard bands
class Guarded:
    """An output tensor that is a view into a larger byte buffer: GUARD sentinel bytes in front of it and at least GUARD behind it, the
    output itself pre-filled with the sentinel.  ``shift`` bytes move the view off its 16-byte alignment (0: the view keeps the
    allocation's alignment, GUARD being a multiple of 256).  An overrun lands in this allocation."""

    def __init__(self, shape, dtype, device, shift=0):
        shape = tuple(int(s) for s in shape)
        es = torch.empty((), dtype=dtype).element_size()
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * es
        assert shift % es == 0
        self.lo = GUARD + shift
        total = (self.lo + self.nbytes + GUARD + 255) // 256 * 256
        self.buf = torch.full((total,), SENTINEL, dtype=torch.uint8, device=device)
        self.t = self.buf[self.lo:self.lo + self.nbytes].view(dtype).view(shape)

    def assert_intact(self, what=""):
        for name, band in (("front", self.buf[:self.lo]), ("back", self.buf[self.lo + self.nbytes:])):
            hit = (band != SENTINEL).nonzero().flatten()
            assert hit.numel() == 0, (f"{what}: {hit.numel()} bytes of the {name} guard band overwritten, first at byte "
                                      f"{int(hit[0]) - (self.lo if name == 'front' else 0)} relative to the output's "
                                      f"{'start' if name == 'front' else 'end'}")


# ---------------------------------------------------------------------------------------------------------------- references
def _slope(z):
    return torch.where(z > 0, 1.0, LRELU).to(z.dtype)


def act(t, kind):
    """SGX_ACT_NONE / LRELU / RELU."""
    if kind == 0:
        return t
    return torch.where(t > 0, t, (LRELU if kind == 1 else 0.0) * t)


def bias_act(x, bias, bscale, kind):
    """y = act(x + bscale * bias[c]); |act(a) - act(b)| <= |a - b|, so S is that of the sum."""
    if bias is None:
        return act(x, kind), x.abs()
    return act(x + bscale * bias, kind), x.abs() + abs(bscale) * bias.abs()


def lrelu_bwd(dy, mask, slope, scale):
    """dx = scale * dy * (mask ? 1 : slope); mask = (y > 0) as a bool tensor."""
    ref = scale * dy * torch.where(mask, 1.0, slope).to(dy.dtype)
    return ref, ref.abs()


def unpack_bits(bits, C):
    """bits[..., C / 8] bytes -> bool [..., C]: bit j of byte v = channel 8 v + j."""
    b = (bits.to(torch.int32).unsqueeze(-1) >> torch.arange(8, device=bits.device, dtype=torch.int32)) & 1
    return b.reshape(*bits.shape[:-1], C).bool()


def pack_bits(mask):
    """bool [..., C] -> uint8 [..., C / 8], the layout sgx_conv3x3_signbits writes."""
    m = mask.reshape(*mask.shape[:-1], mask.shape[-1] // 8, 8).to(torch.int32)
    return (m << torch.arange(8, device=mask.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


def axpby(a, b, alpha, beta):
    if b is None:
        return alpha * a, abs(alpha) * a.abs()
    return alpha * a + beta * b, abs(alpha) * a.abs() + abs(beta) * b.abs()


def _blur121(x):
    """[1,2,1] x [1,2,1] / 16, zero padded, NHWC (the same map as oracle.stylegan_oracle.blur3 on NCHW; tests/test_streaming_coverage.py
    checks the two against each other)."""
    p = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    h = p[:, :, :-2] + 2.0 * p[:, :, 1:-1] + p[:, :, 2:]
    return (h[:, :-2] + 2.0 * h[:, 1:-1] + h[:, 2:]) / 16.0


def blur3x3(x, z, mode):
    """mode 0: blur(x); 1: blur(lrelu(x)); 2: blur(x) * slope(z); 3: blur(x * slope(z)).  z: the pre-activation, or a bool mask (z > 0)."""
    sl = None if z is None else (torch.where(z, 1.0, LRELU).to(x.dtype) if z.dtype == torch.bool else _slope(z))
    pre = act(x, 1) if mode == 1 else (x * sl if mode == 3 else x)
    ref, S = _blur121(pre), _blur121(pre.abs())
    if mode == 2:
        ref, S = ref * sl, S * sl
    return ref, S


def blur_kxk(x, taps, K, pad, OH, OW):
    """y[oy][ox] = sum_{i,j} taps[i*K+j] * x[oy+i-pad][ox+j-pad], zero outside."""
    p = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    ref = torch.zeros(x.shape[0], OH, OW, x.shape[3], dtype=x.dtype, device=x.device)
    S = torch.zeros_like(ref)
    for i in range(K):
        for j in range(K):
            t = float(taps[i * K + j])
            ref += t * p[:, i:i + OH, j:j + OW]
            S += abs(t) * p[:, i:i + OH, j:j + OW].abs()
    return ref, S


def pool2(x, scale):
    s = lambda v: (v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])
    return scale * s(x), abs(scale) * s(x.abs())


def nearest_up2(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def up2(x, scale):
    ref = scale * nearest_up2(x)
    return ref, ref.abs()


def up2_add(x, a, scale):
    u = scale * nearest_up2(x)
    return a + u, a.abs() + u.abs()


def downsample_fade_rgb(x, alpha, beta):
    m, ma = pool2(x, 0.25)
    return alpha * x + beta * nearest_up2(m), abs(alpha) * x.abs() + abs(beta) * nearest_up2(ma)


def images_u8(src, flip, chw):
    """(v / 255 - 0.5) / 0.5 per byte, NHWC out; flip[b] mirrors image b.  src: uint8 [B][H][W][3] or [B][3][H][W]."""
    v = src.to(torch.float64)
    if chw:
        v = v.permute(0, 2, 3, 1)
    if flip is not None:
        v = torch.where(flip.to(v.device).bool().view(-1, 1, 1, 1), v.flip(2), v)
    v = v.contiguous()
    return (v / 255.0 - 0.5) / 0.5, (v / 255.0 + 0.5) / 0.5


def colsum(x, scale):
    """out[c] = scale * sum_p x[p][c], x: [npix][C]."""
    return scale * x.sum(0), abs(scale) * x.abs().sum(0)


def rgb_weight(w, sj, sc, C):
    """W(j, c) = w[j*sj + c*sc] as a [3][C] view of the flat parameter."""
    return torch.as_strided(w, (3, C), (sj, sc))


def rgb_in(img, w, sj, sc, wscale, bias, C, add=None):
    """y[p][c] = bias[c] + sum_j img[p][j] * (wscale * W(j, c)) (+ add[p][c])."""
    W = wscale * rgb_weight(w, sj, sc, C)
    ref, S = img @ W, img.abs() @ W.abs()
    if bias is not None:
        ref, S = ref + bias, S + bias.abs()
    if add is not None:
        ref, S = ref + add, S + add.abs()
    return ref, S


def rgb_out(x, w, sj, sc, wscale, bias, C, low=None, alpha=1.0, beta=0.0, BHW=None):
    """img[p][j] = alpha * (bias[j] + sum_c x[p][c] * wscale * W(j, c)) + beta * nearest_up2(low)[p][j]."""
    W = (alpha * wscale) * rgb_weight(w, sj, sc, C)
    ref, S = x @ W.t(), x.abs() @ W.abs().t()
    if bias is not None:
        ref, S = ref + alpha * bias, S + abs(alpha) * bias.abs()
    if low is not None:
        B, H, Wd = BHW
        u = beta * nearest_up2(low).reshape(B * H * Wd, 3)
        ref, S = ref + u, S + u.abs()
    return ref, S


def rgb_wgrad(img, f, sj, sc, wscale, C):
    """dw[j*sj + c*sc] = wscale * sum_p img[p][j] * f[p][c], returned in the flat parameter layout (3 * C values)."""
    g, ga = wscale * (img.t() @ f), abs(wscale) * (img.abs().t() @ f.abs())          # [3][C]
    ref = torch.zeros(3 * C, dtype=f.dtype, device=f.device)
    S = torch.zeros_like(ref)
    rgb_weight(ref, sj, sc, C).copy_(g)
    rgb_weight(S, sj, sc, C).copy_(ga)
    return ref, S


def sumsq(x):
    r = (x * x).sum().reshape(1)
    return r, r.clone()


def scale_dev(x, s, alpha):
    ref = (alpha * s) * x
    return ref, ref.abs()


def pixelnorm_fwd(x):
    r = torch.rsqrt((x * x).mean(1, keepdim=True) + 1e-8)
    ref = x * r
    return ref, ref.abs()


def pixelnorm_bwd(dy, x):
    """dx = dy r - x r^3 <x, dy> / C  (the derivative of x * rsqrt(mean(x^2) + eps))."""
    C = x.shape[1]
    r = torch.rsqrt((x * x).mean(1, keepdim=True) + 1e-8)
    ref = dy * r - x * (r ** 3 * (x * dy).sum(1, keepdim=True) / C)
    S = dy.abs() * r + x.abs() * (r ** 3 * (x * dy).abs().sum(1, keepdim=True) / C)
    return ref, S


def fade_rgb_bwd2(ggy, ggp, mask, wr, ws, alpha, beta_dev):
    """The three passes sgx_fade_rgb_bwd2 replaces, in exact arithmetic: (alpha ggy) slope(mask) + [beta] ws ggp . wr^T  (wr: [C][3])."""
    t1, s1 = lrelu_bwd(ggy, mask, LRELU, alpha)
    t2 = ggp @ (ws * wr).t()
    s2 = ggp.abs() @ (abs(ws) * wr.abs()).t()
    if beta_dev is not None:
        t2, s2 = beta_dev * t2, abs(beta_dev) * s2
    return t1 + t2, s1 + s2


def epilogue_x2(y, ebias, noise, nw, style, mean, rstd):
    """The generator's last layer epilogue as sgx_rgb_out_epi / sgx_rgb_wgrad_epi apply it per element (include/sgx.h): t = lrelu(y + ebias[c]
    + nw[c] noise[b][p]), x2 = (t - mean[b][c]) rstd[b][c] (style[b][c] + 1) + style[b][C + c], with mean / rstd GIVEN.  y: [B][HW][C],
    noise: [B][HW], style: [B][2C].  -> (x2, the same on absolute values)."""
    C = y.shape[2]
    pre = y + nw * noise.unsqueeze(-1)
    pa = y.abs() + nw.abs() * noise.abs().unsqueeze(-1)
    if ebias is not None:
        pre, pa = pre + ebias, pa + ebias.abs()
    t = act(pre, 1)
    A = (rstd * (style[:, :C] + 1.0)).unsqueeze(1)
    Aa = (rstd.abs() * (style[:, :C].abs() + 1.0)).unsqueeze(1)
    return (t - mean.unsqueeze(1)) * A + style[:, C:].unsqueeze(1), (pa + mean.abs().unsqueeze(1)) * Aa + style[:, C:].abs().unsqueeze(1)


def rgb_out_epi(x2, x2a, w, sj, sc, wscale, rbias, low, alpha, beta, BHW):
    """img = alpha (wscale W x2 + rbias) + beta nearest_up2(low), x2 from epilogue_x2."""
    B, H, Wd = BHW
    C = x2.shape[2]
    ref, S = rgb_out(x2.reshape(B * H * Wd, C), w, sj, sc, wscale, rbias, C, low, alpha, beta, BHW)
    _, S = rgb_out(x2a.reshape(B * H * Wd, C), w, sj, sc, wscale, rbias, C, low, alpha, beta, BHW)
    return ref, S


def rgb_wgrad_epi(x2, x2a, g, sj, sc, scale, bscale):
    """dw[j*sj + c*sc] = scale sum_p g[p][j] x2[p][c] in the parameter layout, db[j] = bscale sum_p g[p][j]; g: [B][HW][3]."""
    C = x2.shape[2]
    ref, _ = rgb_wgrad(g.reshape(-1, 3), x2.reshape(-1, C), sj, sc, scale, C)
    _, S = rgb_wgrad(g.reshape(-1, 3), x2a.reshape(-1, C), sj, sc, scale, C)
    return ref, S, bscale * g.sum((0, 1)), abs(bscale) * g.abs().sum((0, 1))


# ---------------------------------------------------------------------------------------------------------------- kernel names
def kernel_id(name):
    """The demangled name native.prof_records() returns -> the instantiation as the source spells it: no return type, no parameter list,
    bf16_t for its underlying unsigned short."""
    n = name[5:] if name.startswith("void ") else name
    return n.split("(")[0].replace("unsigned short", "bf16_t").strip()


def tname(dtype):
    return "float" if dtype == torch.float32 else "bf16_t"


# ---------------------------------------------------------------------------------------------------------------- launch geometry
# tests/golden/streaming_launch.json: {row id: [[kernel id, grid x, y, z, block x, y, z, dynamic LDS bytes], ...]}, every launch a row makes
# through a launch() helper of the GPU tests, in order, as tests/streaming_runner.py --write-geometry recorded it.  None of these launchers
# sizes a grid from the device, so a row is a function of its arguments and the environment.
GEOMETRY_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "streaming_launch.json")
RECORDER = None                     # tests/streaming_runner.py: a function (row id, launches) that takes the launches in place of the comparison
_geometry, _cursor = None, {}


def check_geometry(row, kernels, launches):
    """One profiled call of a row: kernel_id() of its launches and native.prof_launches() of the same records against the fixture.  A row's
    calls follow each other in the fixture (the cursor starts over when a row is run again); a row id the fixture does not have fails."""
    global _geometry
    got = [[k, *g, *b, int(lds)] for k, (g, b, lds) in zip(kernels, launches)]
    assert len(got) == len(kernels) == len(launches), (row, kernels, launches)
    if RECORDER is not None:
        return RECORDER(row, got)
    if _geometry is None:
        with open(GEOMETRY_PATH) as f:
            _geometry = json.load(f)
    assert row in _geometry, f"{row}: no row in tests/golden/streaming_launch.json"
    want = _geometry[row]
    at = _cursor.get(row, 0)
    at = 0 if at >= len(want) else at
    assert got == want[at:at + len(got)], f"{row}: launched {got}, recorded {want[at:at + len(got)]} (launches {at}.. of the row)"
    _cursor[row] = at + len(got)


# ---------------------------------------------------------------------------------------------------------------- the case table
# entry: the C ABI function; dtype: of the activations; args: what the runner of that entry in tests/test_gpu_streaming_kernels.py reads;
# kernels: kernel_id() of every launch the call is expected to make, in order; why: the launcher rule that selects them for this shape.
Case = namedtuple("Case", "id entry dtype args kernels why")
F, H = torch.float32, torch.bfloat16
CASES = []


def _case(id, entry, dtype, kernels, why, **args):
    CASES.append(Case(id.replace("bf16_t", "bf16").replace("float", "f32"), entry, dtype, args, tuple(kernels), why))


def _ve(dt):
    return 4 if dt == F else 8


BIG_NPIX = 32 * 1024 * 1024         # the headline batch-32 shape: 32 x 1024^2 pixels x 16 bf16 channels = 2^29 elements
BIG = dict(B=32, H=1024, W=1024, C=16)
BLUR_LANES8 = 256 * 512             # blur_launch: fewer strip lanes than this take the 2-row kernel
COLSUM_BLOCKS = 1024

# ---- sgx_bias_act
_case("bias_act-f32-C3-scalar", "sgx_bias_act", F, ["bias_act_scalar_kernel"], "fp32 with C % 4 != 0", npix=211, C=3, act=1)
_case("bias_act-f32-C1-scalar-nobias", "sgx_bias_act", F, ["bias_act_scalar_kernel"], "fp32 with C % 4 != 0, bias NULL", npix=7, C=1, act=0, bias=False)
for _a in (0, 1, 2):
    _case(f"bias_act-f32-C20-act{_a}", "sgx_bias_act", F, ["bias_act_kernel<float>"], "fp32 C % 4 == 0; 5 vectors per pixel, 2 blocks", npix=53, C=20, act=_a)
    _case(f"bias_act-bf16-C24-act{_a}", "sgx_bias_act", H, ["bias_act_kernel<bf16_t>"], "bf16 C % 8 == 0; 3 vectors per pixel, 2 blocks", npix=87, C=24, act=_a)
_case("bias_act-bf16-C8-nobias", "sgx_bias_act", H, ["bias_act_kernel<bf16_t>"], "bias NULL", npix=5, C=8, act=2, bias=False)
_case("bias_act-bf16-headline", "sgx_bias_act", H, ["bias_act_kernel<bf16_t>"], "uncapped grid_all: 262144 blocks", npix=BIG_NPIX, C=16, act=1)

# ---- sgx_lrelu_bwd / sgx_lrelu_bwd_bits
for _dt in (F, H):
    _t = tname(_dt)
    _case(f"lrelu_bwd-{_t}", "sgx_lrelu_bwd", _dt, [f"lrelu_bwd_kernel<{_t}>"], "one kernel per dtype; 2 blocks, partial last block", n=_ve(_dt) * 261, slope=0.2, scale=0.7)
    _case(f"lrelu_bwd-{_t}-relu-one-vector", "sgx_lrelu_bwd", _dt, [f"lrelu_bwd_kernel<{_t}>"], "slope 0 (ReLU), scale 1, a single vector", n=_ve(_dt), slope=0.0, scale=1.0)
    _case(f"lrelu_bwd-{_t}-scale_dev", "sgx_lrelu_bwd", _dt, [f"lrelu_bwd_kernel<{_t}>"], "scale read from device memory: the host call's bits", n=_ve(_dt) * 77, slope=0.2, scale=0.37, dev=True)
_case("lrelu_bwd-bf16-headline", "sgx_lrelu_bwd", H, ["lrelu_bwd_kernel<bf16_t>"], "uncapped grid_all: 262144 blocks", n=BIG_NPIX * 16, slope=0.2, scale=0.7)
_case("lrelu_bwd_bits", "sgx_lrelu_bwd_bits", H, ["lrelu_bwd_bits_kernel"], "plain loads and stores under 192 MB", n=8 * 300, slope=0.2, scale=0.7)
_case("lrelu_bwd_bits-scale_dev", "sgx_lrelu_bwd_bits", H, ["lrelu_bwd_bits_kernel"], "scale read from device memory: the host call's bits", n=8 * 77, slope=0.2, scale=0.37, dev=True)
_case("lrelu_bwd_bits-headline", "sgx_lrelu_bwd_bits", H, ["lrelu_bwd_bits_kernel"], "1 GiB tensor: the nontemporal accesses; 262144 blocks", n=BIG_NPIX * 16, slope=0.2, scale=0.7)

# ---- sgx_axpby / sgx_axpby_dev: n % VE in {0, 1, VE - 1}, n < VE, b NULL
for _dt in (F, H):
    _t, _v = tname(_dt), _ve(_dt)
    for _n, _why in ((_v * 257, "n % VE == 0, 2 blocks"), (_v * 257 + 1, "n % VE == 1: scalar tail of one"), (_v * 257 + _v - 1, "n % VE == VE - 1: the longest scalar tail"),
                     (_v - 1, "n < VE: the tail only")):
        _case(f"axpby-{_t}-n{_n}", "sgx_axpby", _dt, [f"axpby_kernel<{_t}>"], _why, n=_n, alpha=0.3, beta=0.7)
        _case(f"axpby_dev-{_t}-n{_n}", "sgx_axpby_dev", _dt, [f"axpby_kernel<{_t}>"], _why + "; coefficients from device memory: the host call's bits", n=_n, alpha=0.3, beta=0.7)
    _case(f"axpby-{_t}-bnull", "sgx_axpby", _dt, [f"axpby_kernel<{_t}>"], "b NULL, with a tail", n=_v * 31 + 1, alpha=-1.7, beta=0.0, b=False)
    _case(f"axpby_dev-{_t}-bnull", "sgx_axpby_dev", _dt, [f"axpby_kernel<{_t}>"], "b NULL and beta_dev NULL, with a tail", n=_v * 31 + 1, alpha=-1.7, beta=0.0, b=False)
_case("axpby-bf16-headline", "sgx_axpby", H, ["axpby_kernel<bf16_t>"], "uncapped grid_all: 262144 blocks", n=BIG_NPIX * 16, alpha=0.3, beta=0.7)

# ---- sgx_blur3x3_act (modes 0-3) / sgx_blur3x3_bits (modes 2, 3 = kernel modes 4, 5)
#   2-row strips below BLUR_LANES8 strip lanes; above it the one-load kernel (prefetch depth 1 for the modes with a pre-op, 3 otherwise) when
#   mode != 3, C/VE is a power of two <= 16 and (W * C/VE) % 64 == 0, else the three-load kernel with 8-row strips.
def _blur(id, dt, mode, bits, kern, why, B, Hh, W, C):
    km = mode + 2 if bits else mode
    k = {"rows2": f"blur3x3_kernel<{tname(dt)}, {km}, 2>", "rows8": f"blur3x3_kernel<{tname(dt)}, {km}, 8>",
         "shfl": f"blur3x3s_kernel<{tname(dt)}, {km}, 8, {1 if km in (1, 5) else 3}, false>"}[kern]
    _case(id, "sgx_blur3x3_bits" if bits else "sgx_blur3x3_act", dt, [k], why, B=B, H=Hh, W=W, C=C, mode=mode)


for _dt in (F, H):
    _t, _v = tname(_dt), _ve(_dt)
    for _m, _b in [(0, 0), (1, 0), (2, 0), (3, 0)] + ([(2, 1), (3, 1)] if _dt == H else []):
        _s = f"{_t}-m{_m}{'b' if _b else ''}"
        _blur(f"blur-{_s}-small-H9", _dt, _m, _b, "rows2", "small launch; H = 9 is no multiple of the 2-row strip; 3 vectors per pixel", 2, 9, 5, 3 * _v)
        _blur(f"blur-{_s}-rows8-oddW", _dt, _m, _b, "rows8", "large launch, (W * cv) % 64 != 0: the three-load kernel; H = 1043 leaves a 3-row last strip", 1, 1043, 510, 2 * _v)
        if _m != 3:
            _blur(f"blur-{_s}-shfl", _dt, _m, _b, "shfl", "large launch, cv = 2, W * cv = 1024: the one-load kernel; H = 1028 leaves a 4-row last strip", 1, 1028, 512, 2 * _v)
    _blur(f"blur-{_t}-m0-H1-W1", _dt, 0, 0, "rows2", "a single pixel: no neighbour on any side", 1, 1, 1, _v)
    _blur(f"blur-{_t}-m2-H2-W1", _dt, 2, 0, "rows2", "W = 1: no left or right neighbour; H = 2 is one whole strip", 2, 2, 1, 2 * _v)
    _blur(f"blur-{_t}-m1-H52", _dt, 1, 0, "rows2", "H = 52 of 2-row strips, W = 3", 1, 52, 3, 6 * _v)
    _blur(f"blur-{_t}-m0-below-lanes8", _dt, 0, 0, "rows2", "127 strips x 1024 = 130048 strip lanes: the last size of the 2-row kernel", 1, 1012, 512, 2 * _v)
    _blur(f"blur-{_t}-m0-at-lanes8", _dt, 0, 0, "shfl", "128 strips x 1024 = 131072 strip lanes: the first size past the 2-row kernel", 1, 1024, 512, 2 * _v)
    _blur(f"blur-{_t}-m0-cv3", _dt, 0, 0, "rows8", "cv = 3 is no power of two (C = 24 bf16 / 12 fp32)", 1, 683, 512, 3 * _v)
    _blur(f"blur-{_t}-m1-cv12", _dt, 1, 0, "rows8", "cv = 12 is no power of two (C = 96 bf16 / 48 fp32)", 2, 340, 128, 12 * _v)
    _blur(f"blur-{_t}-m0-cv16", _dt, 0, 0, "shfl", "cv = 16: a lane's neighbours are 16 lanes away, W * cv = 1024", 2, 516, 64, 16 * _v)
    _blur(f"blur-{_t}-m1-cv1", _dt, 1, 0, "shfl", "cv = 1: neighbours in the adjacent lanes, prefetch depth 1", 1, 2052, 512, _v)
    _blur(f"blur-{_t}-m0-cv32", _dt, 0, 0, "rows8", "cv = 32 > 16", 1, 257, 128, 32 * _v)
_blur("blur-bf16-m2b-cv16", H, 2, 1, "shfl", "mask bytes of 16 vectors per pixel", 2, 516, 64, 128)
_blur("blur-bf16-m3b-cv1", H, 3, 1, "shfl", "mask byte of the own and of the outer-neighbour vector, cv = 1", 1, 2052, 512, 8)
_blur("blur-bf16-m0-headline", H, 0, 0, "shfl", "32 x 1024^2 x 16: 8.4 M strip lanes, 32768 blocks", **{"B": 32, "Hh": 1024, "W": 1024, "C": 16})
_blur("blur-bf16-m2b-headline", H, 2, 1, "shfl", "32 x 1024^2 x 16 with the sign-bit mask", **{"B": 32, "Hh": 1024, "W": 1024, "C": 16})

# ---- sgx_blur_kxk: non-symmetric taps; pad equal to and different from (K-1)//2; OH / OW below the maximum
for _dt in (F, H):
    _t, _v = tname(_dt), _ve(_dt)
    for _K, _pad, _dOH, _dOW in ((1, 0, 0, 0), (2, 0, 0, 0), (2, 1, 0, 1), (4, 1, 0, 0), (4, 2, 2, 0), (5, 2, 0, 0), (5, 4, 1, 3), (7, 3, 0, 0), (7, 0, 0, 0)):
        _case(f"blur_kxk-{_t}-K{_K}-pad{_pad}-d{_dOH}{_dOW}", "sgx_blur_kxk", _dt, [f"blur_kxk_kernel<{_t}>"],
              f"K = {_K}, pad {'=' if _pad == (_K - 1) // 2 else '!='} (K-1)//2, output {_dOH} x {_dOW} below the maximum; 3 vectors per pixel",
              K=_K, pad=_pad, B=2, IH=11, IW=9, dOH=_dOH, dOW=_dOW, C=3 * _v)

# ---- sgx_pool2
_case("pool2-f32-C8", "sgx_pool2", F, ["pool2_kernel<float, true>"], "fp32 C % 4 == 0", B=2, H=6, W=10, C=8, scale=0.25)
_case("pool2-f32-C5", "sgx_pool2", F, ["pool2_kernel<float, false>"], "fp32 C % 4 != 0, C != 3: scalar", B=2, H=6, W=10, C=5, scale=0.25)
_case("pool2-f32-rgb-W16", "sgx_pool2", F, ["pool2_rgb_kernel"], "C = 3, W % 8 == 0, 16-byte aligned", B=3, H=10, W=16, C=3, scale=0.25)
_case("pool2-f32-rgb-W1024", "sgx_pool2", F, ["pool2_rgb_kernel"], "C = 3, full-width image rows, several blocks", B=2, H=6, W=1024, C=3, scale=0.25)
_case("pool2-f32-rgb-W12", "sgx_pool2", F, ["pool2_kernel<float, false>"], "C = 3, W % 4 == 0 but W % 8 != 0: scalar", B=3, H=10, W=12, C=3, scale=0.25)
_case("pool2-f32-rgb-W10", "sgx_pool2", F, ["pool2_kernel<float, false>"], "C = 3, W % 4 != 0: scalar", B=3, H=10, W=10, C=3, scale=0.25)
_case("pool2-f32-rgb-W16-misaligned", "sgx_pool2", F, ["pool2_kernel<float, false>"], "C = 3, W % 8 == 0, pointers 4 bytes off: scalar, the aligned call's bits",
      B=3, H=10, W=16, C=3, scale=0.25, shift=4)
_case("pool2-bf16-C16", "sgx_pool2", H, ["pool2_kernel<bf16_t, true>"], "bf16 C % 8 == 0", B=2, H=6, W=10, C=16, scale=0.25)
_case("pool2-bf16-C12", "sgx_pool2", H, ["pool2_kernel<bf16_t, false>"], "bf16 C % 8 != 0: scalar", B=2, H=6, W=10, C=12, scale=0.5)
_case("pool2-bf16-headline", "sgx_pool2", H, ["pool2_kernel<bf16_t, true>"], "32 x 1024^2 x 16 input, capped grid", scale=0.25, **BIG)

# ---- sgx_up2 (H, W: the input size)
_case("up2-f32-C8", "sgx_up2", F, ["up2_kernel<float, true>"], "fp32 C % 4 == 0", B=2, H=3, W=5, C=8, scale=1.0)
_case("up2-f32-C5", "sgx_up2", F, ["up2_kernel<float, false>"], "fp32 C % 4 != 0, C != 3: scalar", B=2, H=3, W=5, C=5, scale=0.5)
_case("up2-f32-rgb-W8", "sgx_up2", F, ["up2_rgb4_kernel"], "C = 3, W % 4 == 0 (and % 8), aligned", B=3, H=5, W=8, C=3, scale=1.0)
_case("up2-f32-rgb-W12", "sgx_up2", F, ["up2_rgb4_kernel"], "C = 3, W % 4 == 0 but W % 8 != 0, aligned", B=3, H=5, W=12, C=3, scale=0.25)
_case("up2-f32-rgb-W6", "sgx_up2", F, ["up2_rgb_kernel"], "C = 3, (2 W 3) % 4 == 0 only", B=3, H=5, W=6, C=3, scale=1.0)
_case("up2-f32-rgb-W5", "sgx_up2", F, ["up2_kernel<float, false>"], "C = 3, neither rule: scalar", B=3, H=5, W=5, C=3, scale=1.0)
_case("up2-f32-rgb-W8-misaligned", "sgx_up2", F, ["up2_kernel<float, false>"], "C = 3, W % 4 == 0, pointers 4 bytes off: scalar, the aligned call's bits",
      B=3, H=5, W=8, C=3, scale=1.0, shift=4)
_case("up2-bf16-C16", "sgx_up2", H, ["up2_kernel<bf16_t, true>"], "bf16 C % 8 == 0", B=2, H=3, W=5, C=16, scale=1.0)
_case("up2-bf16-C12", "sgx_up2", H, ["up2_kernel<bf16_t, false>"], "bf16 C % 8 != 0: scalar", B=2, H=3, W=5, C=12, scale=1.0)
_case("up2-bf16-headline", "sgx_up2", H, ["up2_kernel<bf16_t, true>"], "32 x 1024^2 x 16 output: 262144 blocks", B=32, H=512, W=512, C=16, scale=1.0)

# ---- sgx_up2_add
_case("up2_add-f32-rgb-W6", "sgx_up2_add", F, ["up2_add_rgb_kernel"], "fp32 C = 3, (2 W 3) % 4 == 0", B=3, H=5, W=6, C=3, scale=0.25)
_case("up2_add-f32-rgb-W5", "sgx_up2_add", F, ["up2_add_kernel<float>"], "fp32 C = 3, odd W: scalar", B=3, H=5, W=5, C=3, scale=0.25)
_case("up2_add-f32-rgb-W6-misaligned", "sgx_up2_add", F, ["up2_add_kernel<float>"], "fp32 C = 3, pointers 4 bytes off: scalar, the aligned call's bits",
      B=3, H=5, W=6, C=3, scale=0.25, shift=4)
_case("up2_add-f32-C8", "sgx_up2_add", F, ["up2_add_kernel<float>"], "fp32 C != 3: scalar", B=2, H=3, W=5, C=8, scale=0.25)
_case("up2_add-bf16-C12", "sgx_up2_add", H, ["up2_add_kernel<bf16_t>"], "bf16 C % 8 != 0", B=2, H=3, W=5, C=12, scale=0.25)
_case("up2_add-bf16-C16", "sgx_up2_add", H, ["up2_add_kernel<bf16_t>"], "bf16", B=2, H=6, W=8, C=16, scale=0.25)
_case("up2_add-bf16-headline", "sgx_up2_add", H, ["up2_add_kernel<bf16_t>"], "32 x 1024^2 x 16 output, capped grid: 256 trips per thread", B=32, H=512, W=512, C=16, scale=0.25)

# ---- sgx_downsample_fade_rgb
_case("downsample_fade", "sgx_downsample_fade_rgb", F, ["downsample_fade_rgb_kernel"], "one block", B=3, H=6, W=10, alpha=0.3, beta=0.7)
_case("downsample_fade-3-blocks", "sgx_downsample_fade_rgb", F, ["downsample_fade_rgb_kernel"], "540 2x2 cells: 3 blocks, partial last", B=3, H=20, W=36, alpha=0.3, beta=0.7)
_case("downsample_fade-ab_dev", "sgx_downsample_fade_rgb", F, ["downsample_fade_rgb_kernel"], "alpha, beta from device memory: the host call's bits", B=3, H=6, W=10, alpha=0.3, beta=0.7, dev=True)

# ---- sgx_images_u8_to_nhwc: all 256 byte values, flip on images 0 and 2 of 3, both layouts, W = 4 and W = 1024
for _dt in (F, H):
    for _chw in (0, 1):
        for _W, _Hh in ((4, 22), (1024, 2)):
            _case(f"images_u8-{tname(_dt)}-{'chw' if _chw else 'hwc'}-W{_W}", "sgx_images_u8_to_nhwc", _dt,
                  [f"images_u8_kernel<{tname(_dt)}, {'true' if _chw else 'false'}>"], f"{'planar' if _chw else 'interleaved'} source, W = {_W}", B=3, H=_Hh, W=_W, chw=_chw)

# ---- sgx_colsum: one block; exactly COLSUM_BLOCKS blocks; 1024*64 + 64*k pixels, where per * blockIdx passes npix for the trailing blocks
for _npix, _tag in ((50, "one block"), (COLSUM_BLOCKS * 64, "exactly 1024 blocks of 64 pixels"), (COLSUM_BLOCKS * 64 + 64, "65 pixels per block: blocks 1010.. have an empty range")):
    _case(f"colsum-f32-C16-npix{_npix}", "sgx_colsum", F, ["colsum_vec_stage1<float, 1>", "colsum_stage2"], "fp32, C/4 a power of two; " + _tag, npix=_npix, C=16)
    _case(f"colsum-bf16-C16-npix{_npix}", "sgx_colsum", H, ["colsum_vec_stage1<bf16_t, 1>", "colsum_stage2"], "bf16, C/8 a power of two; " + _tag, npix=_npix, C=16)
    _case(f"colsum-f32-C3-npix{_npix}", "sgx_colsum", F, ["colsum_stage1<float>", "colsum_stage2"], "fp32 C % 4 != 0: scalar; " + _tag, npix=_npix, C=3)
    _case(f"colsum-bf16-C12-npix{_npix}", "sgx_colsum", H, ["colsum_stage1<bf16_t>", "colsum_stage2"], "bf16 C % 8 != 0: scalar; " + _tag, npix=_npix, C=12)
_case("colsum-f32-C24", "sgx_colsum", F, ["colsum_stage1<float>", "colsum_stage2"], "C/4 = 6 is no power of two: scalar", npix=777, C=24)
_case("colsum-f32-C300", "sgx_colsum", F, ["colsum_stage1<float>", "colsum_stage2"], "C > 256: two channel passes of the scalar kernel", npix=131, C=300)
_case("colsum-f32-C1024", "sgx_colsum", F, ["colsum_vec_stage1<float, 1>", "colsum_stage2"], "cv = 256: one pixel row per block iteration", npix=131, C=1024)
_case("colsum-bf16-headline", "sgx_colsum", H, ["colsum_vec_stage1<bf16_t, 1>", "colsum_stage2"], "2^25 pixels x 16: 32768 pixels per block", npix=BIG_NPIX, C=16)

# ---- sgx_rgb_in / sgx_rgb_in_add: rgb_in1_kernel from 65536 vectors (C <= 2048), the loop kernel below; layouts (sj, sc) = (1, 3) and (C, 1)
for _dt in (F, H):
    _t, _v = tname(_dt), _ve(_dt)
    for _cv in (1, 3, 6, 12):
        _case(f"rgb_in-{_t}-cv{_cv}", "sgx_rgb_in", _dt, [f"rgb_in_kernel<{_t}>"], f"small launch, {_cv} vectors per pixel" + ("" if 256 % _cv == 0 else ": grid rounded to a multiple of cv"),
              npix=1000, C=_cv * _v, layout="in" if _cv % 2 else "out")
    _case(f"rgb_in-{_t}-65535", "sgx_rgb_in", _dt, [f"rgb_in_kernel<{_t}>"], "65535 vectors: the last size of the loop kernel", npix=65535, C=_v, layout="in")
    _case(f"rgb_in-{_t}-65536", "sgx_rgb_in", _dt, [f"rgb_in1_kernel<{_t}>"], "65536 vectors: the first size of the short-lived blocks; slices equal the loop kernel's bits", npix=65536, C=_v, layout="in", slices=True)
    _case(f"rgb_in-{_t}-in1-cv3", "sgx_rgb_in", _dt, [f"rgb_in1_kernel<{_t}>"], "short-lived blocks with 3 vectors per pixel, 65 blocks, partial last; slices equal the loop kernel's bits", npix=22001, C=3 * _v, layout="out", slices=True)
    _case(f"rgb_in-{_t}-nobias", "sgx_rgb_in", _dt, [f"rgb_in_kernel<{_t}>"], "bias NULL", npix=333, C=2 * _v, layout="in", bias=False)
    _case(f"rgb_in_add-{_t}-cv6", "sgx_rgb_in_add", _dt, [f"rgb_in_kernel<{_t}>"], "small launch, 6 vectors per pixel", npix=1000, C=6 * _v, layout="out")
    _case(f"rgb_in_add-{_t}-in1", "sgx_rgb_in_add", _dt, [f"rgb_in1_kernel<{_t}>"], "short-lived blocks, 4 vectors per pixel", npix=16500, C=4 * _v, layout="out")
_case("rgb_in-f32-C2052-loop", "sgx_rgb_in", F, ["rgb_in_kernel<float>"], "C > 2048 keeps the loop kernel: cv = 513, grid 8192 -> 8208, two trips", npix=4100, C=2052, layout="out")
_case("rgb_in-bf16-headline", "sgx_rgb_in", H, ["rgb_in1_kernel<bf16_t>"], "2^25 pixels x 16: 65536 blocks", npix=BIG_NPIX, C=16, layout="in")
_case("rgb_in_add-bf16-headline", "sgx_rgb_in_add", H, ["rgb_in1_kernel<bf16_t>"], "2^25 pixels x 16: 65536 blocks", npix=BIG_NPIX, C=16, layout="out")

# ---- sgx_rgb_out / sgx_rgb_out_fade: rgb_out1_kernel from 65536 pixels when C/VE <= 16 (a power of two), the loop kernel otherwise
for _dt in (F, H):
    _t, _v = tname(_dt), _ve(_dt)
    for _cv in (1, 2, 4, 8, 16, 17, 32):
        _case(f"rgb_out-{_t}-cv{_cv}", "sgx_rgb_out", _dt, [f"rgb_out_kernel<{_t}>"], f"small launch, C/VE = {_cv}" + (": 16 lanes per pixel, several vectors per lane" if _cv > 16 else ""),
              npix=701, C=_cv * _v, layout="out" if _cv % 2 else "in")
    _case(f"rgb_out-{_t}-65535", "sgx_rgb_out", _dt, [f"rgb_out_kernel<{_t}>"], "65535 pixels: the last size of the loop kernel", npix=65535, C=2 * _v, layout="out")
    _case(f"rgb_out-{_t}-65536", "sgx_rgb_out", _dt, [f"rgb_out1_kernel<{_t}>"], "65536 pixels: the first size of the short-lived blocks; slices equal the loop kernel's bits", npix=65536, C=2 * _v, layout="out", slices=True)
    _case(f"rgb_out-{_t}-out1-cv16", "sgx_rgb_out", _dt, [f"rgb_out1_kernel<{_t}>"], "short-lived blocks, 16 lanes per pixel, partial last block", npix=65601, C=16 * _v, layout="out", slices=True)
    _case(f"rgb_out-{_t}-big-cv32", "sgx_rgb_out", _dt, [f"rgb_out_kernel<{_t}>"], "large launch with C/VE > 16: stays on the loop kernel", npix=65600, C=32 * _v, layout="out")
    _case(f"rgb_out-{_t}-nobias", "sgx_rgb_out", _dt, [f"rgb_out_kernel<{_t}>"], "bias NULL", npix=333, C=4 * _v, layout="out", bias=False)
    _case(f"rgb_out_fade-{_t}-oddB", "sgx_rgb_out_fade", _dt, [f"rgb_out_kernel<{_t}>"], "odd batch, non-square image", B=3, H=4, W=6, C=2 * _v, layout="out", alpha=0.3, beta=0.7)
    _case(f"rgb_out_fade-{_t}-ab_dev", "sgx_rgb_out_fade", _dt, [f"rgb_out_kernel<{_t}>"], "alpha, beta from device memory: the host call's bits", B=3, H=4, W=6, C=2 * _v, layout="out", alpha=0.3, beta=0.7, dev=True)
    _case(f"rgb_out_fade-{_t}-out1", "sgx_rgb_out_fade", _dt, [f"rgb_out1_kernel<{_t}>"], "65536 pixels in 1 x 128 x 512: short-lived blocks with the low-resolution image", B=1, H=128, W=512, C=2 * _v, layout="out", alpha=0.3, beta=0.7)
_case("rgb_out-bf16-C4096", "sgx_rgb_out", H, ["rgb_out_kernel<bf16_t>"], "the widest C the entry point takes: 48 KB of weights in LDS", npix=70, C=4096, layout="out")
_case("rgb_out-bf16-headline", "sgx_rgb_out", H, ["rgb_out1_kernel<bf16_t>"], "2^25 pixels x 16: 65536 blocks", npix=BIG_NPIX, C=16, layout="out")

# ---- sgx_rgb_wgrad: block counts as for colsum; the vector kernel needs C/VE a power of two <= 256
for _npix, _tag in ((50, "one block"), (COLSUM_BLOCKS * 64, "exactly 1024 blocks of 64 pixels"), (COLSUM_BLOCKS * 64 + 64, "65 pixels per block: blocks 1010.. have an empty range")):
    _case(f"rgb_wgrad-f32-C16-npix{_npix}", "sgx_rgb_wgrad", F, ["colsum_vec_stage1<float, 3>", "rgb_wgrad_stage2"], "fp32, C/4 a power of two; " + _tag, npix=_npix, C=16, layout="out")
    _case(f"rgb_wgrad-bf16-C16-npix{_npix}", "sgx_rgb_wgrad", H, ["colsum_vec_stage1<bf16_t, 3>", "rgb_wgrad_stage2"], "bf16, C/8 a power of two; " + _tag, npix=_npix, C=16, layout="in")
    _case(f"rgb_wgrad-f32-C2-npix{_npix}", "sgx_rgb_wgrad", F, ["rgb_wgrad_stage1<float>", "rgb_wgrad_stage2"], "fp32 C % 4 != 0: scalar; " + _tag, npix=_npix, C=2, layout="in")
    _case(f"rgb_wgrad-bf16-C4-npix{_npix}", "sgx_rgb_wgrad", H, ["rgb_wgrad_stage1<bf16_t>", "rgb_wgrad_stage2"], "bf16 C % 8 != 0: scalar; " + _tag, npix=_npix, C=4, layout="out")
_case("rgb_wgrad-f32-C2048", "sgx_rgb_wgrad", F, ["rgb_wgrad_stage1<float>", "rgb_wgrad_stage2"], "C/4 = 512 is above the vector kernel's 256: eight channel passes of the scalar kernel", npix=131, C=2048, layout="out")
_case("rgb_wgrad-bf16-C768", "sgx_rgb_wgrad", H, ["rgb_wgrad_stage1<bf16_t>", "rgb_wgrad_stage2"], "C > 256 with C/8 = 96, no power of two: scalar", npix=131, C=768, layout="in")
_case("rgb_wgrad-bf16-headline", "sgx_rgb_wgrad", H, ["colsum_vec_stage1<bf16_t, 3>", "rgb_wgrad_stage2"], "2^25 pixels x 16: 32768 pixels per block", npix=BIG_NPIX, C=16, layout="out")

# ---- the fade_rgb_bwd family (kernel tests: tests/test_gpu_rgbconv.py), one case each under this criterion
_case("fade_rgb_bwd2-C32", "sgx_fade_rgb_bwd2", H, ["fade_rgb_bwd2_kernel"], "bf16, C = 32; equals its three passes bit for bit", npix=1237, C=32, alpha=0.3)
_case("fade_rgb_bwd-C64", "sgx_fade_rgb_bwd", H, ["fade_rgb_bwd_kernel<8>", "fade_rgb_bwd_finish"], "bf16, C = 64: the one-pass kernel and the parameter-gradient finish", npix=1237, C=64, alpha=0.3)
_case("fade_rgb_bwd-C32-two-calls", "sgx_fade_rgb_bwd", H, ["fade_rgb_bwd_kernel<4>", "fade_rgb_bwd_finish"], "bf16, C = 32: sgx_fade_rgb_bwd without parameter gradients, then sgx_fade_rgb_bwd_finish",
      npix=700, C=32, alpha=0.3, split=True)
_case("fade_rgb_bwd-C128", "sgx_fade_rgb_bwd", H, ["fade_rgb_bwd_kernel<16>", "fade_rgb_bwd_finish"], "bf16, C = 128", npix=300, C=128, alpha=0.6)

# ---- the last epilogue inside to_rgb (kernel tests: tests/test_gpu_fusions.py), one case each under this criterion
_case("rgb_out_epi-bf16-C32-fade", "sgx_rgb_out_epi", H, ["rgb_out_epi_kernel<bf16_t>"], "bf16, 4 lanes per pixel, 4 blocks per image, with the low-resolution image", B=3, H=12, W=20, C=32, layout="out", low=True)
_case("rgb_out_epi-f32-C16", "sgx_rgb_out_epi", F, ["rgb_out_epi_kernel<float>"], "fp32, no low-resolution image, no epilogue bias, from_rgb-style layout", B=2, H=6, W=10, C=16, layout="in", low=False)
_case("rgb_wgrad_epi-bf16-C32", "sgx_rgb_wgrad_epi", H, ["rgb_wgrad_epi_stage1<bf16_t>", "rgb_wgrad_epi_stage2"], "bf16, 3 blocks per image, partial last", B=3, H=23, W=29, C=32, layout="out")
_case("rgb_wgrad_epi-f32-C16", "sgx_rgb_wgrad_epi", F, ["rgb_wgrad_epi_stage1<float>", "rgb_wgrad_epi_stage2"], "fp32, one block per image", B=2, H=6, W=10, C=16, layout="in")

# ---- small.hip: the R1 head and PixelNorm
SUMSQ_GS = 4 * 256 * 1024           # elements one trip of the whole sumsq grid covers
_case("sumsq-n1027", "sgx_sumsq_f32", F, ["sumsq_f32_stage1", "sumsq_f32_stage2"], "n % 4 = 3: one block, single loop and scalar tail", n=1027)
_case("sumsq-n2", "sgx_sumsq_f32", F, ["sumsq_f32_stage1", "sumsq_f32_stage2"], "n < 4: the scalar tail only", n=2)
_case("sumsq-4gs+151", "sgx_sumsq_f32", F, ["sumsq_f32_stage1", "sumsq_f32_stage2"], "just past 4 grid trips: the four-in-flight loop, the single loop (37 lanes) and the scalar tail together", n=4 * SUMSQ_GS + 4 * 37 + 3)
for _n, _why in ((1024, "n % 4 == 0"), (1025, "n % 4 == 1"), (1027, "n % 4 == 3"), (3, "n < 4: the scalar tail only"), (4 * 4096 * 256 + 5, "past the 4096-block cap: two trips, and a tail")):
    _case(f"scale_dev-n{_n}", "sgx_scale_dev_f32", F, ["scale_dev_kernel"], _why, n=_n, alpha=0.5)
for _B, _C in ((5, 512), (1, 70), (9, 64)):
    _case(f"pixelnorm_fwd-B{_B}-C{_C}", "sgx_pixelnorm_fwd", F, ["pixelnorm_fwd_kernel"], "B % 4 != 0: idle waves in the last block" + ("; C % 64 != 0" if _C % 64 else ""), B=_B, C=_C)
    _case(f"pixelnorm_bwd-B{_B}-C{_C}", "sgx_pixelnorm_bwd", F, ["pixelnorm_bwd_kernel"], "B % 4 != 0: idle waves in the last block" + ("; C % 64 != 0" if _C % 64 else ""), B=_B, C=_C)

assert len({c.id for c in CASES}) == len(CASES), "duplicate case id"

# Contract rejections: (id, entry, expected code, why).  They return before any kernel starts; the runner passes valid buffers anyway.
REJECTIONS = [
    ("bias_act-bf16-C12", "sgx_bias_act", -2, "bf16 with C % 8 != 0"),
    ("blur_kxk-K8", "sgx_blur_kxk", -1, "K above SGX_BLUR_MAXK = 7"),
    ("colsum-short-workspace", "sgx_colsum", -3, "workspace one byte short"),
    ("rgb_wgrad-C48", "sgx_rgb_wgrad", -2, "C <= 256 that does not divide 256"),
    ("rgb_out-C4104", "sgx_rgb_out", -2, "C above 4096"),
] + [(f"{e[4:]}-dtype7", e, -1, "a dtype outside {SGX_F32, SGX_BF16}: the one dtype dispatch refuses it")
     for e in ("sgx_bias_act", "sgx_pool2", "sgx_up2", "sgx_up2_add", "sgx_colsum", "sgx_rgb_in", "sgx_rgb_out", "sgx_lrelu_bwd_bits", "sgx_img_in")]

# Launch sites of the covered sources that no case reaches, each with its reason (tests/test_streaming_coverage.py).  Keys are the kernel
# expressions as the hipLaunchKernelGGL sites spell them.
EXCLUDED_SITES = {
    "blur3x3s_kernel<T, 0, ROWS, PF, true>": "SGX_BLUR_NT=1 probe instantiation (nontemporal accesses), off by default",
    "blur3x3s_kernel<T, 1, ROWS, PF, true>": "SGX_BLUR_NT=1 probe instantiation, off by default",
    "blur3x3s_kernel<T, 2, ROWS, PF, true>": "SGX_BLUR_NT=1 probe instantiation, off by default",
    "blur3x3s_kernel<T, 4, ROWS, PF, true>": "SGX_BLUR_NT=1 probe instantiation, off by default",
    "blur3x3s_kernel<T, 5, ROWS, PF, true>": "SGX_BLUR_NT=1 probe instantiation, off by default",
}
# Paths inside a claimed kernel's launcher that the default environment or any tensor under 32 GB cannot select.
EXCLUDED_PATHS = {
    "blur_launch_shfl<T, 2> / blur_launch_shfl<T, 4>": "prefetch depths only SGX_BLUR_SHFL=2 / 4 selects (the default is 1 or 3 by mode)",
    "blur3x3_kernel at lanes8 >= 2^31": "the one-load blur's fallback for >= 2^31 strip lanes: a tensor of 32 GB and more",
    "rgb_in_kernel at nvec >= 2^31 - 1": "rgb_in1_kernel's fallback: 32 GB and more of output",
    "rgb_out_kernel at npix >= 2^31 - 1": "rgb_out1_kernel's fallback: 2^31 pixels",
    "SGX_RGB_IN1=0 / SGX_RGB_OUT1=0 / SGX_GRID_CAP / SGX_GRID_ALL_CAP": "A/B switches read once per process; the defaults are what ships",
}
# The part of small.hip this table covers: launch sites between these two markers of the source are scanned
SMALL_HIP_COVERED = ("pixelnorm_fwd_kernel", "pixelnorm_bwd_kernel", "sumsq_f32_stage1", "sumsq_f32_stage2", "scale_dev_kernel")


# ---------------------------------------------------------------------------------------------------------------- fp32 chain lengths
def colsum_chain(npix, C, dtype, scalar):
    """The fp32 partial chain of the two-stage column sums (csrc/pointwise.hip): the scalar stage 1 flushes its fp32 partial into fp64 every
    64 rows; the vector stage 1 keeps one fp32 partial per lane over its block's range: ceil(per / rows) rows with per = ceil(npix / blocks),
    rows = 256 / (C / VE).  Everything after that is fp64."""
    if scalar:
        return 64
    nblk = max(1, min(COLSUM_BLOCKS, (npix + 63) // 64))
    per = (npix + nblk - 1) // nblk
    rows = 256 // (C // _ve(dtype))
    return max(1, math.ceil(per / rows))
