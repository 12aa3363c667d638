"""fp64 restatements of the discriminator's composed first layer (csrc/rgbconv.hip: from_rgb o conv0 o LeakyReLU o blur, its image gradient
and its four parameter gradients), written from that file's header comment and include/sgx.h; the launcher rules of the file restated in
Python (which kernel, which grid, how much LDS, which tiles a persistent block walks); the per-element criteria; and the table of cases that
walks every launch path.  Test-side only: the product never imports this, and nothing here calls the library under test.  The criterion,
the guard bands, the bit layout and the kernel names are streaming_ref's (assert_elementwise, Guarded, pack_bits, kernel_id), assert_within
is epilogue_ref's, assert_bits small_ref's.

Layouts are the C ABI's: images fp32 [B][H][W][3], activations bf16 [B][H][W][C], sign bits [B][H][W][C / 8], W0 [C][C][3][3], Wr [C][3],
br, b0 [C].  Every reference takes fp64 tensors on any device (the two rows with more tiles than blocks run them on the GPU).

Data kinds of a row (``data``), all drawn on the CPU from seeded generators:
  int   image and gz integers in [-3, 3], W0, Wr, br in [-2, 2], b0 in [-2, 2]; the scales are 1 or, on the ``scaled`` rows, s0 = 0.5,
        sr = 0.25, bscale = 2: every pack value is exact in fp16 and in bf16, every product and every partial sum is a multiple of 1 / 8
        below 2^24 / 8 -- exact in fp32 in any order
  pos   int with b0 = 1024 in every channel: every pre-activation inside the image is positive (checked on the reference), so
        LeakyReLU is the identity and the whole forward is exact
  mix   int with b0 = 128, at unit scales (with the non-unit ones W' shrinks eightfold and no pre-activation is negative: measured, all
        such rows came out exact everywhere): outputs whose 3x3 window holds no negative pre-activation are exact, the others carry the
        rounding of 0.2f * x; both classes hold at least a tenth of the elements (checked on the reference)
  real  Gaussian image and parameters with the He scales of the two layers"""
import functools
from collections import namedtuple

import numpy as np
import torch

import epilogue_ref as ER
import streaming_ref as SR
from small_ref import assert_bits  # noqa: F401  (the runner's exact comparison of fp32 outputs)
from streaming_ref import LRELU, R_BF16, U32, Case, f32

EXACT = float(2 ** 24)
R_F16 = 2.0 ** -11                  # half an fp16 ulp relative to a normal value
TINY_F16 = 2.0 ** -25               # half the spacing of fp16's subnormals: what a value below 2^-14 may be off by
SCALED = (0.5, 0.25, 2.0)           # s0, sr, bscale of the ``scaled`` integer rows
N_CONV = 36                         # fp32 additions on a convolution output's chain: 3 MFMAs x 12 products that are not padding
N_BLUR0 = 5                         # rgbconv_fwdblur_kernel behind the accumulator: x * (0.2f / 16), then a[l - 1] + a[l], t[l] + t[l + 1], h1 + h, vp + vc
N_BLUR1 = 4                         # rgbconv_fwd_kernel<CB, 1> behind the bf16 tile in LDS: (l + 2 m) + r, then (h0 + 2 h1) + h; / 16 is exact


def cdiv(a, b):
    return -(-a // b)


def ceil8(a):
    return cdiv(a, 8) * 8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed, lo, hi):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).double()


def rnd(shape, seed, scale=1.0):
    return (scale * torch.randn(tuple(shape), generator=_gen(seed), dtype=torch.float32)).double()


def bf16_rn(t):
    """fp64 -> the nearest bf16 (through fp32: every value this is used on is an fp32 number)."""
    return t.float().bfloat16()


# ---------------------------------------------------------------------------------------------------------------- launcher rules
KERNELS = ("rgbconv_pack_kernel", "rgbconv_fwd_kernel", "rgbconv_fwdblur_kernel", "rgbconv_dgrad_kernel", "rgbconv_wgrad_kernel", "rgbconv_wfinish_kernel",
           "rgbconv_chain_kernel")
PACK, WFINISH, CHAIN = "rgbconv_pack_kernel", "rgbconv_wfinish_kernel", "rgbconv_chain_kernel"
STRIP, DGRAD_ROWS = 14, 32
BLOCK = (256, 1, 1)
NCU_NOMINAL = 256                   # the MI355X: what the CPU-side checks of the device-dependent rows assume


def fwd_kernel(CB, epi):
    return f"rgbconv_fwd_kernel<{CB}, {epi}>"


def fwdblur_kernel(CB):
    return f"rgbconv_fwdblur_kernel<{CB}>"


def shape_ok(B, H, W, C, bf16=True):
    """rgbconv_shape_ok (sgx_rgbconv_ok with the A/B switch at its default)."""
    return bool(bf16 and C in (16, 32) and B >= 1 and H >= 16 and W >= 64 and H % 16 == 0 and W % 64 == 0)


def nstrips(W):
    return cdiv(W, STRIP)


def stream_grid(items):
    """Four waves (items) per block, a multiple of 8 blocks: ((items + 3) / 4 + 7) / 8 * 8."""
    return ceil8(cdiv(items, 4))


def fwdblur_nit(B, H, W, override=0):
    """Six-row steps per row block: 6 where that leaves 3 * 256 * 24 waves, down to 3 for smaller launches; 1..8 given: that."""
    if override:
        return override
    nit = 6
    while nit > 3 and B * nstrips(W) * ((H + 6 * nit - 3) // (6 * nit - 2)) < 3 * 256 * 24:
        nit -= 1
    return nit


FwdBlur = namedtuple("FwdBlur", "nit rb nrb grid last")


def fwdblur_geom(B, H, W, override=0):
    nit = fwdblur_nit(B, H, W, override)
    rb = 6 * nit - 2
    nrb = cdiv(H, rb)
    return FwdBlur(nit, rb, nrb, stream_grid(B * nstrips(W) * nrb), H - (nrb - 1) * rb)


def fwdblur_walks(H, W, g):
    """{(strip, row block): True where the wave takes the border-free walk} -- rgbconv_fwdblur_kernel's ``inside``."""
    return {(sx, k): sx * STRIP - 2 >= 0 and sx * STRIP + 15 < W and k * g.rb - 2 >= 0 and k * g.rb + g.rb + 1 < H for sx in range(nstrips(W)) for k in range(g.nrb)}


def dgrad_grid(B, H, W):
    return stream_grid(B * nstrips(W) * cdiv(H, DGRAD_ROWS))


RcFwd = namedtuple("RcFwd", "TH TW IH IW ZH ZW NPX IPX IMG_BYTES LDS")


def rc_fwd(CB, epi):
    C, R = 16 * CB, 2 if epi else 1
    TH, TW = ((16 if CB == 1 else 8) if epi else 16), 64
    IH, IW, ZH, ZW = TH + 2 * R, TW + 2 * R, TH + 2 * (R - 1), TW + 2 * (R - 1)
    NPX, IPX = ZH * ZW, IH * IW + 4
    img = cdiv(IPX * 8, 16) * 16
    return RcFwd(TH, TW, IH, IW, ZH, ZW, NPX, IPX, img, img + (NPX * C * 2 if epi else 16))


def fwd_ntiles(B, H, W, CB, epi):
    g = rc_fwd(CB, epi)
    return B * (W // g.TW) * (H // g.TH)


def rc_sched(b, grid, ntiles):
    """Tiles of block b of a persistent grid: XCD b & 7 owns a contiguous eighth of the raster, slot b >> 3 walks every (grid / 8)-th."""
    xcd, slot, per, band = b & 7, b >> 3, grid >> 3, (ntiles + 7) >> 3
    return range(xcd * band + slot, min((xcd + 1) * band, ntiles), per)


def sched_counts(grid, ntiles):
    """Tiles per block; every tile is walked by exactly one block (asserted)."""
    seen = np.zeros(ntiles, np.int64)
    counts = []
    for b in range(grid):
        r = rc_sched(b, grid, ntiles)
        counts.append(len(r))
        if len(r):
            seen[r.start:r.stop:r.step] += 1
    assert bool((seen == 1).all()), (grid, ntiles)
    return counts


def check_rc_grid(grid, ntiles, ncu, per_cu=None):
    """rc_grid sizes a persistent grid from the CU count and, for rgbconv_fwd_kernel, an occupancy query: held by its properties."""
    assert grid % 8 == 0 and 8 <= grid <= ceil8(ntiles) and grid <= ceil8(4 * ncu), (grid, ntiles, ncu)
    if per_cu is not None:
        assert grid == ceil8(min(ntiles, per_cu * ncu)), (grid, ntiles, ncu, per_cu)


def wg_lds(CB):
    C = 16 * CB
    return max(C * (8 * 64 + 8) * 2 + 12 * (10 * 64 + 8) * 2, 4 * CB * 3 * 256 * 4)


def wgrad_ntiles(B, H, W):
    return B * (H // 8) * (W // 64)


def wgrad_blocks(B, H, W, ncu):
    return ceil8(min(wgrad_ntiles(B, H, W), 3 * ncu))


def wgrad_ws_bytes(nblk, C):
    """sgx_rgbconv_wgrad_ws_bytes as a function of the block count: nblk partials and the finished dW', C * 48 floats each."""
    return (nblk + 1) * C * 48 * 4


def wfinish_grid(C):
    return cdiv(C * 48, 8)


def wfinish_trips(nblk):
    """(trips of the slice loop k0 = sl, sl + 256, ..., for slice 0; terms of the last trip that are clamped, k >= nblk)."""
    trips = len(range(0, nblk, 256))
    last = (trips - 1) * 256
    return trips, sum(1 for u in range(8) if last + 32 * u >= nblk)


def chain_blocks(C):
    return C + cdiv(C * C * 9, 256)


def pack_grid(C):
    return 12 if C == 16 else 24


def plan(c, ncu=NCU_NOMINAL):
    """A row's expected (kernel list, [(grid, block, lds)]) from its arguments and the rules above.  A grid of None is rc_grid's for
    rgbconv_fwd_kernel (check_rc_grid)."""
    a = c.args
    C = a["C"]
    CB = C // 16
    B, H, W = a.get("B"), a.get("H"), a.get("W")
    if c.entry == "sgx_rgbconv_pack":
        return (PACK,), [((pack_grid(C), 1, 1), BLOCK, 0)]
    if c.entry == "sgx_rgbconv_dgrad":
        return (f"rgbconv_dgrad_kernel<{CB}>",), [((dgrad_grid(B, H, W), 1, 1), BLOCK, 0)]
    if c.entry == "sgx_rgbconv_wgrad":
        nblk = wgrad_blocks(B, H, W, ncu)
        return (f"rgbconv_wgrad_kernel<{CB}>", WFINISH, CHAIN), [((nblk, 1, 1), BLOCK, wg_lds(CB)), ((wfinish_grid(C), 1, 1), BLOCK, 0), ((chain_blocks(C), 1, 1), BLOCK, 0)]
    epi, v = a["epi"], a["variant"]
    if epi and v == 0:
        return (fwdblur_kernel(CB),), [((fwdblur_geom(B, H, W, a["nit"]).grid, 1, 1), BLOCK, 0)]
    grid = ceil8(fwd_ntiles(B, H, W, CB, epi)) if (epi and v == 2) else None
    return (fwd_kernel(CB, epi),), [((grid, 1, 1) if grid else None, BLOCK, rc_fwd(CB, epi).LDS)]


def persistent_batch(grid_full, tiles_per_image):
    """The batch size of a row with more tiles than blocks: the smallest whose tile count is at least 1.1 times the full grid."""
    return cdiv(int(1.1 * grid_full) + 1, tiles_per_image)


def resolve(c, ncu=NCU_NOMINAL):
    """A row's arguments with the device-dependent batch size filled in (wgrad's tile-loop row: just above 3 blocks per CU)."""
    a = dict(c.args)
    if a.get("B") == "3ncu+":
        a["B"] = 3 * ncu // ((a["H"] // 8) * (a["W"] // 64)) + 1
    return c._replace(args=a)


# ---------------------------------------------------------------------------------------------------------------- references
def compose(w0, wr, br, s0, sr, bscale):
    """W4[o][j][ky][kx]: j < 3 the composed weight W' = s0 sr sum_i W0[o][i] Wr[i][j], j = 3 the bias channel T = s0 sum_i W0[o][i] br[i]
    bscale (zero without br) -> (W4, the same sums over absolute values)."""
    w = torch.einsum("oiyx,ij->ojyx", w0, wr) * (s0 * sr)
    Sw = torch.einsum("oiyx,ij->ojyx", w0.abs(), wr.abs()) * (s0 * sr)
    if br is None:
        T, St = torch.zeros_like(w[:, :1]), torch.zeros_like(w[:, :1])
    else:
        T = (s0 * torch.einsum("oiyx,i->oyx", w0, br * bscale)).unsqueeze(1)
        St = (s0 * torch.einsum("oiyx,i->oyx", w0.abs(), (br * bscale).abs())).unsqueeze(1)
    return torch.cat([w, T], 1), torch.cat([Sw, St], 1)


def pack_wf(W4):
    """wf[ky][o][k], k = kx * 4 + j, k >= 12 zero (fp16 on the device)."""
    C = W4.shape[0]
    wf = torch.zeros(3, C, 4, 4, dtype=W4.dtype)
    wf[:, :, :3, :] = W4.permute(2, 0, 3, 1)                 # [ky][o][kx][j]
    return wf.reshape(3, C, 16)


def pack_wd(W4):
    """wd[ky'][i = kx' * 4 + j][o] = W'[o][j][2 - ky'][2 - kx'], j = 3 and kx' = 3 zero (bf16 on the device)."""
    C = W4.shape[0]
    wd = torch.zeros(3, 4, 4, C, dtype=W4.dtype)
    wd[:, :3, :3, :] = W4[:, :3].flip(2, 3).permute(2, 3, 1, 0)      # [ky'][kx'][j][o]
    return wd.reshape(3, 16, C)


def with_ones(img, ones):
    return torch.cat([img, torch.full_like(img[..., :1], 1.0 if ones else 0.0)], -1)


def conv4(x4, W4, b0=None):
    """z[b][y][x][o] = b0[o] + sum over the taps that fall inside the image of sum_j W4[o][j][tap] x4[p + tap][j], x4 = (r, g, b, 1): NHWC, the
    nine taps as nine small matrix products (torch's fp64 on either device) -> (z, the same expression on absolute values)."""
    B, H, W, _ = x4.shape
    xp = torch.nn.functional.pad(x4, (0, 0, 1, 1, 1, 1))
    z = torch.zeros(B, H, W, W4.shape[0], dtype=x4.dtype, device=x4.device)
    S = torch.zeros_like(z)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, ky:ky + H, kx:kx + W]
            z += win @ W4[:, :, ky, kx].t()
            S += win.abs() @ W4[:, :, ky, kx].abs().t()
    if b0 is not None:
        z, S = z + b0, S + b0.abs()
    return z, S


def adjoint(gz, W4):
    """gi[q][j] = sum_{tap, o} gz[q - tap][o] W'[o][j][tap]: the gradient of sum(z gz) with respect to the image."""
    B, H, W, _ = gz.shape
    gp = torch.nn.functional.pad(gz, (0, 0, 1, 1, 1, 1))
    gi = torch.zeros(B, H, W, 3, dtype=gz.dtype, device=gz.device)
    for ky in range(3):
        for kx in range(3):
            gi += gp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W] @ W4[:, :3, ky, kx]
    return gi


def dwprime(x4, gz):
    """dW'[o][j][ky][kx] = sum_p gz[p][o] x4[p + tap][j] (j = 3: the bias channel)."""
    B, H, W, _ = x4.shape
    xp = torch.nn.functional.pad(x4, (0, 0, 1, 1, 1, 1))
    d = torch.zeros(gz.shape[-1], 4, 3, 3, dtype=x4.dtype, device=x4.device)
    g2 = gz.reshape(-1, gz.shape[-1])
    for ky in range(3):
        for kx in range(3):
            d[:, :, ky, kx] = g2.t() @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, 4)
    return d


def dwp_layout(d):
    """dW' as the workspace holds it: [(o * 3 + ky) * 16 + kx * 4 + j], the slots kx = 3 not compared."""
    C = d.shape[0]
    out = torch.zeros(C, 3, 4, 4, dtype=d.dtype)
    out[:, :, :3, :] = d.permute(0, 2, 3, 1)
    return out.reshape(C * 48)


DWP_USED = (torch.arange(48) % 16 < 12)                      # per output channel: the 36 slots of dW' that mean something


def chain_rule(d, w0, wr, br, s0, sr, bscale):
    """The four parameter gradients from dW' (the header comment of csrc/rgbconv.hip):
      dW0[o][i][tap] = s0 sr sum_j dW'[o][j][tap] Wr[i][j] + s0 dW'[o][3][tap] br[i] bscale     db0[o] = dW'[o][3][centre tap]
      dWr[i][j] = s0 sr sum_{o,tap} dW'[o][j][tap] W0[o][i][tap]                                 dbr[i] = s0 bscale sum_{o,tap} dW'[o][3][tap] W0[o][i][tap]"""
    dw0 = s0 * sr * torch.einsum("ojyx,ij->oiyx", d[:, :3], wr)
    if br is not None:
        dw0 = dw0 + s0 * bscale * torch.einsum("oyx,i->oiyx", d[:, 3], br)
    return {"w0": dw0, "b0": d[:, 3, 1, 1].clone(), "wr": s0 * sr * torch.einsum("ojyx,oiyx->ij", d[:, :3], w0), "br": s0 * bscale * torch.einsum("oyx,oiyx->i", d[:, 3], w0)}


def lrelu(z):
    return torch.where(z > 0, z, LRELU * z)


def blur(x):
    return SR.blur3x3(x, None, 0)[0]


def fwd_exact_mask(z):
    """Outputs whose in-image 3x3 window holds no negative pre-activation (the blur pads with zeros: those are no pre-activations)."""
    return blur((z < 0).double()) == 0


def tile_act(z):
    """What rgbconv_fwd_kernel<CB, 1> leaves in LDS: lrelu in fp32 (one rounding of 0.2f * z), rounded to bf16."""
    return bf16_rn(lrelu(z)).double()


def operand_error(x4, W4, S4, C, S_z):
    """The bound on a ``real`` row's pre-activation: both MFMA operands are fp16 (half an ulp, 2^-11 of a normal value, 2^-25 below the
    normal range; the bias channel's 1 is exact), the pack's value is itself the fp32 sum of C products (C + 3 roundings on S4), and the
    accumulator adds N_CONV products in fp32 (+ 2: assert_elementwise's own slack for the second-order terms)."""
    dx = R_F16 * x4.abs() + TINY_F16
    dx[..., 3] = 0.0
    dw = R_F16 * W4.abs() + TINY_F16 + (C + 3) * U32 * S4
    return conv4(x4.abs(), dw)[0] + conv4(dx, W4.abs() + dw)[0] + (N_CONV + 2) * U32 * S_z


# ---------------------------------------------------------------------------------------------------------------- operands
def he_scales(C):
    return f32((2.0 / (C * 9)) ** 0.5), f32((2.0 / 3) ** 0.5)


@functools.lru_cache(maxsize=None)
def params(C, data, scaled):
    """-> dict of fp64 CPU tensors w0, wr [C][3], br, b0 and the fp32 scales.  Integer kinds: the seeds of test_gpu_image_end.int_params."""
    if data == "real":
        s0, sr = he_scales(C)
        return dict(w0=rnd((C, C, 3, 3), 11), b0=rnd((C,), 12, 0.3), wr=rnd((C, 3), 13), br=rnd((C,), 14, 0.5), s0=s0, sr=sr, bscale=1.0)
    s0, sr, bscale = SCALED if scaled else (1.0, 1.0, 1.0)
    b0 = {"int": ints((C,), 12, -2, 2), "pos": torch.full((C,), 1024.0, dtype=torch.float64), "mix": torch.full((C,), 128.0, dtype=torch.float64)}[data]
    return dict(w0=ints((C, C, 3, 3), 11, -2, 2), b0=b0, wr=ints((C, 3), 13, -2, 2), br=ints((C,), 14, -2, 2), s0=s0, sr=sr, bscale=bscale)


@functools.lru_cache(maxsize=None)
def image(B, H, W, data):
    return rnd((B, H, W, 3), 21) if data == "real" else ints((B, H, W, 3), 41, -3, 3)


@functools.lru_cache(maxsize=None)
def grad(B, H, W, C):
    return ints((B, H, W, C), 42, -3, 3)


def tile_exponents(H, W, k):
    """The power of two per pixel of an EPI 0 row: an int for the whole image, "tiles" for one exponent per 16 x 64 tile that differs by at
    most 12 between neighbours (11 across a corner)."""
    if k != "tiles":
        return torch.full((H, W), float(k), dtype=torch.float64)
    ty, tx = torch.arange(H) // 16, torch.arange(W) // 64
    return (-20.0 - 5.0 * ty.view(-1, 1) - 6.0 * tx.view(1, -1)).double()


def one_scale_mask(kmap):
    """Pixels whose 3x3 window (clamped to the image) lies in one tile's scale."""
    k = kmap.view(1, 1, *kmap.shape)
    kp = torch.nn.functional.pad(k, (1, 1, 1, 1), mode="replicate")
    hi = torch.nn.functional.max_pool2d(kp, 3, 1)
    lo = -torch.nn.functional.max_pool2d(-kp, 3, 1)
    return (hi == lo)[0, 0]


@functools.lru_cache(maxsize=None)
def composed_of(C, data, scaled, with_br=True):
    p = params(C, data, scaled)
    W4, S4 = compose(p["w0"], p["wr"], p["br"] if with_br else None, p["s0"], p["sr"], p["bscale"])
    if data != "real":
        # every pack value is exact in fp16 and in bf16, and small enough for the exact sums behind it
        assert float(W4.abs().max()) <= 2048, float(W4.abs().max())
        assert torch.equal(W4.to(torch.float16).double(), W4) and torch.equal(W4[:, :3].bfloat16().double(), W4[:, :3])
    return W4, S4


@functools.lru_cache(maxsize=None)
def forward_ref(B, H, W, C, data, scaled, ones=1, with_b0=True):
    """-> (z, S_z) of the row on the CPU, computed once per distinct argument set and never written."""
    p = params(C, data, scaled)
    W4, _ = composed_of(C, data, scaled)
    z, S = conv4(with_ones(image(B, H, W, data), ones), W4, p["b0"] if with_b0 else None)
    if data != "real":
        assert float(S.max()) * 8 < EXACT                     # multiples of 1 / 8: every partial sum exact in fp32
    if data == "pos" and with_b0:
        assert float(z.min()) > 0, float(z.min())
    return z, S


# ---------------------------------------------------------------------------------------------------------------- the case table
CASES = []


def _case(id, entry, kernels, why, **args):
    CASES.append(Case(id, entry, torch.bfloat16, args, tuple(kernels), why))


SA, SB, SC = (2, 16, 64, 16), (1, 48, 128, 16), (1, 32, 192, 32)


def _sid(s):
    return f"B{s[0]}-{s[1]}x{s[2]}-C{s[3]}"


# ---- sgx_rgbconv_pack
for _C, _data, _scaled, _br, _why in [
    (16, "int", False, True, "12 blocks; unit scales: the bits of the older exact tests' packs, now with br"),
    (16, "int", True, True, "s0 sr for j < 3 against s0 bscale for the bias channel, both unlike 1"),
    (32, "int", True, True, "24 blocks, C = 32"),
    (32, "int", False, False, "br NULL: the bias slots are +0"),
    (16, "int", True, False, "br NULL with non-unit scales"),
    (16, "real", False, True, "He scales on randn: half an ulp of each pack's format plus the fp32 sum"),
    (32, "real", False, True, "the same at C = 32"),
    (32, "real", False, False, "randn, br NULL"),
]:
    _case(f"pack-C{_C}-{_data}{'-scaled' if _scaled else ''}{'' if _br else '-nobr'}", "sgx_rgbconv_pack", (PACK,), _why, C=_C, data=_data, scaled=_scaled, br=_br)


def _fwd(id, shape, kernel, why, variant=0, epi=1, nit=0, data="int", scaled=False, bits=True, b0=True, ones=1, k=0, special=None):
    B, H, W, C = shape
    _case(id, "sgx_rgbconv_fwd", (kernel,), why, B=B, H=H, W=W, C=C, variant=variant, epi=epi, nit=nit, data=data, scaled=scaled, bits=bits, b0=b0, ones=ones, k=k,
          special=special)


# ---- sgx_rgbconv_fwd, epi 1, the row-streaming kernel (variant 0, the default)
for _s, _why in [(SA, "one row block of 16 rows (nit 3), every walk BORDER, the last strip 8 columns wide"),
                 (SB, "the heuristic's nit 3: three row blocks; block 1 with strips 1..8 takes the border-free walk"),
                 (SC, "C = 32: the second channel block's bias, history and sign byte")]:
    _fwd(f"fwdblur-{_sid(_s)}-pos", _s, fwdblur_kernel(_s[3] // 16), _why + "; all pre-activations positive: exact", data="pos", scaled=True)
    _fwd(f"fwdblur-{_sid(_s)}-mix", _s, fwdblur_kernel(_s[3] // 16), _why + "; both signs", data="mix")
    _fwd(f"fwdblur-{_sid(_s)}-real", _s, fwdblur_kernel(_s[3] // 16), _why + "; randn", data="real")
for _nit, _last in ((1, 4), (2, 8), (4, 4), (6, 14), (8, 2)):
    _fwd(f"fwdblur-{_sid(SB)}-nit{_nit}", SB, fwdblur_kernel(1), f"nit {_nit} by sgx_rgbconv_tune: row blocks of {6 * _nit - 2}, the last one {_last} rows", nit=_nit,
         data="pos" if _nit in (2, 8) else "mix", scaled=_nit in (2, 8))
_fwd(f"fwdblur-{_sid(SA)}-nobits", SA, fwdblur_kernel(1), "bits NULL: no byte stores, y as with them", data="pos", scaled=True, bits=False)
_fwd(f"fwdblur-{_sid(SA)}-nob0", SA, fwdblur_kernel(1), "b0 NULL: the accumulator starts at zero", data="int", scaled=True, b0=False)
_fwd(f"fwdblur-{_sid(SA)}-noones", SA, fwdblur_kernel(1), "ones = 0: the bias channel is 0 everywhere, T does not enter", data="int", scaled=True, ones=0)
_fwd("fwdblur-B8-1024x1024-C16-nit", (8, 1024, 1024, 16), fwdblur_kernel(1), "the heuristic's nit 5 (8 x 74 x 31 < 18432 <= 8 x 74 x 37): same bits as nit 3 and 6", data="mix",
     special="big")
# ---- sgx_rgbconv_fwd, epi 1, the LDS-tile kernel: persistent blocks (variant 1) and one tile per block (variant 2)
for _v in (1, 2):
    for _s in (SA, SC):
        _fwd(f"fwd1-v{_v}-{_sid(_s)}-pos", _s, fwd_kernel(_s[3] // 16, 1), f"variant {_v}: sums of bf16 integers, exact", variant=_v, data="pos", scaled=True)
        _fwd(f"fwd1-v{_v}-{_sid(_s)}-mix", _s, fwd_kernel(_s[3] // 16, 1), f"variant {_v}: both signs, the activation rounded to bf16 before the blur", variant=_v, data="mix")
    _fwd(f"fwd1-v{_v}-{_sid(SA)}-real", SA, fwd_kernel(1, 1), f"variant {_v} on randn", variant=_v, data="real")
_fwd("fwd1-v1-persistent", (None, 256, 1024, 16), fwd_kernel(1, 1), "more tiles than blocks: the next tile's loads in flight behind the staging barrier", variant=1, data="pos",
     special="persistent")
# ---- sgx_rgbconv_fwd, epi 0: the plain convolution with its per-tile power-of-two prescale
for _k in (0, -20, -120, 100):
    _fwd(f"fwd0-{_sid(SA)}-k{_k}", SA, fwd_kernel(1, 0), f"the image times 2^{_k}" + (": the prescale's exponent clamped at 253" if _k == -120 else ""), epi=0, ones=0, k=_k,
         scaled=_k in (-20, 100))
for _k in (0, -20):
    _fwd(f"fwd0-{_sid(SC)}-k{_k}", SC, fwd_kernel(2, 0), f"C = 32, the image times 2^{_k}", epi=0, ones=0, k=_k, scaled=_k == 0)
_fwd(f"fwd0-{_sid(SA)}-zero", SA, fwd_kernel(1, 0), "an all-zero image: maximum 0, scale 1, every output +0", epi=0, ones=0, k="zero")
_fwd("fwd0-B1-32x192-C16-tiles", (1, 32, 192, 16), fwd_kernel(1, 0), "one exponent per 16 x 64 tile, 5 / 6 / 11 apart: a tile's halo at its neighbour's scale", epi=0, ones=0,
     k="tiles", scaled=True)
_fwd("fwd0-persistent", (None, 256, 1024, 16), fwd_kernel(1, 0), "more tiles than blocks: the maxima of the next tile written before the previous tile's are dead", epi=0, ones=0,
     special="persistent", scaled=True)

# ---- sgx_rgbconv_dgrad
for _s, _scaled, _why in [(SA, True, "one row block, every strip at a border of a 64-wide image"), (SB, False, "interior strips, two row blocks, the last one 16 rows"),
                          (SC, True, "C = 32 over odd and even strips")]:
    _case(f"dgrad-{_sid(_s)}", "sgx_rgbconv_dgrad", (f"rgbconv_dgrad_kernel<{_s[3] // 16}>",), _why, B=_s[0], H=_s[1], W=_s[2], C=_s[3], data="int", scaled=_scaled)


# ---- sgx_rgbconv_wgrad: wgrad -> wfinish -> chain
def _wg(id, shape, why, acc=0, scaled=False, ones=1, outs="w0,b0,wr,br", br=True):
    B, H, W, C = shape
    _case(id, "sgx_rgbconv_wgrad", (f"rgbconv_wgrad_kernel<{C // 16}>", WFINISH, CHAIN), why, B=B, H=H, W=W, C=C, data="int", scaled=scaled, acc=acc, ones=ones, outs=outs, br=br)


WA, WB = (2, 16, 64, 16), (1, 32, 128, 32)
_wg(f"wgrad-{_sid(WA)}-acc0", WA, "4 tiles on 8 blocks: four blocks write a zero partial", acc=0)
_wg(f"wgrad-{_sid(WA)}-acc15", WA, "all four outputs accumulated, non-unit scales", acc=15, scaled=True)
_wg(f"wgrad-{_sid(WB)}-acc0", WB, "C = 32, 8 tiles, non-unit scales", acc=0, scaled=True)
_wg(f"wgrad-{_sid(WB)}-acc15", WB, "C = 32 accumulated", acc=15)
for _bit in (1, 2, 4, 8):
    _wg(f"wgrad-{_sid(WA)}-acc{_bit}", WA, f"acc bit {_bit} alone: one output accumulated, three overwritten", acc=_bit, scaled=_bit in (2, 8))
_wg(f"wgrad-{_sid(WA)}-noones", WA, "ones = 0 with br, db0, dbr NULL: no bias terms anywhere", ones=0, outs="w0,wr", br=False, scaled=True)
_wg(f"wgrad-{_sid(WB)}-dw0only", WB, "dw0 alone: the C blocks of dWr / dbr return at once, db0 NULL", outs="w0", scaled=True)
_wg(f"wgrad-{_sid(WA)}-nodb0", WA, "db0 NULL beside three outputs", outs="w0,wr,br", acc=5)
_wg("wgrad-B5-64x512-C16", (5, 64, 512, 16), "320 blocks: wfinish's slice loop takes a second trip whose terms k >= 320 are clamped and dropped", scaled=True)
_wg("wgrad-B3ncu-64x512-C16", ("3ncu+", 64, 512, 16), "more tiles than 3 blocks per CU: the persistent tile loop takes a second trip in some blocks", scaled=True)

assert len({c.id for c in CASES}) == len(CASES), "duplicate case id"
BY_ID = {c.id: c for c in CASES}
ROWS = {"sgx_rgbconv_pack": 8, "sgx_rgbconv_fwd": 38, "sgx_rgbconv_dgrad": 3, "sgx_rgbconv_wgrad": 13}
# by name, with the reason: launches of the file's kernels that no row makes
EXCLUDED_PATHS = {"rgbconv_fwdblur_kernel dbg 4 / 8 / 12": "sgx_rgbconv_tune's profiling ablations (no output stores, no sign bits): wrong results by design; the rejection of any other "
                  "mask and the restored (-1, 0, 0) are tested"}

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
# (id, entry, expected code, words of sgx_last_error, why): each returns before any launch, on pointers that are never followed
REJECTIONS = [
    ("pack-w0-null", "sgx_rgbconv_pack", EINVAL, "rgbconv_pack: null argument", "w0 NULL"),
    ("pack-wd-null", "sgx_rgbconv_pack", EINVAL, "rgbconv_pack: null argument", "wd NULL"),
    ("pack-C24", "sgx_rgbconv_pack", EUNSUPPORTED, "24 channels", "C = 24"),
    ("fwd-img-null", "sgx_rgbconv_fwd", EINVAL, "rgbconv_fwd: null argument", "img NULL"),
    ("fwd-y-null", "sgx_rgbconv_fwd", EINVAL, "rgbconv_fwd: null argument", "y NULL"),
    ("fwd-H8", "sgx_rgbconv_fwd", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "H = 8"),
    ("fwd-W32", "sgx_rgbconv_fwd", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "W = 32"),
    ("fwd-C24", "sgx_rgbconv_fwd", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "C = 24"),
    ("fwd-fp32", "sgx_rgbconv_fwd", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "dtype fp32"),
    ("fwd-epi2", "sgx_rgbconv_fwd", EINVAL, "epilogue 2", "epi = 2"),
    ("fwd-epi0-ones", "sgx_rgbconv_fwd", EINVAL, "no bias channel", "epi = 0 with ones = 1"),
    ("dgrad-gi-null", "sgx_rgbconv_dgrad", EINVAL, "rgbconv_dgrad: null argument", "gi NULL"),
    ("dgrad-H8", "sgx_rgbconv_dgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "H = 8"),
    ("dgrad-W32", "sgx_rgbconv_dgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "W = 32"),
    ("dgrad-C24", "sgx_rgbconv_dgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "C = 24"),
    ("dgrad-fp32", "sgx_rgbconv_dgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "dtype fp32"),
    ("wgrad-ws-null", "sgx_rgbconv_wgrad", EINVAL, "rgbconv_wgrad: null argument", "ws NULL"),
    ("wgrad-wr-null", "sgx_rgbconv_wgrad", EINVAL, "rgbconv_wgrad: null argument", "wr NULL"),
    ("wgrad-H8", "sgx_rgbconv_wgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "H = 8"),
    ("wgrad-W32", "sgx_rgbconv_wgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "W = 32"),
    ("wgrad-C24", "sgx_rgbconv_wgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "C = 24"),
    ("wgrad-fp32", "sgx_rgbconv_wgrad", EUNSUPPORTED, "sgx_rgbconv_ok == 0", "dtype fp32"),
    ("wgrad-noones-db0", "sgx_rgbconv_wgrad", EINVAL, "bias gradients need the bias channel", "ones = 0 with db0 given"),
    ("wgrad-ws-short", "sgx_rgbconv_wgrad", EWORKSPACE, "rgbconv_wgrad: workspace", "a workspace 4 bytes short"),
    ("tune-variant3", "sgx_rgbconv_tune", EINVAL, "forward variant 3", "variant 3"),
    ("tune-nit9", "sgx_rgbconv_tune", EINVAL, "9 six-row steps", "nit = 9"),
    ("tune-dbg1", "sgx_rgbconv_tune", EINVAL, "ablation mask 1", "dbg = 1"),
]


# ---------------------------------------------------------------------------------------------------------------- the criteria
def _first(bad, shape):
    i = int(bad.flatten().nonzero().flatten()[0])
    return i, tuple(int(v) for v in np.unravel_index(i, tuple(shape)))


def assert_bf16_bits(got, exact, what, where=None):
    """A bf16 output (or pack) against bf16_rn of the exact value, bit for bit; ``where``: only those elements."""
    want = bf16_rn(exact).to(got.device)
    ne = got.view(torch.int16) != want.view(torch.int16)
    if where is not None:
        ne &= where.to(got.device)
    if bool(ne.any()):
        i, at = _first(ne, got.shape)
        raise AssertionError(f"{what}: {int(ne.sum())} of {got.numel() if where is None else int(where.sum())} elements differ from the exact value's bf16; first at flat index "
                             f"{i} {at}: got {float(got.flatten()[i])!r}, exact {float(exact.flatten()[i])!r}")
    return 0.0


def assert_sign_bits(bits, z, what, sure=None):
    """bits[..., C / 8] against z > 0 (bit j of byte v: channel 8 v + j); ``sure``: only those elements (a ``real`` row's |z| above its bound)."""
    got = SR.unpack_bits(bits, z.shape[-1])
    ne = got != (z > 0).to(got.device)
    if sure is not None:
        ne &= sure.to(got.device)
    if bool(ne.any()):
        i, at = _first(ne, z.shape)
        raise AssertionError(f"{what}: {int(ne.sum())} sign bits differ from z > 0; first at (b, y, x, channel) = {at}: z = {float(z.flatten()[i])!r}, bit "
                             f"{int(got.flatten()[i])}")


def check_fwd_int(y, bits, z, variant, what):
    """An integer row of the forward with the blur against its exact pre-activation z -> worst err / bound of the elements under the chain
    bound (0 when all are exact).  Variant 0: an output whose window holds no negative z is bf16_rn(blur(lrelu(z))) bit for bit (x / 16 and
    the four adds are exact), the others meet N_BLUR0 roundings on S = blur|lrelu z|.  Variants 1 / 2: the reference is the blur of the tile
    as LDS holds it, bf16_rn(fl32(lrelu z)); exact windows as before, the others N_BLUR1 roundings."""
    a = lrelu(z) if variant == 0 else tile_act(z)
    ref, S = blur(a), blur(a.abs())
    exact = fwd_exact_mask(z)
    assert_bf16_bits(y, ref, what + " (windows without a negative pre-activation)", exact)
    r = SR.assert_elementwise(y, ref, S, N_BLUR0 if variant == 0 else N_BLUR1, torch.bfloat16, what)
    if bits is not None:
        assert_sign_bits(bits, z, what)
    return r if not bool(exact.all()) else 0.0


def check_fwd_real(y, bits, z, dz, variant, what):
    """A ``real`` row: the pre-activation carries dz (operand_error); LeakyReLU is 1-Lipschitz and the blur's weights are positive and
    sum to 1, so dz passes through as blur(dz).  Variant 0 adds N_BLUR0 fp32 roundings on S and the bf16 store.  Variants 1 / 2 round the
    activation a to bf16 in between: against bf16_rn(a) the kernel's tile value is off by at most dz (1 + 2^-8) + 2 * 2^-8 |a| (both are
    roundings of values dz apart).  A sign bit is compared only where |z| > dz."""
    if variant == 0:
        a = lrelu(z)
        da = dz
        n = N_BLUR0
    else:
        a = tile_act(z)
        da = dz * (1 + R_BF16) + 2 * R_BF16 * a.abs()
        n = N_BLUR1
    ref, S = blur(a), blur(a.abs())
    r = ER.assert_within(y, ref, R_BF16 * ref.abs() + (n + 2) * U32 * S + blur(da), what)
    if bits is not None:
        assert_sign_bits(bits, z, what, z.abs() > dz)
    return r


def unpack_wf(wf):
    """wf[ky][o][k = kx * 4 + j] -> W4[o][j][ky][kx]: the forward's weights as the kernel holds them."""
    C = wf.shape[1]
    return wf.reshape(3, C, 4, 4)[:, :, :3, :].permute(1, 3, 0, 2).contiguous()


def check_fwd_operands(y, bits, img, wf, b0, ones, variant, what):
    """A ``real`` row once more, against the kernel's own operands: the fp16 conversion of the image is round-to-nearest-even and wf is what
    the pack kernel wrote (held by the pack rows), so the pre-activation of exactly those operands, zq in fp64, is known, and the kernel's is
    off by the fp32 accumulation alone: N_CONV additions (+ 1 where the bias is added behind the MFMAs) on Sq.  check_fwd_real's operand
    term is a worst case over 27 roundings that no single element comes near; this one leaves 2^-19 of Sq, so a wrong operand format, a
    pixel from the neighbouring column or a sign bit of a pre-activation near zero shows.  wf: fp64 values [3][C][16]."""
    zq, Sq = conv4(with_ones(img.to(torch.float16).double(), ones), unpack_wf(wf), b0)
    return check_fwd_real(y, bits, zq, (N_CONV + 1 + 2) * U32 * Sq, variant, what + " (own operands)"), float((zq.abs() <= (N_CONV + 3) * U32 * Sq).double().mean())


def pack_bound(ref, S, C, half_ulp, tiny):
    """|got - ref| <= half an ulp of the pack's format at ref + (C + 3) 2^-24 S: C products summed in fp32, br * bscale, s0 * sr and the final
    multiply; the rounding's half ulp is taken at the fp32 value, hence the (1 + half_ulp) on the fp32 term."""
    e32 = (C + 3) * U32 * S
    return half_ulp * (ref.abs() + e32) + tiny + e32
