"""fp64 restatements of the forward / data-gradient convolution entry points of libsgx_hip.so (the first half of csrc/conv.hip, csrc/conv2.hip),
written from include/sgx.h; the launcher rules restated as pure functions of the shape, the dtype, the environment and the device's CU
count; and the table of cases that walks the launch paths.  Test-side only: nothing here imports the library under test.

Layouts are the C ABI's: activations NHWC, packed weights w[tap][n][k] (n = output channel of the launch, k = reduction channel), bias fp32.
Every value reference returns ``(ref, S)``: the value and the same expression on absolute values.

Two criteria.  Integer rows (operands and weights in [-3, 3], integer bias, power-of-two coefficients): every product and partial sum is an
exact fp32 number whatever the order (|sum| <= 16 taps x 544 channels x 9 < 2^24), so the output equals the fp64 value put through the
epilogue's fp32 operations and one rounding (``exact_store``), bit for bit -- and so does every other launch path of the same problem.
Rounding rows (randn / |randn|): |got - ref| <= r |ref| + (L + 2) 2^-24 S, r = 2^-8 for a bf16 store and 0 for fp32, L the longest fp32
chain of the path (``chain``)."""
import math
from collections import namedtuple

import torch

import streaming_ref as SR

F, H = torch.float32, torch.bfloat16
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
ACT_NONE, ACT_LRELU = 0, 1
GEO_OF = {"S": 0, "D": 1, "U": 2}
TAPS = {0: 9, 1: 16, 2: 16}
MODES = {"S": 0, "D": 1, "U": 2, "UF": 3}


def tname(dt):
    return "float" if dt == F else "bf16_t"


def dn(dt):
    return "f32" if dt == F else "bf16"


def cdiv(a, b):
    return (a + b - 1) // b


def out_hw(geo, Hh, W):
    return (Hh // 2, W // 2) if geo == 1 else ((2 * Hh, 2 * W) if geo == 2 else (Hh, W))


# ---------------------------------------------------------------------------------------------------------------- fp64 references
def conv(x, w, geo):
    """sgx.h, fp64 in and out.  geo 0: y[b,h,w,n] = sum x[b,h+ty-1,w+tx-1,k] w[ty*3+tx][n][k]; 1: y[b,oy,ox,n] = sum x[b,2oy+ky-1,2ox+kx-1,k]
    w[ky*4+kx][n][k]; 2: y[b,iy,ix,n] = sum over (oy,ky),(ox,kx) with 2oy+ky-1 = iy, 2ox+kx-1 = ix of x[b,oy,ox,k] w[ky*4+kx][n][k]."""
    B, Hh, W, K = x.shape
    N = w.shape[1]
    assert w.shape[0] == TAPS[geo] and w.shape[2] == K
    OH, OW = out_hw(geo, Hh, W)
    if geo == 2:
        yp = torch.zeros(B, OH + 2, OW + 2, N, dtype=x.dtype, device=x.device)
        for ky in range(4):
            for kx in range(4):
                yp[:, ky:ky + 2 * Hh:2, kx:kx + 2 * W:2] += x @ w[ky * 4 + kx].t()
        return yp[:, 1:OH + 1, 1:OW + 1].contiguous()
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(B, OH, OW, N, dtype=x.dtype, device=x.device)
    TK, IS = (3, 1) if geo == 0 else (4, 2)
    for ty in range(TK):
        for tx in range(TK):
            y += xp[:, ty:ty + IS * OH:IS, tx:tx + IS * OW:IS] @ w[ty * TK + tx].t()
    return y


def pre_activation(x, w, bias, geo):
    """conv + bias -> (pre, S)."""
    pre, S = conv(x, w, geo), conv(x.abs(), w.abs(), geo)
    if bias is not None:
        pre, S = pre + bias, S + bias.abs()
    return pre, S


def blur121(y):
    """The UNNORMALISED [1,2,1] x [1,2,1] filter with zero padding (sgx_conv4x4s2_up_blur: the caller folds 1 / 16 into the weights) ->
    (blurred, the vertical pass alone)."""
    p = torch.nn.functional.pad(y, (0, 0, 0, 0, 1, 1))
    v = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    p = torch.nn.functional.pad(v, (0, 0, 1, 1))
    return p[:, :, :-2] + 2 * p[:, :, 1:-1] + p[:, :, 2:], v


def slope(m):
    return torch.where(m > 0, 1.0, SR.LRELU).to(torch.float64)


def rgb_resid(pimg, wr, ws, rb, bs1, bs2):
    """sgx_conv4x4s2_down_fade_rgb's residual before its rounding: (rb bs1) bs2 + ws (r wr[c][0] + g wr[c][1] + b wr[c][2]) -> (ref, S)."""
    v, S = ws * (pimg @ wr.t()), abs(ws) * (pimg.abs() @ wr.abs().t())
    if rb is not None:
        v, S = v + rb * bs1 * bs2, S + (rb * bs1 * bs2).abs()
    return v, S


def pack_weight(w, Ipad, mode, scale):
    """sgx_pack_weight -> (fwd [taps][O][Ipad], adj [taps][Ipad][O], S_fwd, S_adj) in fp64 from the parameter w [O][I][3][3]."""
    O, I = w.shape[:2]

    def taps(w):
        if mode == "S":
            return scale * w.reshape(O, I, 9).permute(2, 0, 1)
        k3 = w.flip(2, 3) if mode == "UF" else w
        p = torch.nn.functional.pad(k3, (1, 1, 1, 1))                  # sum over (a, b) in {0, 1}^2 of w[ky - a][kx - b], zero outside
        k4 = p[:, :, 1:5, 1:5] + p[:, :, 0:4, 1:5] + p[:, :, 1:5, 0:4] + p[:, :, 0:4, 0:4]
        return scale * (0.25 if mode == "D" else 1.0) * k4.reshape(O, I, 16).permute(2, 0, 1)

    out = []
    for t in (taps(w), taps(w.abs()).abs()):
        fwd = torch.nn.functional.pad(t, (0, Ipad - I))
        adj = fwd.permute(0, 2, 1)
        out.append((fwd.contiguous(), (adj.flip(0) if mode == "S" else adj).contiguous()))
    return out[0][0], out[0][1], out[1][0], out[1][1]


# sgx_pack_upblur's 1-D composition (the table in its comment; k = [1, 2, 1] blur taps, w = the four taps of the transposed kernel, output
# Y = 2 i + p, input rows i - 1, i, i + 1 <-> d = 0, 1, 2): (p, d) -> [(blur tap, kernel tap), ...]
UPBLUR_TERMS = {(0, 0): ((0, 2), (1, 3)), (0, 1): ((0, 0), (1, 1), (2, 2)), (0, 2): ((2, 0),), (1, 0): ((0, 3),), (1, 1): ((0, 1), (1, 2), (2, 3)), (1, 2): ((1, 0), (2, 1))}


def upblur_taps(w, mode, adjoint, scale):
    """The 4x4 taps T[ky * 4 + kx][n][k] of the transposed convolution behind sgx_pack_upblur: the layer's own pack (modes U / UF, adjoint 0:
    (n, k) = (o, i)) or the adjoint pack of a down layer (mode D, adjoint 1: (n, k) = (i, o)), as sgx_pack_weight synthesises them."""
    fwd, adj, _, _ = pack_weight(w, w.shape[1], mode, scale)
    return adj if adjoint else fwd


def pack_upblur_main(w, mode, adjoint, scale):
    """The 9 composite taps of sgx_pack_upblur, [9][4 N][K] in fp64: slot dy * 3 + dx, row (px * 2 + py) * N + n."""
    T = upblur_taps(w, mode, adjoint, scale)
    N, K = T.shape[1:]
    kb = (1.0, 2.0, 1.0)
    out = torch.zeros(9, 4 * N, K, dtype=torch.float64, device=w.device)
    for dy in range(3):
        for dx in range(3):
            for py in range(2):
                for px in range(2):
                    v = sum(kb[ay] * kb[ax] * T[wy * 4 + wx] for ay, wy in UPBLUR_TERMS[py, dy] for ax, wx in UPBLUR_TERMS[px, dx])
                    out[dy * 3 + dx, (px * 2 + py) * N:(px * 2 + py + 1) * N] = v
    return out


def conv_upblur(x, w, mode, adjoint, scale):
    """sgx_conv_upblur on top of sgx_pack_upblur(w): blur3x3(conv_transpose(x)) with the blur's 1 / 16 inside `scale` -> (ref, the transposed
    convolution, its vertical pass)."""
    ct = conv(x, upblur_taps(w, mode, adjoint, scale), 2)
    blur, vert = blur121(ct)
    return blur, ct, vert


def exact_store(pre, bias, act, mask, dtype):
    """An integer row's expected output: the exact pre-bias sums (fp64 integers below 2^24) through the store epilogue's fp32 operations --
    + bias, LeakyReLU (one fp32 product with the slope as the kernels hold it), ONE rounding to the storage type, and the output mask on the
    rounded value (bf16: bf16 -> fp32, times the slope, rounded again: sgx_lrelu_bwd on the stored tensor; fp32: one product)."""
    v = pre.float()
    assert torch.equal(v.double(), pre), "the sums of an integer row are exact in fp32"
    if bias is not None:
        v = v + bias.float()
    if act == ACT_LRELU:
        v = torch.where(v > 0, v, v * torch.tensor(SR.LRELU, dtype=F, device=v.device))
    y = v.to(dtype)
    if mask is not None:
        y = (y.float() * torch.where(mask.float() > 0, 1.0, SR.LRELU).float()).to(dtype)
    return y


def chain(geo, Cin, bias=True, act=True, splits=1, extra=0):
    """L of a convolution's store: the taps that meet in one output (9 / 16 / 4 for the transposed geometry: one 2x2 class) x Cin products
    accumulated in fp32, any order; + 1 for the bias, + 1 for the LeakyReLU product; split-K adds the sum of the splits; ``extra`` what a
    fused epilogue adds."""
    return {0: 9, 1: 16, 2: 4}[geo] * Cin + (1 if bias else 0) + (1 if act else 0) + (splits if splits > 1 else 0) + extra


# ---------------------------------------------------------------------------------------------------------------- launcher rules
ENV0 = {"SGX_CONV2": 15, "SGX_CONV2_NW": 0, "SGX_CONV2_NW16": 0, "SGX_CONV2_SMALL": 1, "SGX_CONV2_BPC": 2, "SGX_CONV_NT": 0, "SGX_CONVU_REGSTORE": 0,
        "SGX_CONV_UPBLUR": 1, "SGX_UPBLUR_BPC": 1, "SGX_CONV_UP_BLUR": 1, "SGX_SIGNBITS": 1, "SGX_FUSE_FADE": 1, "SGX_CONV_PERCU": 0, "SGX_CONV_MAXCT": 4,
        "SGX_CONV_MAXBP": 256, "SGX_CONV_MINBLOCKS": 0, "SGX_CONV_DEEPK": 1, "SGX_CONV_UPA": 1, "SGX_CONV_SPLITK": 1, "SGX_TILE_BANDS": 1, "SGX_NT_MIN_MB": 192}
GROUPS = {"default": {}, "conv2_0": {"SGX_CONV2": "0"}, "conv2_31": {"SGX_CONV2": "31"}, "nw4": {"SGX_CONV2_NW": "4", "SGX_CONV2_NW16": "4"},
          "nw8": {"SGX_CONV2_NW": "8", "SGX_CONV2_NW16": "8"}, "small0": {"SGX_CONV2_SMALL": "0"}, "bpc1": {"SGX_CONV2_BPC": "1"},
          "regstore": {"SGX_CONVU_REGSTORE": "1"}, "nt3": {"SGX_CONV_NT": "3", "SGX_NT_MIN_MB": "0.001"}, "bands0": {"SGX_TILE_BANDS": "0"},
          "deepk0_upa0": {"SGX_CONV_DEEPK": "0", "SGX_CONV_UPA": "0"}, "splitk0": {"SGX_CONV_SPLITK": "0"}, "splitk2": {"SGX_CONV_SPLITK": "2"},
          "percu1": {"SGX_CONV_PERCU": "1"}, "bigtile": {"SGX_CONV_MINBLOCKS": "1"}, "smalltile": {"SGX_CONV_MINBLOCKS": "1000000", "SGX_CONV_MAXBP": "64", "SGX_CONV_MAXCT": "1"},
          "upblur_bpc2": {"SGX_UPBLUR_BPC": "2"},
          "fused0": {"SGX_CONV_UP_BLUR": "0", "SGX_SIGNBITS": "0", "SGX_FUSE_FADE": "0", "SGX_CONV_UPBLUR": "0"}}


def group_env(group):
    return dict(ENV0, **{k: (float(v) if "." in v else int(v)) for k, v in GROUPS[group].items()})


Pick = namedtuple("Pick", "nw mf2 k16")
NONE = Pick(0, False, False)


def conv2_pick(geo, B, Hh, W, Cin, Cout, env, ncu, variant=-1, allow_u16=False):
    """conv2.hip conv2_pick: nw = 0 leaves the shape to the first generation."""
    on = env["SGX_CONV2"]
    if variant < 0 and not (on >> geo) & 1:
        return NONE
    gw, gh = (W // 2, Hh // 2) if geo == 1 else (W, Hh)
    t8, t4 = B * cdiv(gh, 16) * (gw // 32), B * cdiv(gh, 8) * (gw // 32)
    kc16, co16 = Cin == 16, Cout == 16
    odd = geo == 1 and ((Hh | W) & 1)
    if kc16 or co16:
        ok = (geo == 0 and kc16 and co16) or (geo == 1 and kc16 and Cout == 32) or (geo == 2 and Cin == 32 and co16)
        if not ok or gw % 32 or gh < 1 or odd:
            return NONE
        if variant < 0 and not on & 8:
            return NONE
        if variant < 0 and geo == 2 and not on & 16 and not allow_u16:
            return NONE
        if variant < 0 and t4 < ncu:
            return NONE
        f16 = env["SGX_CONV2_NW16"]
        return Pick(variant if variant > 0 else (f16 or (8 if t8 >= 2 * ncu else 4)), False, True)
    bco = 64 if geo == 0 and Cout % 64 == 0 else 32
    if Cin % 32 or Cout % bco or gw % 32 or Cout // bco > 32 or gh < 1 or odd:
        return NONE
    mf2 = geo != 2 and Cout % 64 == 0
    if variant < 0 and geo == 1 and not mf2:
        return NONE
    fnw, c64, c32 = env["SGX_CONV2_NW"], Cout // 64, Cout // 32
    if mf2 and variant < 0 and not fnw and env["SGX_CONV2_SMALL"] and t8 * c64 < ncu:
        if t8 * c32 >= ncu:
            return Pick(8, False, False)
        if geo == 0:
            return Pick(4, False, False) if t4 * c32 >= ncu else NONE
    nb = c64 if mf2 else c32
    if variant < 0 and not fnw and t4 * nb < ncu:
        return NONE
    return Pick(variant if variant > 0 else (fnw or (8 if t8 * nb >= ncu else 4)), mf2, False)


def conv2_inst(geo, p, epi=0):
    """conv2_run: (NW, MF, KC, CO16) of the instantiation that runs a pick."""
    if p.k16:
        return (p.nw, 1, 32 if geo == 2 else 16, geo != 1)
    return (p.nw, 2 if (p.mf2 and geo != 2) else 1, 32, False)


def conv2_name(geo, p, epi=0):
    nw, mf, kc, co16 = conv2_inst(geo, p)
    return f"conv2_kernel<{geo}, {nw}, {mf}, {kc}, {'true' if co16 else 'false'}, {epi}>"


G2 = {0: dict(HALO=2, NTW=9), 1: dict(HALO=1, NTW=4), 2: dict(HALO=2, NTW=16)}


def c2_lds(geo, nw, mf, kc, epi):
    """C2Lds<GEO, NW, MF, KC>::TOTAL + the epilogue's coefficient table, as launch_conv2 asks for it."""
    th, bco, spr = 2 * nw, mf * 32, kc // 8
    prows, wrows, orow = (th + G2[geo]["HALO"]) * (32 + G2[geo]["HALO"]), G2[geo]["NTW"] * bco, bco * 2 + 16
    scratch = 0 if mf > 2 else nw * (64 if geo == 2 else 32) * orow
    p_bytes = cdiv(max(cdiv(prows * spr, 64) * 1024, scratch), 1024) * 1024
    return 2 * (p_bytes + wrows * spr // 64 * 1024) + (1024 if epi != 0 or geo == 1 else 0)


Grid = namedtuple("Grid", "tiles_x tiles_y ntiles ncb nslots bands blocks")


def plan_grid(geo, B, Hh, W, Cout, th, lds, nw, kc, bco, env, ncu, ub=0, overlap=False):
    """conv2.hip conv2_plan_grid."""
    gh, gw = (Hh // 2, W // 2) if geo == 1 else (Hh, W)
    tx, ty = cdiv(gw, 32), cdiv(gh, th)
    if overlap:
        ty = 1 if gh <= th else (gh - th + th - 2) // (th - 1) + 1
        tx = 1 if gw <= 32 else (gw - 32 + 30) // 31 + 1
    ntiles, ncb = B * ty * tx, Cout // bco
    bpc = 1
    if kc == 16:
        bpc = max(1, min(160 * 1024 // lds, 32 // nw, env["SGX_CONV2_BPC"]))
    elif ub == 2:
        bpc = 160 * 1024 // lds
    per = max(1, min(ncu * bpc // (8 * ncb), cdiv(ntiles, 8)))
    bands = 1 if env["SGX_TILE_BANDS"] and ntiles >= 8 * per * 8 else 0
    return Grid(tx, ty, ntiles, ncb, per * 8, bands, ncb * per * 8)


def conv2_grid(geo, p, B, Hh, W, Cout, env, ncu, epi=0):
    nw, mf, kc, co16 = conv2_inst(geo, p)
    return plan_grid(geo, B, Hh, W, Cout, 2 * nw, c2_lds(geo, nw, mf, kc, epi), nw, kc, 16 if co16 else mf * 32, env, ncu, overlap=epi == 2)


Cfg = namedtuple("Cfg", "bp ct th tw ni")
CAND = {0: ((256, 4), (256, 2), (128, 4), (256, 1), (128, 2), (128, 1), (64, 2), (64, 1)), 1: ((128, 2), (128, 1), (64, 2), (64, 1)),
        3: ((256, 2), (256, 1), (128, 2), (128, 1), (64, 2), (64, 1))}
CAND[2] = CAND[0]


def tile_shape(bp, ohc, owc):
    th, tw = (bp // 16, 16) if ohc >= 16 and owc >= 16 else ((8, 8) if ohc >= 8 and owc >= 8 else (4, 4))
    return th, tw, bp // (th * tw)


def tile_extent(geo, n):
    return n // 2 if geo == 1 else n                       # (the transposed geometry tiles its coarse input)


def pick_cfg(geo, B, ohc, owc, Cout, env):
    """conv.hip pick_cfg (geo 3 = GUPA): the first candidate that reaches the block target, else the last that fits."""
    best = Cfg(0, 0, 0, 0, 0)
    for bp, ct in CAND[geo]:
        if ct > env["SGX_CONV_MAXCT"] or bp > env["SGX_CONV_MAXBP"] or Cout % (16 * ct):
            continue
        th, tw, ni = tile_shape(bp, ohc, owc)
        if ni < 1:
            continue
        best = Cfg(bp, ct, th, tw, ni)
        blocks = cdiv(B, ni) * cdiv(ohc, th) * cdiv(owc, tw) * (Cout // (16 * ct)) * (4 if geo == 2 else 1)
        if blocks >= (env["SGX_CONV_MINBLOCKS"] if env["SGX_CONV_MINBLOCKS"] > 0 else 512):
            break
    return best


def conv_deep_k(geo, B, ohc, owc, Cin, Cout, env):
    if not env["SGX_CONV_DEEPK"] or Cin % 128 or geo == 1:
        return False
    c = pick_cfg(geo, B, ohc, owc, Cout, env)
    return c.bp == 64 and c.ct in (1, 2)


def g1name(dt, kc, geo, th, tw, bp, ct, sk=False):
    return f"conv_kernel<{tname(dt)}, {kc}, {geo}, {th}, {tw}, {bp}, {ct}, {'true' if sk else 'false'}>"


def dispatch_conv(geo, dt, B, Hh, W, Cin, Cout, env, sk=False):
    """conv.hip dispatch_conv / dispatch_cfg / dispatch_tile -> (rc, the conv_kernel instantiation)."""
    if Cout % 16 or Cin % 16:
        return EUNSUPPORTED, None
    if B <= 0 or Hh <= 0 or W <= 0:
        return EINVAL, None
    ohc, owc = tile_extent(geo, Hh), tile_extent(geo, W)
    if dt == F:
        kc, g = 16, geo
    elif geo != 1 and conv_deep_k(geo, B, ohc, owc, Cin, Cout, env):
        c = pick_cfg(geo, B, ohc, owc, Cout, env)
        return 0, g1name(dt, 128, geo, c.th, c.tw, 64, 2 if c.ct == 2 else 1, sk)
    else:
        kc, g = (32 if Cin % 32 == 0 else 16), (3 if geo == 2 and env["SGX_CONV_UPA"] else geo)
    c = pick_cfg(g, B, ohc, owc, Cout, env)
    if not c.bp:
        return EUNSUPPORTED, None
    if sk and (c.bp > 128 or c.ct > 2):
        return EUNSUPPORTED, None
    return 0, g1name(dt, kc, g, c.th, c.tw, c.bp, c.ct, sk)


def conv_config(geo, dt, B, Hh, W, Cin, Cout, env):
    """sgx_conv_config's cfg5.  geo 3: the transposed convolution as its launch runs it (the bf16 launch without deep K-chunks: the all-class
    kernel, whose candidates are its own); geo 2 answers for the per-class kernel whatever runs."""
    launched, geo = geo == 3, min(geo, 2)
    ohc, owc = tile_extent(geo, Hh), tile_extent(geo, W)
    deep = dt != F and conv_deep_k(geo, B, ohc, owc, Cin, Cout, env)
    c = pick_cfg(3 if launched and dt == H and not deep and env["SGX_CONV_UPA"] else geo, B, ohc, owc, Cout, env)
    return [16 if dt == F else (128 if deep else (32 if Cin % 32 == 0 else 16)), c.th, c.tw, c.bp, c.ct]


def conv_splitk_plan(geo, dt, B, Hh, W, Cin, Cout, env, ncu):
    on = 1 if env["SGX_CONV_SPLITK"] < 0 else env["SGX_CONV_SPLITK"]
    if not on or dt != H or geo not in (0, 1, 2) or Cin % 16 or Cout % 16 or geo != 1:
        return 0
    if conv2_pick(geo, B, Hh, W, Cin, Cout, env, ncu).nw:
        return 0
    ohc, owc = tile_extent(geo, Hh), tile_extent(geo, W)
    c = pick_cfg(geo, B, ohc, owc, Cout, env)
    if not c.bp or c.bp > 128 or c.ct > 2:
        return 0
    nk = Cin // (32 if Cin % 32 == 0 else 16)
    blocks = cdiv(B, c.ni) * cdiv(ohc, c.th) * cdiv(owc, c.tw) * (Cout // (16 * c.ct))
    if nk < 4 or blocks > ncu:
        return 0
    want = min(cdiv(2 * ncu, blocks), on if on > 1 else 8, nk // 2)
    return want if want >= 2 else 0


def splitk_ws_bytes(geo, dt, B, Hh, W, Cin, Cout, env, ncu):
    OH, OW = out_hw(geo, Hh, W)
    return conv_splitk_plan(geo, dt, B, Hh, W, Cin, Cout, env, ncu) * B * OH * OW * Cout * 4


def stats_nparts(dt, B, Hh, W, Cin, Cout, env, ncu):
    if dt != H:
        return 0
    p = conv2_pick(0, B, Hh, W, Cin, Cout, env, ncu)
    return conv2_grid(0, p, B, Hh, W, Cout, env, ncu, epi=1).nslots if p.nw else 0


def signbits_ok(dt, B, Hh, W, Cin, Cout, env, ncu):
    return int(dt == H and Cout % 8 == 0 and bool(env["SGX_SIGNBITS"]) and conv2_pick(0, B, Hh, W, Cin, Cout, env, ncu).nw != 0)


def down_fade_ok(dt, B, Hh, W, Cin, Cout, env, ncu):
    return int(dt == H and Cout % 8 == 0 and bool(env["SGX_FUSE_FADE"]) and conv2_pick(1, B, Hh, W, Cin, Cout, env, ncu).nw != 0)


def up_blur_ok(dt, B, Hh, W, Cin, Cout, env, ncu):
    return int(dt == H and bool(env["SGX_CONV_UP_BLUR"]) and conv2_pick(2, B, Hh, W, Cin, Cout, env, ncu, allow_u16=True).nw != 0)


def upblur_ok(dt, B, Hh, W, Cin, Cout, env):
    return int(bool(env["SGX_CONV_UPBLUR"]) and dt == H and Cin == 32 and Cout == 16 and W % 32 == 0 and B > 0 and Hh > 0)


def upblur_kernel(B, Hh, W, env, ncu):
    """sgx_conv_upblur: 8-wave blocks once their tiles fill the chip, else 4 waves; SGX_UPBLUR_BPC=2: the compact block."""
    t8, t4 = B * cdiv(Hh, 16) * (W // 32), B * cdiv(Hh, 8) * (W // 32)
    if env["SGX_UPBLUR_BPC"] == 2 and t4 >= 2 * ncu:
        return "conv3_kernel<0, 4, 2, 2, 2, 0, 2>"
    return "conv3_kernel<0, 8, 2, 2, 2, 0, 1>" if t8 >= ncu else "conv3_kernel<0, 4, 2, 2, 2, 0, 1>"


C3 = {0: (8, 2, 1, 0), 1: (8, 2, 2, 0), 2: (8, 2, 2, 1), 3: (4, 4, 1, 0), 4: (4, 4, 2, 0), 5: (4, 4, 1, 1), 6: (4, 2, 2, 0)}    # id -> NW, RPW, PD, DIL


def conv3_name(geo, vid):
    nw, rpw, pd, dil = C3[vid]
    return f"conv3_kernel<{geo}, {nw}, 2, {rpw}, {pd}, {dil}, 0>"


def shape_s(B, Hh, W, Cin, Cout):
    return f"B{B} {Hh}x{W} {Cin}->{Cout}"


Plan = namedtuple("Plan", "rc kernels notes ksplit")


def plan(entry, dt, a, env, ncu):
    """What one call launches -> (return code, the kernel instantiations in order, the launch notes the profiler shows, the split-K ways)."""
    B, Hh, W, Cin, Cout = a["B"], a["H"], a["W"], a["Cin"], a["Cout"]
    s = shape_s(B, Hh, W, Cin, Cout)
    fail = lambda rc: Plan(rc, (), (), 0)
    one = lambda k, note: Plan(0, (k,), (note,), 0)
    if entry in ("sgx_conv3x3", "sgx_conv4x4s2_down", "sgx_conv4x4s2_up"):
        geo = {"sgx_conv3x3": 0, "sgx_conv4x4s2_down": 1, "sgx_conv4x4s2_up": 2}[entry]
        if geo == 1 and (Hh % 2 or W % 2):
            return fail(EINVAL)
        note = f"conv{'SDU'[geo]} {s}"
        if dt == H:
            p = conv2_pick(geo, B, Hh, W, Cin, Cout, env, ncu)
            if p.nw:
                return one(conv2_name(geo, p), note)
        rc, k = dispatch_conv(geo, dt, B, Hh, W, Cin, Cout, env)
        return one(k, note) if rc == 0 else fail(rc)
    if entry == "sgx_conv_variant":
        geo, v = a["geo"], a["variant"]
        if geo == 1 and (Hh % 2 or W % 2):
            return fail(EINVAL)
        note = f"conv{'SDU'[geo]}/v{v} {s}"
        if v == 0:
            rc, k = dispatch_conv(geo, dt, B, Hh, W, Cin, Cout, env)
            return one(k, note) if rc == 0 else fail(rc)
        if dt != H:
            return fail(EINVAL)
        if v >= 30:
            gw = W // 2 if geo == 1 else W
            if geo not in (0, 1) or Cin % 32 or Cout % 64 or gw % 32 or Cout // 64 > 32 or (geo == 1 and ((Hh | W) & 1)) or v > 36:
                return fail(EUNSUPPORTED)
            return one(conv3_name(geo, v - 30), note)
        p = conv2_pick(geo, B, Hh, W, Cin, Cout, env, ncu, variant=v)
        return one(conv2_name(geo, p), note) if p.nw else fail(EUNSUPPORTED)
    if entry == "sgx_conv_splitk":
        geo = a.get("geo", 1)
        ks = conv_splitk_plan(geo, dt, B, Hh, W, Cin, Cout, env, ncu)
        if ks <= 1:
            return fail(EUNSUPPORTED)
        if a.get("ws") == "short":
            return fail(EWORKSPACE)
        rc, k = dispatch_conv(1, dt, B, Hh, W, Cin, Cout, env, sk=True)
        return Plan(0, (k, "conv_splitk_finish"), (f"convD/k{ks} {s}", f"conv_splitk_finish {B * (Hh // 2) * (W // 2)}x{Cout}"), ks)
    if entry in ("sgx_conv3x3_signbits", "sgx_conv3x3_stats"):
        if dt != H:
            return fail(EUNSUPPORTED)
        p = conv2_pick(0, B, Hh, W, Cin, Cout, env, ncu)
        if not p.nw or Cout % 8:
            return fail(EUNSUPPORTED)
        if entry == "sgx_conv3x3_stats":
            if a.get("part") == "short":
                return fail(EWORKSPACE)
            if a.get("part") == "other":
                return fail(EINVAL)
            return one(conv2_name(0, p, 1), f"convS+stats {s}")
        return one(conv2_name(0, p), f"convS+bits {s}")
    if entry in ("sgx_conv4x4s2_up_blur", "sgx_conv4x4s2_up_blur_bits"):
        if dt != H:
            return fail(EUNSUPPORTED)
        p = conv2_pick(2, B, Hh, W, Cin, Cout, env, ncu, allow_u16=True)
        if not p.nw:
            return fail(EUNSUPPORTED)
        tag = "*bits" if entry.endswith("bits") else ("*mask" if a.get("mask") else "")
        return one(conv2_name(2, p, 2), f"convU+blur{tag} {s}")
    if entry in ("sgx_conv4x4s2_down_fade", "sgx_conv4x4s2_down_fade_rgb"):
        if dt != H:
            return fail(EUNSUPPORTED)
        p = conv2_pick(1, B, Hh, W, Cin, Cout, env, ncu)
        if not p.nw or Cout % 8:
            return fail(EUNSUPPORTED)
        return one(conv2_name(1, p), f"convD+fade{'(rgb)' if entry.endswith('rgb') else ''} {s}")
    if entry == "sgx_conv_upblur":
        if not (dt == H and Cin == 32 and Cout == 16 and W % 32 == 0 and B > 0 and Hh > 0):
            return fail(EUNSUPPORTED)
        return one(upblur_kernel(B, Hh, W, env, ncu), f"convU*blur{'*bits' if a.get('bits') else ''} {s}")
    if entry == "sgx_pack_upblur":
        return Plan(0, ("pack_upblur_kernel",), (None,), 0)               # (the launch carries no note)
    if entry == "sgx_pack_weight":
        return one(f"pack_weight_kernel<{tname(dt)}>", f"pack {a['O']}x{a['I']} m{MODES[a['mode']]}")
    if entry == "sgx_pack_weight_multi":
        return one(f"pack_weight_multi_kernel<{tname(dt)}>", f"pack_multi n{a['n']}")
    raise KeyError(entry)


# ---------------------------------------------------------------------------------------------------------------- the case table
# entry: the C ABI function; group: the environment it needs (GROUPS); args: B, H, W (the INPUT's size, as the ABI takes it), Cin, Cout, data
# ("int" | "randn" | "abs"), bias / act / mask (the store epilogue), twin: the default-environment row whose bits an integer row must
# equal, rc: the documented return code (rows with rc != 0 launch nothing and write nothing); kernels: every launch in order at 256 CUs
# (k304: at 304 CUs, where it differs); why: the launcher rule that selects them.
Case = namedtuple("Case", "id entry dtype group args kernels why")
CASES = []
ENTRY = {"S": "sgx_conv3x3", "D": "sgx_conv4x4s2_down", "U": "sgx_conv4x4s2_up"}


def _case(id, entry, dt, kernels, why, B, Hh, W, Cin, Cout, data="int", bias=True, act=ACT_LRELU, mask=False, group="default", twin=None, rc=0, k304=None, **more):
    geo_less = entry in ("sgx_conv4x4s2_up", "sgx_conv4x4s2_up_blur", "sgx_conv4x4s2_up_blur_bits", "sgx_conv_upblur", "sgx_pack_upblur") or more.get("geo") == 2
    args = dict(B=B, H=Hh, W=W, Cin=Cin, Cout=Cout, data=data, bias=bias and not geo_less, act=ACT_NONE if geo_less else act, mask=mask, twin=twin, rc=rc,
                k304=tuple(k304) if k304 else None, **more)
    CASES.append(Case(id, entry, dt, group, args, tuple(kernels), why))


def k2(geo, nw, mf, kc=32, co16=False, epi=0):
    return f"conv2_kernel<{geo}, {nw}, {mf}, {kc}, {'true' if co16 else 'false'}, {epi}>"


FIN = "conv_splitk_finish"

# ---- every conv_kernel / conv2_kernel instantiation the default environment reaches over the shape grid of tests/test_conv_coverage.py, each
# on the smallest ragged shape of that grid that selects it at 256 AND at 304 CUs (the first generation's choice does not read the CU count;
# the second generation's shapes sit clear of its thresholds): kernel, geometry, dtype, B, H, W, Cin, Cout.  An integer row each, with bias,
# LeakyReLU and (3x3) the output mask; a randn row too where the operands stay under AUTO_RANDN_BYTES.
AUTO = (
    ("conv2_kernel<0, 4, 1, 16, true, 0>", "S", H, 33, 34, 64, 16, 16),   # 4.4 MB
    ("conv2_kernel<0, 4, 1, 32, false, 0>", "S", H, 5, 9, 32, 32, 1024),   # 2.9 MB
    ("conv2_kernel<0, 8, 1, 16, true, 0>", "S", H, 17, 136, 128, 16, 16),   # 18.1 MB
    ("conv2_kernel<0, 8, 1, 32, false, 0>", "S", H, 5, 17, 32, 32, 1024),   # 5.5 MB
    ("conv2_kernel<0, 8, 2, 32, false, 0>", "S", H, 5, 17, 32, 32, 2048),   # 10.8 MB
    ("conv2_kernel<1, 4, 1, 16, false, 0>", "D", H, 17, 136, 128, 16, 32),   # 13.5 MB
    ("conv2_kernel<1, 8, 1, 16, false, 0>", "D", H, 5, 520, 512, 16, 32),   # 62.0 MB: 680 tiles of 16x32 >= 2 x 304 CUs, the smallest ragged batch of 520x512 images
    ("conv2_kernel<1, 8, 1, 32, false, 0>", "D", H, 5, 34, 64, 32, 1024),   # 6.0 MB
    ("conv2_kernel<1, 8, 2, 32, false, 0>", "D", H, 2, 136, 128, 32, 1024),   # 19.1 MB
    ("conv2_kernel<2, 4, 1, 32, false, 0>", "U", H, 5, 9, 32, 32, 1024),   # 11.3 MB
    ("conv2_kernel<2, 8, 1, 32, false, 0>", "U", H, 5, 17, 32, 32, 1024),   # 21.4 MB
    ("conv_kernel<bf16_t, 128, 0, 4, 16, 64, 1, false>", "S", H, 1, 17, 19, 128, 16),   # 0.1 MB
    ("conv_kernel<bf16_t, 128, 0, 4, 4, 64, 1, false>", "S", H, 1, 1, 1, 128, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 128, 0, 8, 8, 64, 1, false>", "S", H, 1, 9, 13, 128, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 128, 2, 4, 16, 64, 1, false>", "U", H, 1, 17, 19, 128, 16),   # 0.1 MB
    ("conv_kernel<bf16_t, 128, 2, 4, 4, 64, 1, false>", "U", H, 1, 1, 1, 128, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 128, 2, 8, 8, 64, 1, false>", "U", H, 1, 9, 13, 128, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 0, 16, 16, 256, 1, false>", "S", H, 17, 17, 19, 16, 128),   # 1.5 MB
    ("conv_kernel<bf16_t, 16, 0, 16, 16, 256, 2, false>", "S", H, 33, 17, 19, 16, 128),   # 2.9 MB
    ("conv_kernel<bf16_t, 16, 0, 16, 16, 256, 4, false>", "S", H, 33, 33, 35, 16, 128),   # 10.5 MB
    ("conv_kernel<bf16_t, 16, 0, 4, 16, 64, 1, false>", "S", H, 1, 17, 19, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 0, 4, 4, 64, 1, false>", "S", H, 1, 1, 1, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 0, 8, 16, 128, 1, false>", "S", H, 17, 17, 19, 16, 96),   # 1.2 MB
    ("conv_kernel<bf16_t, 16, 0, 8, 8, 128, 1, false>", "S", H, 33, 9, 13, 16, 128),   # 1.1 MB
    ("conv_kernel<bf16_t, 16, 0, 8, 8, 256, 1, false>", "S", H, 33, 9, 32, 16, 128),   # 2.6 MB
    ("conv_kernel<bf16_t, 16, 0, 8, 8, 64, 1, false>", "S", H, 1, 9, 13, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 1, 4, 16, 64, 1, false>", "D", H, 1, 34, 38, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 1, 4, 4, 64, 1, false>", "D", H, 1, 2, 2, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 1, 8, 16, 128, 1, false>", "D", H, 17, 34, 38, 16, 96),   # 1.7 MB
    ("conv_kernel<bf16_t, 16, 1, 8, 16, 128, 2, false>", "D", H, 33, 34, 38, 16, 96),   # 3.3 MB
    ("conv_kernel<bf16_t, 16, 1, 8, 8, 128, 1, false>", "D", H, 33, 18, 26, 16, 128),   # 1.4 MB
    ("conv_kernel<bf16_t, 16, 1, 8, 8, 64, 1, false>", "D", H, 1, 18, 26, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 3, 16, 16, 256, 1, false>", "U", H, 33, 17, 19, 16, 64),   # 5.5 MB
    ("conv_kernel<bf16_t, 16, 3, 16, 16, 256, 2, false>", "U", H, 33, 17, 19, 16, 128),   # 10.7 MB
    ("conv_kernel<bf16_t, 16, 3, 4, 16, 64, 1, false>", "U", H, 1, 17, 19, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 3, 4, 4, 64, 1, false>", "U", H, 1, 1, 1, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 16, 3, 8, 16, 128, 1, false>", "U", H, 17, 17, 19, 16, 96),   # 4.2 MB
    ("conv_kernel<bf16_t, 16, 3, 8, 8, 128, 1, false>", "U", H, 33, 9, 13, 16, 128),   # 3.9 MB
    ("conv_kernel<bf16_t, 16, 3, 8, 8, 256, 1, false>", "U", H, 33, 9, 32, 16, 128),   # 9.6 MB
    ("conv_kernel<bf16_t, 16, 3, 8, 8, 64, 1, false>", "U", H, 1, 9, 13, 16, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 32, 0, 16, 16, 256, 1, false>", "S", H, 1, 17, 19, 32, 2048),   # 1.3 MB
    ("conv_kernel<bf16_t, 32, 0, 16, 16, 256, 2, false>", "S", H, 2, 17, 19, 32, 2048),   # 2.6 MB
    ("conv_kernel<bf16_t, 32, 0, 16, 16, 256, 4, false>", "S", H, 17, 17, 19, 32, 512),   # 5.7 MB
    ("conv_kernel<bf16_t, 32, 0, 4, 16, 64, 1, false>", "S", H, 1, 17, 19, 32, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 32, 0, 4, 4, 128, 1, false>", "S", H, 33, 1, 1, 32, 2048),   # 0.1 MB
    ("conv_kernel<bf16_t, 32, 0, 4, 4, 256, 1, false>", "S", H, 1, 5, 7, 32, 2048),   # 0.1 MB
    ("conv_kernel<bf16_t, 32, 0, 4, 4, 256, 2, false>", "S", H, 17, 5, 7, 32, 2048),   # 2.4 MB
    ("conv_kernel<bf16_t, 32, 0, 4, 4, 256, 4, false>", "S", H, 33, 6, 10, 32, 2048),   # 7.9 MB
    ("conv_kernel<bf16_t, 32, 0, 4, 4, 64, 1, false>", "S", H, 1, 1, 1, 32, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 32, 0, 8, 16, 128, 1, false>", "S", H, 3, 17, 19, 32, 512),   # 1.0 MB
    ("conv_kernel<bf16_t, 32, 0, 8, 8, 128, 1, false>", "S", H, 3, 9, 13, 32, 1024),   # 0.7 MB
    ("conv_kernel<bf16_t, 32, 0, 8, 8, 256, 1, false>", "S", H, 1, 9, 13, 32, 2048),   # 0.5 MB
    ("conv_kernel<bf16_t, 32, 0, 8, 8, 256, 2, false>", "S", H, 1, 9, 32, 32, 2048),   # 1.1 MB
    ("conv_kernel<bf16_t, 32, 0, 8, 8, 256, 4, false>", "S", H, 33, 9, 13, 32, 1024),   # 7.8 MB
    ("conv_kernel<bf16_t, 32, 0, 8, 8, 64, 1, false>", "S", H, 1, 9, 13, 32, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 32, 1, 4, 16, 64, 1, false>", "D", H, 1, 34, 38, 32, 16),   # 0.1 MB
    ("conv_kernel<bf16_t, 32, 1, 4, 4, 128, 1, false>", "D", H, 33, 2, 2, 32, 2048),   # 0.1 MB
    ("conv_kernel<bf16_t, 32, 1, 4, 4, 128, 2, false>", "D", H, 9, 10, 14, 32, 2048),   # 1.3 MB
    ("conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, false>", "D", H, 1, 2, 2, 32, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 32, 1, 8, 16, 128, 1, false>", "D", H, 3, 34, 38, 32, 512),   # 1.2 MB
    ("conv_kernel<bf16_t, 32, 1, 8, 16, 128, 2, false>", "D", H, 3, 34, 38, 32, 1024),   # 2.1 MB
    ("conv_kernel<bf16_t, 32, 1, 8, 8, 128, 1, false>", "D", H, 1, 18, 26, 32, 2048),   # 0.5 MB
    ("conv_kernel<bf16_t, 32, 1, 8, 8, 128, 2, false>", "D", H, 3, 18, 26, 32, 2048),   # 1.5 MB
    ("conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, false>", "D", H, 1, 18, 26, 32, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 32, 3, 16, 16, 256, 1, false>", "U", H, 1, 17, 19, 32, 2048),   # 5.1 MB
    ("conv_kernel<bf16_t, 32, 3, 16, 16, 256, 2, false>", "U", H, 2, 17, 19, 32, 2048),   # 10.1 MB
    ("conv_kernel<bf16_t, 32, 3, 4, 16, 64, 1, false>", "U", H, 1, 17, 19, 32, 16),   # 0.1 MB
    ("conv_kernel<bf16_t, 32, 3, 4, 4, 128, 1, false>", "U", H, 33, 1, 1, 32, 2048),   # 0.5 MB
    ("conv_kernel<bf16_t, 32, 3, 4, 4, 256, 1, false>", "U", H, 1, 5, 7, 32, 2048),   # 0.5 MB
    ("conv_kernel<bf16_t, 32, 3, 4, 4, 256, 2, false>", "U", H, 17, 5, 7, 32, 2048),   # 9.3 MB
    ("conv_kernel<bf16_t, 32, 3, 4, 4, 64, 1, false>", "U", H, 1, 1, 1, 32, 16),   # 0.0 MB
    ("conv_kernel<bf16_t, 32, 3, 8, 16, 128, 1, false>", "U", H, 3, 17, 19, 32, 512),   # 3.8 MB
    ("conv_kernel<bf16_t, 32, 3, 8, 8, 128, 1, false>", "U", H, 3, 9, 13, 32, 1024),   # 2.8 MB
    ("conv_kernel<bf16_t, 32, 3, 8, 8, 256, 1, false>", "U", H, 1, 9, 13, 32, 2048),   # 1.8 MB
    ("conv_kernel<bf16_t, 32, 3, 8, 8, 256, 2, false>", "U", H, 1, 9, 32, 32, 2048),   # 4.5 MB
    ("conv_kernel<bf16_t, 32, 3, 8, 8, 64, 1, false>", "U", H, 1, 9, 13, 32, 16),   # 0.0 MB
    ("conv_kernel<float, 16, 0, 16, 16, 256, 1, false>", "S", F, 1, 17, 19, 32, 2048),   # 2.6 MB
    ("conv_kernel<float, 16, 0, 16, 16, 256, 2, false>", "S", F, 2, 17, 19, 32, 2048),   # 5.1 MB
    ("conv_kernel<float, 16, 0, 16, 16, 256, 4, false>", "S", F, 17, 17, 19, 32, 512),   # 11.4 MB
    ("conv_kernel<float, 16, 0, 4, 16, 64, 1, false>", "S", F, 1, 17, 19, 16, 16),   # 0.0 MB
    ("conv_kernel<float, 16, 0, 4, 4, 128, 1, false>", "S", F, 33, 1, 1, 32, 2048),   # 0.3 MB
    ("conv_kernel<float, 16, 0, 4, 4, 256, 1, false>", "S", F, 1, 5, 7, 32, 2048),   # 0.3 MB
    ("conv_kernel<float, 16, 0, 4, 4, 256, 2, false>", "S", F, 17, 5, 7, 32, 2048),   # 4.7 MB
    ("conv_kernel<float, 16, 0, 4, 4, 256, 4, false>", "S", F, 33, 6, 10, 32, 2048),   # 15.7 MB
    ("conv_kernel<float, 16, 0, 4, 4, 64, 1, false>", "S", F, 1, 1, 1, 16, 16),   # 0.0 MB
    ("conv_kernel<float, 16, 0, 8, 16, 128, 1, false>", "S", F, 3, 17, 19, 32, 512),   # 2.0 MB
    ("conv_kernel<float, 16, 0, 8, 8, 128, 1, false>", "S", F, 3, 9, 13, 32, 1024),   # 1.4 MB
    ("conv_kernel<float, 16, 0, 8, 8, 256, 1, false>", "S", F, 1, 9, 13, 32, 2048),   # 0.9 MB
    ("conv_kernel<float, 16, 0, 8, 8, 256, 2, false>", "S", F, 1, 9, 32, 32, 2048),   # 2.3 MB
    ("conv_kernel<float, 16, 0, 8, 8, 256, 4, false>", "S", F, 5, 9, 32, 32, 2048),   # 11.4 MB
    ("conv_kernel<float, 16, 0, 8, 8, 64, 1, false>", "S", F, 1, 9, 13, 16, 16),   # 0.0 MB
    ("conv_kernel<float, 16, 1, 4, 16, 64, 1, false>", "D", F, 1, 34, 38, 16, 16),   # 0.1 MB
    ("conv_kernel<float, 16, 1, 4, 4, 128, 1, false>", "D", F, 33, 2, 2, 32, 2048),   # 0.3 MB
    ("conv_kernel<float, 16, 1, 4, 4, 128, 2, false>", "D", F, 9, 10, 14, 32, 2048),   # 2.6 MB
    ("conv_kernel<float, 16, 1, 4, 4, 64, 1, false>", "D", F, 1, 2, 2, 16, 16),   # 0.0 MB
    ("conv_kernel<float, 16, 1, 8, 16, 128, 1, false>", "D", F, 3, 34, 38, 32, 512),   # 2.4 MB
    ("conv_kernel<float, 16, 1, 8, 16, 128, 2, false>", "D", F, 3, 34, 38, 32, 1024),   # 4.3 MB
    ("conv_kernel<float, 16, 1, 8, 8, 128, 1, false>", "D", F, 1, 18, 26, 32, 2048),   # 1.0 MB
    ("conv_kernel<float, 16, 1, 8, 8, 128, 2, false>", "D", F, 3, 18, 26, 32, 2048),   # 2.9 MB
    ("conv_kernel<float, 16, 1, 8, 8, 64, 1, false>", "D", F, 1, 18, 26, 16, 16),   # 0.0 MB
    ("conv_kernel<float, 16, 2, 16, 16, 256, 1, false>", "U", F, 1, 17, 19, 32, 512),   # 2.6 MB
    ("conv_kernel<float, 16, 2, 16, 16, 256, 2, false>", "U", F, 1, 17, 19, 32, 1024),   # 5.1 MB
    ("conv_kernel<float, 16, 2, 16, 16, 256, 4, false>", "U", F, 1, 17, 19, 32, 2048),   # 10.1 MB
    ("conv_kernel<float, 16, 2, 4, 16, 64, 1, false>", "U", F, 1, 17, 19, 16, 16),   # 0.1 MB
    ("conv_kernel<float, 16, 2, 4, 4, 128, 1, false>", "U", F, 9, 1, 1, 32, 1024),   # 0.1 MB
    ("conv_kernel<float, 16, 2, 4, 4, 256, 1, false>", "U", F, 1, 1, 1, 32, 2048),   # 0.0 MB
    ("conv_kernel<float, 16, 2, 4, 4, 256, 2, false>", "U", F, 17, 1, 1, 32, 2048),   # 0.5 MB
    ("conv_kernel<float, 16, 2, 4, 4, 256, 4, false>", "U", F, 1, 5, 7, 32, 2048),   # 1.1 MB
    ("conv_kernel<float, 16, 2, 4, 4, 64, 1, false>", "U", F, 1, 1, 1, 16, 16),   # 0.0 MB
    ("conv_kernel<float, 16, 2, 8, 16, 128, 1, false>", "U", F, 3, 17, 19, 16, 128),   # 2.0 MB
    ("conv_kernel<float, 16, 2, 8, 8, 128, 1, false>", "U", F, 3, 9, 13, 32, 256),   # 1.4 MB
    ("conv_kernel<float, 16, 2, 8, 8, 256, 1, false>", "U", F, 1, 9, 13, 32, 512),   # 0.9 MB
    ("conv_kernel<float, 16, 2, 8, 8, 256, 2, false>", "U", F, 1, 9, 13, 32, 1024),   # 1.8 MB
    ("conv_kernel<float, 16, 2, 8, 8, 256, 4, false>", "U", F, 1, 9, 13, 32, 2048),   # 3.7 MB
    ("conv_kernel<float, 16, 2, 8, 8, 64, 1, false>", "U", F, 1, 9, 13, 16, 16),   # 0.0 MB
)
AUTO_RANDN_BYTES = 12 << 20


def operand_bytes(geo, dt, B, Hh, W, Cin, Cout):
    OH, OW = out_hw(geo, Hh, W)
    return B * (Hh * W * Cin + OH * OW * Cout) * (2 if dt == H else 4)


for _k, _g, _dt, _B, _H, _W, _ci, _co in AUTO:
    _id = "auto-" + _k.replace("conv_kernel<", "g1<").replace("conv2_kernel<", "c2<").replace(", false>", ">").replace("bf16_t", "bf16").replace("float", "f32").replace(" ", "")
    _why = f"the smallest ragged shape of the grid that selects this instantiation: {_g} B{_B} {_H}x{_W} {_ci}->{_co}"
    _case(_id + "-int", ENTRY[_g], _dt, [_k], _why, _B, _H, _W, _ci, _co, mask=_g == "S")
    if operand_bytes(GEO_OF[_g], _dt, _B, _H, _W, _ci, _co) <= AUTO_RANDN_BYTES:
        _case(_id + "-randn", ENTRY[_g], _dt, [_k], _why, _B, _H, _W, _ci, _co, data="randn")

# ---- fp32: every geometry at Cin = 16 with odd sizes; the store epilogue's variants
_case("f32-S-17x19-int", "sgx_conv3x3", F, ['conv_kernel<float, 16, 0, 4, 16, 64, 1, false>'], "fp32 3x3, 17x19: 4x16 tiles ragged in both directions, B 3", 3, 17, 19, 16, 16, mask=True)
_case("f32-S-17x19-randn", "sgx_conv3x3", F, ['conv_kernel<float, 16, 0, 4, 16, 64, 1, false>'], "fp32 3x3, 17x19: 4x16 tiles ragged in both directions, B 3", 3, 17, 19, 16, 16, data='randn')
_case("f32-S-17x19-abs", "sgx_conv3x3", F, ['conv_kernel<float, 16, 0, 4, 16, 64, 1, false>'], "fp32 3x3, 17x19: 4x16 tiles ragged in both directions, B 3", 3, 17, 19, 16, 16, data='abs')
_case("f32-D-18x26-int", "sgx_conv4x4s2_down", F, ['conv_kernel<float, 16, 1, 8, 8, 64, 1, false>'], "fp32 stride 2, 18x26 -> 9x13: 8x8 tiles ragged", 3, 18, 26, 16, 32)
_case("f32-D-18x26-randn", "sgx_conv4x4s2_down", F, ['conv_kernel<float, 16, 1, 8, 8, 64, 1, false>'], "fp32 stride 2, 18x26 -> 9x13: 8x8 tiles ragged", 3, 18, 26, 16, 32, data='randn')
_case("f32-D-18x26-abs", "sgx_conv4x4s2_down", F, ['conv_kernel<float, 16, 1, 8, 8, 64, 1, false>'], "fp32 stride 2, 18x26 -> 9x13: 8x8 tiles ragged", 3, 18, 26, 16, 32, data='abs')
_case("f32-U-9x13-int", "sgx_conv4x4s2_up", F, ['conv_kernel<float, 16, 2, 8, 8, 64, 1, false>'], "fp32 transposed, odd coarse size 9x13: per-class GUP blocks", 3, 9, 13, 16, 16)
_case("f32-U-9x13-randn", "sgx_conv4x4s2_up", F, ['conv_kernel<float, 16, 2, 8, 8, 64, 1, false>'], "fp32 transposed, odd coarse size 9x13: per-class GUP blocks", 3, 9, 13, 16, 16, data='randn')
_case("f32-U-9x13-abs", "sgx_conv4x4s2_up", F, ['conv_kernel<float, 16, 2, 8, 8, 64, 1, false>'], "fp32 transposed, odd coarse size 9x13: per-class GUP blocks", 3, 9, 13, 16, 16, data='abs')
_case("f32-S-1x1", "sgx_conv3x3", F, ['conv_kernel<float, 16, 0, 4, 4, 64, 1, false>'], "a 1x1 image: every tap but the centre is halo", 1, 1, 1, 16, 16)
_case("f32-S-plain-int", "sgx_conv3x3", F, ['conv_kernel<float, 16, 0, 4, 4, 64, 1, false>'], "bias NULL, no activation, no mask", 3, 5, 7, 16, 16, bias=False, act=0)
_case("f32-S-plain-randn", "sgx_conv3x3", F, ['conv_kernel<float, 16, 0, 4, 4, 64, 1, false>'], "bias NULL, no activation, no mask", 3, 5, 7, 16, 16, bias=False, act=0, data='randn')
_case("f32-D-plain-int", "sgx_conv4x4s2_down", F, ['conv_kernel<float, 16, 1, 4, 4, 64, 1, false>'], "bias NULL, no activation", 3, 6, 10, 16, 16, bias=False, act=0)
_case("f32-D-plain-randn", "sgx_conv4x4s2_down", F, ['conv_kernel<float, 16, 1, 4, 4, 64, 1, false>'], "bias NULL, no activation", 3, 6, 10, 16, 16, bias=False, act=0, data='randn')

# ---- first generation, bf16: K-chunk forms, deep-K, the all-class transposed kernel
_case("g1-S-48-96-int", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 16, 64, 1, false>'], "Cin 48 is no multiple of 32: three 16-channel chunks; Cout 96", 3, 17, 19, 48, 96, mask=True)
_case("g1-S-48-96-randn", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 16, 64, 1, false>'], "Cin 48 is no multiple of 32: three 16-channel chunks; Cout 96", 3, 17, 19, 48, 96, data='randn')
_case("g1-S-48-96-abs", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 16, 64, 1, false>'], "Cin 48 is no multiple of 32: three 16-channel chunks; Cout 96", 3, 17, 19, 48, 96, data='abs')
_case("g1-D-96-48-int", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, false>'], "three 32-channel chunks; Cout 48", 3, 18, 26, 96, 48)
_case("g1-D-96-48-randn", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, false>'], "three 32-channel chunks; Cout 48", 3, 18, 26, 96, 48, data='randn')
_case("g1-D-96-48-abs", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, false>'], "three 32-channel chunks; Cout 48", 3, 18, 26, 96, 48, data='abs')
_case("g1-UPA-48-32-int", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 64, 1, false>'], "transposed, all four classes in one block (GUPA), 16-channel chunks, odd coarse size", 3, 9, 13, 48, 32)
_case("g1-UPA-48-32-randn", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 64, 1, false>'], "transposed, all four classes in one block (GUPA), 16-channel chunks, odd coarse size", 3, 9, 13, 48, 32, data='randn')
_case("g1-UPA-48-32-abs", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 64, 1, false>'], "transposed, all four classes in one block (GUPA), 16-channel chunks, odd coarse size", 3, 9, 13, 48, 32, data='abs')
_case("g1-S-1x1", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 4, 4, 64, 1, false>'], "a 1x1 image", 1, 1, 1, 32, 16)
_case("g1-S-plain-int", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 8, 8, 64, 1, false>'], "bias NULL, no activation, no mask", 3, 9, 13, 32, 16, bias=False, act=0)
_case("g1-S-plain-randn", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 8, 8, 64, 1, false>'], "bias NULL, no activation, no mask", 3, 9, 13, 32, 16, bias=False, act=0, data='randn')
_case("g1-deepk-S-256-int", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 128, 0, 4, 4, 64, 1, false>'], "Cin % 128 == 0 and a 64-pixel tile: deep K-chunks, two of them", 1, 5, 7, 256, 32)
_case("g1-deepk-S-256-randn", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 128, 0, 4, 4, 64, 1, false>'], "Cin % 128 == 0 and a 64-pixel tile: deep K-chunks, two of them", 1, 5, 7, 256, 32, data='randn')
_case("g1-deepk-U-128-int", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 128, 2, 4, 4, 64, 1, false>'], "deep K-chunks on the transposed geometry: per-class GUP blocks, one chunk", 1, 5, 7, 128, 32)
_case("g1-deepk-U-128-randn", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 128, 2, 4, 4, 64, 1, false>'], "deep K-chunks on the transposed geometry: per-class GUP blocks, one chunk", 1, 5, 7, 128, 32, data='randn')
_case("g1-S-544-int", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 4, 4, 64, 1, false>'], "Cin 544 is no multiple of 128: 17 chunks of 32", 1, 5, 7, 544, 32)
_case("g1-S-544-abs", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 4, 4, 64, 1, false>'], "Cin 544 is no multiple of 128: 17 chunks of 32", 1, 5, 7, 544, 32, data='abs')
_case("g1-S-co33", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 16, 16, 256, 2, false>'], "Cout / 64 = 33 > 32 channel blocks: the second generation declines a shape it would otherwise take", 3, 17, 32, 32, 2112)

# ---- second generation: K-chunks 1, 2, 3, 4 (static / re-staged weights), the persistent grid, channel blocks
_case("c2-S-k1", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "small grid: 8 waves x 32 channels, 64 channel blocks; 1 K-chunk(s); 6 tiles in 8 slots; 17 rows: a ragged second tile row", 3, 17, 32, 32, 2048, mask=False)
_case("c2-S-k2", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "small grid: 8 waves x 32 channels, 64 channel blocks; 2 K-chunk(s); 6 tiles in 8 slots; 17 rows: a ragged second tile row", 3, 17, 32, 64, 2048, mask=True)
_case("c2-S-k3-int", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "small grid: 8 waves x 32 channels, 64 channel blocks; 3 K-chunk(s); 6 tiles in 8 slots; 17 rows: a ragged second tile row", 3, 17, 32, 96, 2048, mask=False)
_case("c2-S-k3-randn", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "small grid: 8 waves x 32 channels, 64 channel blocks; 3 K-chunk(s); 6 tiles in 8 slots; 17 rows: a ragged second tile row", 3, 17, 32, 96, 2048, data='randn')
_case("c2-S-k3-abs", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "small grid: 8 waves x 32 channels, 64 channel blocks; 3 K-chunk(s); 6 tiles in 8 slots; 17 rows: a ragged second tile row", 3, 17, 32, 96, 2048, data='abs')
_case("c2-S-k4", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "small grid: 8 waves x 32 channels, 64 channel blocks; 4 K-chunk(s); 6 tiles in 8 slots; 17 rows: a ragged second tile row", 3, 17, 32, 128, 2048, mask=False)
_case("c2-S-40x64-int", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "tile-grid width 64, 40 rows: ragged last tile row; 6 tiles in 8 slots", 1, 40, 64, 32, 2048)
_case("c2-S-40x64-randn", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "tile-grid width 64, 40 rows: ragged last tile row; 6 tiles in 8 slots", 1, 40, 64, 32, 2048, data='randn')
_case("c2-S-slot-each", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "16 tiles in 16 slots at 256 CUs: exactly one tile per slot (304 CUs: the small-grid rule takes 32-channel blocks, 16 tiles in 8 slots)", 1, 64, 128, 32, 1024, k304=['conv2_kernel<0, 8, 1, 32, false, 0>'])
_case("c2-S-k16-int", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "16 -> 16: two 4-wave blocks per CU; 264 rows = 33 tile rows", 2, 264, 256, 16, 16, mask=True)
_case("c2-S-k16-randn", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "16 -> 16: two 4-wave blocks per CU; 264 rows = 33 tile rows", 2, 264, 256, 16, 16, data='randn')
_case("c2-S-k16-abs", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "16 -> 16: two 4-wave blocks per CU; 264 rows = 33 tile rows", 2, 264, 256, 16, 16, data='abs')
_case("c2-S-k16-bands", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 16, true, 0>'], "5120 tiles of 16x32 >= 8 x 512 slots (256 CUs) and >= 8 x 608 (304 CUs): the smallest batch of 512^2 images whose grid takes the XCD-band order", 10, 512, 512, 16, 16)
_case("c2-D-mf2-randn", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "stride 2, 8 waves x 64 channels; coarse 68x64: ragged last tile row", 2, 136, 128, 32, 1024, data='randn')
_case("c2-D-mf2-abs", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "stride 2, 8 waves x 64 channels; coarse 68x64: ragged last tile row", 2, 136, 128, 32, 1024, data='abs')
_case("c2-D-mf1", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "stride 2, small grid: 8 waves x 32 channels; coarse 17x32", 5, 34, 64, 32, 1024, data='randn')
_case("c2-D-k3", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "stride 2, three K-chunks", 5, 34, 64, 96, 1024)
_case("c2-U-randn", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "transposed, 4-wave blocks, coarse 9x32: ragged", 5, 9, 32, 32, 1024, data='randn')
_case("c2-U-abs", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "transposed, 4-wave blocks, coarse 9x32: ragged", 5, 9, 32, 32, 1024, data='abs')
_case("c2-U-k2", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "transposed, two K-chunks", 5, 9, 32, 64, 1024)

# ---- split-K: 2 ways (want > nk / 2), 4 ways, the 8-way cap over 17 chunks (uneven ranges), one step outside the plan
_case("sk-2-int", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "4 chunks: the block target asks for 8 ways, nk / 2 caps it at 2", 1, 6, 10, 128, 32, twin='sk-2-unsplit')
_case("sk-2-randn", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "4 chunks: the block target asks for 8 ways, nk / 2 caps it at 2", 1, 6, 10, 128, 32, data='randn')
_case("sk-2-abs", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "4 chunks: the block target asks for 8 ways, nk / 2 caps it at 2", 1, 6, 10, 128, 32, data='abs')
_case("sk-4-int", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, true>', 'conv_splitk_finish'], "8 chunks: 4 ways", 3, 18, 26, 256, 128, twin='sk-4-unsplit')
_case("sk-4-randn", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, true>', 'conv_splitk_finish'], "8 chunks: 4 ways", 3, 18, 26, 256, 128, data='randn')
_case("sk-8-of-17-int", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "17 chunks over the 8-way cap: ranges of 2 and 3 chunks", 1, 6, 10, 544, 32, twin='sk-8-of-17-unsplit')
_case("sk-8-of-17-randn", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "17 chunks over the 8-way cap: ranges of 2 and 3 chunks", 1, 6, 10, 544, 32, data='randn')
_case("sk-8-of-17-abs", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "17 chunks over the 8-way cap: ranges of 2 and 3 chunks", 1, 6, 10, 544, 32, data='abs')
_case("sk-nobias", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "bias NULL, no activation in the finishing launch", 1, 6, 10, 128, 32, bias=False, act=0, twin='sk-nobias-unsplit')
_case("sk-outside", "sgx_conv_splitk", H, [], "3 chunks < 4: the shape does not split: SGX_EUNSUPPORTED, nothing written", 1, 6, 10, 96, 32, rc=-2)
_case("sk-outside-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, false>'], "... and runs unsplit through sgx_conv4x4s2_down", 1, 6, 10, 96, 32)
_case("sk-2-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, false>'], "the unsplit twin of sk-2", 1, 6, 10, 128, 32)
_case("sk-4-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, false>'], "the unsplit twin of sk-4", 3, 18, 26, 256, 128)
_case("sk-8-of-17-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, false>'], "the unsplit twin of sk-8-of-17", 1, 6, 10, 544, 32)
_case("sk-nobias-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, false>'], "the unsplit twin of sk-nobias", 1, 6, 10, 128, 32, bias=False, act=0)
_case("sk-short", "sgx_conv_splitk", H, [], "a workspace one byte short: SGX_EWORKSPACE", 1, 6, 10, 128, 32, ws='short', rc=-3)
_case("sk-geo0", "sgx_conv_splitk", H, [], "geometry 0 has no split form", 1, 6, 10, 128, 32, geo=0, rc=-2)
_case("sk-geo2", "sgx_conv_splitk", H, [], "geometry 2 has no split form", 1, 6, 10, 128, 32, geo=2, rc=-2)

# ---- sgx_conv_variant: first generation = second generation (4 = 8 waves) = each conv3_kernel configuration
_case("v0-S-int", "sgx_conv_variant", H, ['conv_kernel<bf16_t, 32, 0, 4, 16, 64, 1, false>'], "variant 0: the first generation", 1, 17, 32, 64, 64, geo=0, variant=0)
_case("v0-S-randn", "sgx_conv_variant", H, ['conv_kernel<bf16_t, 32, 0, 4, 16, 64, 1, false>'], "variant 0: the first generation", 1, 17, 32, 64, 64, geo=0, variant=0, data='randn')
_case("v4-S-int", "sgx_conv_variant", H, ['conv2_kernel<0, 4, 2, 32, false, 0>'], "variant 4: conv2_kernel with 4 waves whatever the grid", 1, 17, 32, 64, 64, geo=0, variant=4, twin='v0-S-int')
_case("v4-S-randn", "sgx_conv_variant", H, ['conv2_kernel<0, 4, 2, 32, false, 0>'], "variant 4: conv2_kernel with 4 waves whatever the grid", 1, 17, 32, 64, 64, geo=0, variant=4, data='randn')
_case("v8-S-int", "sgx_conv_variant", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "variant 8: conv2_kernel with 8 waves whatever the grid", 1, 17, 32, 64, 64, geo=0, variant=8, twin='v0-S-int')
_case("v8-S-randn", "sgx_conv_variant", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "variant 8: conv2_kernel with 8 waves whatever the grid", 1, 17, 32, 64, 64, geo=0, variant=8, data='randn')
_case("v30-S-int", "sgx_conv_variant", H, ['conv3_kernel<0, 8, 2, 2, 1, 0, 0>'], "variant 30: conv3_kernel configuration 0", 1, 17, 32, 64, 64, geo=0, variant=30, twin='v0-S-int')
_case("v30-S-randn", "sgx_conv_variant", H, ['conv3_kernel<0, 8, 2, 2, 1, 0, 0>'], "variant 30: conv3_kernel configuration 0", 1, 17, 32, 64, 64, geo=0, variant=30, data='randn')
_case("v31-S", "sgx_conv_variant", H, ['conv3_kernel<0, 8, 2, 2, 2, 0, 0>'], "variant 31: conv3_kernel configuration 1", 1, 17, 32, 64, 64, geo=0, variant=31, twin='v0-S-int')
_case("v32-S", "sgx_conv_variant", H, ['conv3_kernel<0, 8, 2, 2, 2, 1, 0>'], "variant 32: conv3_kernel configuration 2", 1, 17, 32, 64, 64, geo=0, variant=32, twin='v0-S-int')
_case("v33-S-int", "sgx_conv_variant", H, ['conv3_kernel<0, 4, 2, 4, 1, 0, 0>'], "variant 33: conv3_kernel configuration 3", 1, 17, 32, 64, 64, geo=0, variant=33, twin='v0-S-int')
_case("v33-S-randn", "sgx_conv_variant", H, ['conv3_kernel<0, 4, 2, 4, 1, 0, 0>'], "variant 33: conv3_kernel configuration 3", 1, 17, 32, 64, 64, geo=0, variant=33, data='randn')
_case("v34-S", "sgx_conv_variant", H, ['conv3_kernel<0, 4, 2, 4, 2, 0, 0>'], "variant 34: conv3_kernel configuration 4", 1, 17, 32, 64, 64, geo=0, variant=34, twin='v0-S-int')
_case("v35-S", "sgx_conv_variant", H, ['conv3_kernel<0, 4, 2, 4, 1, 1, 0>'], "variant 35: conv3_kernel configuration 5", 1, 17, 32, 64, 64, geo=0, variant=35, twin='v0-S-int')
_case("v36-S-int", "sgx_conv_variant", H, ['conv3_kernel<0, 4, 2, 2, 2, 0, 0>'], "variant 36: conv3_kernel configuration 6", 1, 17, 32, 64, 64, geo=0, variant=36, twin='v0-S-int')
_case("v36-S-randn", "sgx_conv_variant", H, ['conv3_kernel<0, 4, 2, 2, 2, 0, 0>'], "variant 36: conv3_kernel configuration 6", 1, 17, 32, 64, 64, geo=0, variant=36, data='randn')
_case("v0-D-int", "sgx_conv_variant", H, ['conv_kernel<bf16_t, 32, 1, 4, 16, 64, 1, false>'], "variant 0: the first generation", 1, 34, 64, 64, 64, geo=1, variant=0)
_case("v0-D-randn", "sgx_conv_variant", H, ['conv_kernel<bf16_t, 32, 1, 4, 16, 64, 1, false>'], "variant 0: the first generation", 1, 34, 64, 64, 64, geo=1, variant=0, data='randn')
_case("v4-D-int", "sgx_conv_variant", H, ['conv2_kernel<1, 4, 2, 32, false, 0>'], "variant 4: conv2_kernel with 4 waves whatever the grid", 1, 34, 64, 64, 64, geo=1, variant=4, twin='v0-D-int')
_case("v4-D-randn", "sgx_conv_variant", H, ['conv2_kernel<1, 4, 2, 32, false, 0>'], "variant 4: conv2_kernel with 4 waves whatever the grid", 1, 34, 64, 64, 64, geo=1, variant=4, data='randn')
_case("v8-D-int", "sgx_conv_variant", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "variant 8: conv2_kernel with 8 waves whatever the grid", 1, 34, 64, 64, 64, geo=1, variant=8, twin='v0-D-int')
_case("v8-D-randn", "sgx_conv_variant", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "variant 8: conv2_kernel with 8 waves whatever the grid", 1, 34, 64, 64, 64, geo=1, variant=8, data='randn')
_case("v30-D-int", "sgx_conv_variant", H, ['conv3_kernel<1, 8, 2, 2, 1, 0, 0>'], "variant 30: conv3_kernel configuration 0", 1, 34, 64, 64, 64, geo=1, variant=30, twin='v0-D-int')
_case("v30-D-randn", "sgx_conv_variant", H, ['conv3_kernel<1, 8, 2, 2, 1, 0, 0>'], "variant 30: conv3_kernel configuration 0", 1, 34, 64, 64, 64, geo=1, variant=30, data='randn')
_case("v31-D", "sgx_conv_variant", H, ['conv3_kernel<1, 8, 2, 2, 2, 0, 0>'], "variant 31: conv3_kernel configuration 1", 1, 34, 64, 64, 64, geo=1, variant=31, twin='v0-D-int')
_case("v32-D", "sgx_conv_variant", H, ['conv3_kernel<1, 8, 2, 2, 2, 1, 0>'], "variant 32: conv3_kernel configuration 2", 1, 34, 64, 64, 64, geo=1, variant=32, twin='v0-D-int')
_case("v33-D-int", "sgx_conv_variant", H, ['conv3_kernel<1, 4, 2, 4, 1, 0, 0>'], "variant 33: conv3_kernel configuration 3", 1, 34, 64, 64, 64, geo=1, variant=33, twin='v0-D-int')
_case("v33-D-randn", "sgx_conv_variant", H, ['conv3_kernel<1, 4, 2, 4, 1, 0, 0>'], "variant 33: conv3_kernel configuration 3", 1, 34, 64, 64, 64, geo=1, variant=33, data='randn')
_case("v34-D", "sgx_conv_variant", H, ['conv3_kernel<1, 4, 2, 4, 2, 0, 0>'], "variant 34: conv3_kernel configuration 4", 1, 34, 64, 64, 64, geo=1, variant=34, twin='v0-D-int')
_case("v35-D", "sgx_conv_variant", H, ['conv3_kernel<1, 4, 2, 4, 1, 1, 0>'], "variant 35: conv3_kernel configuration 5", 1, 34, 64, 64, 64, geo=1, variant=35, twin='v0-D-int')
_case("v36-D-int", "sgx_conv_variant", H, ['conv3_kernel<1, 4, 2, 2, 2, 0, 0>'], "variant 36: conv3_kernel configuration 6", 1, 34, 64, 64, 64, geo=1, variant=36, twin='v0-D-int')
_case("v36-D-randn", "sgx_conv_variant", H, ['conv3_kernel<1, 4, 2, 2, 2, 0, 0>'], "variant 36: conv3_kernel configuration 6", 1, 34, 64, 64, 64, geo=1, variant=36, data='randn')
_case("v0-U", "sgx_conv_variant", H, ['conv_kernel<bf16_t, 32, 3, 4, 16, 64, 1, false>'], "variant 0, transposed", 1, 17, 32, 64, 64, geo=2, variant=0, bias=False, act=0)
_case("v4-U-int", "sgx_conv_variant", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "variant 4, transposed", 1, 17, 32, 64, 64, geo=2, variant=4, bias=False, act=0, twin='v0-U')
_case("v4-U-randn", "sgx_conv_variant", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "variant 4, transposed", 1, 17, 32, 64, 64, geo=2, variant=4, bias=False, act=0, data='randn')
_case("v8-U", "sgx_conv_variant", H, ['conv2_kernel<2, 8, 1, 32, false, 0>'], "variant 8, transposed", 1, 17, 32, 64, 64, geo=2, variant=8, bias=False, act=0, twin='v0-U')
_case("v0-f32", "sgx_conv_variant", F, ['conv_kernel<float, 16, 0, 4, 4, 64, 1, false>'], "variant 0 in fp32", 3, 5, 7, 16, 16, geo=0, variant=0)

# ---- fused epilogues as the entry points pick them
_case("bits-c2-S-int", "sgx_conv3x3_signbits", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "sign bits from the register epilogue, 32-channel blocks, with the output mask", 3, 17, 32, 64, 2048, mask=True, twin='c2-S-k2')
_case("bits-c2-S-randn", "sgx_conv3x3_signbits", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "sign bits from the register epilogue, 32-channel blocks, with the output mask", 3, 17, 32, 64, 2048, data='randn')
_case("bits-c2-S-k16-int", "sgx_conv3x3_signbits", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "sign bits of the 16-channel form: one 16-bit store per pixel", 2, 264, 256, 16, 16, mask=True, twin='c2-S-k16-int')
_case("bits-c2-S-k16-randn", "sgx_conv3x3_signbits", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "sign bits of the 16-channel form: one 16-bit store per pixel", 2, 264, 256, 16, 16, data='randn')
_case("bits-c2-S-mf2-int", "sgx_conv3x3_signbits", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "sign bits, 64-channel blocks", 5, 17, 32, 32, 2048, twin='plain-c2-S-mf2')
_case("bits-c2-S-mf2-abs", "sgx_conv3x3_signbits", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "sign bits, 64-channel blocks", 5, 17, 32, 32, 2048, data='abs')
_case("plain-c2-S-mf2", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "the plain twin of bits-c2-S-mf2 and stats-c2-S-mf2", 5, 17, 32, 32, 2048)
_case("stats-c2-S-mf2-int", "sgx_conv3x3_stats", H, ['conv2_kernel<0, 8, 2, 32, false, 1>'], "statistics epilogue, 64-channel blocks", 5, 17, 32, 32, 2048, twin='plain-noact-c2-S-mf2')
_case("stats-c2-S-mf2-randn", "sgx_conv3x3_stats", H, ['conv2_kernel<0, 8, 2, 32, false, 1>'], "statistics epilogue, 64-channel blocks", 5, 17, 32, 32, 2048, data='randn')
_case("plain-noact-c2-S-mf2", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "no bias, no activation: the y of sgx_conv3x3_stats", 5, 17, 32, 32, 2048, bias=False, act=0)
_case("stats-c2-S-k16-int", "sgx_conv3x3_stats", H, ['conv2_kernel<0, 4, 1, 16, true, 1>'], "statistics epilogue of the 16-channel form", 2, 264, 256, 16, 16, twin='plain-noact-c2-S-k16')
_case("stats-c2-S-k16-randn", "sgx_conv3x3_stats", H, ['conv2_kernel<0, 4, 1, 16, true, 1>'], "statistics epilogue of the 16-channel form", 2, 264, 256, 16, 16, data='randn')
_case("plain-noact-c2-S-k16", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "no bias, no activation: the y of sgx_conv3x3_stats", 2, 264, 256, 16, 16, bias=False, act=0)
_case("stats-short", "sgx_conv3x3_stats", H, [], "partials one byte short: SGX_EWORKSPACE", 2, 264, 256, 16, 16, part='short', rc=-3)
_case("fade-c2-D-mf2-int", "sgx_conv4x4s2_down_fade", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "the fade-in lerp and the sign bits in the store, host coefficients", 2, 136, 128, 32, 1024)
_case("fade-c2-D-mf2-randn", "sgx_conv4x4s2_down_fade", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "the fade-in lerp and the sign bits in the store, host coefficients", 2, 136, 128, 32, 1024, data='randn')
_case("fade-dev-c2-D-mf2", "sgx_conv4x4s2_down_fade", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "coefficients from device memory: the host call's bits", 2, 136, 128, 32, 1024, ab_dev=True, twin='fade-c2-D-mf2-int')
_case("plain-c2-D-mf2", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "the stored activation the fade twins start from", 2, 136, 128, 32, 1024)
_case("fade-c2-D-mf1-int", "sgx_conv4x4s2_down_fade", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "32-channel blocks", 5, 34, 64, 32, 1024)
_case("fade-c2-D-mf1-randn", "sgx_conv4x4s2_down_fade", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "32-channel blocks", 5, 34, 64, 32, 1024, data='randn')
_case("plain-c2-D-mf1", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "the stored activation the fade twins start from", 5, 34, 64, 32, 1024)
_case("fade-rgb-c2-D-mf1-int", "sgx_conv4x4s2_down_fade_rgb", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "the residual from_rgb(pimg) computed in the store, with from_rgb's bias", 5, 34, 64, 32, 1024, rb=True)
_case("fade-rgb-c2-D-mf1-randn", "sgx_conv4x4s2_down_fade_rgb", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "the residual from_rgb(pimg) computed in the store, with from_rgb's bias", 5, 34, 64, 32, 1024, rb=True, data='randn')
_case("fade-rgb-norb-c2-D-mf1-int", "sgx_conv4x4s2_down_fade_rgb", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "... rb NULL", 5, 34, 64, 32, 1024, rb=False)
_case("fade-rgb-norb-c2-D-mf1-randn", "sgx_conv4x4s2_down_fade_rgb", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "... rb NULL", 5, 34, 64, 32, 1024, rb=False, data='randn')
_case("upblur-c2-U", "sgx_conv4x4s2_up_blur", H, ['conv2_kernel<2, 4, 1, 32, false, 2>'], "blur epilogue, overlapping tiles (steps 7 rows x 31 columns), no mask", 5, 9, 32, 32, 1024, data='sparse')
_case("upblur-mask-c2-U", "sgx_conv4x4s2_up_blur", H, ['conv2_kernel<2, 4, 1, 32, false, 2>'], "blur epilogue with a mask tensor", 5, 9, 32, 32, 1024, mask=True, data='sparse')
_case("upblur-bits-c2-U", "sgx_conv4x4s2_up_blur_bits", H, ['conv2_kernel<2, 4, 1, 32, false, 2>'], "blur epilogue with the mask as sign bits: the bits of upblur-mask-c2-U", 5, 9, 32, 32, 1024, twin='upblur-mask-c2-U', data='sparse')
_case("upblur-c2-U16", "sgx_conv4x4s2_up_blur", H, ['conv2_kernel<2, 4, 1, 32, true, 2>'], "32 -> 16: only the blur entry takes the 16-channel transposed form (allow_u16)", 1, 136, 576, 32, 16, mask=True, data='sparse')
_case("upblur-bits-c2-U16", "sgx_conv4x4s2_up_blur_bits", H, ['conv2_kernel<2, 4, 1, 32, true, 2>'], "... with sign bits", 1, 136, 576, 32, 16, twin='upblur-c2-U16', data='sparse')
_case("up-g1-32-16", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 32, 3, 8, 16, 128, 1, false>'], "32 -> 16 without the blur entry: the first generation's all-class kernel", 1, 136, 576, 32, 16)

# ---- contract rejections: the documented code, nothing written
_case("rej-D-odd-H", "sgx_conv4x4s2_down", H, [], "odd H for stride 2", 1, 7, 10, 32, 32, rc=-1)
_case("rej-S-cin-24", "sgx_conv3x3", H, [], "Cin no multiple of 16", 1, 5, 7, 24, 32, rc=-2)
_case("rej-S-cout-24-f32", "sgx_conv3x3", F, [], "Cout no multiple of 16", 1, 5, 7, 16, 24, rc=-2)
_case("rej-bits-no-variant", "sgx_conv3x3_signbits", H, [], "sgx_conv3x3_signbits_ok == 0: the shape stays with the first generation", 1, 5, 7, 32, 32, rc=-2)
_case("rej-stats-no-variant", "sgx_conv3x3_stats", H, [], "sgx_conv3x3_stats_nparts == 0", 1, 5, 7, 32, 32, rc=-2)
_case("rej-fade-no-variant", "sgx_conv4x4s2_down_fade", H, [], "sgx_conv4x4s2_down_fade_ok == 0", 1, 6, 10, 32, 32, rc=-2)
_case("rej-fade-rgb-no-variant", "sgx_conv4x4s2_down_fade_rgb", H, [], "sgx_conv4x4s2_down_fade_ok == 0", 1, 6, 10, 32, 32, rb=True, rc=-2)
_case("rej-upblur-no-variant", "sgx_conv4x4s2_up_blur", H, [], "sgx_conv4x4s2_up_blur_ok == 0", 1, 5, 7, 32, 32, rc=-2)
_case("rej-upblur-bits-no-variant", "sgx_conv4x4s2_up_blur_bits", H, [], "sgx_conv4x4s2_up_blur_ok == 0", 1, 5, 7, 32, 32, rc=-2)
_case("rej-bits-f32", "sgx_conv3x3_signbits", F, [], "bf16 only", 3, 17, 32, 64, 2048, rc=-2)
_case("rej-v4-narrow", "sgx_conv_variant", H, [], "variant 4 on a tile-grid width that is no multiple of 32", 1, 5, 7, 32, 64, geo=0, variant=4, rc=-2)
_case("rej-v30-cout32", "sgx_conv_variant", H, [], "conv3_kernel wants Cout % 64 == 0", 1, 17, 32, 32, 32, geo=0, variant=30, rc=-2)

# ---- switch groups: one child process each; an integer row gives the bits of its default-environment twin
_case("conv2_0-c2-S-k2", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 16, 16, 256, 2, false>'], "SGX_CONV2=0: the first generation on a second-generation shape", 3, 17, 32, 64, 2048, twin='c2-S-k2', mask=True, group='conv2_0')
_case("conv2_0-c2-S-k16-int", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 16, 16, 256, 1, false>'], "SGX_CONV2=0: the first generation on a second-generation shape", 2, 264, 256, 16, 16, twin='c2-S-k16-int', mask=True, group='conv2_0')
_case("conv2_0-plain-c2-D-mf2", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 16, 128, 2, false>'], "SGX_CONV2=0: the first generation on a second-generation shape", 2, 136, 128, 32, 1024, twin='plain-c2-D-mf2', group='conv2_0')
_case("conv2_0-plain-c2-D-mf1", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 16, 128, 2, false>'], "SGX_CONV2=0: the first generation on a second-generation shape", 5, 34, 64, 32, 1024, twin='plain-c2-D-mf1', group='conv2_0')
_case("conv2_0-c2-U-k2", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 32, 3, 8, 8, 256, 2, false>'], "SGX_CONV2=0: the first generation on a second-generation shape", 5, 9, 32, 64, 1024, twin='c2-U-k2', group='conv2_0')
_case("conv2_0-plain-c2-S-mf2", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 16, 16, 256, 4, false>'], "SGX_CONV2=0: the first generation on a second-generation shape", 5, 17, 32, 32, 2048, twin='plain-c2-S-mf2', group='conv2_0')
_case("conv2_31-U16", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 4, 1, 32, true, 0>'], "SGX_CONV2=31: bit 4 lets sgx_conv4x4s2_up take the transposed 32 -> 16 form", 1, 136, 576, 32, 16, twin='up-g1-32-16', group='conv2_31')
_case("nw4-c2-S-k2", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 2, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 4: that block shape whatever the grid", 3, 17, 32, 64, 2048, twin='c2-S-k2', mask=True, group='nw4')
_case("nw4-c2-S-k16-int", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 4: that block shape whatever the grid", 2, 264, 256, 16, 16, twin='c2-S-k16-int', mask=True, group='nw4')
_case("nw4-plain-c2-D-mf2", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 4, 2, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 4: that block shape whatever the grid", 2, 136, 128, 32, 1024, twin='plain-c2-D-mf2', group='nw4')
_case("nw4-c2-U-k2", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 4: that block shape whatever the grid", 5, 9, 32, 64, 1024, twin='c2-U-k2', group='nw4')
_case("nw4-plain-c2-S-mf2", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 2, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 4: that block shape whatever the grid", 5, 17, 32, 32, 2048, twin='plain-c2-S-mf2', group='nw4')
_case("nw8-c2-S-k2", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 8: that block shape whatever the grid", 3, 17, 32, 64, 2048, twin='c2-S-k2', mask=True, group='nw8')
_case("nw8-c2-S-k16-int", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 16, true, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 8: that block shape whatever the grid", 2, 264, 256, 16, 16, twin='c2-S-k16-int', mask=True, group='nw8')
_case("nw8-plain-c2-D-mf2", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 8: that block shape whatever the grid", 2, 136, 128, 32, 1024, twin='plain-c2-D-mf2', group='nw8')
_case("nw8-c2-U-k2", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 8, 1, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 8: that block shape whatever the grid", 5, 9, 32, 64, 1024, twin='c2-U-k2', group='nw8')
_case("nw8-plain-c2-S-mf2", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 2, 32, false, 0>'], "SGX_CONV2_NW = SGX_CONV2_NW16 = 8: that block shape whatever the grid", 5, 17, 32, 32, 2048, twin='plain-c2-S-mf2', group='nw8')
_case("small0-c2-S-k2", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 2, 32, false, 0>'], "SGX_CONV2_SMALL=0: the round-2 shape rule (64-channel blocks or the first generation)", 3, 17, 32, 64, 2048, twin='c2-S-k2', mask=True, group='small0', k304=['conv_kernel<bf16_t, 32, 0, 16, 16, 256, 2, false>'])
_case("small0-c2-D-mf1", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 16, 128, 2, false>'], "SGX_CONV2_SMALL=0 on the stride-2 small grid", 5, 34, 64, 32, 1024, twin='plain-c2-D-mf1', group='small0')
_case("bpc1-c2-S-k16", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "SGX_CONV2_BPC=1: one resident block per CU, half the slots", 2, 264, 256, 16, 16, twin='c2-S-k16-int', mask=True, group='bpc1')
_case("bpc1-stats-c2-S-k16", "sgx_conv3x3_stats", H, ['conv2_kernel<0, 4, 1, 16, true, 1>'], "... and half the statistics partials", 2, 264, 256, 16, 16, twin='plain-noact-c2-S-k16', group='bpc1')
_case("regstore-c2-U-k2", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "SGX_CONVU_REGSTORE=1: the register store of the transposed geometry", 5, 9, 32, 64, 1024, twin='c2-U-k2', group='regstore')
_case("nt3-c2-S-k2", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "SGX_CONV_NT=3 with SGX_NT_MIN_MB=0.001: nontemporal stores and patch DMA at a test-sized output", 3, 17, 32, 64, 2048, twin='c2-S-k2', mask=True, group='nt3')
_case("nt3-c2-S-k16-int", "sgx_conv3x3", H, ['conv2_kernel<0, 4, 1, 16, true, 0>'], "SGX_CONV_NT=3 with SGX_NT_MIN_MB=0.001: nontemporal stores and patch DMA at a test-sized output", 2, 264, 256, 16, 16, twin='c2-S-k16-int', mask=True, group='nt3')
_case("nt3-c2-U-k2", "sgx_conv4x4s2_up", H, ['conv2_kernel<2, 4, 1, 32, false, 0>'], "SGX_CONV_NT=3 with SGX_NT_MIN_MB=0.001: nontemporal stores and patch DMA at a test-sized output", 5, 9, 32, 64, 1024, twin='c2-U-k2', group='nt3')
_case("nt3-plain-c2-D-mf2", "sgx_conv4x4s2_down", H, ['conv2_kernel<1, 8, 2, 32, false, 0>'], "SGX_CONV_NT=3 with SGX_NT_MIN_MB=0.001: nontemporal stores and patch DMA at a test-sized output", 2, 136, 128, 32, 1024, twin='plain-c2-D-mf2', group='nt3')
_case("bands0-c2-S-k16-bands", "sgx_conv3x3", H, ['conv2_kernel<0, 8, 1, 16, true, 0>'], "SGX_TILE_BANDS=0: the plain tile order on the band-ordered grid", 10, 512, 512, 16, 16, twin='c2-S-k16-bands', group='bands0')
_case("deepk0-S-256", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 4, 4, 64, 1, false>'], "SGX_CONV_DEEPK=0: 32-channel chunks", 1, 5, 7, 256, 32, twin='g1-deepk-S-256-int', group='deepk0_upa0')
_case("deepk0-U-128", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 32, 2, 4, 4, 64, 1, false>'], "SGX_CONV_DEEPK=0 and SGX_CONV_UPA=0: per-class GUP blocks on 32-channel chunks", 1, 5, 7, 128, 32, twin='g1-deepk-U-128-int', group='deepk0_upa0')
_case("upa0-48-32", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 16, 2, 8, 8, 64, 1, false>'], "SGX_CONV_UPA=0: per-class GUP blocks, 16-channel chunks", 3, 9, 13, 48, 32, twin='g1-UPA-48-32-int', group='deepk0_upa0')
_case("upa0-32-16", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 32, 2, 16, 16, 256, 1, false>'], "SGX_CONV_UPA=0 on the 16x-wide tiles", 1, 136, 576, 32, 16, twin='up-g1-32-16', group='deepk0_upa0')
_case("splitk0-sk-2", "sgx_conv_splitk", H, [], "SGX_CONV_SPLITK=0: nothing splits: SGX_EUNSUPPORTED, workspace query 0", 1, 6, 10, 128, 32, group='splitk0', rc=-2)
_case("splitk2-sk-8-of-17", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "SGX_CONV_SPLITK=2: capped at 2 ways: 8 and 9 chunks", 1, 6, 10, 544, 32, twin='sk-8-of-17-int', group='splitk2')
_case("percu1-g1-S-48-96", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 16, 64, 1, false>'], "SGX_CONV_PERCU=1: one resident block per CU", 3, 17, 19, 48, 96, twin='g1-S-48-96-int', mask=True, group='percu1')
_case("percu1-g1-bands", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 16, 16, 256, 1, false>'], "SGX_CONV_PERCU=1: 2560 tiles of 16x16 >= 8 x 256 blocks (256 CUs) and >= 8 x 304: the first generation's XCD-band order", 1, 512, 1280, 32, 16, twin='g1-bands-twin', group='percu1')
_case("g1-bands-twin", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 16, 16, 256, 1, false>'], "the default twin of percu1-g1-bands: more resident blocks, fewer tiles per block than the band order wants", 1, 512, 1280, 32, 16)
_case("bigtile-g1-S-48-96-int", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 16, 16, 256, 2, false>'], "SGX_CONV_MINBLOCKS=1: the first candidate -- the biggest tile -- on a tiny ragged shape", 3, 17, 19, 48, 96, twin='g1-S-48-96-int', mask=True, group='bigtile')
_case("smalltile-g1-S-48-96-int", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 16, 64, 1, false>'], "SGX_CONV_MINBLOCKS=1000000, MAXBP=64, MAXCT=1: the 64-pixel, 16-channel tile", 3, 17, 19, 48, 96, twin='g1-S-48-96-int', mask=True, group='smalltile')
_case("bigtile-g1-D-96-48-int", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 128, 1, false>'], "SGX_CONV_MINBLOCKS=1: the first candidate -- the biggest tile -- on a tiny ragged shape", 3, 18, 26, 96, 48, twin='g1-D-96-48-int', group='bigtile')
_case("smalltile-g1-D-96-48-int", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 8, 8, 64, 1, false>'], "SGX_CONV_MINBLOCKS=1000000, MAXBP=64, MAXCT=1: the 64-pixel, 16-channel tile", 3, 18, 26, 96, 48, twin='g1-D-96-48-int', group='smalltile')
_case("bigtile-g1-UPA-48-32-int", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 256, 2, false>'], "SGX_CONV_MINBLOCKS=1: the first candidate -- the biggest tile -- on a tiny ragged shape", 3, 9, 13, 48, 32, twin='g1-UPA-48-32-int', group='bigtile')
_case("smalltile-g1-UPA-48-32-int", "sgx_conv4x4s2_up", H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 64, 1, false>'], "SGX_CONV_MINBLOCKS=1000000, MAXBP=64, MAXCT=1: the 64-pixel, 16-channel tile", 3, 9, 13, 48, 32, twin='g1-UPA-48-32-int', group='smalltile')
_case("bigtile-g1-S-5x7-64", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 4, 256, 4, false>'], "SGX_CONV_MINBLOCKS=1: the first candidate -- the biggest tile -- on a tiny ragged shape", 3, 5, 7, 16, 64, twin='g1-S-5x7-64', group='bigtile')
_case("smalltile-g1-S-5x7-64", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 4, 64, 1, false>'], "SGX_CONV_MINBLOCKS=1000000, MAXBP=64, MAXCT=1: the 64-pixel, 16-channel tile", 3, 5, 7, 16, 64, twin='g1-S-5x7-64', group='smalltile')
_case("bigtile-g1-S-9x13-64", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 8, 8, 256, 4, false>'], "SGX_CONV_MINBLOCKS=1: the first candidate -- the biggest tile -- on a tiny ragged shape", 3, 9, 13, 32, 64, twin='g1-S-9x13-64', group='bigtile')
_case("smalltile-g1-S-9x13-64", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 8, 8, 64, 1, false>'], "SGX_CONV_MINBLOCKS=1000000, MAXBP=64, MAXCT=1: the 64-pixel, 16-channel tile", 3, 9, 13, 32, 64, twin='g1-S-9x13-64', group='smalltile')
_case("g1-S-5x7-64", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 16, 0, 4, 4, 64, 1, false>'], "the default twin of the 4x4-tile rows of the groups bigtile / smalltile", 3, 5, 7, 16, 64)
_case("g1-S-9x13-64", "sgx_conv3x3", H, ['conv_kernel<bf16_t, 32, 0, 8, 8, 64, 1, false>'], "the default twin of the 8x8-tile rows of the groups bigtile / smalltile", 3, 9, 13, 32, 64)
_case("bigtile-f32-S-17x19-int", "sgx_conv3x3", F, ['conv_kernel<float, 16, 0, 16, 16, 256, 1, false>'], "SGX_CONV_MINBLOCKS=1 in fp32", 3, 17, 19, 16, 16, twin='f32-S-17x19-int', mask=True, group='bigtile')
_case("bigtile-f32-U-9x13-int", "sgx_conv4x4s2_up", F, ['conv_kernel<float, 16, 2, 8, 8, 256, 1, false>'], "SGX_CONV_MINBLOCKS=1 in fp32", 3, 9, 13, 16, 16, twin='f32-U-9x13-int', group='bigtile')
_case("fused0-bits", "sgx_conv3x3_signbits", H, ['conv2_kernel<0, 8, 1, 32, false, 0>'], "SGX_SIGNBITS=0 turns sgx_conv3x3_signbits_ok to 0; the entry point itself still runs", 3, 17, 32, 64, 2048, twin='c2-S-k2', mask=True, group='fused0')
_case("fused0-fade", "sgx_conv4x4s2_down_fade", H, ['conv2_kernel<1, 8, 1, 32, false, 0>'], "SGX_FUSE_FADE=0 turns sgx_conv4x4s2_down_fade_ok to 0", 5, 34, 64, 32, 1024, twin='fade-c2-D-mf1-int', group='fused0')
_case("fused0-upblur", "sgx_conv4x4s2_up_blur", H, ['conv2_kernel<2, 4, 1, 32, false, 2>'], "SGX_CONV_UP_BLUR=0 turns sgx_conv4x4s2_up_blur_ok to 0", 5, 9, 32, 32, 1024, twin='upblur-c2-U', data='sparse', group='fused0')

# ---- every conv_kernel instantiation that only a group's switches reach over the grid (operands up to 8 MB), each on the smallest shape that
# selects it at both CU counts, with the default-environment row of the same shape as its twin
_case("gtwin-S-bf16-B1-1x1-16-16", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 1, 1, 16, 16, mask=True)
_case("gtwin-S-bf16-B1-1x1-16-32", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 1, 1, 16, 32, mask=True)
_case("gtwin-S-bf16-B1-9x13-16-32", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 9, 13, 16, 32, mask=True)
_case("gtwin-S-bf16-B1-9x13-16-64", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 9, 13, 16, 64, mask=True)
_case("gtwin-D-bf16-B1-2x2-16-16", ENTRY["D"], H, ['conv_kernel<bf16_t, 16, 1, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 2, 2, 16, 16)
_case("gtwin-D-bf16-B1-2x2-16-32", ENTRY["D"], H, ['conv_kernel<bf16_t, 16, 1, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 2, 2, 16, 32)
_case("gtwin-D-bf16-B1-18x26-16-32", ENTRY["D"], H, ['conv_kernel<bf16_t, 16, 1, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 18, 26, 16, 32)
_case("gtwin-U-bf16-B1-1x1-16-16", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 1, 1, 16, 16)
_case("gtwin-U-bf16-B1-1x1-16-32", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 1, 1, 16, 32)
_case("gtwin-U-bf16-B17-17x19-16-32", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 16, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 17, 17, 19, 16, 32)
_case("gtwin-U-bf16-B17-17x19-16-64", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 16, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 17, 17, 19, 16, 64)
_case("gtwin-U-bf16-B33-17x19-16-64", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 16, 16, 256, 1, false>'], "the default-environment twin of the switched rows on this shape", 33, 17, 19, 16, 64)
_case("gtwin-U-bf16-B1-17x19-16-16", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 16, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 17, 19, 16, 16)
_case("gtwin-U-bf16-B17-6x10-16-128", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 17, 6, 10, 16, 128)
_case("gtwin-U-bf16-B33-6x10-16-128", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 33, 6, 10, 16, 128)
_case("gtwin-U-bf16-B3-17x19-16-128", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 16, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 3, 17, 19, 16, 128)
_case("gtwin-U-bf16-B3-9x32-16-128", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 3, 9, 32, 16, 128)
_case("gtwin-U-bf16-B5-9x32-16-128", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 5, 9, 32, 16, 128)
_case("gtwin-U-bf16-B33-9x13-16-128", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 8, 8, 128, 1, false>'], "the default-environment twin of the switched rows on this shape", 33, 9, 13, 16, 128)
_case("gtwin-U-bf16-B1-17x19-32-1024", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 4, 16, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 17, 19, 32, 1024)
_case("gtwin-U-bf16-B1-17x19-32-2048", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 16, 16, 256, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 17, 19, 32, 2048)
_case("gtwin-U-bf16-B1-17x19-32-16", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 4, 16, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 17, 19, 32, 16)
_case("gtwin-U-bf16-B9-1x1-32-1024", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 9, 1, 1, 32, 1024)
_case("gtwin-U-bf16-B1-1x1-32-2048", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 1, 1, 32, 2048)
_case("gtwin-U-bf16-B17-1x1-32-2048", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 4, 4, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 17, 1, 1, 32, 2048)
_case("gtwin-U-bf16-B1-5x7-32-2048", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 4, 4, 256, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 5, 7, 32, 2048)
_case("gtwin-U-bf16-B3-17x19-32-128", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 4, 16, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 3, 17, 19, 32, 128)
_case("gtwin-U-bf16-B3-9x13-32-256", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 3, 9, 13, 32, 256)
_case("gtwin-U-bf16-B1-9x13-32-512", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 9, 13, 32, 512)
_case("gtwin-U-bf16-B1-9x13-32-1024", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 9, 13, 32, 1024)
_case("gtwin-U-bf16-B1-9x13-32-2048", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 8, 8, 256, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 9, 13, 32, 2048)
_case("gtwin-U-bf16-B1-9x13-32-16", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 3, 8, 8, 64, 1, false>'], "the default-environment twin of the switched rows on this shape", 1, 9, 13, 32, 16)
_case("bigtile-g1<bf16,16,0,4,4,256,1>", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 4, 4, 256, 1, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 1, 1, 16, 16, group="bigtile", twin="gtwin-S-bf16-B1-1x1-16-16", mask=True)   # 0.00 MB
_case("bigtile-g1<bf16,16,0,4,4,256,2>", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 4, 4, 256, 2, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 1, 1, 16, 32, group="bigtile", twin="gtwin-S-bf16-B1-1x1-16-32", mask=True)   # 0.00 MB
_case("bigtile-g1<bf16,16,0,8,8,256,2>", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 8, 8, 256, 2, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 9, 13, 16, 32, group="bigtile", twin="gtwin-S-bf16-B1-9x13-16-32", mask=True)   # 0.01 MB
_case("bigtile-g1<bf16,16,0,8,8,256,4>", ENTRY["S"], H, ['conv_kernel<bf16_t, 16, 0, 8, 8, 256, 4, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 9, 13, 16, 64, group="bigtile", twin="gtwin-S-bf16-B1-9x13-16-64", mask=True)   # 0.02 MB
_case("bigtile-g1<bf16,16,1,4,4,128,1>", ENTRY["D"], H, ['conv_kernel<bf16_t, 16, 1, 4, 4, 128, 1, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 2, 2, 16, 16, group="bigtile", twin="gtwin-D-bf16-B1-2x2-16-16")   # 0.00 MB
_case("bigtile-g1<bf16,16,1,4,4,128,2>", ENTRY["D"], H, ['conv_kernel<bf16_t, 16, 1, 4, 4, 128, 2, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 2, 2, 16, 32, group="bigtile", twin="gtwin-D-bf16-B1-2x2-16-32")   # 0.00 MB
_case("bigtile-g1<bf16,16,1,8,8,128,2>", ENTRY["D"], H, ['conv_kernel<bf16_t, 16, 1, 8, 8, 128, 2, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 18, 26, 16, 32, group="bigtile", twin="gtwin-D-bf16-B1-18x26-16-32")   # 0.02 MB
_case("bigtile-g1<bf16,16,3,4,4,256,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 4, 256, 1, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 1, 1, 16, 16, group="bigtile", twin="gtwin-U-bf16-B1-1x1-16-16")   # 0.00 MB
_case("bigtile-g1<bf16,16,3,4,4,256,2>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 3, 4, 4, 256, 2, false>'], "reached only under the switches of the group `bigtile`: the smallest shape of the grid that selects it", 1, 1, 1, 16, 32, group="bigtile", twin="gtwin-U-bf16-B1-1x1-16-32")   # 0.00 MB
_case("deepk0_upa0-g1<bf16,16,2,16,16,256,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 16, 16, 256, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 17, 17, 19, 16, 32, group="deepk0_upa0", twin="gtwin-U-bf16-B17-17x19-16-32")   # 1.51 MB
_case("deepk0_upa0-g1<bf16,16,2,16,16,256,2>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 16, 16, 256, 2, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 17, 17, 19, 16, 64, group="deepk0_upa0", twin="gtwin-U-bf16-B17-17x19-16-64")   # 2.85 MB
_case("deepk0_upa0-g1<bf16,16,2,16,16,256,4>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 16, 16, 256, 4, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 33, 17, 19, 16, 64, group="deepk0_upa0", twin="gtwin-U-bf16-B33-17x19-16-64")   # 5.53 MB
_case("deepk0_upa0-g1<bf16,16,2,4,16,64,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 4, 16, 64, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 17, 19, 16, 16, group="deepk0_upa0", twin="gtwin-U-bf16-B1-17x19-16-16")   # 0.05 MB
_case("deepk0_upa0-g1<bf16,16,2,4,4,128,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 4, 4, 128, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 17, 6, 10, 16, 128, group="deepk0_upa0", twin="gtwin-U-bf16-B17-6x10-16-128")   # 1.03 MB
_case("deepk0_upa0-g1<bf16,16,2,4,4,256,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 4, 4, 256, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 33, 6, 10, 16, 128, group="deepk0_upa0", twin="gtwin-U-bf16-B33-6x10-16-128")   # 1.99 MB
_case("deepk0_upa0-g1<bf16,16,2,4,4,64,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 4, 4, 64, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 1, 1, 16, 16, group="deepk0_upa0", twin="gtwin-U-bf16-B1-1x1-16-16")   # 0.00 MB
_case("deepk0_upa0-g1<bf16,16,2,8,16,128,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 8, 16, 128, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 3, 17, 19, 16, 128, group="deepk0_upa0", twin="gtwin-U-bf16-B3-17x19-16-128")   # 0.98 MB
_case("deepk0_upa0-g1<bf16,16,2,8,8,128,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 8, 8, 128, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 3, 9, 32, 16, 128, group="deepk0_upa0", twin="gtwin-U-bf16-B3-9x32-16-128")   # 0.87 MB
_case("deepk0_upa0-g1<bf16,16,2,8,8,256,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 8, 8, 256, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 5, 9, 32, 16, 128, group="deepk0_upa0", twin="gtwin-U-bf16-B5-9x32-16-128")   # 1.45 MB
_case("deepk0_upa0-g1<bf16,16,2,8,8,256,2>", ENTRY["U"], H, ['conv_kernel<bf16_t, 16, 2, 8, 8, 256, 2, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 33, 9, 13, 16, 128, group="deepk0_upa0", twin="gtwin-U-bf16-B33-9x13-16-128")   # 3.89 MB
_case("deepk0_upa0-g1<bf16,32,2,16,16,256,2>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 16, 16, 256, 2, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 17, 19, 32, 1024, group="deepk0_upa0", twin="gtwin-U-bf16-B1-17x19-32-1024")   # 2.54 MB
_case("deepk0_upa0-g1<bf16,32,2,16,16,256,4>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 16, 16, 256, 4, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 17, 19, 32, 2048, group="deepk0_upa0", twin="gtwin-U-bf16-B1-17x19-32-2048")   # 5.07 MB
_case("deepk0_upa0-g1<bf16,32,2,4,16,64,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 4, 16, 64, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 17, 19, 32, 16, group="deepk0_upa0", twin="gtwin-U-bf16-B1-17x19-32-16")   # 0.06 MB
_case("deepk0_upa0-g1<bf16,32,2,4,4,128,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 4, 4, 128, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 9, 1, 1, 32, 1024, group="deepk0_upa0", twin="gtwin-U-bf16-B9-1x1-32-1024")   # 0.07 MB
_case("deepk0_upa0-g1<bf16,32,2,4,4,256,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 4, 4, 256, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 1, 1, 32, 2048, group="deepk0_upa0", twin="gtwin-U-bf16-B1-1x1-32-2048")   # 0.02 MB
_case("deepk0_upa0-g1<bf16,32,2,4,4,256,2>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 4, 4, 256, 2, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 17, 1, 1, 32, 2048, group="deepk0_upa0", twin="gtwin-U-bf16-B17-1x1-32-2048")   # 0.27 MB
_case("deepk0_upa0-g1<bf16,32,2,4,4,256,4>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 4, 4, 256, 4, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 5, 7, 32, 2048, group="deepk0_upa0", twin="gtwin-U-bf16-B1-5x7-32-2048")   # 0.55 MB
_case("deepk0_upa0-g1<bf16,32,2,8,16,128,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 8, 16, 128, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 3, 17, 19, 32, 128, group="deepk0_upa0", twin="gtwin-U-bf16-B3-17x19-32-128")   # 1.01 MB
_case("deepk0_upa0-g1<bf16,32,2,8,8,128,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 8, 8, 128, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 3, 9, 13, 32, 256, group="deepk0_upa0", twin="gtwin-U-bf16-B3-9x13-32-256")   # 0.71 MB
_case("deepk0_upa0-g1<bf16,32,2,8,8,256,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 8, 8, 256, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 9, 13, 32, 512, group="deepk0_upa0", twin="gtwin-U-bf16-B1-9x13-32-512")   # 0.46 MB
_case("deepk0_upa0-g1<bf16,32,2,8,8,256,2>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 8, 8, 256, 2, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 9, 13, 32, 1024, group="deepk0_upa0", twin="gtwin-U-bf16-B1-9x13-32-1024")   # 0.92 MB
_case("deepk0_upa0-g1<bf16,32,2,8,8,256,4>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 8, 8, 256, 4, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 9, 13, 32, 2048, group="deepk0_upa0", twin="gtwin-U-bf16-B1-9x13-32-2048")   # 1.84 MB
_case("deepk0_upa0-g1<bf16,32,2,8,8,64,1>", ENTRY["U"], H, ['conv_kernel<bf16_t, 32, 2, 8, 8, 64, 1, false>'], "reached only under the switches of the group `deepk0_upa0`: the smallest shape of the grid that selects it", 1, 9, 13, 32, 16, group="deepk0_upa0", twin="gtwin-U-bf16-B1-9x13-32-16")   # 0.02 MB

# ---- the other four split-K instantiations the plan reaches: 16-channel chunks on every tile, 32-channel chunks on the 4x16 tile
_case("sk-16ch-4x4-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 16, 1, 4, 4, 64, 1, false>'], "the unsplit twin of sk-16ch-4x4", 1, 6, 10, 112, 16)
_case("sk-16ch-4x4", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 16, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "Cin 112: seven 16-channel chunks over 3 ways (2, 2, 3), the 4x4 tile: 3 ways", 1, 6, 10, 112, 16, twin="sk-16ch-4x4-unsplit")
_case("sk-16ch-4x4-randn", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 16, 1, 4, 4, 64, 1, true>', 'conv_splitk_finish'], "Cin 112: seven 16-channel chunks over 3 ways (2, 2, 3), the 4x4 tile: 3 ways", 1, 6, 10, 112, 16, data="randn")
_case("sk-16ch-8x8-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 16, 1, 8, 8, 64, 1, false>'], "the unsplit twin of sk-16ch-8x8", 1, 18, 26, 112, 16)
_case("sk-16ch-8x8", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 16, 1, 8, 8, 64, 1, true>', 'conv_splitk_finish'], "16-channel chunks, the 8x8 tile: 3 ways", 1, 18, 26, 112, 16, twin="sk-16ch-8x8-unsplit")
_case("sk-16ch-8x8-randn", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 16, 1, 8, 8, 64, 1, true>', 'conv_splitk_finish'], "16-channel chunks, the 8x8 tile: 3 ways", 1, 18, 26, 112, 16, data="randn")
_case("sk-16ch-4x16-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 16, 1, 4, 16, 64, 1, false>'], "the unsplit twin of sk-16ch-4x16", 1, 34, 38, 112, 16)
_case("sk-16ch-4x16", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 16, 1, 4, 16, 64, 1, true>', 'conv_splitk_finish'], "16-channel chunks, the 4x16 tile, ragged: 3 ways", 1, 34, 38, 112, 16, twin="sk-16ch-4x16-unsplit")
_case("sk-16ch-4x16-randn", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 16, 1, 4, 16, 64, 1, true>', 'conv_splitk_finish'], "16-channel chunks, the 4x16 tile, ragged: 3 ways", 1, 34, 38, 112, 16, data="randn")
_case("sk-4x16-unsplit", "sgx_conv4x4s2_down", H, ['conv_kernel<bf16_t, 32, 1, 4, 16, 64, 1, false>'], "the unsplit twin of sk-4x16", 1, 34, 38, 128, 16)
_case("sk-4x16", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 16, 64, 1, true>', 'conv_splitk_finish'], "32-channel chunks, the 4x16 tile, ragged: 2 ways", 1, 34, 38, 128, 16, twin="sk-4x16-unsplit")
_case("sk-4x16-randn", "sgx_conv_splitk", H, ['conv_kernel<bf16_t, 32, 1, 4, 16, 64, 1, true>', 'conv_splitk_finish'], "32-channel chunks, the 4x16 tile, ragged: 2 ways", 1, 34, 38, 128, 16, data="randn")

# ---- sgx_pack_weight / sgx_pack_weight_multi: both packs, every mode, both dtypes; O and I off the 32 x 32 pack tile, Ipad > I (zero padding),
# and whole tiles (the 16-byte load / store paths).  Cout = O, Cin = Ipad in the shape columns.
PACK_SHAPES = {"edge": (48, 33, 48, "O 48, I 33 padded to 48: edge tiles element-wise, scalar loads, the padding written as zeros"),
               "full": (64, 64, 64, "O = I = 64: whole tiles, 16-byte loads and stores"),
               "mixed": (40, 64, 64, "O 40: a whole tile row over a partial one")}
for _dt in (F, H):
    for _m in MODES:
        for _s, (_O, _I, _Ip, _why) in PACK_SHAPES.items():
            for _data in ("int", "randn") if _s == "edge" else ("int",):
                _case(f"pack-{_m}-{_s}-{_data}-{dn(_dt)}", "sgx_pack_weight", _dt, [f"pack_weight_kernel<{tname(_dt)}>"], f"mode {_m}; " + _why, 1, 1, 1, _Ip, _O, data=_data, bias=False,
                      act=ACT_NONE, O=_O, I=_I, Ipad=_Ip, mode=_m)
    _case(f"pack-multi-{dn(_dt)}", "sgx_pack_weight_multi", _dt, [f"pack_weight_multi_kernel<{tname(_dt)}>"], "five parameters of every mode and tile kind in one launch: the bits of the single launches",
          1, 1, 1, 0, 0, bias=False, act=ACT_NONE, n=5, params=(("S", "edge"), ("D", "full"), ("U", "mixed"), ("UF", "edge"), ("S", "full")))

# ---- sgx_conv_upblur on top of sgx_pack_upblur (conv3_kernel<UB>): integer rows -- parameters in [-3, 3] and scale 2^-4 (x 0.25 in mode D) make
# every composite tap and correction tile an integer of at most 192 times a power of two, exact in bf16, and every sum exact in fp32, so y is
# the fp64 blur3x3(conv_transpose(x)) rounded once, bit for bit, image borders (the correction tiles) included.  Cin = 32, Cout = 16.
UPB8, UPB4, UPBC = "conv3_kernel<0, 8, 2, 2, 2, 0, 1>", "conv3_kernel<0, 4, 2, 2, 2, 0, 1>", "conv3_kernel<0, 4, 2, 2, 2, 0, 2>"
_UPB = "sgx_conv_upblur"
_case("upb-4w-U", _UPB, H, [UPB4], "B3 9x32: 6 tiles of 8x32 < CUs: the 4-wave block; 9 rows: a ragged second tile row, every border correction in one tile column; mode U", 3, 9, 32, 32, 16, mode="U", adjoint=0, bits=False)
_case("upb-4w-UF-bits", _UPB, H, [UPB4], "mode UF (the flipped kernel) with the mask as sign bits", 3, 9, 32, 32, 16, mode="UF", adjoint=0, bits=True)
_case("upb-4w-D-bits", _UPB, H, [UPB4], "mode D, adjoint: the data gradient of a down layer (parameter [32][16]), B1 17x64: two tile columns, three tile rows, sign bits", 1, 17, 64, 32, 16, mode="D", adjoint=1, bits=True)
_case("upb-8w-U-bits", _UPB, H, [UPB8], "B5 40x832: 390 tiles of 16x32 >= CUs at 256 and 304: the 8-wave block; 40 rows: a ragged third tile row", 5, 40, 832, 32, 16, mode="U", adjoint=0, bits=True)
_case("upb-8w-D", _UPB, H, [UPB8], "the 8-wave block on the adjoint pack, no mask", 5, 40, 832, 32, 16, mode="D", adjoint=1, bits=False)
_case("upb-compact-U-bits", _UPB, H, [UPBC], "SGX_UPBLUR_BPC=2 and 650 tiles of 8x32 >= 2 x CUs: two compact 4-wave blocks per CU", 5, 40, 832, 32, 16, mode="U", adjoint=0, bits=True, group="upblur_bpc2", twin="upb-8w-U-bits")
_case("upb-compact-D", _UPB, H, [UPBC], "the compact block on the adjoint pack", 5, 40, 832, 32, 16, mode="D", adjoint=1, bits=False, group="upblur_bpc2", twin="upb-8w-D")
_case("upb-bpc2-small", _UPB, H, [UPB4], "SGX_UPBLUR_BPC=2 below 2 x CUs tiles: the plain 4-wave block", 3, 9, 32, 32, 16, mode="U", adjoint=0, bits=False, group="upblur_bpc2", twin="upb-4w-U")
_case("fused0-upb", _UPB, H, [UPB4], "SGX_CONV_UPBLUR=0 turns sgx_conv_upblur_ok to 0; the entry point itself still runs", 3, 9, 32, 32, 16, mode="U", adjoint=0, bits=False, group="fused0", twin="upb-4w-U")
_case("rej-upb-cin64", _UPB, H, [], "sgx_conv_upblur_ok == 0: Cin 64", 1, 9, 32, 64, 16, mode="U", adjoint=0, bits=False, rc=EUNSUPPORTED)
_case("rej-upb-w48", _UPB, H, [], "sgx_conv_upblur_ok == 0: W no multiple of 32", 1, 9, 48, 32, 16, mode="U", adjoint=0, bits=False, rc=EUNSUPPORTED)
for _m, _adj in (("U", 0), ("UF", 0), ("D", 1)):
    _case(f"pack-upblur-{_m}", "sgx_pack_upblur", H, ["pack_upblur_kernel"], f"mode {_m}, adjoint {_adj}: the 9 composite taps against the 1-D composition table, bit for bit", 1, 1, 1, 32, 16, mode=_m, adjoint=_adj)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), [c.id for c in CASES if sum(1 for d in CASES if d.id == c.id) > 1]

# Launch sites no row claims by name, by the text of the site, with the reason
EXCLUDED_SITES = {
    "kern": "conv_kernel / conv2_kernel / conv3_kernel through the function pointer of launch_conv / launch_conv2 / launch_conv3: the instantiation scan of tests/test_conv_coverage.py enumerates them",
}
# Paths no row takes, by name, with the reason
EXCLUDED_PATHS = {
    "SGX_CONV_DBG": "probe builds only: ablations of conv_kernel that compute wrong results by design",
    "SGX_CONV3_DBG": "probe builds only: DMA ablations of conv3_kernel that compute wrong results by design",
    "sgx_conv_variant 20..23": "probe configurations (128-channel blocks on 16-channel K-steps; 32-channel blocks whatever Cout): tools/conv2_probe.py, not a launch path of the library",
    "conv3x3_stats EINVAL": "launch_conv2 refuses partials sized for another slot count, but sgx_conv3x3_stats sizes part_slots from the same plan as the launch: the code is not reachable through the C ABI",
    "sgx_pack_upblur correction tiles": "the 22 border-correction tiles have no table of their own here: the integer rows of sgx_conv_upblur pin them through the image borders of the result (9 and 17 rows, "
                                        "one and two tile columns), bit for bit against blur3x3(conv_transpose(x)); the 9 composite taps are compared with the 1-D composition table directly (pack-upblur-*)",
    "sgx_conv_upblur randn": "its rounding rows need the composite taps' one rounding to bf16 restated through the correction tiles: integer rows only, as for the blur epilogue",
    "up_blur randn": "conv2_kernel's blur epilogue rounds the vertical pass and the rows exchanged between waves to bf16 before the horizontal pass (as the passes it replaces round the convolution's output): "
                     "one rounding of the fp64 value does not bound it, and where the extra roundings fall depends on the tile a pixel lands in.  Its rows are `sparse` integer rows whose every intermediate is "
                     "bf16-exact (asserted from the reference), so any placement of the roundings gives the exact bits",
    "mask on randn rows": "the output mask multiplies the ROUNDED value and rounds again (bit for bit sgx_lrelu_bwd on the stored tensor): pinned bit for bit on the integer rows, not restated for the rounding rows",
}

ALPHA_INT, BETA_INT = 0.5, 0.25                   # fade coefficients of the integer rows: powers of two, every product exact
ALPHA_RND, BETA_RND = SR.f32(0.7), SR.f32(0.3)
SPARSE = 1.0 / 16                                 # share of non-zero inputs of the `sparse` rows
BITS_CAP = 0.005                                  # share of a row's sign bits that may be left out (|pre-activation| within its own bound)


def row_plan(c, ncu):
    return plan(c.entry, c.dtype, c.args, group_env(c.group), ncu)


def row_kernels(c, ncu):
    return c.args["k304"] if ncu == 304 and c.args["k304"] is not None else c.kernels


def geo_of(c):
    if c.entry in ("sgx_conv_variant", "sgx_conv_splitk"):
        return c.args.get("geo", 1)
    return {"sgx_conv3x3": 0, "sgx_conv3x3_signbits": 0, "sgx_conv3x3_stats": 0, "sgx_conv4x4s2_down": 1, "sgx_conv4x4s2_down_fade": 1, "sgx_conv4x4s2_down_fade_rgb": 1,
            "sgx_conv4x4s2_up": 2, "sgx_conv4x4s2_up_blur": 2, "sgx_conv4x4s2_up_blur_bits": 2, "sgx_conv_upblur": 2, "sgx_pack_upblur": 2}[c.entry]


def weight_scale(geo, Cin):
    """Rounding rows: weights ~ N(0, 1 / (taps that meet in an output x Cin)) so that outputs are O(1)."""
    return 1.0 / math.sqrt({0: 9, 1: 16, 2: 4}[geo] * Cin)
