"""fp64 restatements of the weight-gradient entry points of libsgx_hip.so (sgx_wgrad3x3_param, sgx_wgrad4x4s2_param, sgx_wgrad_ws_bytes: the
second half of csrc/conv.hip and all of csrc/wgrad2.hip), written from include/sgx.h and the pack definitions above pack_tap in conv.hip; the
launcher rules restated as functions of the shape, the workspace, the environment and the device's CU count; and the table of cases that
walks every launch path.  Test-side only: nothing here imports the library under test.

Layouts are the C ABI's: activations NHWC, dW[O][I][3][3] fp32, db[O] fp32.  "k side" = x (3x3) / the fine tensor (4x4 stride 2), "n side" =
dy / the coarse tensor, as in conv.hip.  Every reference returns ``(ref, S)``: the value and the same expression on absolute values.

Two criteria.  Integer rows (operands in [-3, 3], a power-of-two scale, integer prefill): every product, partial, fold and scaled sum is an
exact fp32 number whatever the order, so dW / db equal the fp64 reference bit for bit -- and every other path that computes the same row.
Rounding rows (randn and |randn| operands): |got - ref| <= (L + 2) 2^-24 S with L = ceil(ntiles / nsplit) * BP + nsplit + 16, the longest fp32
chain of the path (the pixels one block walks, any order of summing the splits, the fold and the scale); dW is fp32: no output rounding."""
import math
from collections import namedtuple

import torch

F, H = torch.float32, torch.bfloat16
EWORKSPACE = -3
MODES = {"S": 0, "D": 1, "U": 2, "UF": 3}


def tname(dt):
    return "float" if dt == F else "bf16_t"


# ---------------------------------------------------------------------------------------------------------------- fp64 references
def tap_partials(xk, xn, geo):
    """P[t][n][k] = sum over (b, y, x) of xn[b, y, x, n] * xk[b, IS*y + ty - 1, IS*x + tx - 1, k], zero outside: 3x3 stride 1 (geo 0, t = 3 ty +
    tx) or 4x4 stride 2 (geo 1, t = 4 ty + tx).  fp64 in, fp64 out."""
    IS, TK = (1, 3) if geo == 0 else (2, 4)
    B, Hn, Wn, Cn = xn.shape
    assert xk.shape[1] == IS * Hn and xk.shape[2] == IS * Wn
    xp = torch.nn.functional.pad(xk, (0, 0, 1, 1, 1, 1))
    a = xn.reshape(-1, Cn)
    out = []
    for ty in range(TK):
        for tx in range(TK):
            out.append(a.t() @ xp[:, ty:ty + IS * Hn:IS, tx:tx + IS * Wn:IS, :].reshape(a.shape[0], -1))
    return torch.stack(out)


def fold(P, mode, scale, adjoint=0):
    """Raw partials [t][n][k] -> the parameter-layout value [O][Ip][3][3] (before the I < Ip cut and the accumulate).  S: scale * P[tap], with
    flip_t (tap 8 - t) and (o, i) = (k, n) for the adjoint launch; D / U / UF: scale * sum of the four 4x4 taps (y + a, x + b), x 0.25 for D,
    (o, i) = (k, n) for U / UF, the 3x3 result spatially flipped for UF."""
    if mode == "S":
        v = P.flip(0) if adjoint else P
    else:
        P4 = P.view(4, 4, *P.shape[1:])
        v = (P4[:3, :3] + P4[:3, 1:] + P4[1:, :3] + P4[1:, 1:]).reshape(9, *P.shape[1:])
        if mode == "UF":
            v = v.flip(0)
    if adjoint or mode in ("U", "UF"):
        v = v.transpose(1, 2)
    c = scale * (0.25 if mode == "D" else 1.0)
    return (c * v).permute(1, 2, 0).reshape(v.shape[1], v.shape[2], 3, 3)


def wgrad(xk, xn, mode, scale, I, adjoint=0, accumulate=0, dW0=None, db0=None, want_db=True):
    """-> (dW, S_dW, db, S_db) in fp64.  dW[O][I][3][3]: rows i >= I of the padded channel axis do not exist.  db = column sums of the n side,
    unscaled (only asked where the n side has the O channels)."""
    geo = 0 if mode == "S" else 1
    v, Sv = fold(tap_partials(xk, xn, geo), mode, scale, adjoint), fold(tap_partials(xk.abs(), xn.abs(), geo), mode, abs(scale), adjoint)
    v, Sv = v[:, :I].contiguous(), Sv[:, :I].contiguous()
    if accumulate & 1:
        v, Sv = v + dW0, Sv + dW0.abs()
    db = Sb = None
    if want_db:
        db, Sb = xn.sum((0, 1, 2)), xn.abs().sum((0, 1, 2))
        if accumulate & 2:
            db, Sb = db + db0, Sb + db0.abs()
    return v, Sv, db, Sb


# ---------------------------------------------------------------------------------------------------------------- launcher rules
ENV0 = {"SGX_WGRAD_BLOCKS": 0, "SGX_WGRAD_MAXSPLIT": 0, "SGX_WGRAD_BLOCKS_MID": 0, "SGX_WGRAD_TR": 1, "SGX_WGRAD_PRE": 32, "SGX_WGRAD_PRE_MIN": 256,
        "SGX_WGRAD2": 7, "SGX_WGRAD2_MAXCT": 32}
GROUPS = {"default": {}, "w2_0": {"SGX_WGRAD2": "0"}, "w2_3": {"SGX_WGRAD2": "3"}, "w2_5": {"SGX_WGRAD2": "5"}, "w2_6": {"SGX_WGRAD2": "6"},
          "tr0": {"SGX_WGRAD_TR": "0"}, "pre0": {"SGX_WGRAD_PRE": "0"}, "pre4": {"SGX_WGRAD_PRE": "4", "SGX_WGRAD_PRE_MIN": "8"},
          "maxsplit3": {"SGX_WGRAD_MAXSPLIT": "3"}, "blocks": {"SGX_WGRAD_BLOCKS": "4096"}, "maxct1": {"SGX_WGRAD2_MAXCT": "1"}}


def group_env(group):
    return dict(ENV0, **{k: int(v) for k, v in GROUPS[group].items()})


def cdiv(a, b):
    return (a + b - 1) // b


def wgrad_nsplit(pairs, ntiles, elems, env):
    tiny = elems <= 16 * 32 * 32
    target = env["SGX_WGRAD_BLOCKS"] or (2048 if tiny else (env["SGX_WGRAD_BLOCKS_MID"] or 512))
    cap = env["SGX_WGRAD_MAXSPLIT"] or (1024 if tiny else 512)
    want = cdiv(target, pairs)
    if not env["SGX_WGRAD_BLOCKS"] and pairs >= 512 and ntiles <= 64:
        want = 1
    return max(1, min(want, cap, ntiles))


def wgrad_ch(geo, B, Hn, Wn, Ck, Cn):
    """-> (NSUB, KSUB, lowres_big)"""
    n32, k32 = Cn % 32 == 0, Ck % 32 == 0
    if geo == 1:
        return (2, 1, False) if n32 else (1, 1, False)
    BP = 128
    lowres_big = B * Hn * Wn <= 64 * BP and (Cn // 32) * (Ck // 32) < 512 and (Cn // 32) * (Ck // 16) >= 512
    if n32 and k32 and not lowres_big:
        return 2, 2, False
    if n32:
        return 2, 1, lowres_big and k32
    return (1, 2, False) if k32 else (1, 1, False)


def wgrad_tile(geo, Hn, Wn):
    """-> (TH, TW, BP)"""
    BP = 128 if geo == 0 else 64
    if Hn >= 16 and Wn >= 16:
        return BP // 16, 16, BP
    if Hn >= 8 and Wn >= 8:
        return 8, 8, BP
    return 4, 4, BP


def pre_bytes(total, nsplit, env):
    G = env["SGX_WGRAD_PRE"]
    return G * total * 4 if G > 0 and nsplit >= env["SGX_WGRAD_PRE_MIN"] and nsplit > G and total % 4 == 0 else 0


def wgrad2_plan(geo, B, Hn, Wn, Ck, Cn, env, ncu):
    """sgx_wgrad2_plan -> (ns, kernel, ntiles): ns = 0 when the shape stays with the first generation."""
    sw, maxct = env["SGX_WGRAD2"], env["SGX_WGRAD2_MAXCT"]
    if not (sw >> geo) & 1:
        return 0, None, 0
    if geo == 0 and Ck == 16 and Cn == 16:
        if not sw & 4 or Wn % 32:
            return 0, None, 0
        ntiles = B * cdiv(Hn, 16) * (Wn // 32)
        ns = 2 * ncu // 8 * 8
        if ntiles < 2 * ns:
            ns = ntiles // 2 // 8 * 8
        return (ns, "wgrad16_s_kernel", ntiles) if ns >= 8 else (0, None, ntiles)
    if geo == 0:
        if Ck % 64 or Cn % 64 or Wn % 32 or Hn % 8:
            return 0, None, 0
        th, tw, kt, kern = 8, 32, 64, "wgrad2_s_kernel<8>"
    else:
        if Cn % 64 or Ck % 32 or Wn % 16 or Hn % 4:
            return 0, None, 0
        kbw = 2 if Ck % 64 == 0 else 1
        th, tw, kt, kern = 4, 16, 32 * kbw, f"wgrad2_d_kernel<{kbw}>"
    nct = (Cn // 64) * (Ck // kt)
    ntiles = B * (Hn // th) * (Wn // tw)
    if nct > 2 * maxct:
        return 0, None, ntiles
    ns = max(8, ncu // nct // 8 * 8)
    if nct > maxct and ntiles < 8 * ns:
        return 0, None, ntiles
    if ntiles < 2 * ns:
        ns = ntiles // 2 // 8 * 8
    return (ns, kern, ntiles) if ns >= 8 else (0, None, ntiles)


def ws_bytes(taps, B, Hf, Wf, Ck, Cn, env, ncu):
    """sgx_wgrad_ws_bytes (H, W: the k side's size, as the C ABI takes it)."""
    total = taps * Ck * Cn + Cn
    pairs = max(Ck // 32, 1) * max(Cn // 32, 1)
    ns = wgrad_nsplit(pairs, min(B * cdiv(Hf, 4) * cdiv(Wf, 4), 1 << 30), taps * Ck * Cn, env)
    need = total * 4 * ns + pre_bytes(total, ns, env)
    ns2 = wgrad2_plan(0, B, Hf, Wf, Ck, Cn, env, ncu)[0] if taps == 9 else wgrad2_plan(1, B, Hf // 2, Wf // 2, Ck, Cn, env, ncu)[0]
    return max(need, total * 4 * ns2 + pre_bytes(total, ns2, env) if ns2 else 0)


def finish_epb(O, Ip):
    ne = O * Ip
    return 64 if ne // 64 >= 128 else 16 if ne // 16 >= 128 else 8 if ne // 8 >= 128 else 4


Plan = namedtuple("Plan", "rc kernels nsplit finish_ns L gen")


def plan(entry, dt, B, Hf, Wf, Ck, Cn, O, Ip, wsb, env, ncu):
    """What one call launches: the kernel instantiations in order, the pixel splits of the gradient kernel, the ``ns`` the finishing launch
    reports (None for the direct epilogue), the fp32 chain L of the bound, and the generation (1 / 2) that ran."""
    geo = 0 if entry == "sgx_wgrad3x3_param" else 1
    Hn, Wn, NT = (Hf, Wf, 9) if geo == 0 else (Hf // 2, Wf // 2, 16)
    total = NT * Cn * Ck + Cn
    kernels, gen = [], 1
    ns, kern, ntiles = wgrad2_plan(geo, B, Hn, Wn, Ck, Cn, env, ncu) if dt == H else (0, None, 0)
    if ns and ns * total * 4 <= wsb:
        kernels, gen = [kern], 2
        bp = {"wgrad16_s_kernel": 512, "wgrad2_s_kernel<8>": 256}.get(kern, 64)             # pixels of one tile
    else:
        NS, KS, _ = wgrad_ch(geo, B, Hn, Wn, Ck, Cn)
        TH, TW, bp = wgrad_tile(geo, Hn, Wn)
        ntiles = cdiv(B, bp // (TH * TW)) * cdiv(Hn, TH) * cdiv(Wn, TW)
        ns = min(wgrad_nsplit((Cn // (16 * NS)) * (Ck // (16 * KS)), ntiles, NT * Cn * Ck, env), wsb // (total * 4))
        if ns < 1:
            return Plan(EWORKSPACE, (), 0, None, 0, 1)
        tr = "true" if dt == H and env["SGX_WGRAD_TR"] else "false"
        kernels = [f"wgrad_kernel<{tname(dt)}, {geo}, {TH}, {TW}, {bp}, {NS}, {KS}, {tr}>"]
    L = cdiv(ntiles, ns) * bp + ns + 16
    if gen == 1 and ns == 1:
        return Plan(0, tuple(kernels), 1, None, L, 1)
    fns = ns
    pre = pre_bytes(total, ns, env)
    if pre and wsb >= ns * total * 4 + pre:
        kernels.append("wgrad_prereduce_kernel")
        fns = env["SGX_WGRAD_PRE"]
    kernels.append(f"wgrad_finish_kernel<{finish_epb(O, Ip)}>")
    return Plan(0, tuple(kernels), ns, fns, L, gen)


# ---------------------------------------------------------------------------------------------------------------- the case table
# entry: the C ABI function; group: the environment it needs (GROUPS); args: B, H, W (the k side's size, as the ABI takes it), Ck, Cn, mode,
# adjoint, O, I, acc(umulate), bias (db given), data ("int" | "randn" | "abs"), ws ("query": exactly sgx_wgrad_ws_bytes; ("splits", k): room
# for k splits; ("pre", d): the splits plus the pre-reduction's output plus d bytes; "short": 4 bytes less than one split), ns: the pixel
# splits, fns: the ``ns`` of the finishing launch (None: direct epilogue), twin: the default row whose bits it must equal; kernels: every
# launch in order at 256 CUs; why: the launcher rule that selects them.
Case = namedtuple("Case", "id entry dtype group args kernels why")
CASES = []
S3, S4 = "sgx_wgrad3x3_param", "sgx_wgrad4x4s2_param"
PRE, W2S, W16 = "wgrad_prereduce_kernel", "wgrad2_s_kernel<8>", "wgrad16_s_kernel"


def g1(dt, geo, TH, TW, NS, KS, tr=None):
    tr = (dt == H) if tr is None else tr
    return f"wgrad_kernel<{tname(dt)}, {geo}, {TH}, {TW}, {128 if geo == 0 else 64}, {NS}, {KS}, {'true' if tr else 'false'}>"


def fin(epb):
    return f"wgrad_finish_kernel<{epb}>"


def w2d(kbw):
    return f"wgrad2_d_kernel<{kbw}>"


def _case(id, dt, kernels, why, B, Hh, W, Ck, Cn, ns, fns, mode="S", adjoint=0, I=None, acc=0, bias=True, data="int", ws="query", group="default", twin=None, rc=0):
    transposed = adjoint or mode in ("U", "UF")
    O, Ip = (Ck, Cn) if transposed else (Cn, Ck)
    args = dict(B=B, H=Hh, W=W, Ck=Ck, Cn=Cn, mode=mode, adjoint=adjoint, O=O, Ip=Ip, I=Ip if I is None else I, acc=acc, bias=bias and not transposed,
                data=data, ws=ws, ns=ns, fns=fns, twin=twin, rc=rc)
    CASES.append(Case(id, S3 if mode == "S" else S4, dt, group, args, tuple(kernels), why))


def dn(dt):
    return "f32" if dt == F else "bf16"


# ---- first generation, every reachable instantiation: tile x channel pair x dtype.  bf16 shapes are ones the second generation declines
# (Cn or Ck not a multiple of 64 / W not a multiple of 32 / 16x16 channels at W = 48).  Ragged on purpose: H, W, B no multiples of the tile.
CH3 = {(2, 2): (32, 32, 8), (2, 1): (48, 32, 8), (1, 2): (32, 48, 8), (1, 1): (16, 16, 4)}           # (NSUB, KSUB) -> (Ck, Cn, EPB of the finish)
TILES3 = {(8, 16): (3, 20, 24, 18), (8, 8): (3, 12, 8, 4), (4, 4): (5, 4, 4, None)}                    # tile -> B, H, W, nsplit (None: direct)
TILES4 = {(4, 16): (3, 36, 40, 30), (8, 8): (3, 24, 24, 12), (4, 4): (5, 8, 8, 2)}                   # tile -> B, fine H, fine W, nsplit
for dt in (F, H):
    for (NS, KS), (Ck, Cn, epb) in CH3.items():
        for (TH, TW), (B, Hh, W, ns) in TILES3.items():
            if (TH, TW) == (8, 16) and (Ck, Cn) == (16, 16):
                W = 48                                                                               # (bf16: wgrad16_s_kernel wants W % 32 == 0)
                ns = 3 * 3 * 3
            k = [g1(dt, 0, TH, TW, NS, KS)] + ([] if ns is None else [fin(epb)])
            for data in ("int", "randn", "abs") if (TH, TW) == (8, 16) else ("int",):
                _case(f"g1-3x3-{TH}x{TW}-n{NS}k{KS}-{data}-{dn(dt)}", dt, k, f"Cn {Cn} Ck {Ck} -> sub-tiles ({NS}, {KS}); {Hh}x{W} -> tile {TH}x{TW}; B {B}: ragged in every dimension",
                      B, Hh, W, Ck, Cn, ns or 1, ns, data=data)
    for (NS, KS), (Ck, Cn) in {(2, 1): (32, 32), (1, 1): (32, 48)}.items():
        for (TH, TW), (B, Hh, W, ns) in TILES4.items():
            for data in ("int", "randn", "abs") if (TH, TW) == (4, 16) else ("int",):
                _case(f"g1-4x4-{TH}x{TW}-n{NS}k{KS}-{data}-{dn(dt)}", dt, [g1(dt, 1, TH, TW, NS, KS), fin(8)],
                      f"stride 2 keeps the k side at 16 channels; Cn {Cn} -> NSUB {NS}; coarse {Hh // 2}x{W // 2} -> tile {TH}x{TW}", B, Hh, W, Ck, Cn, ns, ns, mode="D", data=data)

# ---- direct epilogue: one pixel split, no finishing launch
for dt in (F, H):
    _case(f"direct-one-tile-{dn(dt)}", dt, [g1(dt, 0, 8, 8, 2, 2)], "B2 8x8 is one 8x8 tile of two images: nsplit 1", 2, 8, 8, 32, 32, 1, None)
    _case(f"direct-lowres-big-B1-4x4-{dn(dt)}", dt, [g1(dt, 0, 4, 4, 2, 1)], "512x512 channels, 16 pixels: lowres_big takes (2, 1) = 512 pairs, one tile", 1, 4, 4, 512, 512, 1, None)
    _case(f"direct-lowres-big-B4-8x8-{dn(dt)}", dt, [g1(dt, 0, 8, 8, 2, 1)], "lowres_big; 2 tiles, pairs >= 512 and ntiles <= 64: one split", 4, 8, 8, 512, 512, 1, None, data="abs" if dt == H else "int")
    _case(f"direct-lowres-big-B4-16x16-{dn(dt)}", dt, [g1(dt, 0, 8, 16, 2, 1)], "1024 pixels <= 64 * BP: still lowres_big, 8 tiles, one split (W = 16: the second generation declines)", 4, 16, 16, 512, 512, 1, None)
    _case(f"lowres-480-{dn(dt)}", dt, [g1(dt, 0, 4, 4, 2, 2)], "480x480 channels: 15 * 30 < 512 pairs with (2, 1), so not lowres_big: (2, 2), one tile, direct", 1, 4, 4, 480, 480, 1, None)
_case("lowres-npix-other-side-bf16", H, [g1(H, 0, 8, 16, 2, 2), fin(64)], "8448 pixels > 64 * BP: (2, 2) = 256 pairs, 2 splits (W = 88: the second generation declines)", 1, 96, 88, 512, 512, 2, 2)
_case("direct-528-from-513-f32", F, [g1(F, 0, 4, 4, 2, 1)], "the discriminator's last conv: Ck 528 padded from I = 513: (2, 1), 528 pairs, direct, rows i >= 513 not written", 4, 4, 4, 528, 512, 1, None, I=513)
_case("direct-528-from-513-bf16", H, [g1(H, 0, 4, 4, 2, 1)], "as above in bf16 (Ck % 64 != 0: first generation)", 4, 4, 4, 528, 512, 1, None, I=513)

# ---- modes and flags, each on the direct path (B2 8x8 / fine 16x16 B1) and the finish path (B2 16x16 / fine 24x40 B3)
for dt in (F, H):
    for path, (B3_, H3, W3, ns3, B4_, H4, W4, ns4) in {"direct": (2, 8, 8, None, 1, 16, 16, None), "finish": (2, 16, 16, 4, 3, 24, 40, 18)}.items():
        k3 = [g1(dt, 0, 8, 8 if path == "direct" else 16, 2, 2)] + ([fin(8)] if ns3 else [])
        k4 = [g1(dt, 1, 8, 8, 2, 1)] + ([fin(8)] if ns4 else [])
        why3, why4 = f"32x32 channels, B{B3_} {H3}x{W3}: {path}", f"32x32 channels, B{B4_} fine {H4}x{W4}: {path}"
        for acc in (0, 1, 2, 3):
            _case(f"S-acc{acc}-{path}-{dn(dt)}", dt, k3, why3 + f"; accumulate {acc} on prefilled dW, db", B3_, H3, W3, 32, 32, ns3 or 1, ns3, acc=acc)
            _case(f"D-acc{acc}-{path}-{dn(dt)}", dt, k4, why4 + f"; mode D with bias, accumulate {acc}", B4_, H4, W4, 32, 32, ns4 or 1, ns4, mode="D", acc=acc)
        _case(f"S-adjoint-{path}-{dn(dt)}", dt, k3, why3 + "; adjoint: flip_t and (o, i) = (k, n)", B3_, H3, W3, 32, 32, ns3 or 1, ns3, adjoint=1, acc=1)
        _case(f"S-nodb-{path}-{dn(dt)}", dt, k3, why3 + "; db = NULL", B3_, H3, W3, 32, 32, ns3 or 1, ns3, bias=False)
        _case(f"S-I17-{path}-{dn(dt)}", dt, k3, why3 + "; I = 17 < Ip = 32", B3_, H3, W3, 32, 32, ns3 or 1, ns3, I=17)
        _case(f"S-adjoint-I17-{path}-{dn(dt)}", dt, k3, why3 + "; adjoint with I = 17 < Ip = 32 (the padded axis is the n side)", B3_, H3, W3, 32, 32, ns3 or 1, ns3, adjoint=1, I=17)
        _case(f"D-nodb-{path}-{dn(dt)}", dt, k4, why4 + "; db = NULL", B4_, H4, W4, 32, 32, ns4 or 1, ns4, mode="D", bias=False, data="randn")
        for m in ("U", "UF"):
            _case(f"{m}-{path}-{dn(dt)}", dt, k4, why4 + f"; mode {m}: (o, i) = (k, n)" + (", the 3x3 result flipped" if m == "UF" else ""), B4_, H4, W4, 32, 32, ns4 or 1, ns4, mode=m, acc=1)

# ---- the finishing kernel: O * Ip on both sides of 8192, 2048, 1024; nsplit below and above 256 / EPB; bias blocks with O % EPB != 0
for (Ck, Cn, epb, NS, KS) in ((64, 128, 64, 2, 2), (64, 112, 16, 1, 2), (32, 64, 16, 2, 2), (32, 48, 8, 1, 2), (32, 32, 8, 2, 2), (16, 48, 4, 1, 1)):
    nsl = 256 // epb
    for (B, Hh, W) in ((1, 16, 16), (2, 32, 32) if epb == 64 else (6, 48, 32) if epb == 4 else (3, 48, 32)):
        TH, TW, bp = wgrad_tile(0, Hh, W)
        nt = B * cdiv(Hh, TH) * cdiv(W, TW)
        ns = wgrad_nsplit((Cn // (16 * NS)) * (Ck // (16 * KS)), nt, 9 * Cn * Ck, ENV0)
        assert ns != nsl
        _case(f"finish-epb{epb}-{Cn}x{Ck}-ns{ns}-f32", F, [g1(F, 0, 8, 16, NS, KS), fin(epb)], f"O * Ip = {Cn * Ck}: EPB {epb}; {ns} splits {'<' if ns < nsl else '>'} {nsl} split lanes", B, Hh, W, Ck, Cn, ns, ns)
_case("finish-epb64-O48-f32", F, [g1(F, 0, 8, 16, 1, 1), fin(64)], "O = 48, Ip = 176: EPB 64 with a partial trailing bias block", 2, 16, 16, 176, 48, 4, 4, acc=2)
_case("finish-epb64-O48-abs-f32", F, [g1(F, 0, 8, 16, 1, 1), fin(64)], "as above on |randn| data", 2, 16, 16, 176, 48, 4, 4, data="abs")

# ---- the workspace
for dt in (F, H):
    _case(f"ws-room-for-3-{dn(dt)}", dt, [g1(dt, 0, 8, 16, 2, 2), fin(8)], "32x32 channels B4 16x16 wants 8 splits; the workspace holds 3: ns = 3", 4, 16, 16, 32, 32, 3, 3, ws=("splits", 3))
    _case(f"ws-room-for-1-{dn(dt)}", dt, [g1(dt, 0, 8, 16, 2, 2)], "the workspace holds one split: the direct epilogue", 4, 16, 16, 32, 32, 1, None, ws=("splits", 1), twin=f"ws-room-for-3-{dn(dt)}")
    _case(f"ws-short-{dn(dt)}", dt, [], "4 bytes less than one split: SGX_EWORKSPACE before any launch", 4, 16, 16, 32, 32, 0, None, ws="short", rc=EWORKSPACE)
_case("ws-gen2-declines-3-bf16", H, [g1(H, 0, 8, 16, 2, 2), fin(16)], "64x64 channels B4 32x32: the second generation plans 8 splits, the workspace holds 3: the first generation runs with 3",
      4, 32, 32, 64, 64, 3, 3, ws=("splits", 3), twin="w2s-bias-int-bf16")
_case("ws-gen2-declines-1-bf16", H, [g1(H, 0, 8, 16, 2, 2)], "... holds 1: the first generation's direct epilogue", 4, 32, 32, 64, 64, 1, None, ws=("splits", 1), twin="w2s-bias-int-bf16")

# ---- the pre-reduction at the default thresholds (>= 256 splits into 32 groups)
for data in ("int", "randn", "abs"):
    _case(f"pre-f32-{data}", F, [g1(F, 0, 8, 16, 1, 1), PRE, fin(4)], "16x16 channels B2 128x128: 256 tiles, 256 splits", 2, 128, 128, 16, 16, 256, 32, data=data)
    _case(f"pre-w16-{data}-bf16", H, [W16, PRE, fin(4)], "16x16 channels B2 256x512: 512 tiles of 16x32, ns = 256 from 128 CUs up", 2, 256, 512, 16, 16, 256, 32, data=data)
_case("pre-f32-tight", F, [g1(F, 0, 8, 16, 1, 1), PRE, fin(4)], "the workspace ends with the pre-reduction's output", 2, 128, 128, 16, 16, 256, 32, ws=("pre", 0), twin="pre-f32-int")
_case("pre-f32-4-bytes-short", F, [g1(F, 0, 8, 16, 1, 1), fin(4)], "4 bytes less: no pre-reduction, the finishing kernel reads 256 splits", 2, 128, 128, 16, 16, 256, 256, ws=("pre", -4), twin="pre-f32-int")
_case("pre-w16-tight-bf16", H, [W16, PRE, fin(4)], "the workspace ends with the pre-reduction's output", 2, 256, 512, 16, 16, 256, 32, ws=("pre", 0), twin="pre-w16-int-bf16")

# ---- second generation
for data in ("int", "randn", "abs"):
    _case(f"w2s-bias-{data}-bf16", H, [W2S, fin(16)], "64x64 channels B4 32x32: 16 tiles of 8x32 < 2 ns: 8 splits", 4, 32, 32, 64, 64, 8, 8, data=data)
    _case(f"w2d2-D-{data}-bf16", H, [w2d(2), fin(16)], "64x64 channels B4 coarse 16x16: 16 tiles of 4x16, 8 splits, mode D with bias", 4, 32, 32, 64, 64, 8, 8, mode="D", data=data, acc=3 if data == "int" else 0)
    _case(f"w2d1-D-{data}-bf16", H, [w2d(1), fin(16)], "fine 32 channels: KBW 1", 4, 32, 32, 32, 64, 8, 8, mode="D", data=data)
    _case(f"w16-H40-{data}-bf16", H, [W16, fin(4)], "16x16 channels B3 40x64: ragged last tile row, 18 tiles in 8 bands, 8 splits", 3, 40, 64, 16, 16, 8, 8, data=data)
_case("w2s-nodb-bf16", H, [W2S, fin(16)], "db = NULL", 4, 32, 32, 64, 64, 8, 8, bias=False, acc=1)
_case("w2s-I33-bf16", H, [W2S, fin(16)], "I = 33 < Ip = 64 through wgrad_finish", 4, 32, 32, 64, 64, 8, 8, I=33)
_case("w2s-adjoint-I33-bf16", H, [W2S, fin(16)], "adjoint with I = 33 < Ip = 64", 4, 32, 32, 64, 64, 8, 8, adjoint=1, I=33)
_case("w2d2-U-bf16", H, [w2d(2), fin(16)], "mode U through the second generation", 4, 32, 32, 64, 64, 8, 8, mode="U")
_case("w2d2-UF-bf16", H, [w2d(2), fin(16)], "mode UF through the second generation", 4, 32, 32, 64, 64, 8, 8, mode="UF", acc=1)
_case("w2s-ncu-bf16", H, [W2S, fin(64)], "256x512 channels = 32 channel tiles: ns = ncu / 32 = 8 from the CU count, 16 tiles >= 2 ns", 4, 32, 32, 256, 512, 8, 8)
_case("w2s-ncu-nct4-bf16", H, [W2S, fin(64)], "128x128 channels = 4 channel tiles, B9 64x64 = 144 tiles: ns = ncu / 4 to a multiple of 8 = 64 at 256 CUs (72 at 304)", 9, 64, 64, 128, 128, 64, 64)
_case("w2s-too-few-tiles-bf16", H, [g1(H, 0, 8, 16, 2, 2), fin(16)], "64x64 channels B3 32x32: 12 tiles -> ns 0: the first generation", 3, 32, 32, 64, 64, 24, 24)
_case("w2s-nct40-64-tiles-bf16", H, [W2S, fin(64)], "320x512 channels = 40 channel tiles > 32: B16 32x32 = 64 tiles >= 8 ns", 16, 32, 32, 320, 512, 8, 8)
_case("w2s-nct40-60-tiles-bf16", H, [g1(H, 0, 8, 16, 2, 2), fin(64)], "... B15 32x32 = 60 tiles < 8 ns: the first generation", 15, 32, 32, 320, 512, 4, 4)

# ---- switched rows: one child process per group; an integer row gives the bits of its default twin
for g, sw in (("w2_0", 0), ("w2_3", 3), ("w2_5", 5), ("w2_6", 6)):
    s_on, d_on, s16_on = sw & 1, sw & 2, (sw & 1) and (sw & 4)
    _case(f"{g}-S", H, [W2S, fin(16)] if s_on else [g1(H, 0, 8, 16, 2, 2), fin(16)], f"SGX_WGRAD2={sw}: bit 0 {'on' if s_on else 'off'}", 4, 32, 32, 64, 64, 8 if s_on else 32, 8 if s_on else 32, group=g, twin="w2s-bias-int-bf16")
    _case(f"{g}-D", H, [w2d(2), fin(16)] if d_on else [g1(H, 1, 4, 16, 2, 1), fin(16)], f"SGX_WGRAD2={sw}: bit 1 {'on' if d_on else 'off'}", 4, 32, 32, 64, 64, 8 if d_on else 16, 8 if d_on else 16, mode="D", acc=3, group=g, twin="w2d2-D-int-bf16")
    _case(f"{g}-16", H, [W16, fin(4)] if s16_on else [g1(H, 0, 8, 16, 1, 1), fin(4)], f"SGX_WGRAD2={sw}: bits 0 and 2 {'on' if s16_on else 'not both on'}", 3, 40, 64, 16, 16, 8 if s16_on else 60, 8 if s16_on else 60, group=g, twin="w16-H40-int-bf16")
for c in [c for c in CASES if c.group == "default" and c.dtype == H and c.id.startswith("g1-") and c.args["data"] == "int"]:
    a = c.args
    _case("tr0-" + c.id, H, [c.kernels[0].replace("true>", "false>")] + list(c.kernels[1:]), "SGX_WGRAD_TR=0: the plain bf16 operand path; " + c.why, a["B"], a["H"], a["W"], a["Ck"], a["Cn"], a["ns"], a["fns"],
          mode=a["mode"], group="tr0", twin=c.id)
_case("tr0-direct-one-tile", H, [g1(H, 0, 8, 8, 2, 2, False)], "SGX_WGRAD_TR=0 with the direct epilogue", 2, 8, 8, 32, 32, 1, None, group="tr0", twin="direct-one-tile-bf16")
_case("pre0-f32", F, [g1(F, 0, 8, 16, 1, 1), fin(4)], "SGX_WGRAD_PRE=0: the finishing kernel reads 256 splits", 2, 128, 128, 16, 16, 256, 256, group="pre0", twin="pre-f32-int")
_case("pre0-w16-bf16", H, [W16, fin(4)], "SGX_WGRAD_PRE=0: the finishing kernel reads 256 splits", 2, 256, 512, 16, 16, 256, 256, group="pre0", twin="pre-w16-int-bf16")
_case("fin-ns9-f32", F, [g1(F, 0, 8, 16, 1, 1), fin(4)], "16x16 channels B1 24x48: 9 tiles, 9 splits (the default twin of pre4-ns9)", 1, 24, 48, 16, 16, 9, 9)
_case("fin-ns10-f32", F, [g1(F, 0, 8, 16, 1, 1), fin(4)], "16x16 channels B1 16x80: 10 tiles, 10 splits (the default twin of pre4-ns10)", 1, 16, 80, 16, 16, 10, 10)
_case("pre4-ns9", F, [g1(F, 0, 8, 16, 1, 1), PRE, fin(4)], "4 groups, from 8 splits up: 9 splits = 3 + 3 + 3 + 0, an empty last group", 1, 24, 48, 16, 16, 9, 4, group="pre4", twin="fin-ns9-f32")
_case("pre4-ns10", F, [g1(F, 0, 8, 16, 1, 1), PRE, fin(4)], "10 splits = 3 + 3 + 3 + 1, an uneven last group", 1, 16, 80, 16, 16, 10, 4, group="pre4", twin="fin-ns10-f32")
_case("pre4-ns9-abs", F, [g1(F, 0, 8, 16, 1, 1), PRE, fin(4)], "as pre4-ns9 on |randn| data", 1, 24, 48, 16, 16, 9, 4, group="pre4", data="abs")
_case("pre4-ns4", F, [g1(F, 0, 8, 16, 2, 2), fin(8)], "4 splits < SGX_WGRAD_PRE_MIN: no pre-reduction", 2, 16, 16, 32, 32, 4, 4, group="pre4", twin="S-acc0-finish-f32")
for dt in (F, H):
    _case(f"maxsplit3-{dn(dt)}", dt, [g1(dt, 0, 8, 16, 2, 2), fin(8)], "SGX_WGRAD_MAXSPLIT=3 caps 8 wanted splits", 4, 16, 16, 32, 32, 3, 3, group="maxsplit3", twin=f"ws-room-for-3-{dn(dt)}")
_case("maxsplit3-w2s-bf16", H, [W2S, fin(16)], "the cap does not reach the second generation's plan", 4, 32, 32, 64, 64, 8, 8, group="maxsplit3", twin="w2s-bias-int-bf16")
_case("blocks-epb64-ns32-f32", F, [g1(F, 0, 8, 16, 2, 2), fin(64)], "SGX_WGRAD_BLOCKS=4096: 256x256 channels, 64 pairs want 64 splits, 32 tiles: 32 > 4 split lanes at EPB 64", 4, 32, 32, 256, 256, 32, 32, group="blocks", twin="fin-256x256-ns8-f32")
_case("fin-256x256-ns8-f32", F, [g1(F, 0, 8, 16, 2, 2), fin(64)], "256x256 channels B4 32x32: 64 pairs want 8 splits (the default twin of blocks-epb64-ns32)", 4, 32, 32, 256, 256, 8, 8)
_case("blocks-lowres-big-f32", F, [g1(F, 0, 8, 8, 2, 1), fin(64)], "with a block target the one-split rule is off: 2 tiles, 2 splits, finish", 4, 8, 8, 512, 512, 2, 2, group="blocks", twin="direct-lowres-big-B4-8x8-f32")
_case("maxct1-nct2-bf16", H, [g1(H, 0, 8, 16, 2, 2), fin(64)], "SGX_WGRAD2_MAXCT=1: 64x128 channels = 2 channel tiles > 1 and 16 tiles < 8 ns: the first generation", 4, 32, 32, 64, 128, 32, 32, group="maxct1", twin="w2s-nct2-bf16")
_case("maxct1-nct4-bf16", H, [g1(H, 0, 8, 16, 2, 2), fin(64)], "128x128 channels = 4 channel tiles > 2 * 1: declined outright", 4, 32, 32, 128, 128, 32, 32, group="maxct1", twin="w2s-nct4-bf16")
_case("w2s-nct4-bf16", H, [W2S, fin(64)], "128x128 channels = 4 channel tiles, 16 tiles: 8 splits (the default twin of maxct1-nct4)", 4, 32, 32, 128, 128, 8, 8)
_case("maxct1-nct1-bf16", H, [W2S, fin(16)], "one channel tile: still the second generation", 4, 32, 32, 64, 64, 8, 8, group="maxct1", twin="w2s-bias-int-bf16")
_case("w2s-nct2-bf16", H, [W2S, fin(64)], "64x128 channels = 2 channel tiles, 16 tiles: 8 splits (the default twin of maxct1-nct2)", 4, 32, 32, 64, 128, 8, 8)

NS_AT_304 = {"w2s-ncu-nct4-bf16": 72}          # rows whose split count follows the CU count: what 304 CUs give
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), [c.id for c in CASES if sum(1 for d in CASES if d.id == c.id) > 1]

# Launch sites no row claims, by the text of the site, with the reason; and switches no row sets
EXCLUDED_SITES = {}
EXCLUDED_PATHS = {"SGX_WGRAD_BLOCKS_MID": "an experiment's block target for the mid layers: the same arithmetic as SGX_WGRAD_BLOCKS, whose rows run in the group `blocks`"}


def c_of(a):
    return 0.5 * (0.25 if a["mode"] == "D" else 1.0)


def scale_of(c):
    """Integer rows: a power of two (every scaled sum stays exact); rounding rows: an equalized-lr multiplier, as fp32."""
    return 0.5 if c.args["data"] == "int" else float(torch.tensor(math.sqrt(2.0 / (9 * c.args["Ip"])), dtype=torch.float32))


PREFILL = 50                        # |prefilled dW, db| <= 50, integers


def exact_ok(c):
    """The integer rows' condition: (36 B Hn Wn + |prefill| / c) < 2^24 -- the unscaled sum plus the prefill in units of c is an integer below
    2^24 (c = scale x 0.25 for mode D, a power of two <= 1: no weaker than 36 B Hn Wn + |prefill| < 2^24)."""
    a = c.args
    npix = a["B"] * a["H"] * a["W"] // (1 if a["mode"] == "S" else 4)
    return 36 * npix + PREFILL / c_of(a) < 2 ** 24 and 36 * npix + PREFILL < 2 ** 24


def row_plan(c, ncu, wsb=None):
    a = c.args
    env = group_env(c.group)
    return plan(c.entry, c.dtype, a["B"], a["H"], a["W"], a["Ck"], a["Cn"], a["O"], a["Ip"], row_ws(c, ncu) if wsb is None else wsb, env, ncu)


def row_ws(c, ncu):
    """The workspace size the row passes, from the restated rules (the runner takes "query" from the library itself)."""
    a, env = c.args, group_env(c.group)
    taps = 9 if a["mode"] == "S" else 16
    total = taps * a["Ck"] * a["Cn"] + a["Cn"]
    q = ws_bytes(taps, a["B"], a["H"], a["W"], a["Ck"], a["Cn"], env, ncu)
    w = a["ws"]
    if w == "query":
        return q
    if w == "short":
        return total * 4 - 4
    if w[0] == "splits":
        return w[1] * total * 4
    p = plan(c.entry, c.dtype, a["B"], a["H"], a["W"], a["Ck"], a["Cn"], a["O"], a["Ip"], q, env, ncu)
    return p.nsplit * total * 4 + pre_bytes(total, p.nsplit, env) + w[1]
