"""fp64 restatements of the generator layer epilogue (csrc/gepi.hip: sgx_gepi_fwd, sgx_gepi_bwd, sgx_gepi_stats, sgx_blur3x3_stats) and of
the multi-tensor optimizer kernels (csrc/optim.hip), written from their definitions in include/sgx.h, the criterion they are held to, the
launcher rules restated, and the table of cases that walks every launch path.  Test-side only: nothing here imports or calls the library.

The instance norm makes one per-element bound on y useless (the statistics' error is amplified by rstd), so the criterion is decoupled:
  statistics  mean / rstd against fp64 with a bound from the accumulation: fp32 per lane over L values, fp64 beyond (stats_bounds);
  apply pass  y per element against the fp64 expression evaluated on the kernel's OWN returned mean / rstd (streaming_ref.assert_elementwise);
  backward    dstyle / dnw / dbias are the reductions themselves (chain-length bound on the sum of |terms|); dx per element, with the error of
              the two statistics-gradient coefficients folded into S through the same sums.
Layouts: x, y, dy, dx [B][HW][C]; noise [B][HW]; bias, nw [C]; style [B][2C]; mean, rstd [B][C]."""
import math
from collections import namedtuple

import numpy as np
import torch

from streaming_ref import LRELU, U32, _blur121, act, tname

EPS = float(np.float32(1e-5))       # GEPI_EPS as the kernels hold it
EPI_ACT, EPI_NORM = 1, 2
F, H = torch.float32, torch.bfloat16
N_FWD = 9                           # fp32 chain of y: nw*noise, two sums, the slope, - mean, * rstd, style + 1, the product, + shift
N_DX_LOCAL = 11                     # of dx: xh (6: p 3, slope, - mean, * rstd), xh * k2, two differences, * rstd, the slope
KINK = 4                            # |p| <= KINK 2^-24 S_p: the fp32 pre-activation may fall on the other side of zero


def _ve(dt):
    return 4 if dt == F else 8


# ---------------------------------------------------------------------------------------------------------------- references
def pre_activation(x, bias, noise, nw):
    """p = x + bias[c] + nw[c] noise[b][hw] and the same on absolute values."""
    t = nw * noise.unsqueeze(-1)
    p, Sp = x + t, x.abs() + t.abs()
    if bias is not None:
        p, Sp = p + bias, Sp + bias.abs()
    return p, Sp


def stats_bounds(Sp, mean, rstd, L):
    """|d mean| <= (L+4) u A, |d var| <= (L+4) u A2 + 2 |mean| |d mean|, |d rstd| <= rstd^3 |d var| / 2 + 2 u rstd, with A = mean(S_p), A2 =
    mean(S_p^2): a lane's fp32 chain of L sums behind the 4 roundings of a = act(p) (everything after the lane is fp64, the results are
    rounded to fp32 once)."""
    A, A2 = Sp.mean(1), (Sp * Sp).mean(1)
    dmean = (L + 4) * U32 * A
    dvar = (L + 4) * U32 * A2 + 2.0 * mean.abs() * dmean
    return dmean, 0.5 * rstd ** 3 * dvar + 2.0 * U32 * rstd


def gepi_stats(x, bias, noise, nw, flags, L):
    """sgx_gepi_stats / the statistics half of sgx_gepi_fwd: mean and rstd = 1 / sqrt(var + eps) (biased variance) of a = act(p) per (image,
    channel).  -> ((mean, rstd), (bound of mean, bound of rstd)); norm off: 0 / 1 exactly."""
    B, HW, C = x.shape
    if not flags & EPI_NORM:
        z = torch.zeros(B, C, dtype=x.dtype, device=x.device)
        return (z, z + 1.0), (z, z.clone())
    p, Sp = pre_activation(x, bias, noise, nw)
    a = act(p, 1 if flags & EPI_ACT else 0)
    mean = a.mean(1)
    var = ((a - mean.unsqueeze(1)) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (mean, rstd), stats_bounds(Sp, mean, rstd, L)


def gepi_fwd(x, bias, noise, nw, style, mean, rstd, flags):
    """The apply pass of sgx_gepi_fwd on GIVEN mean / rstd: y = (act(p) - mean) rstd (style[:, :C] + 1) + style[:, C:].  -> (y, S); N_FWD."""
    C = x.shape[2]
    p, Sp = pre_activation(x, bias, noise, nw)
    a = act(p, 1 if flags & EPI_ACT else 0)
    m, r = mean.unsqueeze(1), rstd.unsqueeze(1)
    s0, s1 = style[:, :C].unsqueeze(1), style[:, C:].unsqueeze(1)
    return (a - m) * r * (s0 + 1.0) + s1, (Sp + m.abs()) * r.abs() * (s0.abs() + 1.0) + s1.abs()


Bwd = namedtuple("Bwd", "dx dx_alt kink S_dx n_dx dstyle S_dstyle n_dstyle dnw S_dnw n_dnw dbias S_dbias n_dbias")


def gepi_bwd(dy, x, bias, noise, nw, style, mean, rstd, flags, L1, L2):
    """sgx_gepi_bwd on given mean / rstd.  L1: fp32 chain of the reduction pass (sum dy, sum dy xh), L2: of the apply pass's sums (d noise
    weight, d bias).  With xh = (act(p) - mean) rstd, sc = style[:, :C] + 1:
        dstyle = (sum dy xh, sum dy);  k1 = sc sum dy / HW, k2 = sc sum dy xh / HW (0 without the norm);
        dx = rstd (dy sc - k1 - xh k2) slope(p);  dnw = sum_{b,hw} dx noise;  dbias = sum_{b,hw} dx.
    The kernel's k1 / k2 come from its own sums: within (L1 + 3) u and (L1 + 8) u of the same expressions on absolute values, which are
    terms of S_dx, so they add L1 + 8 to dx's chain.  dx_alt / kink: the value under the other slope and where it is admissible."""
    B, HW, C = x.shape
    on, norm = bool(flags & EPI_ACT), bool(flags & EPI_NORM)
    p, Sp = pre_activation(x, bias, noise, nw)
    m, r = mean.unsqueeze(1), rstd.unsqueeze(1)
    xh, XH = (act(p, 1 if on else 0) - m) * r, (Sp + m.abs()) * r.abs()
    sdy, sdx, Sdy, Sdx = dy.sum(1), (dy * xh).sum(1), dy.abs().sum(1), (dy.abs() * XH).sum(1)
    sc, sca = style[:, :C] + 1.0, style[:, :C].abs() + 1.0
    da, Sda = dy * sc.unsqueeze(1), dy.abs() * sca.unsqueeze(1)
    if norm:
        da = da - (sc * sdy / HW).unsqueeze(1) - xh * (sc * sdx / HW).unsqueeze(1)
        Sda = Sda + (sca * Sdy / HW).unsqueeze(1) + XH * (sca * Sdx / HW).unsqueeze(1)
    da, Sda = r * da, r.abs() * Sda
    n_dx = N_DX_LOCAL + (L1 + 8 if norm else 0)
    nz = noise.unsqueeze(-1)
    if on:
        pos = p > 0
        dx, alt = da * torch.where(pos, 1.0, LRELU), da * torch.where(pos, LRELU, 1.0)
        kink = p.abs() <= KINK * U32 * Sp
        Sda = Sda * torch.where(pos | kink, 1.0, LRELU)      # the scale of dx carries the slope (either one at a kink)
        # a kink element that takes the other slope moves the two channel sums by (1 - slope) |da| (|noise|): granted as absolute slack
        slack = (1.0 - LRELU) * da.abs() * kink
        slack_nw, slack_b = (slack * nz.abs()).sum((0, 1)), slack.sum((0, 1))
    else:
        dx, alt, kink, slack_nw, slack_b = da, None, None, 0.0, 0.0
    # the sums add the kernel's fp32 dx (each within (n_dx + 2) u S_dx) along a lane's chain of L2, the product with the noise first
    n_nw, n_b = n_dx + 2 + 1 + L2, n_dx + 2 + L2
    return Bwd(dx, alt, kink, Sda, n_dx, torch.cat([sdx, sdy], 1), torch.cat([Sdx, Sdy], 1), L1 + 7,
               (dx * nz).sum((0, 1)), (Sda * nz.abs()).sum((0, 1)) + slack_nw / ((n_nw + 2) * U32), n_nw,
               dx.sum((0, 1)), Sda.sum((0, 1)) + slack_b / ((n_b + 2) * U32), n_b)


def blur3x3_stats(x, bias, noise, nw, on):
    """sgx_blur3x3_stats: y = blur3x3(x) ([B][H][W][C]; 9 terms) -> (y, S)."""
    return _blur121(x), _blur121(x.abs())


def activation_sums(y, bias, noise, nw, on):
    """... and its partials summed per (image, channel): (sum a, sum a^2) of a = act(y + bias + nw noise) over the STORED y ([B][HW][C]), with the
    same on absolute values.  A lane's chain of L: a within 4 u, a^2 within 9 u -> chains L + 4 and L + 9."""
    p, Sp = pre_activation(y, bias, noise, nw)
    a = act(p, 1 if on else 0)
    return torch.stack([a.sum(1), (a * a).sum(1)], -1), torch.stack([Sp.sum(1), (Sp * Sp).sum(1)], -1)


def partials(x, bias, noise, nw, flags, npart):
    """The producer's partials built in fp64: pixels split into npart contiguous ranges of unequal length -> double [B][npart][C][2]."""
    B, HW, C = x.shape
    p, _ = pre_activation(x, bias, noise, nw)
    a = act(p, 1 if flags & EPI_ACT else 0)
    cuts = [0] + sorted({max(1, min(HW - 1, (k * HW) // npart + (k % 3) - 1)) for k in range(1, npart)}) + [HW] if npart > 1 else [0, HW]
    while len(cuts) < npart + 1:                             # (ranges that collapsed: empty partials at the end)
        cuts.append(HW)
    out = torch.zeros(B, npart, C, 2, dtype=torch.float64, device=x.device)
    for k in range(npart):
        s = a[:, cuts[k]:cuts[k + 1]]
        out[:, k, :, 0], out[:, k, :, 1] = s.sum(1), (s * s).sum(1)
    return out


def assert_within(got, ref, bound, what=""):
    """Every element: |got - ref| <= bound, NaN failing (as streaming_ref.assert_elementwise) -> the worst err / bound."""
    g = got.detach().to(torch.float64)
    assert tuple(g.shape) == tuple(ref.shape) == tuple(bound.shape), (what, tuple(g.shape), tuple(ref.shape), tuple(bound.shape))
    err = (g - ref.to(g.device)).abs()
    ok = err <= bound.to(g.device)
    if not bool(ok.all()):
        bad = (~ok).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {g.numel()} values outside the bound; first at {tuple(int(v) for v in np.unravel_index(i, tuple(g.shape)))}: "
                             f"got {float(g.flatten()[i])!r}, ref {float(ref.flatten()[i])!r}, err {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e}")
    z = bound <= 0
    return float((err / bound.clamp_min(1e-300))[~z].max()) if bool((~z).any()) else 0.0


def choose_slope(got, b):
    """dx's reference with the LeakyReLU kink resolved: where |p| <= KINK u S_p the kernel's fp32 p may have the other sign, so the value under
    either slope is admissible -- the nearer one is taken.  No other element is touched.  -> (reference, number of kink elements)."""
    if b.kink is None:
        return b.dx, 0
    g = got.detach().to(torch.float64)
    take = b.kink & ((g - b.dx_alt).abs() < (g - b.dx).abs())
    return torch.where(take, b.dx_alt, b.dx), int(b.kink.sum())


def kink_cap(n):
    return max(2, int(1e-5 * n))


# ---------------------------------------------------------------------------------------------------------------- launcher rules
# csrc/gepi.hip restated: which kernels a call launches, and the fp32 chain lengths that follow from the geometry.
Geom = namedtuple("Geom", "cvt rows rpt chunk nchunk")
ENV_DEFAULT = dict(apply1=1, bwd2s=1, fold=1, nt_mb=192.0, small=1, rpt=64)
GROUPS = {                                                   # the process-wide switches of a group: read once per process
    "default": {},
    "switch": {"SGX_GEPI_APPLY1": "2", "SGX_GEPI_BWD2S": "2"},
    "switch_nt": {"SGX_GEPI_APPLY1": "2", "SGX_GEPI_BWD2S": "2", "SGX_NT_MIN_MB": "0.001"},
    "nofold": {"SGX_GEPI_FOLD": "0"},
}


def group_env(group):
    e, g = dict(ENV_DEFAULT), GROUPS[group]
    e.update(apply1=int(g.get("SGX_GEPI_APPLY1", 1)), bwd2s=int(g.get("SGX_GEPI_BWD2S", 1)), fold=int(g.get("SGX_GEPI_FOLD", 1)),
             nt_mb=float(g.get("SGX_NT_MIN_MB", 192.0)), small=int(g.get("SGX_GEPI_SMALL", 1)), rpt=int(g.get("SGX_GEPI_RPT", 64)))
    return e


def gepi_geom(B, HW, C, ve, rpt=64):
    """rpt: SGX_GEPI_RPT, the most pixel rows per thread (<= 0: 64)."""
    cv = C // ve
    cvt = min(cv, 256)
    rows = 256 // cvt
    rpt = rpt if rpt > 0 else 64
    while rpt > 8 and B * ((HW + rows * rpt - 1) // (rows * rpt)) < 512:
        rpt >>= 1
    return Geom(cvt, rows, rpt, rows * rpt, (HW + rows * rpt - 1) // (rows * rpt))


def gs_plan(dt, HW):
    """GsPlan: (MAX_HW, variant): 256 threads x 2 pixels per lane up to 2 (256 / NV) pixels, 512 x 4 above."""
    nv = 16 // _ve(dt)
    return 4 * (512 // nv), (0 if HW <= 2 * (256 // nv) else 1)


def gepi_small_ok(B, HW, C, dt, small=1):
    mx, _ = gs_plan(dt, HW)
    nbytes = B * HW * C * (4 if dt == F else 2)
    return small != 0 and C % 16 == 0 and B * (C // 16) >= 64 and (HW <= mx // 4 or (HW <= mx and nbytes <= (8 << 20)))


def _small(kind, dt, HW):
    return f"gepi_small_{kind}<{tname(dt)}, 256, 2>" if gs_plan(dt, HW)[1] == 0 else f"gepi_small_{kind}<{tname(dt)}, 512, 4>"


def fwd_kernels(B, HW, C, dt, flags, pre, env):
    t, nb, norm = tname(dt), (4 if dt == F else 2) * B * HW * C, bool(flags & EPI_NORM)
    apply1 = env["apply1"] != 0 and C <= 128 and (env["apply1"] == 2 or nb >= 192e6)
    tail = ["gepi_fin_stats", f"gepi_apply1<{t}>"] if apply1 else None
    if norm and pre:
        return tail or ["gepi_fin_stats", f"gepi_apply<{t}>"]
    if gepi_small_ok(B, HW, C, dt, env["small"]):
        return [_small("fwd", dt, HW)]
    k = [f"gepi_pass<{t}, 0, false>"] if norm else []
    if tail:
        return k + tail
    return k + ([f"gepi_apply<{t}>"] if env["fold"] else ["gepi_fin_stats", f"gepi_apply<{t}>"])


def bwd2s_route(B, HW, C, dt, rpt=64):
    """(blocks per image, rows left for gepi_fin_bwd2 after the pre-reduction or 0 when it reads the block partials itself)."""
    ve = _ve(dt)
    nblk = (HW * (C // ve) + 1023) // 1024
    K = B * nblk
    NB = min(K, 256)
    return nblk, (NB if NB <= B * gepi_geom(B, HW, C, ve, rpt).nchunk and 2 * C <= 256 else 0)


def bwd_kernels(B, HW, C, dt, env):
    t, ve, nb = tname(dt), _ve(dt), (4 if dt == F else 2) * B * HW * C
    if gepi_small_ok(B, HW, C, dt, env["small"]):
        return [_small("bwd", dt, HW), "gepi_fin_bwd2"]
    k, cv = [f"gepi_pass<{t}, 1, false>"], C // ve
    if env["bwd2s"] != 0 and C <= 128 and cv in (1, 2, 4, 8, 16) and (env["bwd2s"] == 2 or nb >= 800e6):
        return k + ["gepi_fin_bwd1", f"gepi_bwd2s<{t}>"] + (["gepi_rows_prereduce"] if bwd2s_route(B, HW, C, dt, env["rpt"])[1] else []) + ["gepi_fin_bwd2"]
    if env["fold"]:
        return k + [f"gepi_pass<{t}, 2, {'true' if nb >= env['nt_mb'] * 1e6 else 'false'}>", "gepi_fin_bwd2"]
    return k + ["gepi_fin_bwd1", f"gepi_pass<{t}, 2, false>", "gepi_fin_bwd2"]


def stats_kernels(B, HW, C, dt, flags, pre):
    return ([f"gepi_pass<{tname(dt)}, 0, false>"] if flags & EPI_NORM and not pre else []) + ["gepi_fin_stats"]


def blur_stats_geom(B, Hh, W, C, ve):
    """-> (rt: output rows per strip = the fp32 chain of a lane, npart)."""
    cols = 256 // min(C // ve, 256)
    wch = (W + cols - 1) // cols
    rt = 64
    while rt > 8 and B * ((Hh + rt - 1) // rt) * wch < 1024:
        rt >>= 1
    return rt, ((Hh + rt - 1) // rt) * wch


def conv_stats_chain(Hh, W, C, npart):
    """sgx_conv3x3_stats keeps a lane's fp32 sums across the tiles its slot of the persistent grid stores for an image: C / 8 pixels per tile
    (2 nw x 32 pixels x C / 8 vectors over nw x 64 lanes), at most ceil(tiles / slots) + 1 tiles, tiles counted at the smaller tile height 8;
    the lanes of a wave with the same channel vector are then added in fp32 too (log2(64 / (C / 8)) exchange steps, C <= 64 per block), the
    waves in fp64."""
    tiles, vpr = ((Hh + 7) // 8) * ((W + 31) // 32), min(C, 64) // 8
    return vpr * ((tiles + npart - 1) // npart + 1) + int(math.log2(64 // vpr))


def chain_fwd(B, HW, C, dt, kernels, L_pre=1):
    """L of the statistics: the one-launch kernels keep IT pixels per lane, gepi_pass<T, 0> rpt rows per thread; producer partials: L_pre."""
    k = kernels[0]
    if k.startswith("gepi_small"):
        return 2 if k.endswith("256, 2>") else 4
    return gepi_geom(B, HW, C, _ve(dt)).rpt if k.startswith("gepi_pass") else L_pre


def chain_bwd(B, HW, C, dt, kernels):
    """(L1, L2): the one-launch kernel IT twice; gepi_pass<T, 1> rpt, then gepi_pass<T, 2> rpt or gepi_bwd2s' 4 vectors per thread and
    log2(16 / cv) row-rotation sums."""
    if kernels[0].startswith("gepi_small"):
        it = 2 if kernels[0].endswith("256, 2>") else 4
        return it, it
    rpt = gepi_geom(B, HW, C, _ve(dt)).rpt
    if any(k.startswith("gepi_bwd2s") for k in kernels):
        return rpt, 4 + 4 - int(math.log2(C // _ve(dt)))
    return rpt, rpt


# ---------------------------------------------------------------------------------------------------------------- the case table
# entry: the C ABI function; group: the environment it needs (GROUPS); args: what the runner reads (B, HW, C, flags; bias: given or NULL; data:
# "normal" | "int" | "const"; pre: producer partials; twin: the default-group row whose y / dx it must equal bit for bit); kernels: kernel_id()
# of every launch, in order; why: the launcher rule that selects them.
Case = namedtuple("Case", "id entry dtype group args kernels why")
CASES = []
FLAGS = EPI_ACT | EPI_NORM


def _case(id, entry, dt, kernels, why, group="default", **args):
    args.setdefault("flags", FLAGS); args.setdefault("bias", True); args.setdefault("data", "normal")
    if args["data"] == "int":                                # nw = 0, no bias, no activation: every partial sum is exact in every order
        args.update(flags=args["flags"] & EPI_NORM, bias=False)
    sfx = "-f32" if dt == F else "-bf16"
    if "twin" in args:
        args["twin"] += sfx
    CASES.append(Case(id + sfx, entry, dt, group, args, tuple(kernels), why))


def _fwd(id, dt, kernels, why, **a):
    _case("fwd-" + id, "sgx_gepi_fwd", dt, kernels, why, **a)


def _bwd(id, dt, kernels, why, **a):
    _case("bwd-" + id, "sgx_gepi_bwd", dt, kernels, why, **a)


for _dt in (F, H):
    _t, _v = tname(_dt), _ve(_dt)
    _mx = 512 if _dt == F else 1024
    _s0, _s1 = f"<{_t}, 256, 2>", f"<{_t}, 512, 4>"
    _p0, _p1, _p2, _ap = f"gepi_pass<{_t}, 0, false>", f"gepi_pass<{_t}, 1, false>", f"gepi_pass<{_t}, 2, false>", f"gepi_apply<{_t}>"
    _two_f, _two_b = [_p0, _ap], [_p1, _p2, "gepi_fin_bwd2"]
    # ---- the one-launch kernels at their seams (B 16, C 64: 64 channel groups), forward and backward
    for _hw, _k, _why in ((_mx // 4, _s0, "HW = 2 (256 / NV): the last size of 256 threads x 2 pixels"), (_mx // 4 + 1, _s1, "one pixel past it: 512 threads x 4, under 8 MB"),
                          (_mx, _s1, "HW = MAX_HW: every lane holds 4 pixels"), (4, _s0, "HW = 4 < the block's pixel rows"), (1, _s0, "a single pixel: variance 0")):
        _fwd(f"small-HW{_hw}", _dt, ["gepi_small_fwd" + _k], _why, B=16, HW=_hw, C=64)
        _bwd(f"small-HW{_hw}", _dt, ["gepi_small_bwd" + _k, "gepi_fin_bwd2"], _why, B=16, HW=_hw, C=64)
    _fwd(f"past-max-HW{_mx + 1}", _dt, _two_f, "HW = MAX_HW + 1: two-pass", B=16, HW=_mx + 1, C=64)
    _bwd(f"past-max-HW{_mx + 1}", _dt, _two_b, "HW = MAX_HW + 1: two-pass", B=16, HW=_mx + 1, C=64)
    _fwd("8MB-B8", _dt, ["gepi_small_fwd" + _s1], "HW = MAX_HW, C 512, B 8: exactly 8 MiB is one launch", B=8, HW=_mx, C=512)
    _fwd("8MB-B9", _dt, _two_f, "B 9: past 8 MiB, two-pass", B=9, HW=_mx, C=512)
    _bwd("8MB-B8", _dt, ["gepi_small_bwd" + _s1, "gepi_fin_bwd2"], "exactly 8 MiB is one launch", B=8, HW=_mx, C=512)
    _bwd("8MB-B9", _dt, _two_b, "B 9: past 8 MiB, two-pass", B=9, HW=_mx, C=512)
    _fwd("groups64", _dt, ["gepi_small_fwd" + _s0], "B C / 16 = 64 blocks: one launch", B=64, HW=16, C=16)
    _fwd("groups63", _dt, _two_f, "B C / 16 = 63: two-pass", B=63, HW=16, C=16)
    _bwd("groups64", _dt, ["gepi_small_bwd" + _s0, "gepi_fin_bwd2"], "B C / 16 = 64 blocks: one launch", B=64, HW=16, C=16)
    _bwd("groups63", _dt, _two_b, "B C / 16 = 63: two-pass", B=63, HW=16, C=16)
    _fwd("small-int", _dt, ["gepi_small_fwd" + _s1], "integer row of the one-launch kernel, 3 pixels short of full lanes", B=16, HW=_mx - 3, C=64, data="int")
    _bwd("small-int", _dt, ["gepi_small_bwd" + _s1, "gepi_fin_bwd2"], "integer row of the one-launch kernel", B=16, HW=_mx - 3, C=64, data="int")
    _fwd("small0-int", _dt, ["gepi_small_fwd" + _s0], "integer row, 256 threads x 2", B=16, HW=_mx // 4 - 1, C=64, data="int")
    _bwd("small0-int", _dt, ["gepi_small_bwd" + _s0, "gepi_fin_bwd2"], "integer row, 256 threads x 2", B=16, HW=_mx // 4 - 1, C=64, data="int")
    _fwd("small-const", _dt, ["gepi_small_fwd" + _s1], "constant channels: variance 0, the clamp and rstd = 1 / sqrt(eps)", B=16, HW=_mx // 2 + 5, C=64, data="const")
    for _fl in range(4):
        _fwd(f"small-flags{_fl}", _dt, ["gepi_small_fwd" + _s0], "flags; bias NULL on odd flags", B=16, HW=61, C=64, flags=_fl, bias=_fl % 2 == 0)
        _bwd(f"small-flags{_fl}", _dt, ["gepi_small_bwd" + _s0, "gepi_fin_bwd2"], "flags; bias NULL on odd flags", B=16, HW=61, C=64, flags=_fl, bias=_fl % 2 == 0)
    # ---- two-pass with the finalize folded into the apply pass
    for _hw, _why in ((4, "HW = 4 < the block's pixel rows"), (1, "a single pixel")):
        _fwd(f"fold-HW{_hw}", _dt, _two_f, _why, B=2, HW=_hw, C=32)
        _bwd(f"fold-HW{_hw}", _dt, _two_b, _why, B=2, HW=_hw, C=32)
    for _tag, _B, _hw, _C, _why in (("tail", 2, 1300, 4 * _v, "cv = 4: 3 chunks of 512 pixels, the last partial; 3 partials for 8 lanes x 8 in gepi_block_totals"),
                                    ("C256", 2, 700, 256, "C = 256: one lane per channel, 11 (bf16) / 22 (fp32) partials in trips of 8"),
                                    ("cv1", 2, 2500, _v, "cv = 1: 256 pixel rows per block, 2 chunks"),
                                    ("C512", 1, 100, 512, "C = 512: two channel passes of gepi_block_totals")):
        _fwd(f"fold-{_tag}", _dt, _two_f, _why, B=_B, HW=_hw, C=_C)
        _bwd(f"fold-{_tag}", _dt, _two_b, _why, B=_B, HW=_hw, C=_C)
    _fwd("fold-int", _dt, _two_f, "integer row: a dropped or doubled pixel fails at any HW", B=2, HW=1300, C=4 * _v, data="int")
    _bwd("fold-int", _dt, _two_b, "integer row", B=2, HW=1300, C=4 * _v, data="int")
    _fwd("fold-const", _dt, _two_f, "constant channels: variance 0", B=2, HW=1300, C=4 * _v, data="const")
    for _fl in range(4):
        for _bi in (True, False):
            _n = f"fold-flags{_fl}-{'bias' if _bi else 'nobias'}"
            _fwd(_n, _dt, _two_f if _fl & 2 else [_ap], "flags x bias" + ("" if _fl & 2 else "; norm off: no statistics pass"), B=2, HW=300, C=32, flags=_fl, bias=_bi)
            _bwd(_n, _dt, _two_b, "flags x bias (norm off: the statistics terms are dropped); dbias NULL without a bias", B=2, HW=300, C=32, flags=_fl, bias=_bi, dbias=_bi)
    # ---- producer partials
    for _np in (1, 7, 17, 129):
        _fwd(f"pre-{_np}", _dt, ["gepi_fin_stats", _ap], f"pre_part with {_np} partials built in fp64: 16 lanes stride over them", B=2, HW=300, C=32, pre=_np)
    _fwd("pre-int", _dt, ["gepi_fin_stats", _ap], "integer row from 17 producer partials", B=2, HW=300, C=32, pre=17, data="int")
    _case("blur_stats", "sgx_blur3x3_stats", _dt, [f"blur_stats_kernel<{_t}>", "gepi_fin_stats", _ap], "the blur's partials (3 strips x 2 column chunks) feed the epilogue",
          B=2, H=20, W=70, C=32)
    _case("blur_stats-cv1-noact", "sgx_blur3x3_stats", _dt, [f"blur_stats_kernel<{_t}>", "gepi_fin_stats", _ap], "cv = 1: 256 columns per block; no activation, bias NULL",
          B=1, H=9, W=300, C=_v, flags=EPI_NORM, bias=False)
    # ---- sgx_gepi_stats
    _case("stats", "sgx_gepi_stats", _dt, [_p0, "gepi_fin_stats"], "the statistics half alone", B=2, HW=1300, C=4 * _v)
    _case("stats-pre", "sgx_gepi_stats", _dt, ["gepi_fin_stats"], "from 7 producer partials", B=2, HW=300, C=32, pre=7)
    _case("stats-nonorm", "sgx_gepi_stats", _dt, ["gepi_fin_stats"], "norm off: 0 / 1 written", B=2, HW=300, C=32, flags=EPI_ACT)
    _case("stats-int", "sgx_gepi_stats", _dt, [_p0, "gepi_fin_stats"], "integer row", B=2, HW=1300, C=4 * _v, data="int")
    # ---- SGX_GEPI_APPLY1=2 SGX_GEPI_BWD2S=2: the short-lived blocks at small sizes, against the default rows they promise the bits of
    _a1 = ["gepi_fin_stats", f"gepi_apply1<{_t}>"]
    _fwd("apply1", _dt, [_p0] + _a1, "own statistics; 1300 x 4 vectors: 21 blocks, the last partial", group="switch", B=2, HW=1300, C=4 * _v, twin="fwd-fold-tail")
    _fwd("apply1-cv1", _dt, [_p0] + _a1, "cv = 1", group="switch", B=2, HW=2500, C=_v, twin="fwd-fold-cv1")
    _fwd("apply1-pre", _dt, _a1, "from 17 producer partials", group="switch", B=2, HW=300, C=32, pre=17, twin="fwd-pre-17")
    _fwd("apply1-int", _dt, [_p0] + _a1, "integer row", group="switch", B=2, HW=1300, C=4 * _v, data="int", twin="fwd-fold-int")
    _fwd("apply1-nonorm", _dt, _a1, "norm off: the table carries 0 / 1", group="switch", B=2, HW=300, C=32, flags=1, bias=False, twin="fwd-fold-flags1-nobias")
    for _cv in (1, 2, 4, 8, 16):
        _b2 = [_p1, "gepi_fin_bwd1", f"gepi_bwd2s<{_t}>"]
        _rot = f"cv = {_cv}: {4 - int(math.log2(_cv))} row-rotation sums"
        _bwd(f"bwd2s-cv{_cv}-one-block", _dt, _b2 + ["gepi_rows_prereduce", "gepi_fin_bwd2"], _rot + "; HW cv < 256: one partial block per image, the 2 block rows pre-reduced one to one",
             group="switch", B=2, HW=max(1, 200 // _cv), C=_cv * _v)
        _bwd(f"bwd2s-cv{_cv}-3-blocks", _dt, _b2 + ["gepi_fin_bwd2"], _rot + "; 3 blocks per image, the last partial; 6 block rows > 4 chunks: gepi_fin_bwd2 on the block partials",
             group="switch", B=2, HW=2500 // _cv + 1, C=_cv * _v)
        _bwd(f"bwd2s-cv{_cv}-int", _dt, _b2 + ["gepi_fin_bwd2"], _rot + "; integer row, 5 blocks per image", group="switch", B=2, HW=4500 // _cv + 1, C=_cv * _v, data="int")
    _bwd("bwd2s-twin", _dt, [_p1, "gepi_fin_bwd1", f"gepi_bwd2s<{_t}>", "gepi_fin_bwd2"], "the default row's bits", group="switch", B=2, HW=1300, C=4 * _v, twin="bwd-fold-tail")
    _bwd("bwd2s-twin-flags1", _dt, [_p1, "gepi_fin_bwd1", f"gepi_bwd2s<{_t}>", "gepi_fin_bwd2"], "norm off: the table's two coefficients are 0; dbias NULL",
         group="switch", B=2, HW=300, C=32, flags=1, bias=False, dbias=False, twin="bwd-fold-flags1-nobias")
    _bwd("bwd2s-prereduce", _dt, [_p1, "gepi_fin_bwd1", f"gepi_bwd2s<{_t}>", "gepi_rows_prereduce", "gepi_fin_bwd2"],
         "B nblk = 512 > 256 block rows, B nchunk = 256: pre-reduced to 256 rows of 2 each", group="switch", B=64, HW=4096, C=2 * _v, data="int")
    # ---- ... plus SGX_NT_MIN_MB=0.001: C = 256 keeps the loop kernel, with the nontemporal accesses
    _nt = [_p1, f"gepi_pass<{_t}, 2, true>", "gepi_fin_bwd2"]
    _bwd("nt-C256", _dt, _nt, "C = 256 > 128 and past the nontemporal threshold", group="switch_nt", B=2, HW=700, C=256, twin="bwd-fold-C256")
    _bwd("nt-C256-int", _dt, _nt, "integer row", group="switch_nt", B=2, HW=700, C=256, data="int")
    # ---- SGX_GEPI_FOLD=0: the separate finalize launches and the coefficient pairs they write
    _nf_f, _nf_b = [_p0, "gepi_fin_stats", _ap], [_p1, "gepi_fin_bwd1", _p2, "gepi_fin_bwd2"]
    for _tag, _hw, _C in (("tail", 1300, 4 * _v), ("C256", 700, 256)):
        _fwd(f"nofold-{_tag}", _dt, _nf_f, "separate gepi_fin_stats", group="nofold", B=2, HW=_hw, C=_C, twin=f"fwd-fold-{_tag}")
        _bwd(f"nofold-{_tag}", _dt, _nf_b, "separate gepi_fin_bwd1 with coef", group="nofold", B=2, HW=_hw, C=_C, twin=f"bwd-fold-{_tag}")
    _fwd("nofold-int", _dt, _nf_f, "integer row", group="nofold", B=2, HW=1300, C=4 * _v, data="int", twin="fwd-fold-int")
    _bwd("nofold-int", _dt, _nf_b, "integer row", group="nofold", B=2, HW=1300, C=4 * _v, data="int", twin="bwd-fold-int")
    _fwd("nofold-nonorm", _dt, ["gepi_fin_stats", _ap], "norm off: gepi_fin_stats writes 0 / 1", group="nofold", B=2, HW=300, C=32, flags=1, bias=False, twin="fwd-fold-flags1-nobias")

_fwd("fold-C2048", F, ["gepi_pass<float, 0, false>", "gepi_apply<float>"], "cv = 512 > 256: two channel-vector passes per thread, 65 chunks of 8 pixels", B=1, HW=520, C=2048)
_bwd("fold-C2048", F, ["gepi_pass<float, 1, false>", "gepi_pass<float, 2, false>", "gepi_fin_bwd2"], "cv = 512 > 256", B=1, HW=520, C=2048)
# ---- the default policy at its real thresholds (bf16 1024^2 x 16; fp64 references computed on the GPU)
_P = 1 << 20
_fwd("headline-B6", H, ["gepi_pass<bf16_t, 0, false>", "gepi_fin_stats", "gepi_apply1<bf16_t>"], "201 MB >= 192 MB: the short-lived apply blocks", B=6, HW=_P, C=16)
_fwd("headline-B5", H, ["gepi_pass<bf16_t, 0, false>", "gepi_apply<bf16_t>"], "168 MB < 192 MB: the loop kernel with the folded finalize", B=5, HW=_P, C=16)
_bwd("headline-B24", H, ["gepi_pass<bf16_t, 1, false>", "gepi_fin_bwd1", "gepi_bwd2s<bf16_t>", "gepi_rows_prereduce", "gepi_fin_bwd2"],
     "805 MB >= 800 MB: the short-lived backward blocks, 49152 block rows pre-reduced to 256", B=24, HW=_P, C=16)

_case("conv_stats", "sgx_conv3x3_stats", H, ["gepi_fin_stats", "gepi_apply<bf16_t>"], "the convolution's per-slot partials feed the epilogue (the profiler brackets sgx_gepi_fwd alone)",
      B=1, H=256, W=256, C=16)

assert len({c.id for c in CASES}) == len(CASES), "duplicate case id"
BY_ID = {c.id: c for c in CASES}

# the three gepi_check rejections: (id, B, HW, C, dtype, workspace bytes short, expected code, why)
REJECTIONS = [
    ("gepi-C10", 2, 16, 10, F, 0, -2, "C % VE != 0"),
    ("gepi-cv3", 2, 16, 12, F, 0, -2, "cv = 3 does not divide 256"),
    ("gepi-short-workspace", 2, 16, 32, F, 1, -3, "workspace one byte short"),
]

# Launch sites of csrc/gepi.hip / csrc/optim.hip that no row reaches, with the reason (tests/test_epilogue_coverage.py)
EXCLUDED_SITES = {}
EXCLUDED_PATHS = {
    "SGX_GEPI_SMALL=0 / SGX_GEPI_RPT / SGX_GEPI_APPLY1=0 / SGX_GEPI_BWD2S=0": "A/B switches read once per process; their kernels are the two-pass rows', "
                                                                             "and what they select is planned on the CPU by tests/test_gepi_plan.py",
}
# Launch paths (group, kernel list with the dtype written T) that have no integer row, each with the reason; every other path must have one
NO_INTEGER_ROW = {
    ("default", ("gepi_apply<T>",)): "norm off: no statistics pass, so there is no sum that integers would make exact",
    ("default", ("gepi_fin_stats",)): "sgx_gepi_stats from fp64 partials or with the norm off: the finalize alone, which fwd-pre-int runs on integer partials",
    ("default", ("blur_stats_kernel<T>", "gepi_fin_stats", "gepi_apply<T>")): "the blur's partials are checked against fp64 sums of the stored y by the strip's chain length, its rows are 1400 / 2700 pixels",
    ("switch", ("gepi_fin_stats", "gepi_apply1<T>")): "gepi_apply1 behind partials or with the norm off: the kernels of fwd-apply1-int minus the statistics pass, and the default twin's bits",
    ("nofold", ("gepi_fin_stats", "gepi_apply<T>")): "norm off: gepi_fin_stats writes the constants 0 / 1, no sum",
    ("default", ("gepi_pass<T, 0, false>", "gepi_fin_stats", "gepi_apply1<T>")): "fwd-headline-B6 pins the 192 MB threshold on normal data; the same kernels have fwd-apply1-int",
    ("default", ("gepi_pass<T, 1, false>", "gepi_fin_bwd1", "gepi_bwd2s<T>", "gepi_rows_prereduce", "gepi_fin_bwd2")):
        "bwd-headline-B24 pins the 800 MB threshold on normal data; the same kernels have bwd-bwd2s-prereduce, an integer row",
}


# ---------------------------------------------------------------------------------------------------------------- optimizer kernels
MT_SWEEP = 32 * 256                 # lanes of sumsq_stage1's grid per tensor; a sweep of the 16-byte loop covers 4 x this many floats
OPTIM_KERNELS = {"sgx_gradnorm_clip_coef": ("sumsq_stage1", "sumsq_stage2"), "sgx_adam_multi": ("adam_multi_kernel",), "sgx_ema_multi": ("ema_multi_kernel",)}
# (n, 4-byte shift): why
GRADNORM_SIZES = [
    (1, 0, "the scalar tail only"), (3, 0, "n < 4"), (4, 0, "one vector"), (98304, 0, "3 sweeps: the last size below the four-in-flight loop"),
    (98309, 0, "four in flight + one lane of the single loop + tail 1"), (98310, 0, "tail 2"), (98311, 0, "tail 3"),
    (4 * 4 * 4 * MT_SWEEP + 4 * 5 + 1, 0, "524 309: four trips of four in flight: the fp32 flush"), (32 * MT_SWEEP + 1, 1, "262 145 misaligned: the scalar branch and its flush every 32"),
    (1027, 1, "misaligned, no flush"),
]
ADAM_SIZES = (1, 65536, 65537, 2359296)
N_ADAM_M, N_ADAM_V, N_ADAM_P, N_EMA = 3, 4, 18, 2


def adam(p, g, m, v, beta1, beta2, eps, step, bc2, gs):
    """One Adam step in fp64 on the fp32 coefficients the kernel holds (1 - beta rounded in fp32) -> ((p, m, v), (S_p, S_m, S_v)).
    fp32 chains: m: g gs, (1 - b1) gi, the sum (3); v: + the square (4); p: m (3), v (4 + 2, halved by the root) + sqrtf (2) + / bc2 + eps (2): 8
    on the denominator, the division (3), the step, the difference: 16, taken as 18."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    o1, o2 = float(np.float32(1) - np.float32(beta1)), float(np.float32(1) - np.float32(beta2))
    gi = g * gs
    mi, Sm = b1 * m + o1 * gi, b1 * m.abs() + o1 * gi.abs()
    vi = b2 * v + o2 * gi * gi
    den = vi.sqrt() / bc2 + eps
    return (p - step * (mi / den), mi, vi), (p.abs() + step * (Sm / den), Sm, vi)


def ema(a, b, beta):
    bt, ob = float(np.float32(beta)), float(np.float32(1) - np.float32(beta))
    return bt * a + ob * b, bt * a.abs() + ob * b.abs()
